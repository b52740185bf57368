"""The fp32 form of csrc/conv_taps.hip -- the REAL kernel source, launchers and C-ABI entries (mdetr_conv_taps_f32,
mdetr_conv_taps_f32_split, mdetr_conv_dgrad_s2_f32) -- on the HIP-on-CPU shim (tests/native_emul.py) through
monodetr_amd/conv_taps_ext.py with the family MDETR_CONV_STRIDED_F32 on: the exact and random cases of tests/conv_strided_f32_cases.py on
the shapes with 64 input channels, every (rows, width) the launcher builds on one small ragged image, the split entry, and the entries'
refusals.  (The shim is slow: the 192-channel shape runs on the GPU only.)"""
import pytest
import torch

import conv_strided_f32_cases as X
import native_emul
from conftest import tune

SHAPES = [s for s in X.SHAPES if s[3] == 64]
SWEEP_SHAPE = (1, 5, 67, 64, 192)         # 3 x 34 outputs: ragged in both directions at 4 and at 2 rows; last channel group ragged at NB = 4


@pytest.fixture()
def ext(monkeypatch):
    from monodetr_amd import conv_taps_ext
    monkeypatch.setattr(conv_taps_ext, "_backend", native_emul.lib())
    monkeypatch.setattr(conv_taps_ext, "ENABLED_F32", True)
    X.lift_shape_rule(conv_taps_ext, monkeypatch)
    tune(monkeypatch, conv_taps_f32_rows=None, conv_taps_f32_nb=None, conv_taps_split=None)
    return conv_taps_ext


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv_strided_f32_exact_and_random_cases(ext, monkeypatch, shape):
    assert len(SHAPES) == 5
    calls = X.record_launches(ext, monkeypatch)
    X.check_exact(ext, "cpu", shape)
    on_kernel = X.dx_on_kernel(shape[3], shape[4])
    assert all(c[1] == torch.float32 for c in calls) and [c[0] for c in calls] == (["fwd", "fwd", "dx"] if on_kernel else ["fwd"]) * 3, calls
    X.check_small_integers(ext, "cpu", shape, calls)
    X.check_random(ext, "cpu", shape, twice=True)


@pytest.mark.parametrize("rows,nb", X.GEOMETRIES)
def test_conv_strided_f32_every_forward_geometry(ext, monkeypatch, rows, nb):
    tune(monkeypatch, conv_taps_f32_rows=rows, conv_taps_f32_nb=nb)
    tag = "rows %d nb %d" % (rows, nb)
    X.check_random(ext, "cpu", SWEEP_SHAPE, tag)
    X.check_exact(ext, "cpu", SWEEP_SHAPE, ("int", "x"), tag)


@pytest.mark.parametrize("nb", X.DGRAD_NBS)
def test_conv_strided_f32_every_input_gradient_width(ext, monkeypatch, nb):
    """C = 192 outputs of the input gradient: three groups at NB = 2, a ragged second group at NB = 4; 5 x 7 pixels: four class sizes."""
    tune(monkeypatch, conv_taps_f32_nb=nb)
    shape = (1, 5, 7, 192, 64)
    X.check_random(ext, "cpu", shape, "dgrad nb %d" % nb)
    X.check_exact(ext, "cpu", shape, ("int", "x"), "dgrad nb %d" % nb)


def test_conv_strided_f32_split_entry_and_route(ext, monkeypatch):
    X.check_split_entry(native_emul.lib(), "cpu")
    shape = (1, 3, 3, 512, 32)                                          # the smallest shape _split_count admits: 16 slabs of 32 channels -> 4 splits
    assert ext._split_count(1, 2, 2, 32, 512, 3, False) == 4 and ext._split_count(1, 2, 2, 32, 480, 3, False) == 0
    calls = X.record_launches(ext, monkeypatch)
    X.check_random(ext, "cpu", shape, "split route")
    assert calls == [("split", torch.float32)], calls
    X.check_exact(ext, "cpu", shape, ("x",), "split route")


def test_conv_strided_f32_refusals():
    lib = native_emul.lib()
    x, w, y = torch.randn(1, 4, 4, 64), torch.randn(32, 3, 3, 64), torch.empty(1, 2, 2, 32)
    dims = lambda B=1, H=4, W=4, C=64, N=32: torch.tensor(X.taps_dims(B, H, W, C, N), dtype=torch.int64)        # noqa: E731
    fwd = lambda xp, wp, yp, d: lib.mdetr_conv_taps_f32(xp, wp, None, yp, d.data_ptr(), 0, -1, None)            # noqa: E731
    assert fwd(x.data_ptr(), w.data_ptr(), y.data_ptr(), dims()) == 0
    assert fwd(x.data_ptr(), w.data_ptr(), y.data_ptr(), dims(C=96)) != 0                                       # C % 64
    assert b"mdetr_conv_taps_f32" in lib.mdetr_last_error()
    assert fwd(x.data_ptr(), w.data_ptr(), y.data_ptr(), dims(N=48)) != 0                                       # N % 32
    for i in range(3):                                                  # a misaligned x, w or y
        p = [x.data_ptr(), w.data_ptr(), y.data_ptr()]
        p[i] += 4
        assert fwd(*p, dims()) != 0, i
    assert fwd(None, w.data_ptr(), y.data_ptr(), dims()) != 0                                                   # null pointer
    assert fwd(None, None, None, dims(B=0)) == 0                                                                # empty batch
    one = X.taps_dims(1, 4, 4, 64, 32)
    one[8] = one[9] = 1; one[10] = one[11] = 0                          # the 1x1 / stride-2 forward: a token GEMM in fp32, refused
    assert fwd(x.data_ptr(), w.data_ptr(), y.data_ptr(), torch.tensor(one, dtype=torch.int64)) != 0
    assert b"mdetr_conv_taps_f32" in lib.mdetr_last_error()
    assert fwd(x.data_ptr(), w.data_ptr(), y.data_ptr(), dims(B=1 << 15, H=128, W=128)) != 0                    # B H W C = 2^35 >= 2^29
    assert fwd(x.data_ptr(), w.data_ptr(), y.data_ptr(), dims(B=1 << 9, H=128, W=128)) != 0                     # B H W C = 2^29 exactly

    part = torch.empty(4, 1, 2, 2, 32)
    d1 = dims()
    split = lambda ks, d=d1, floats=part.numel(): lib.mdetr_conv_taps_f32_split(                                 # noqa: E731
        x.data_ptr(), w.data_ptr(), None, part.data_ptr(), floats, d.data_ptr(), ks, -1, None)
    assert split(2) == 0 and split(4) == 0
    assert split(1) != 0 and split(8) != 0 and split(3) != 0                                                    # ksplit < 2; 64 % (16 x 8); 64 % 48
    assert b"mdetr_conv_taps_f32_split" in lib.mdetr_last_error()
    assert split(4, floats=part.numel() - 1) != 0                                                               # a short partial buffer
    assert split(2, dims(B=0)) == 0

    dy, wt, dx = torch.randn(1, 2, 2, 64), torch.randn(32, 3, 3, 64), torch.empty(1, 4, 4, 32)
    dgrad = lambda a, b, c, *s: lib.mdetr_conv_dgrad_s2_f32(a, b, c, *s, -1, None)                              # noqa: E731
    sizes = (1, 2, 2, 64, 4, 4, 32, 3)                                   # B OH OW N H W C K
    assert dgrad(dy.data_ptr(), wt.data_ptr(), dx.data_ptr(), *sizes) == 0
    assert dgrad(dy.data_ptr(), wt.data_ptr(), dx.data_ptr(), 1, 2, 2, 96, 4, 4, 32, 3) != 0                    # N % 64
    assert b"mdetr_conv_dgrad_s2_f32" in lib.mdetr_last_error()
    assert dgrad(dy.data_ptr(), wt.data_ptr(), dx.data_ptr(), 1, 2, 2, 64, 4, 4, 48, 3) != 0                    # C % 32
    assert dgrad(dy.data_ptr(), wt.data_ptr(), dx.data_ptr(), 1, 2, 2, 64, 4, 4, 32, 1) != 0                    # K = 1: the shortcut
    assert dgrad(dy.data_ptr(), wt.data_ptr(), dx.data_ptr(), 1, 2, 2, 64, 5, 4, 32, 3) != 0                    # OH != (H - 1) / 2 + 1
    for i in range(3):
        p = [dy.data_ptr(), wt.data_ptr(), dx.data_ptr()]
        p[i] += 4
        assert dgrad(*p, *sizes) != 0, i
    assert dgrad(dy.data_ptr(), None, dx.data_ptr(), *sizes) != 0
    assert dgrad(dy.data_ptr(), wt.data_ptr(), dx.data_ptr(), 1 << 11, 128, 128, 64, 256, 256, 32, 3) != 0      # B OH OW N = 2^31 >= 2^29
    assert dgrad(dy.data_ptr(), wt.data_ptr(), dx.data_ptr(), 1 << 10, 64, 64, 64, 128, 128, 64, 3) != 0        # B H W C = 2^30 (B OH OW N = 2^28 fits)
    big = torch.tensor(X.taps_dims(1, 4, 4, 64, 32), dtype=torch.int64)
    big[12] = 1 << 32                                                   # a tap offset that would narrow to 0
    assert fwd(x.data_ptr(), w.data_ptr(), y.data_ptr(), big) != 0 and b"mdetr_conv_taps_f32" in lib.mdetr_last_error()
    assert dgrad(None, None, None, 0, 2, 2, 64, 4, 4, 32, 3) == 0                                               # empty batch
