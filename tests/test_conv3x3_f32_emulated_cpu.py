"""The fp32 form of csrc/conv3x3.hip -- the REAL kernel source, launcher and C-ABI entry (mdetr_conv3x3_f32) -- on the HIP-on-CPU shim
(tests/native_emul.py) through monodetr_amd/conv3x3_ext.py with the family MDETR_CONV3X3_F32 on: the exact and random cases of
tests/conv3x3_f32_cases.py on the five shapes with 64 input channels, every (tile, width) the launcher builds on a small ragged image,
and the entry's refusals.  (The shim is slow: the 192- and 128-channel shapes run on the GPU only.)"""
import pytest
import torch

import conv3x3_f32_cases as X
import native_emul
from conftest import tune

SHAPES = [s for s in X.SHAPES if s[3] == 64]
SWEEP_SHAPE = (1, 5, 19, 64, 64)          # ragged in H and W for every tile, two slabs, dx on the kernel


@pytest.fixture()
def ext(monkeypatch):
    from monodetr_amd import conv3x3_ext
    monkeypatch.setattr(conv3x3_ext, "_backend", native_emul.lib())
    monkeypatch.setattr(conv3x3_ext, "ENABLED_F32", True)
    tune(monkeypatch, conv3x3_f32_tile=None, conv3x3_f32_nb=None)
    return conv3x3_ext


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv3x3_f32_exact_and_random_cases(ext, monkeypatch, shape):
    assert len(SHAPES) == 5
    calls = X.record_launches(ext, monkeypatch)
    X.check_exact(ext, "cpu", shape)
    assert all(c[0] == torch.float32 for c in calls) and len(calls) == (9 if X.dx_on_kernel(shape[3], shape[4]) else 3), calls
    X.check_small_integers(ext, "cpu", shape, calls)
    X.check_random(ext, "cpu", shape, twice=True)


@pytest.mark.parametrize("nb", X.NBS)
@pytest.mark.parametrize("tile", X.TILES)
def test_conv3x3_f32_every_tile_and_width(ext, monkeypatch, tile, nb):
    tune(monkeypatch, conv3x3_f32_tile=tile, conv3x3_f32_nb=nb)
    lib = native_emul.lib()
    B, H, W, C, N = SWEEP_SHAPE
    assert lib.mdetr_conv3x3_f32_plan(B, H, W, N) == 10 * tile + nb
    tag = "tile %d nb %d" % (tile, nb)
    X.check_random(ext, "cpu", SWEEP_SHAPE, tag)
    X.check_exact(ext, "cpu", SWEEP_SHAPE, ("int", "x"), tag)


def test_conv3x3_f32_refusals():
    lib = native_emul.lib()
    x = torch.randn(1, 4, 4, 64)
    w = torch.randn(32, 3, 3, 64)
    y = torch.empty(1, 4, 4, 32)
    args = lambda *p: p + (-1, None)                                    # noqa: E731
    assert lib.mdetr_conv3x3_f32(*args(x.data_ptr(), w.data_ptr(), None, None, y.data_ptr(), 1, 4, 4, 64, 32, 0)) == 0
    assert lib.mdetr_conv3x3_f32(*args(x.data_ptr(), w.data_ptr(), None, None, y.data_ptr(), 1, 4, 4, 48, 32, 0)) != 0       # C % 64
    assert b"mdetr_conv3x3_f32" in lib.mdetr_last_error()
    assert lib.mdetr_conv3x3_f32(*args(x.data_ptr(), w.data_ptr(), None, None, y.data_ptr(), 1, 4, 4, 64, 40, 0)) != 0       # N % 32
    for i in range(4):                                                  # a misaligned x, w, mask or y
        p = [x.data_ptr(), w.data_ptr(), None, y.data_ptr(), y.data_ptr()]
        p[(0, 1, 3, 4)[i]] += 4
        assert lib.mdetr_conv3x3_f32(*args(*p, 1, 4, 4, 64, 32, 0)) != 0, i
    assert lib.mdetr_conv3x3_f32(*args(None, w.data_ptr(), None, None, y.data_ptr(), 1, 4, 4, 64, 32, 0)) != 0               # null pointer
    assert lib.mdetr_conv3x3_f32(*args(None, None, None, None, None, 0, 4, 4, 64, 32, 0)) == 0                               # empty batch
    assert lib.mdetr_conv3x3_f32_plan(0, 4, 4, 32) < 0
