"""The fp32 form of csrc/conv_stem.hip -- the REAL kernel source, launcher and C-ABI entry (conv_stem_f32_kernel, mdetr_conv_stem_f32) -- on
the HIP-on-CPU shim (tests/native_emul.py) through monodetr_amd/conv_stem_ext.py with the family MDETR_CONV_STEM_F32 on: every kind of
tests/conv_stem_f32_cases.py on every shape (the widest one, six column tiles, with the "x", random and non-finite kinds only: the shim
is slow), the packed planes, the entry's refusals one by one and the empty problem."""
import pytest
import torch

import conv_stem_f32_cases as X
import native_emul


@pytest.fixture()
def ext(monkeypatch):
    from monodetr_amd import conv_stem_ext
    monkeypatch.setattr(conv_stem_ext, "_backend", native_emul.lib())
    monkeypatch.setattr(conv_stem_ext, "ENABLED_F32", True)
    return conv_stem_ext


_ids = lambda s: "x".join(map(str, s))                                # noqa: E731
WIDE = (1, 9, 330)            # six column tiles: 3.5 s per kind on the shim -- the "x" and the random kind only here; every kind on the GPU


@pytest.mark.parametrize("shape", X.SHAPES, ids=_ids)
def test_conv_stem_f32_exact_cases(ext, monkeypatch, shape):
    assert len(X.SHAPES) == 5 and WIDE in X.SHAPES
    calls = X.record_launches(ext, monkeypatch)
    kinds = ("x",) if shape == WIDE else X.KINDS
    X.check_exact(ext, "cpu", shape, kinds)
    assert calls == [torch.float32] * len(kinds), calls


@pytest.mark.parametrize("shape", [s for s in X.SHAPES if s != WIDE], ids=_ids)
def test_conv_stem_f32_small_integers(ext, shape):
    X.check_small_integers(ext, "cpu", shape)


@pytest.mark.parametrize("shape", X.SHAPES, ids=_ids)
def test_conv_stem_f32_random_case_twice(ext, monkeypatch, shape):
    calls = X.record_launches(ext, monkeypatch)
    X.check_random(ext, "cpu", shape, twice=True)
    assert calls == [torch.float32] * 2, calls


@pytest.mark.parametrize("shape", X.SHAPES, ids=_ids)
def test_conv_stem_f32_nonfinite_pixel(ext, shape):
    X.check_nonfinite(ext, "cpu", shape)


def test_conv_stem_f32_packed_planes(ext):
    X.check_packed_planes(ext)


def _operands(B=1, H=4, W=6):
    from monodetr_amd import conv_stem_ext
    x = torch.randn(B, H, W, 3)
    planes = conv_stem_ext.pack_weight_f32(torch.randn(64, 3, 7, 7) / 12.0)
    OH, OW = X.out_hw(H, W)
    return x, planes, torch.randn(64), torch.full((B, OH, OW, 64), float("nan"))


def test_conv_stem_f32_entry_without_shift_and_empty_problem():
    lib = native_emul.lib()
    x, planes, shift, y = _operands()
    assert X.entry(lib, x, planes, shift, y, 1, 4, 6) == 0 and bool(torch.isfinite(y).all()) and bool((y >= 0).all())
    y0 = torch.full_like(y, float("nan"))
    assert X.entry(lib, x, planes, None, y0, 1, 4, 6) == 0 and bool(torch.isfinite(y0).all()) and not torch.equal(y0, y)       # shift = NULL
    # an empty problem returns 0, launches nothing and looks at no pointer
    for sizes in ((0, 4, 6), (1, 0, 6), (1, 4, 0)):
        assert lib.mdetr_conv_stem_f32(None, None, None, None, *sizes, -1, None) == 0, sizes
    untouched = torch.full_like(y, float("nan"))
    assert X.entry(lib, x, planes, shift, untouched, 0, 4, 6) == 0 and bool(untouched.isnan().all())


def test_conv_stem_f32_refusals():
    lib = native_emul.lib()
    x, planes, shift, y = _operands()
    assert x.data_ptr() % 16 == 0 and planes.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 0

    def refused(word, *sizes, **over):
        before = y.clone()
        rc = X.entry(lib, x, planes, shift, y, *(sizes or (1, 4, 6)), **over)
        msg = lib.mdetr_last_error()
        assert rc == -1 and msg.startswith(b"mdetr_conv_stem_f32") and word in msg, (rc, msg)        # MDETR_E_ARG
        assert torch.equal(before.view(torch.int32), y.view(torch.int32))                              # nothing written
    assert X.entry(lib, x, planes, shift, y, 1, 4, 6) == 0
    for sizes in ((-1, 4, 6), (1, -4, 6), (1, 4, -6)):                  # negative sizes
        refused(b"bad sizes", *sizes)
    assert lib.mdetr_conv_stem_f32(None, planes.data_ptr(), None, y.data_ptr(), 1, 4, 6, -1, None) == -1 and b"null pointer" in lib.mdetr_last_error()
    assert lib.mdetr_conv_stem_f32(x.data_ptr(), None, None, y.data_ptr(), 1, 4, 6, -1, None) == -1 and b"null pointer" in lib.mdetr_last_error()
    assert lib.mdetr_conv_stem_f32(x.data_ptr(), planes.data_ptr(), None, None, 1, 4, 6, -1, None) == -1 and b"null pointer" in lib.mdetr_last_error()
    refused(b"planes are not 16-byte aligned", wp=planes.data_ptr() + 8)
    refused(b"y is not 16-byte aligned", yp=y.data_ptr() + 8)
    refused(b"x is not 4-byte aligned", xp=x.data_ptr() + 2)
    # 32-bit byte offsets, judged from the sizes before any pointer is followed: 256 x 1024 x 683 x 12 is the first size at or beyond 2^31
    assert 256 * 1024 * 682 * 12 < 1 << 31 <= 256 * 1024 * 683 * 12
    refused(b"below 2 GiB", 256, 1024, 683)
    refused(b"below 2 GiB", 1 << 14, 1 << 14, 1 << 14)                  # (a product beyond 64 bits of nothing: 2^42 x 12)
    # x at a 4-byte (not 16-byte) boundary is taken
    xs = torch.randn(1 * 4 * 6 * 3 + 1)[1:]
    assert xs.data_ptr() % 16 == 4 and lib.mdetr_conv_stem_f32(xs.data_ptr(), planes.data_ptr(), None, y.data_ptr(), 1, 4, 6, -1, None) == 0
