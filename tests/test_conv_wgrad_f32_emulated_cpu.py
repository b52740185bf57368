"""The fp32 form of csrc/conv_wgrad.hip -- the REAL kernel source, launcher and C-ABI entry (mdetr_conv_wgrad_f32) -- on the HIP-on-CPU
shim (tests/native_emul.py) through conv_wgrad_ext.weight_gradient with the family MDETR_CONV_WGRAD_F32 on, its partials added by the
emulated mdetr_chunk_sums: the exact and random cases of tests/conv_wgrad_f32_cases.py on the first three shapes, the chunking as a
partition of the pixel tiles, and the entry's refusals.  (The shim is slow: the fourth shape and the large ones run on the GPU only.)"""
import pytest
import torch

import conv_wgrad_f32_cases as X
import native_emul
from conftest import tune
from gemm_bounds import assert_product_close

SHAPES = X.SHAPES[:3]
MDETR_E_ARG = -1


@pytest.fixture()
def ext(monkeypatch):
    from monodetr_amd import chunk_sums, conv_wgrad_ext
    L = native_emul.lib()
    L.mdetr_conv_wgrad_f32                                              # (AttributeError without the feature)
    monkeypatch.setattr(conv_wgrad_ext, "_backend", L)
    monkeypatch.setattr(conv_wgrad_ext, "ENABLED_CONV_F32", True)
    X.lift_shape_rule(conv_wgrad_ext, monkeypatch)                     # the kernel is under test here, on every shape the entry takes
    monkeypatch.setattr(chunk_sums, "_backend", L)                      # the partials go through the chunk-sum kernel, as in the step
    monkeypatch.setattr(chunk_sums, "ENABLED", True)
    tune(monkeypatch, conv_wgrad_wgs=None)
    return conv_wgrad_ext


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv_wgrad_f32_exact_and_random_cases(ext, shape):
    wgrad = X.direct(ext)
    X.check_exact(wgrad, "cpu", shape)
    X.check_small_integers(wgrad, "cpu", shape)
    X.check_random(wgrad, "cpu", shape, twice=True)


def test_conv_wgrad_f32_chunking_is_a_partition(ext, monkeypatch):
    """conv_wgrad_wgs moves the chunk count; every partial of every chunk is written (the buffer starts as NaN); the chunks added in
    order are within the bound of fp64, and the integer case is exact at every chunk count."""
    L = native_emul.lib()
    shape = (2, 5, 37, 64, 64)                                          # 6 pixel tiles; 3 tap rows x 1 x 1 blocks
    B, H, W, C, N = shape
    x, dy = X.random_operands(shape, "cpu")
    ref, mag = X.random_reference(shape, "cpu")
    xi, dyi, want = X.exact_case(B, H, W, C, N, "int")
    seen = {}
    for wgs in (64, None, 8192):                                        # layer3's problem (host arithmetic only): 120 tiles, 3 x 2 x 4 blocks
        tune(monkeypatch, conv_wgrad_wgs=wgs)
        seen[wgs] = L.mdetr_conv_wgrad_f32_chunks(8, 24, 80, 256, 24, 80, 256, 3, 1)
    assert seen == {64: 2, None: 10, 8192: 120}, seen                   # lowered, the default 256 workgroups, raised up to one tile per chunk
    many = (4, 9, 40, 64, 32)                                           # 24 tiles, 3 blocks: 64 -> 21 chunks (3 of them get two tiles), otherwise 24
    Bm, Hm, Wm, Cm, Nm = many
    xm, dym = X.random_operands(many, "cpu")
    refm, magm = X.random_reference(many, "cpu")
    counts = {}
    for wgs in (64, None, 8192):
        tune(monkeypatch, conv_wgrad_wgs=wgs)
        chunks = L.mdetr_conv_wgrad_f32_chunks(Bm, Hm, Wm, Cm, Hm, Wm, Nm, 3, 1)
        counts[wgs] = chunks
        part = torch.full((chunks, Nm * 9 * Cm), float("nan"))
        assert L.mdetr_conv_wgrad_f32(xm.data_ptr(), dym.data_ptr(), part.data_ptr(), part.numel(), Bm, Hm, Wm, Cm, Hm, Wm, Nm, 3, 1, -1, None) == 0
        assert not bool(part.isnan().any()), "wgs %s: a partial stayed unwritten" % wgs
        dw = torch.zeros(Nm * 9 * Cm)
        for k in range(chunks):                                         # chunk order
            dw += part[k]
        assert_product_close(dw.view(Nm, 3, 3, Cm).permute(0, 3, 1, 2), refm, magm, Bm * Hm * Wm, "chunks %d" % chunks)
    assert counts == {64: 21, None: 24, 8192: 24}, counts
    tune(monkeypatch, conv_wgrad_wgs=64)
    assert_product_close(ext.weight_gradient(x, dy, 3, 1, torch.float32), ref, mag, B * H * W, "through weight_gradient")
    from exact_cases import assert_bits_equal
    assert_bits_equal(ext.weight_gradient(xi, dyi, 3, 1, torch.float32), want, "integers through the chunk sums")


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def test_conv_wgrad_f32_refusals():
    L = native_emul.lib()
    B, H, W, C, N = 1, 4, 5, 64, 32
    x, dy = _nhwc(torch.randn(B, C, H, W)), _nhwc(torch.randn(B, N, H, W))
    part = torch.empty(L.mdetr_conv_wgrad_f32_chunks(B, H, W, C, H, W, N, 3, 1) * N * 9 * C + 4)
    ok = dict(x=x.data_ptr(), dy=dy.data_ptr(), part=part.data_ptr(), floats=part.numel() - 4, B=B, H=H, W=W, C=C, OH=H, OW=W, N=N, k=3, stride=1)

    def call(**kv):
        a = dict(ok, **kv)
        return L.mdetr_conv_wgrad_f32(a["x"], a["dy"], a["part"], a["floats"], a["B"], a["H"], a["W"], a["C"], a["OH"], a["OW"], a["N"], a["k"],
                                      a["stride"], -1, None)

    def chunks(**kv):
        a = dict(ok, **kv)
        return L.mdetr_conv_wgrad_f32_chunks(a["B"], a["H"], a["W"], a["C"], a["OH"], a["OW"], a["N"], a["k"], a["stride"])
    assert call() == 0 and chunks() > 0
    bad = [dict(x=None), dict(dy=None), dict(part=None), dict(C=48), dict(N=40), dict(stride=2, OH=2, OW=3), dict(stride=2), dict(k=1), dict(OH=H - 1),
           dict(OW=W + 1), dict(floats=ok["floats"] - 1), dict(x=ok["x"] + 4), dict(dy=ok["dy"] + 8)]
    for kv in bad:
        assert call(**kv) == MDETR_E_ARG, kv
        assert L.mdetr_last_error().startswith(b"mdetr_conv_wgrad_f32:"), (kv, L.mdetr_last_error())
    for kv in (dict(C=48), dict(N=40), dict(stride=2, OH=2, OW=3), dict(k=1), dict(OH=H - 1), dict(B=0), dict(B=1 << 20, H=64, W=64)):
        assert chunks(**kv) == 0, kv
    assert call(B=1 << 20, H=64, W=64) == MDETR_E_ARG                   # B H W C = 2^38 elements: refused before any pointer is read
    assert call(part=ok["part"] + 16) == 0                              # (the partials need no more than their floats)
