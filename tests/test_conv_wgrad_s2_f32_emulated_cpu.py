"""The stride-2 fp32 form of csrc/conv_wgrad.hip -- the REAL kernel source, launcher and C-ABI entry (mdetr_conv_wgrad_s2_f32) -- on the
HIP-on-CPU shim (tests/native_emul.py) through conv_wgrad_ext.weight_gradient with the family MDETR_CONV_WGRAD_S2_F32 on, its partials added
by the emulated mdetr_chunk_sums: the exact and random cases of tests/conv_wgrad_s2_f32_cases.py on the first three shapes, the chunking as
a partition of the pixel tiles, and the entry's refusals.  (The shim is slow: the fourth shape and the large ones run on the GPU only.)"""
import pytest
import torch

import conv_wgrad_s2_f32_cases as X
import native_emul
from conftest import tune
from exact_cases import assert_bits_equal
from gemm_bounds import assert_product_close

SHAPES = X.SHAPES[:3]
MDETR_E_ARG = -1


@pytest.fixture()
def ext(monkeypatch):
    from monodetr_amd import chunk_sums, conv_wgrad_ext
    L = native_emul.lib()
    L.mdetr_conv_wgrad_s2_f32                                           # (AttributeError without the feature)
    monkeypatch.setattr(conv_wgrad_ext, "_backend", L)
    monkeypatch.setattr(conv_wgrad_ext, "ENABLED_CONV_S2_F32", True)
    X.lift_shape_rule(conv_wgrad_ext, monkeypatch)                     # the kernel is under test here, on every shape the entry takes
    monkeypatch.setattr(chunk_sums, "_backend", L)                      # the partials go through the chunk-sum kernel, as in the step
    monkeypatch.setattr(chunk_sums, "ENABLED", True)
    tune(monkeypatch, conv_wgrad_wgs=None)
    return conv_wgrad_ext


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv_wgrad_s2_f32_exact_and_random_cases(ext, shape):
    wgrad = X.direct(ext)
    X.check_exact(wgrad, "cpu", shape)
    X.check_small_integers(wgrad, "cpu", shape)
    X.check_random(wgrad, "cpu", shape, twice=True)


def _chunks(L, shape):
    B, H, W, C, N = shape
    OH, OW = X.out_hw(H, W)
    return L.mdetr_conv_wgrad_s2_f32_chunks(B, H, W, C, OH, OW, N, 3, 2)


def test_conv_wgrad_s2_f32_chunking_is_a_partition(ext, monkeypatch):
    """conv_wgrad_wgs moves the chunk count; every partial of every chunk is written (the buffer starts as NaN); the chunks added in
    order are within the bound of fp64, and the integer case is exact at every chunk count."""
    L = native_emul.lib()
    seen = {}
    for wgs in (64, None, 8192):                                        # layer3.0.conv2's problem (host arithmetic only): 8 x 3 x 10 tiles, 3 x 4 x 4 blocks
        tune(monkeypatch, conv_wgrad_wgs=wgs)
        seen[wgs] = _chunks(L, (8, 48, 160, 256, 256))
    assert seen == {64: 1, None: 10, 8192: 170}, seen                   # lowered, the default 512 workgroups, raised
    assert all(seen[w] == X.expected_chunks((8, 48, 160, 256, 256), w) for w in seen)
    many = (4, 18, 37, 64, 32)                                          # 9 x 19 outputs: 4 x 2 x 3 = 24 tiles, 3 workgroups per chunk
    B, H, W, C, N = many
    OH, OW = X.out_hw(H, W)
    assert X.tiles(many) == 24
    x, dy = X.random_operands(many, "cpu")
    ref, mag = X.random_reference(many, "cpu")
    xi, dyi, want = X.exact_case(B, H, W, C, N, "int")
    counts = {}
    for wgs in (64, None, 8192):
        tune(monkeypatch, conv_wgrad_wgs=wgs)
        chunks = _chunks(L, many)
        counts[wgs] = chunks
        for a, b, exact in ((x, dy, False), (xi, dyi, True)):
            part = torch.full((chunks, N * 9 * C), float("nan"))
            assert L.mdetr_conv_wgrad_s2_f32(a.data_ptr(), b.data_ptr(), part.data_ptr(), part.numel(), B, H, W, C, OH, OW, N, 3, 2, -1, None) == 0
            assert not bool(part.isnan().any()), "wgs %s: a partial stayed unwritten" % wgs
            dw = torch.zeros(N * 9 * C)
            for k in range(chunks):                                     # chunk order
                dw += part[k]
            dw = dw.view(N, 3, 3, C).permute(0, 3, 1, 2)
            if exact:
                assert_bits_equal(dw, want, "integers on %d chunks" % chunks)
            else:
                assert_product_close(dw, ref, mag, B * OH * OW, "chunks %d" % chunks)
        assert_bits_equal(ext.weight_gradient(xi, dyi, 3, 2, torch.float32), want, "integers through the chunk sums, wgs %s" % wgs)
    assert counts == {64: 21, None: 24, 8192: 24}, counts               # 21 chunks: three of them get two tiles
    assert all(counts[w] == X.expected_chunks(many, w) for w in counts)
    tune(monkeypatch, conv_wgrad_wgs=64)
    assert_product_close(ext.weight_gradient(x, dy, 3, 2, torch.float32), ref, mag, B * OH * OW, "through weight_gradient")


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def test_conv_wgrad_s2_f32_refusals():
    L = native_emul.lib()
    B, H, W, C, N = 1, 6, 9, 64, 32
    OH, OW = X.out_hw(H, W)
    x, dy = _nhwc(torch.randn(B, C, H, W)), _nhwc(torch.randn(B, N, OH, OW))
    part = torch.empty(L.mdetr_conv_wgrad_s2_f32_chunks(B, H, W, C, OH, OW, N, 3, 2) * N * 9 * C + 4)
    ok = dict(x=x.data_ptr(), dy=dy.data_ptr(), part=part.data_ptr(), floats=part.numel() - 4, B=B, H=H, W=W, C=C, OH=OH, OW=OW, N=N, k=3, stride=2)

    def call(**kv):
        a = dict(ok, **kv)
        return L.mdetr_conv_wgrad_s2_f32(a["x"], a["dy"], a["part"], a["floats"], a["B"], a["H"], a["W"], a["C"], a["OH"], a["OW"], a["N"], a["k"],
                                         a["stride"], -1, None)

    def chunks(**kv):
        a = dict(ok, **kv)
        return L.mdetr_conv_wgrad_s2_f32_chunks(a["B"], a["H"], a["W"], a["C"], a["OH"], a["OW"], a["N"], a["k"], a["stride"])
    assert call() == 0 and chunks() > 0
    big = dict(B=1 << 20, H=63, W=63, OH=32, OW=32)                     # B H W C = 2^38 elements; the output map belongs to the input
    tall = dict(B=1 << 20, H=1, W=1, OH=1, OW=1, N=512)                # B OH OW N = 2^29 elements of dy against 2^26 of x
    wide = dict(C=1 << 14, N=1 << 11)                                   # 9 N C = 9 x 2^25 >= 2^28, both operands far below 2^29 elements
    bad = [dict(x=None), dict(dy=None), dict(part=None), dict(k=1), dict(k=1, OH=3, OW=5), dict(stride=1), dict(stride=1, OH=H, OW=W), dict(OH=OH - 1),
           dict(OW=OW + 1), dict(OH=H, OW=W), dict(C=48), dict(N=40), dict(x=ok["x"] + 4), dict(dy=ok["dy"] + 8), dict(floats=ok["floats"] - 1),
           dict(B=0), dict(H=0, OH=0), dict(OW=0), big, dict(big, x=None, dy=None, part=None), tall, wide]
    for kv in bad:
        assert call(**kv) == MDETR_E_ARG, kv
        assert L.mdetr_last_error().startswith(b"mdetr_conv_wgrad_s2_f32:"), (kv, L.mdetr_last_error())
    assert call(**dict(big, x=1 << 40, dy=1 << 40)) == MDETR_E_ARG      # (refused on its sizes: pointers that lead nowhere are never read)
    for kv in (dict(k=1), dict(stride=1), dict(stride=1, OH=H, OW=W), dict(OH=OH - 1), dict(OW=OW + 1), dict(C=48), dict(N=40), dict(B=0), dict(OW=0),
               big, wide):
        assert chunks(**kv) == 0, kv
    assert call(part=ok["part"] + 16) == 0                              # (the partials need no more than their floats)
