"""csrc/tgemm.hip's fp32 form -- the REAL kernel source, launcher and C-ABI entries `mdetr_tgemm_f32[_masked]` -- on the HIP-on-CPU shim
(tests/native_emul.py): the three-way bf16 split on its way into LDS, the six product terms, the three tile shapes and both pipeline
depths, ragged T / N / K, strided operands, the NN form's 4 x 4 blocks, every part of the epilogue (bias, residual, in-place
accumulation, ReLU, dropout, the masked tail), held element by element to the fp64 product of the same fp32 operands
(tests/gemm_bounds.py: the bound of an fp32-accumulated product, and -- for plain products -- the tighter c = 1 bound that a two-part
split does not meet)."""
import ctypes

import pytest
import torch

import native_emul
from gemm_bounds import assert_product_close, product_bound
from conftest import tune

TILES = ["64x64", "128x64", "128x128"]


def run(a, w, bias=None, res=None, relu=False, nn=False, out=None, p=0.0, seed=0):
    from monodetr_amd import tgemm_ext
    old = tgemm_ext._backend
    tgemm_ext._backend = native_emul.lib()
    try:
        assert tgemm_ext.supported(a, w, nn=nn, res=res, bias=bias, out=out)
        y = tgemm_ext.tgemm(a, w, bias, res, relu=relu, nn=nn, out=out, dropout_p=p, seed=seed)
        assert y.dtype == torch.float32
        return y
    finally:
        tgemm_ext._backend = old


def problem(T, K, N, nn, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(T, K, generator=g) * 0.5
    w = torch.randn(K, N, generator=g) * 0.1 if nn else torch.randn(N, K, generator=g) * 0.1
    b = torch.randn(N, generator=g)
    r = torch.randn(T, N, generator=g)
    return a, w, b, r


def reference(a, w, nn, bias=None, res=None, relu=False):
    wd = w.double() if nn else w.double().t()
    ref = a.double() @ wd
    mag = a.double().abs() @ wd.abs()
    if bias is not None:
        ref = ref + bias.double()
        mag = mag + bias.double().abs()
    if res is not None:
        ref = ref + res.double()
        mag = mag + res.double().abs()
    if relu:
        ref = ref.clamp(min=0)
    return ref, mag


SHAPES = [
    # T, K, N
    (300, 256, 256),        # ragged last token tile
    (64, 64, 64),           # one slab (two of the 32-value slab, four of the 16-value one)
    (1, 8, 8),              # one token, one piece, K below a slab
    (97, 128, 264),         # N = 264: a ragged feature tile with 8 live features
    (130, 1032, 72),        # K = 1032: 17 slabs of 64; here 33 / 65 slabs, the last with 8 live values
    (260, 192, 136),
    (2100, 320, 128),
]


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("pf", ["1", "2"])
@pytest.mark.parametrize("nn", [False, True])
def test_tgemm_f32_plain_products_every_tile_and_pipeline(monkeypatch, tile, pf, nn):
    tune(monkeypatch, tgemm_f32_tile=tile)
    tune(monkeypatch, tgemm_f32_pf=pf)
    for T, K, N in SHAPES[:6]:
        a, w, _, _ = problem(T, K, N, nn, T + K + N)
        y = run(a, w, nn=nn)
        ref, mag = reference(a, w, nn)
        assert_product_close(y, ref, mag, K, "T=%d K=%d N=%d" % (T, K, N))


@pytest.mark.parametrize("nn", [False, True])
@pytest.mark.parametrize("T,K,N", [(64, 8, 8), (97, 128, 264), (1000, 64, 256)])
def test_tgemm_f32_precision_class(T, K, N, nn):
    """Plain products against `product_bound(c = 1)`: sqrt(K) 2^-23 |a||w| + 2^-22 |ref|.  The six-term split sits well inside; a
    two-part (16-bit) split of the operands is 2 - 22 times over it -- this is what tells fp32-accurate from better-than-bf16."""
    a, w, _, _ = problem(T, K, N, nn, 3 * T + K + N)
    y = run(a, w, nn=nn)
    ref, mag = reference(a, w, nn)
    ratio = float(((y.double() - ref).abs() / product_bound(ref, mag, K, torch.float32, c=1.0)).max())
    print("precision class T=%d K=%d N=%d nn=%s: worst error / bound = %.3f" % (T, K, N, nn, ratio))
    assert ratio <= 1.0


@pytest.mark.parametrize("nn", [False, True])
@pytest.mark.parametrize("T,K,N", SHAPES)
def test_tgemm_f32_launcher_default_tiles_with_the_whole_tail(T, K, N, nn):
    a, w, b, r = problem(T, K, N, nn, 7 * T + K + N)
    y = run(a, w, bias=b, res=r, relu=True, nn=nn)
    ref, mag = reference(a, w, nn, b, r, True)
    assert_product_close(y, ref, mag, K, "bias + residual + relu")
    y = run(a, w, bias=b, nn=nn)
    ref, mag = reference(a, w, nn, b)
    assert_product_close(y, ref, mag, K, "bias alone")


@pytest.mark.parametrize("tile", TILES)
def test_tgemm_f32_accumulates_into_its_output_and_respects_row_strides(monkeypatch, tile):
    tune(monkeypatch, tgemm_f32_tile=tile)
    T, K, N = 200, 128, 136
    a, w, b, r = problem(T, K, N, True, 5)
    big_a = torch.zeros(T, K + 12)                                             # row strides: multiples of 4 elements
    big_a[:, :K] = a
    big_w = torch.zeros(K, N + 4)
    big_w[:, :N] = w
    out = torch.full((T, N + 20), 3.0)
    out[:, :N] = r
    view = out[:, :N]
    y = run(big_a[:, :K], big_w[:, :N], res=view, nn=True, out=view)          # y += a w
    assert y.data_ptr() == out.data_ptr()
    ref, mag = reference(a, w, True, None, r)
    assert_product_close(out[:, :N], ref, mag, K, "in-place accumulation")
    assert bool((out[:, N:] == 3.0).all())                                     # nothing written beyond column N
    big_wt = torch.zeros(N, K + 4)                                             # the NT form with padded rows
    big_wt[:, :K] = w.t()
    y = run(big_a[:, :K], big_wt[:, :K], bias=b)
    ref, mag = reference(a, w, True, b)
    assert_product_close(y, ref, mag, K, "strided NT")


@pytest.mark.parametrize("tile", TILES)
def test_tgemm_f32_dropout_makes_the_decisions_of_bias_act(monkeypatch, tile):
    """relu + dropout in the epilogue == mdetr_bias_act_forward(relu, dropout) on the product's fp32 pre-activation: same hash, same
    element index t N + n, same scale."""
    tune(monkeypatch, tgemm_f32_tile=tile)
    T, K, N, p, seed = 150, 64, 72, 0.25, 1234
    a, w, b, _ = problem(T, K, N, False, 11)
    y = run(a, w, bias=b, relu=True, p=p, seed=seed)
    pre = run(a, w, bias=b)
    L = native_emul.lib()
    want = torch.empty(T, N, dtype=torch.float32)
    rc = L.mdetr_bias_act_forward(0, 0, pre.data_ptr(), None, None, want.data_ptr(), T, N, 1, p, seed, None, -1, None)
    assert rc == 0, ctypes.string_at(L.mdetr_last_error())
    assert torch.equal(y, want)
    kept = (y != 0).float().mean().item()
    assert 0.2 < kept < 0.55                                                   # ~ half positive, three quarters of those kept


def test_tgemm_f32_rejects_what_it_cannot_run():
    L = native_emul.lib()
    a = torch.zeros(16, 64)
    w = torch.zeros(8, 64)
    y = torch.zeros(16, 8)
    m = torch.zeros(16, 64)
    args = lambda **kw: [kw.get("a", a.data_ptr()), w.data_ptr(), None, None, y.data_ptr(), kw.get("T", 16), kw.get("N", 8), kw.get("K", 64),
                         kw.get("lda", 64), 64, 0, kw.get("ldy", 8), kw.get("flags", 0), kw.get("p", 0.0), 0, None, -1, None]
    assert L.mdetr_tgemm_f32(*args()) == 0
    assert L.mdetr_tgemm_f32(*args(T=0)) == 0
    assert L.mdetr_tgemm_f32(*args(flags=4 | 8)) == 0                          # BIAS_F32 | OUT_F32: implied
    for bad in (dict(K=60), dict(N=12), dict(lda=62), dict(ldy=10), dict(flags=64), dict(p=0.5), dict(a=a.data_ptr() + 4), dict(T=-1),
                dict(T=1 << 24, lda=64)):                                      # (T lda = 2^30 elements: beyond a buffer resource)
        assert L.mdetr_tgemm_f32(*args(**bad)) < 0, bad
        assert b"mdetr_tgemm_f32" in ctypes.string_at(L.mdetr_last_error())
    # masked: a [16, 8] w [8, 64] -> y [16, 64]
    g = torch.zeros(16, 8)
    w2 = torch.zeros(8, 64)
    y2 = torch.zeros(16, 64)
    margs = lambda **kw: [g.data_ptr(), w2.data_ptr(), None, kw.get("mask", m.data_ptr()), y2.data_ptr(), 16, 64, 8, 8, 64, 0, kw.get("ldm", 64), 64,
                          -1, None]
    assert L.mdetr_tgemm_f32_masked(*margs()) == 0
    for bad in (dict(mask=None), dict(ldm=62), dict(ldm=32), dict(mask=m.data_ptr() + 4)):
        assert L.mdetr_tgemm_f32_masked(*margs(**bad)) < 0, bad
        assert b"mdetr_tgemm_f32_masked" in ctypes.string_at(L.mdetr_last_error())


def test_tgemm_f32_python_wrapper_refuses_mixed_dtypes(monkeypatch):
    from monodetr_amd import tgemm_ext
    monkeypatch.setattr(tgemm_ext, "_backend", native_emul.lib())
    a, w, b, r = problem(64, 64, 64, False, 1)
    assert tgemm_ext.supported(a, w, bias=b, res=r)
    assert not tgemm_ext.supported(a, w.bfloat16())
    assert not tgemm_ext.supported(a.bfloat16(), w)
    assert not tgemm_ext.supported(a, w, bias=b.bfloat16())
    assert not tgemm_ext.supported(a, w, res=r.bfloat16())
    assert not tgemm_ext.supported(a, w, out=r.bfloat16())
    assert not tgemm_ext.masked_supported(r, w, a.bfloat16())
    assert not tgemm_ext.supported(a[:, :60], w[:, :60])


@pytest.mark.parametrize("grid", ["8", "16"])
@pytest.mark.parametrize("pf", ["1", "2"])
@pytest.mark.parametrize("nn", [False, True])
def test_tgemm_f32_persistent_workgroups_walk_several_tiles(monkeypatch, grid, pf, nn):
    """Few workgroups, many tiles each: the slab sequence runs across tile boundaries, dead row tiles are skipped."""
    tune(monkeypatch, tgemm_grid=grid)
    tune(monkeypatch, tgemm_f32_pf=pf)
    tune(monkeypatch, tgemm_f32_tile="64x64")
    for T, K, N in ((700, 192, 136), (1500, 64, 72), (330, 328, 200)):
        a, w, b, r = problem(T, K, N, nn, T + K + N + 1)
        y = run(a, w, bias=b, res=r, relu=True, nn=nn)
        ref, mag = reference(a, w, nn, b, r, True)
        assert_product_close(y, ref, mag, K, "grid=%s T=%d K=%d N=%d" % (grid, T, K, N))
    for tile in ("128x64", "128x128"):
        tune(monkeypatch, tgemm_f32_tile=tile)
        a, w, b, r = problem(2100, 320, 264, nn, 99)
        y = run(a, w, bias=b, nn=nn)
        ref, mag = reference(a, w, nn, b)
        assert_product_close(y, ref, mag, 320, tile + " persistent")


@pytest.mark.parametrize("T,K,N", [(300, 256, 256), (97, 128, 264), (1, 8, 8), (2100, 64, 128), (130, 72, 1032)])
@pytest.mark.parametrize("with_res", [False, True])
def test_tgemm_f32_masked_input_gradient(T, K, N, with_res, monkeypatch):
    """mdetr_tgemm_f32_masked: y = mask <= 0 ? 0 : a w + res (threshold_backward's test: a NaN in the mask lets the gradient pass)."""
    from monodetr_amd import tgemm_ext
    monkeypatch.setattr(tgemm_ext, "_backend", native_emul.lib())
    a, w, _, r = problem(T, K, N, True, T + K + N)
    g = torch.Generator().manual_seed(7)
    mask = torch.randn(T, N, generator=g).clamp(min=0)
    mask[0, 0] = float("nan") if T * N > 1 else mask[0, 0]
    res = r if with_res else None
    assert tgemm_ext.masked_supported(a, w, mask, res)
    y = tgemm_ext.tgemm_masked(a, w, mask, res)
    assert y.dtype == torch.float32
    ref, mag = reference(a, w, True, None, res)
    keep = ~(mask.double() <= 0)
    assert bool(keep[0, 0])
    assert bool((y[~keep] == 0).all())
    assert_product_close(torch.where(keep, y.double(), torch.zeros_like(ref)).to(y.dtype), torch.where(keep, ref, torch.zeros_like(ref)), mag, K)
    want = torch.ops.aten.threshold_backward(run(a, w, res=res, nn=True), mask, 0.0)      # the unmasked product, then autograd's own mask
    assert torch.equal(torch.nan_to_num(y), torch.nan_to_num(want))
    for tile in TILES:
        tune(monkeypatch, tgemm_f32_tile=tile)
        for pf in ("1", "2"):
            tune(monkeypatch, tgemm_f32_pf=pf)
            assert torch.equal(tgemm_ext.tgemm_masked(a, w, mask, res), y)
