"""csrc/tgemm.hip's fp32 form on the GPU (mdetr_tgemm_f32 / mdetr_tgemm_f32_masked: fp32 operands through a three-way bf16 split on the
matrix cores): every token-wise product shape of the training iteration held ELEMENT BY ELEMENT to the fp64 product of the same fp32
operands (tests/gemm_bounds.py: the bound of an fp32-accumulated product), determinism, each tile shape and pipeline depth on three
awkward shapes, the precision class relative to the library's fp32 GEMM, dropout against bias_act, the masked tail, and fp32 modules
with MDETR_TGEMM_F32 on against the same modules with it off."""
import pytest
import torch

from gemm_bounds import assert_product_close, product_bound
from conftest import tune
from test_tgemm_gpu import STEP_SHAPES

pytestmark = pytest.mark.gpu


def _operands(T, K, N, nn, seed, dev):
    g = torch.Generator(device="cpu").manual_seed(seed)
    a = (torch.randn(T, K, generator=g) * 0.5).to(dev)
    w = ((torch.randn(K, N, generator=g) if nn else torch.randn(N, K, generator=g)) * 0.1).to(dev)
    b = torch.randn(N, generator=g).to(dev)
    r = torch.randn(T, N, generator=g).to(dev)
    return a, w, b, r


def _reference(a, w, nn, bias, res, relu):
    wd = w.double() if nn else w.double().t()
    ref = a.double() @ wd
    mag = a.double().abs() @ wd.abs()
    if bias is not None:
        ref += bias.double()
        mag += bias.double().abs()
    if res is not None:
        ref += res.double()
        mag += res.double().abs()
    return (ref.clamp_(min=0) if relu else ref), mag


@pytest.mark.parametrize("T,K,N,nn,tail", STEP_SHAPES)
def test_tgemm_f32_step_shapes_element_wise_against_fp64(T, K, N, nn, tail):
    from monodetr_amd import tgemm_ext
    dev = torch.device("cuda", 0)
    a, w, b, r = _operands(T, K, N, nn, T + 3 * K + N, dev)
    bias = b if "bias" in tail else None
    res = r.clone() if tail in ("res_relu", "accum") else None
    relu = "relu" in tail
    assert tgemm_ext.supported(a, w, nn=nn, res=res, bias=bias)
    out = res if tail == "accum" else None
    keep = res.clone() if res is not None else None
    y = tgemm_ext.tgemm(a, w, bias, res, relu=relu, nn=nn, out=out)
    torch.cuda.synchronize()
    assert y.dtype == torch.float32
    ref, mag = _reference(a, w, nn, bias, keep, relu)
    assert_product_close(y, ref, mag, K, "T=%d K=%d N=%d nn=%s %s" % (T, K, N, nn, tail))
    y2 = tgemm_ext.tgemm(a, w, bias, keep, relu=relu, nn=nn)        # (out of place, also where y was accumulated into its residual)
    assert torch.equal(y, y2)                                        # deterministic


@pytest.mark.parametrize("tile", ["64x64", "128x64", "128x128"])
@pytest.mark.parametrize("pf", ["1", "2"])
@pytest.mark.parametrize("nn", [False, True])
def test_tgemm_f32_every_tile_shape_and_pipeline_depth(monkeypatch, tile, pf, nn):
    from monodetr_amd import tgemm_ext
    tune(monkeypatch, tgemm_f32_tile=tile)
    tune(monkeypatch, tgemm_f32_pf=pf)
    dev = torch.device("cuda", 0)
    for T, K, N in ((4133, 456, 264), (300, 64, 72), (9000, 1032, 136)):
        a, w, b, r = _operands(T, K, N, nn, T + K, dev)
        y = tgemm_ext.tgemm(a, w, b, r, relu=True, nn=nn)
        ref, mag = _reference(a, w, nn, b, r, True)
        assert_product_close(y, ref, mag, K, "%s pf%s nn=%s T=%d" % (tile, pf, nn, T))
        y = tgemm_ext.tgemm(a, w, None, None, nn=nn)
        ref, mag = _reference(a, w, nn, None, None, False)
        assert_product_close(y, ref, mag, K, "plain")


def test_tgemm_f32_precision_class_relative_to_the_library():
    """Plain products, K <= 128, against product_bound(c = 1) = sqrt(K) 2^-23 |a||w| + 2^-22 |ref|: the worst error / bound ratio of the
    kernel may be at most max(1, 2 x the ratio of torch.mm on the same fp32 operands) -- the split drops terms of <= 2^-23 per product,
    one more rounding-sized error beside the accumulation's; a two-part (16-bit) split is 2 - 22 x over the bound."""
    from monodetr_amd import tgemm_ext
    dev = torch.device("cuda", 0)
    for T, K, N in ((64, 8, 8), (97, 128, 264), (1000, 64, 256)):
        for nn in (False, True):
            a, w, _, _ = _operands(T, K, N, nn, 3 * T + K + N, dev)
            ref, mag = _reference(a, w, nn, None, None, False)
            bound = product_bound(ref, mag, K, torch.float32, c=1.0)
            mine = float(((tgemm_ext.tgemm(a, w, nn=nn).double() - ref).abs() / bound).max())
            lib = float(((torch.mm(a, w if nn else w.t()).double() - ref).abs() / bound).max())
            print("precision class T=%d K=%d N=%d nn=%s: kernel %.3f library %.3f of the c = 1 bound" % (T, K, N, nn, mine, lib))
            assert mine <= max(1.0, 2.0 * lib), (T, K, N, nn, mine, lib)


def test_tgemm_f32_dropout_tail_is_the_bias_act_decision():
    from monodetr_amd import bias_act_ext, tgemm_ext
    dev = torch.device("cuda", 0)
    T, K, N = 81600, 256, 256
    a, w, b, _ = _operands(T, K, N, False, 9, dev)
    y = tgemm_ext.tgemm(a, w, b, None, relu=True, dropout_p=0.1, seed=77)
    pre = tgemm_ext.tgemm(a, w, b, None)
    want = bias_act_ext.bias_act(pre, None, None, relu=True, dropout_p=0.1, seed=77)
    assert torch.equal(y, want)
    frac = (y == 0).float().mean().item()
    assert 0.5 < frac < 0.6                                          # half negative + a tenth of the rest dropped


@pytest.mark.parametrize("T,K,N,with_res", [(61440, 128, 512, True), (15360, 256, 1024, True), (3840, 512, 2048, True),
                                            (61440, 512, 128, False), (15360, 1024, 256, False), (4403, 72, 264, True)])
def test_tgemm_f32_masked_input_gradient_equals_the_product_followed_by_threshold_backward(T, K, N, with_res):
    from monodetr_amd import tgemm_ext
    g = torch.Generator(device="cuda").manual_seed(T + K + N)
    dy = torch.randn(T, K, device="cuda", generator=g)
    w = torch.randn(K, N, device="cuda", generator=g) * 0.05
    x = torch.randn(T, N, device="cuda", generator=g).clamp(min=0)                            # a ReLU output
    x[0, 0] = float("nan")                                                                      # (NaN <= 0 is false: the gradient passes)
    r = torch.randn(T, N, device="cuda", generator=g) if with_res else None
    assert tgemm_ext.masked_supported(dy, w, x, r)
    want = torch.ops.aten.threshold_backward(tgemm_ext.tgemm(dy, w, None, r, nn=True), x, 0.0)
    got = tgemm_ext.tgemm_masked(dy, w, x, r)
    assert torch.equal(got, want)                                        # the same fp32 sum, then the same zeros
    ref = dy.double() @ w.double() + (r.double() if with_res else 0.0)
    mag = dy.double().abs() @ w.double().abs() + (r.double().abs() if with_res else 0.0)
    keep = ~(x <= 0)
    assert bool(keep[0, 0])
    assert_product_close(got, torch.where(keep, ref, torch.zeros_like(ref)), mag, K)


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def test_fp32_modules_with_the_switch_bottleneck_stage_against_fp64(monkeypatch):
    """A ResNet stage at layer2's shape in fp32, forward and backward, with MDETR_TGEMM_F32 on and off, both against the stage in fp64
    on the same parameters.  Both routes are fp32-accumulated products (the same element-wise bound holds for either), so the
    switched route's error per tensor may be at most twice the library route's (the factor of the precision-class bar: the split adds
    one rounding-sized error per product beside the accumulation's).  Floors: 2^-22 relative for the output (fp32's own rounding; the
    forward is continuous); 1e-3 -- the project's fp32 parity bar -- for the gradients, whose ReLU masks are discontinuous: among the
    ~5e7 pre-activations of the stage a few lie within rounding of zero, each flipped mask element moves a gradient tensor by
    ~1 / sqrt(its elements) ~ 3e-4 relative, and WHICH route meets one is chance, so below that level the ratio says nothing."""
    import copy
    from monodetr_amd import tgemm_ext
    from monodetr_amd.monodetr import backbone, linear
    dev = torch.device("cuda", 0)
    torch.manual_seed(2)
    down = torch.nn.Sequential(torch.nn.Conv2d(256, 512, 1, 1, bias=False), backbone.FrozenBatchNorm2d(512))
    stage = torch.nn.Sequential(backbone.Bottleneck(256, 128, 1, down), backbone.Bottleneck(512, 128)).to(dev).to(memory_format=torch.channels_last)
    for m in stage.modules():
        if isinstance(m, backbone.FrozenBatchNorm2d):
            m.weight.uniform_(0.5, 1.5); m.bias.normal_(0, 0.2); m.running_mean.normal_(0, 0.2); m.running_var.uniform_(0.5, 1.5)
    x = (torch.randn(4, 256, 48, 160, device=dev) * 0.5).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    proj = torch.linspace(-1, 1, 4 * 512 * 48 * 160, device=dev).view(4, 48, 160, 512).permute(0, 3, 1, 2)
    calls = []
    real = tgemm_ext.tgemm
    monkeypatch.setattr(tgemm_ext, "tgemm", lambda *a, **k: (calls.append(a[0].dtype), real(*a, **k))[1])
    res = {}
    for on in (False, True):
        monkeypatch.setattr(linear, "_TGEMM_F32", on)
        calls.clear()
        stage.zero_grad(set_to_none=True)
        x.grad = None
        y = stage(x)
        (y * proj).sum().backward()
        res[on] = (y.detach().clone(), x.grad.clone(), {n: p.grad.clone() for n, p in stage.named_parameters() if p.grad is not None})
        # 5 token products forward (conv1 and conv3 of both blocks, the projection shortcut) and their 5 input gradients
        assert (len(calls) >= 10 and all(d == torch.float32 for d in calls)) if on else calls == [], calls
    monkeypatch.setattr(linear, "_TGEMM_F32", False)
    ref = copy.deepcopy(stage).double()
    x64 = x.detach().double().requires_grad_(True)
    y64 = ref(x64)
    (y64 * proj.double()).sum().backward()
    want = (y64.detach(), x64.grad, {n: p.grad for n, p in ref.named_parameters() if p.grad is not None})
    for name, got_on, got_off, w64 in [("output", res[True][0], res[False][0], want[0]), ("input gradient", res[True][1], res[False][1], want[1])] + \
            [(n, res[True][2][n], res[False][2][n], g) for n, g in want[2].items()]:
        e_on, e_off = _rel(got_on, w64), _rel(got_off, w64)
        print("stage %-28s relative error: switch on %.3e, off %.3e" % (name, e_on, e_off))
        assert e_on <= max(2.0 * e_off, 2.0 ** -22 if name == "output" else 1e-3), (name, e_on, e_off)


def test_fp32_modules_with_the_switch_encoder_layer_matches_the_library_route(monkeypatch):
    """One visual encoder layer (deformable self-attention + FFN, dropout off) at the encoder's level shapes, B = 2, in fp32 with the
    switch on against the same layer with it off.  Every product of either route carries a relative error of ~sqrt(K) 2^-24 x
    (|a||w| / |a w| ~ sqrt(K)) <= 1024 x 2^-24 = 6e-5 at the widest contraction here (K = 1024, worst case; typical: a tenth of it);
    the layer chains four products and two LayerNorms, so the two routes' OUTPUTS may differ by 1e-4 in relative L2 norm -- bf16-class
    products would show as 1e-3 ... 1e-2.  (Measured: 7.7e-7.)
    Gradients are NOT continuous in the forward values, so rounding-level differences between two correct routes show far above
    rounding level, by two mechanisms that set the bars below (each route's own products are held to fp64 by the tests above):
      * ReLU masks.  A hidden pre-activation within the routes' difference of zero flips its mask in one route; one flip moves the
        gradient of linear1's weight / bias (sums over T / 2 random-signed terms per element) by 1 / sqrt(1024 T / 2) = 3.1e-4 of its
        norm at T = 20 400.  About 30 of the 2.1e7 pre-activations lie within 1e-6 of zero and the routes differ by a few 1e-7 there:
        ~10 flips expected; the bar allows 100 (the estimate is good to a small factor): 3.1e-3 for linear1's parameters.
      * Sampling cells.  d out / d location jumps where a sampling point crosses a pixel boundary; locations of the two routes differ
        by ~1e-5 pixel, so ~2e-5 of the 2.6e6 samples (~50) change cell, each moving one of the T terms of a row of the
        sampling-offset projection's weight gradient by its own size: sqrt(50) 16 / (256 sqrt(T)) ~ 3e-3 of the norm; bar 1e-2.
      * Everything else (fed by both, diluted): 1e-3, the project's fp32 parity bar."""
    from monodetr_amd import tgemm_ext
    from monodetr_amd.monodetr import linear
    from monodetr_amd.monodetr.depthaware_transformer import VisualEncoder, VisualEncoderLayer
    dev = torch.device("cuda", 0)
    torch.manual_seed(3)
    enc = VisualEncoder(VisualEncoderLayer(256, 1024, 0.0), 1).to(dev)
    with torch.no_grad():
        enc.layers[0].self_attn.sampling_offsets.weight.normal_(0, 0.02)
        enc.layers[0].self_attn.attention_weights.weight.normal_(0, 0.2)
    shapes = torch.tensor([(48, 160), (24, 80), (12, 40), (6, 20)], dtype=torch.int64, device=dev)
    start = torch.cat((shapes.new_zeros(1), shapes.prod(1).cumsum(0)[:-1]))
    S = int(shapes.prod(1).sum())
    src = torch.randn(2, S, 256, device=dev, requires_grad=True)
    pos = torch.randn(2, S, 256, device=dev)
    proj = torch.randn(2, S, 256, device=dev)
    calls = []
    real = tgemm_ext.tgemm
    monkeypatch.setattr(tgemm_ext, "tgemm", lambda *a, **k: (calls.append(a[0].dtype), real(*a, **k))[1])
    res = {}
    for on in (False, True):
        monkeypatch.setattr(linear, "_TGEMM_F32", on)
        calls.clear()
        enc.zero_grad(set_to_none=True)
        src.grad = None
        out = enc(src, shapes, start, None, pos=pos)
        (out * proj).sum().backward()
        res[on] = (out.detach().clone(), src.grad.clone(), {n: p.grad.clone() for n, p in enc.named_parameters() if p.grad is not None})
        assert (len(calls) >= 8 and all(d == torch.float32 for d in calls)) if on else calls == [], calls
    for name, a, b in [("output", res[True][0], res[False][0]), ("input gradient", res[True][1], res[False][1])] + \
            [(n, res[True][2][n], g) for n, g in res[False][2].items()]:
        e = _rel(a, b)
        print("encoder layer %-40s switch on vs off: %.3e" % (name, e))
        bar = 1e-4 if name == "output" else 1e-2 if "sampling_offsets" in name else 3.1e-3 if "linear1" in name else 1e-3
        assert e <= bar, (name, e, bar)
