"""The fp32 form of csrc/twgrad.hip (mdetr_token_wgrad_f32; family MDETR_TWGRAD_F32) on the GPU: element-wise against fp64 within the
fp32-accumulation bound (tests/gemm_bounds.py) and deterministic, bit for bit on the exact cases of tests/twgrad_f32_cases.py for every
tile shape, in the library's precision class, and through the modules of a ResNet stage with both fp32 switches on."""
import pytest
import torch

import twgrad_f32_cases as X
from conftest import tune
from exact_cases import assert_bits_equal
from gemm_bounds import assert_product_close, product_bound

pytestmark = pytest.mark.gpu

# launch geometry the small shapes cannot reach: chunks in whole eights per XCD, slabs >= 256, more tiles than one
BIG_SHAPES = [(8264, 256, 256), (81600, 256, 256), (61440, 128, 512)]


@pytest.fixture
def ext(monkeypatch):
    from monodetr_amd import conv_wgrad_ext
    monkeypatch.setattr(conv_wgrad_ext, "ENABLED_F32", True)
    return conv_wgrad_ext


def _dev():
    return torch.device("cuda", 0)


@pytest.mark.parametrize("T,C,N", X.SHAPES + BIG_SHAPES)
def test_twgrad_f32_element_wise_against_fp64_and_deterministic(monkeypatch, ext, T, C, N):
    tune(monkeypatch, twgrad_f32_tile=None, twgrad_wgs=None)
    dev = _dev()
    g = torch.Generator(device="cuda").manual_seed(T + C + N)
    x = torch.randn(T, C, device=dev, generator=g) * 0.5
    dy = torch.randn(T, N, device=dev, generator=g) * 0.2
    assert ext.token_supported_f32(x, dy)
    dw, db = ext.token_weight_gradient(x, dy, torch.float32, bias=True)
    dw, db = dw.clone(), db.clone()                                    # (the partials live in a shared workspace; the sums are new tensors)
    x64, dy64 = x.double(), dy.double()
    assert_product_close(dw, dy64.t() @ x64, dy64.abs().t() @ x64.abs(), T, "T=%d C=%d N=%d dW" % (T, C, N))
    assert_product_close(db, dy64.sum(0), dy64.abs().sum(0), T, "T=%d C=%d N=%d db" % (T, C, N))
    dw2, db2 = ext.token_weight_gradient(x, dy, torch.float32, bias=True)
    assert torch.equal(dw2, dw) and torch.equal(db2, db)               # no atomics: the same bits on a second call
    dw3, none = ext.token_weight_gradient(x, dy, torch.float32, bias=False)
    assert none is None and torch.equal(dw3, dw)


@pytest.mark.parametrize("tile", X.TILES)
@pytest.mark.parametrize("T,C,N", X.EXACT_SHAPES)
def test_twgrad_f32_exact_cases_for_every_tile(monkeypatch, ext, T, C, N, tile):
    tune(monkeypatch, twgrad_f32_tile=tile)
    dev = _dev()
    for kind in X.KINDS:
        x, dy, want, want_db, rb, mb = X.exact_case(T, C, N, kind)
        what = "twgrad f32 %s T=%d C=%d N=%d tile %s" % (kind, T, C, N, tile)
        dw, db = ext.token_weight_gradient(x.to(dev), dy.to(dev), torch.float32, bias=True)
        assert_bits_equal(dw, want, what + " dW")
        if want_db is not None:
            assert_bits_equal(db, want_db, what + " db")
        else:
            assert_product_close(db.cpu(), rb, mb, T, what + " db")
    what = "twgrad f32 T=%d C=%d N=%d tile %s" % (T, C, N, tile)
    x, dy, want_db = X.db_single_case(T, C, N)
    _, db = ext.token_weight_gradient(x.to(dev), dy.to(dev), torch.float32, bias=True)
    assert_bits_equal(db, want_db, what + " db of one full-mantissa value per column")
    x, dy, want, want_db = X.integer_case(T, C, N)
    dw, db = ext.token_weight_gradient(x.to(dev), dy.to(dev), torch.float32, bias=True)
    assert_bits_equal(dw, want, what + " integer dW")
    assert_bits_equal(db, want_db, what + " integer db")


def test_twgrad_f32_precision_class_relative_to_the_library(ext):
    """The rule of test_tgemm_f32_precision_class_relative_to_the_library: against product_bound(c = 1, K = T) the worst error / bound
    ratio of the kernel may be at most max(1, 2 x the ratio of torch.mm(dy^T, x) on the same fp32 operands)."""
    dev = _dev()
    for T, C, N in ((64, 8, 8), (97, 64, 256), (128, 264, 72)):
        g = torch.Generator(device="cuda").manual_seed(3 * T + C + N)
        x = torch.randn(T, C, device=dev, generator=g) * 0.5
        dy = torch.randn(T, N, device=dev, generator=g) * 0.2
        ref, mag = dy.double().t() @ x.double(), dy.double().abs().t() @ x.double().abs()
        bound = product_bound(ref, mag, T, torch.float32, c=1.0)
        dw, _ = ext.token_weight_gradient(x, dy, torch.float32, bias=True)
        mine = float(((dw.double() - ref).abs() / bound).max())
        lib = float(((torch.mm(dy.t(), x).double() - ref).abs() / bound).max())
        print("precision class T=%d C=%d N=%d: kernel %.3f library %.3f of the c = 1 bound" % (T, C, N, mine, lib))
        assert mine <= max(1.0, 2.0 * lib), (T, C, N, mine, lib)


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def test_fp32_stage_with_both_switches_against_fp64(monkeypatch):
    """The ResNet stage of test_tgemm_f32_gpu.py's bottleneck-stage test (layer2's shape, fp32, forward and backward) with MDETR_TGEMM_F32
    + MDETR_TWGRAD_F32 on against both off, each against the stage in fp64 on the same parameters.  That test's bars: per tensor the
    switched route's error may be at most twice the library route's, with floors of 2^-22 for the output (fp32's own rounding) and
    1e-3 -- the project's fp32 parity bar -- for the gradients (ReLU masks within rounding of zero flip by chance on either route).
    The five 1x1 weights (conv1 and conv3 of both blocks, the projection shortcut) must take the kernel entry."""
    import copy
    from monodetr_amd import conv_wgrad_ext
    from monodetr_amd.monodetr import backbone, linear
    dev = _dev()
    torch.manual_seed(2)
    down = torch.nn.Sequential(torch.nn.Conv2d(256, 512, 1, 1, bias=False), backbone.FrozenBatchNorm2d(512))
    stage = torch.nn.Sequential(backbone.Bottleneck(256, 128, 1, down), backbone.Bottleneck(512, 128)).to(dev).to(memory_format=torch.channels_last)
    for m in stage.modules():
        if isinstance(m, backbone.FrozenBatchNorm2d):
            m.weight.uniform_(0.5, 1.5); m.bias.normal_(0, 0.2); m.running_mean.normal_(0, 0.2); m.running_var.uniform_(0.5, 1.5)
    x = (torch.randn(4, 256, 48, 160, device=dev) * 0.5).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    proj = torch.linspace(-1, 1, 4 * 512 * 48 * 160, device=dev).view(4, 48, 160, 512).permute(0, 3, 1, 2)
    calls = []
    real = conv_wgrad_ext.token_weight_gradient
    monkeypatch.setattr(conv_wgrad_ext, "token_weight_gradient", lambda *a, **k: (calls.append((a[0].dtype, tuple(a[0].shape), a[1].shape[1])), real(*a, **k))[1])
    res = {}
    for on in (False, True):
        monkeypatch.setattr(linear, "_TGEMM_F32", on)
        monkeypatch.setattr(conv_wgrad_ext, "ENABLED_F32", on)
        calls.clear()
        stage.zero_grad(set_to_none=True)
        x.grad = None
        y = stage(x)
        (y * proj).sum().backward()
        res[on] = (y.detach().clone(), x.grad.clone(), {n: p.grad.clone() for n, p in stage.named_parameters() if p.grad is not None})
        if on:
            assert len(calls) == 5 and all(c[0] == torch.float32 and c[1][0] == 4 * 48 * 160 for c in calls), calls
            assert sorted((c[1][1], c[2]) for c in calls) == [(128, 512), (128, 512), (256, 128), (256, 512), (512, 128)], calls
        else:
            assert calls == [], calls
    monkeypatch.setattr(linear, "_TGEMM_F32", False)
    monkeypatch.setattr(conv_wgrad_ext, "ENABLED_F32", False)
    ref = copy.deepcopy(stage).double()
    x64 = x.detach().double().requires_grad_(True)
    y64 = ref(x64)
    (y64 * proj.double()).sum().backward()
    want = (y64.detach(), x64.grad, {n: p.grad for n, p in ref.named_parameters() if p.grad is not None})
    for name, got_on, got_off, w64 in [("output", res[True][0], res[False][0], want[0]), ("input gradient", res[True][1], res[False][1], want[1])] + \
            [(n, res[True][2][n], res[False][2][n], g) for n, g in want[2].items()]:
        e_on, e_off = _rel(got_on, w64), _rel(got_off, w64)
        print("stage %-28s relative error: both switches on %.3e, off %.3e" % (name, e_on, e_off))
        assert e_on <= max(2.0 * e_off, 2.0 ** -22 if name == "output" else 1e-3), (name, e_on, e_off)
