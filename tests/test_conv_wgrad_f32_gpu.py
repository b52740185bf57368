"""The fp32 form of csrc/conv_wgrad.hip (mdetr_conv_wgrad_f32; family MDETR_CONV_WGRAD_F32) on the GPU, reached the way the step reaches
it -- the backward pass of conv3x3_ext.conv3x3 with MDETR_CONV3X3_F32 on: the exact cases of tests/conv_wgrad_f32_cases.py bit for bit
and the random case element-wise against fp64 within the fp32-accumulation bound (tests/gemm_bounds.py) on every shape; every chunk
count; launch geometries only large shapes reach, deterministic; the library's precision class; and an fp32 ResNet stage with the four
fp32 switches on."""
import pytest
import torch

import conv_wgrad_f32_cases as X
from conftest import tune
from gemm_bounds import product_bound

pytestmark = pytest.mark.gpu

# launch geometry the small shapes cannot reach: layer3 (24 blocks x 10 chunks of 12 tiles), layer4 (96 blocks, 2 chunks of 24 tiles),
# layer1's width with thousands of tiles on 85 chunks
BIG_SHAPES = [(8, 24, 80, 256, 256), (8, 12, 40, 512, 512), (2, 96, 320, 64, 64)]


@pytest.fixture
def route(monkeypatch):
    """-> (wgrad, calls): the weight gradient through conv3x3's backward pass, its route recorded and asserted per call."""
    from monodetr_amd import conv3x3_ext, conv_wgrad_ext
    monkeypatch.setattr(conv3x3_ext, "ENABLED_F32", True)
    monkeypatch.setattr(conv_wgrad_ext, "ENABLED_CONV_F32", True)
    X.lift_shape_rule(conv_wgrad_ext, monkeypatch)                     # the kernel is under test here, on every shape the entry takes
    tune(monkeypatch, conv_wgrad_wgs=None, conv3x3_f32_tile=None, conv3x3_f32_nb=None)
    calls = X.record_routes(conv_wgrad_ext, monkeypatch)
    return X.through_conv3x3(conv3x3_ext, calls), calls


def _dev():
    return torch.device("cuda", 0)


def _chunks(shape):
    from monodetr_amd import _capi
    B, H, W, C, N = shape
    return _capi.lib().mdetr_conv_wgrad_f32_chunks(B, H, W, C, H, W, N, 3, 1)


CASES = [(s, None) for s in X.SHAPES] + [(X.WRAP_SHAPE, X.WRAP_WGS)]


@pytest.mark.parametrize("shape,wgs", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else "wgs%s" % v)
def test_conv_wgrad_f32_exact_and_random_cases(route, monkeypatch, shape, wgs):
    wgrad, _ = route                                                    # (every call asserts: the entry, once, fp32 -- never the library)
    tune(monkeypatch, conv_wgrad_wgs=wgs)
    if shape == X.WRAP_SHAPE:
        assert _chunks(shape) == (X.WRAP_CHUNKS if wgs else X.WRAP_UNITS)       # four tiles per chunk / one
    X.check_exact(wgrad, _dev(), shape)
    X.check_small_integers(wgrad, _dev(), shape)
    X.check_random(wgrad, _dev(), shape, twice=True)


def test_conv_wgrad_f32_chunk_counts(route, monkeypatch):
    wgrad, _ = route
    seen = []
    for wgs in (64, None, 8192):
        tune(monkeypatch, conv_wgrad_wgs=wgs)
        seen.append(_chunks(X.WRAP_SHAPE))
        X.check_random(wgrad, _dev(), X.WRAP_SHAPE, "wgs %s" % wgs)
        X.check_exact(wgrad, _dev(), X.WRAP_SHAPE, ("int",), "wgs %s" % wgs)
    assert seen == [X.WRAP_CHUNKS, X.WRAP_UNITS, X.WRAP_UNITS], seen


@pytest.mark.parametrize("shape", BIG_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv_wgrad_f32_launch_geometry_of_large_shapes(route, shape):
    """The random case only, fp64 on the GPU; a second call returns the same bits (no atomics)."""
    wgrad, _ = route
    X.check_random(wgrad, _dev(), shape, twice=True)


def test_conv_wgrad_f32_precision_class_relative_to_the_library(route):
    """The rule of test_tgemm_f32_precision_class_relative_to_the_library: against product_bound(c = 1, K = B H W) the worst error / bound
    ratio of the kernel may be at most max(1, 2 x the ratio of aten.convolution_backward on the same fp32 operands)."""
    wgrad, calls = route
    dev = _dev()
    for shape in ((3, 3, 3, 64, 32), (2, 5, 37, 64, 64), (2, 9, 40, 192, 256)):
        B, H, W, C, N = shape
        x, dy = X.random_operands(shape, dev)
        ref, mag = X.random_reference(shape, dev)
        bound = product_bound(ref, mag, B * H * W, torch.float32, c=1.0)
        mine = float(((wgrad(x, dy).double() - ref).abs() / bound).max())
        w = torch.zeros(N, C, 3, 3, device=dev).contiguous(memory_format=torch.channels_last)
        del calls[:]
        lib_dw = torch.ops.aten.convolution_backward(dy, x, w, None, (1, 1), (1, 1), (1, 1), False, (0, 0), 1, (False, True, False))[1]
        assert calls == [("library", (False, True, False))]
        lib = float(((lib_dw.double() - ref).abs() / bound).max())
        print("precision class %s: kernel %.3f library %.3f of the c = 1 bound" % (shape, mine, lib))
        assert mine <= max(1.0, 2.0 * lib), (shape, mine, lib)


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def test_fp32_stage_with_the_conv_wgrad_switch_against_fp64(monkeypatch):
    """The fp32 ResNet stage of test_conv3x3_f32_gpu.py::test_fp32_stage_with_the_conv3x3_switch_against_fp64 with MDETR_TGEMM_F32,
    MDETR_TWGRAD_F32 and MDETR_CONV3X3_F32 on in both runs, MDETR_CONV_WGRAD_F32 on against off, each against the stage in fp64.  That
    test's bars: per tensor the switched route's relative error may be at most twice the other route's, with floors of 2^-22 for the
    output and 1e-3 for the gradients.  With the switch on both conv2 weight gradients take the entry, with it off neither does."""
    import copy
    from monodetr_amd import conv3x3_ext, conv_wgrad_ext
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
    calls = X.record_routes(conv_wgrad_ext, monkeypatch)
    monkeypatch.setattr(linear, "_TGEMM_F32", True)
    monkeypatch.setattr(conv_wgrad_ext, "ENABLED_F32", True)
    monkeypatch.setattr(conv3x3_ext, "ENABLED_F32", True)
    tune(monkeypatch, conv_wgrad_wgs=None, conv3x3_f32_tile=None, conv3x3_f32_nb=None)
    res = {}
    for on in (False, True):
        monkeypatch.setattr(conv_wgrad_ext, "ENABLED_CONV_F32", on)
        del calls[:]
        stage.zero_grad(set_to_none=True)
        x.grad = None
        y = stage(x)
        (y * proj).sum().backward()
        res[on] = (y.detach().clone(), x.grad.clone(), {n: p.grad.clone() for n, p in stage.named_parameters() if p.grad is not None})
        entry = [c for c in calls if c[0] == "entry"]
        library_dw = [c for c in calls if c[0] == "library" and c[1][1]]
        if on:
            assert entry == [("entry", torch.float32, torch.float32)] * 2 and library_dw == [], calls
        else:
            assert entry == [] and len(library_dw) == 2, calls
    for m, name in ((conv3x3_ext, "ENABLED_F32"), (linear, "_TGEMM_F32"), (conv_wgrad_ext, "ENABLED_F32"), (conv_wgrad_ext, "ENABLED_CONV_F32")):
        monkeypatch.setattr(m, name, False)
    ref = copy.deepcopy(stage).double()
    x64 = x.detach().double().requires_grad_(True)
    y64 = ref(x64)
    (y64 * proj.double()).sum().backward()
    want = (y64.detach(), x64.grad, {n: p.grad for n, p in ref.named_parameters() if p.grad is not None})
    for name, got_on, got_off, w64 in [("output", res[True][0], res[False][0], want[0]), ("input gradient", res[True][1], res[False][1], want[1])] + \
            [(n, res[True][2][n], res[False][2][n], g) for n, g in want[2].items()]:
        e_on, e_off = _rel(got_on, w64), _rel(got_off, w64)
        print("stage %-28s relative error: conv_wgrad_f32 on %.3e, off %.3e" % (name, e_on, e_off))
        assert e_on <= max(2.0 * e_off, 2.0 ** -22 if name == "output" else 1e-3), (name, e_on, e_off)
