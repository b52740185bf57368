"""The stride-2 fp32 form of csrc/conv_wgrad.hip (mdetr_conv_wgrad_s2_f32; family MDETR_CONV_WGRAD_S2_F32) on the GPU, reached the way the
step reaches it -- the backward pass of conv_taps_ext.conv_strided with MDETR_CONV_STRIDED_F32 on: the exact cases of
tests/conv_wgrad_s2_f32_cases.py bit for bit and the random case element-wise against fp64 within the fp32-accumulation bound
(tests/gemm_bounds.py) on every shape; every chunk count; launch geometries only large shapes reach, deterministic; the library's
precision class; and an fp32 ResNet stage whose first block strides with the five earlier fp32 switches on."""
import pytest
import torch

import conv_wgrad_s2_f32_cases as X
from conftest import tune
from gemm_bounds import product_bound

pytestmark = pytest.mark.gpu

# launch geometry the small shapes cannot reach: layer2.0.conv2 (12 blocks x 42 chunks of 36 - 37 tiles), layer3.0.conv2 and the depth
# predictor's downsample (48 blocks x 10 chunks of 24 tiles), layer4.0.conv2 (192 blocks, 2 chunks of 120 tiles)
BIG_SHAPES = [(8, 96, 320, 128, 128), (8, 48, 160, 256, 256), (8, 24, 80, 512, 512)]


@pytest.fixture
def route(monkeypatch):
    """-> (wgrad, calls): the weight gradient through conv_strided's backward pass, its route recorded and asserted per call."""
    from monodetr_amd import conv_taps_ext, conv_wgrad_ext
    monkeypatch.setattr(conv_taps_ext, "ENABLED_F32", True)
    monkeypatch.setattr(conv_wgrad_ext, "ENABLED_CONV_S2_F32", True)
    X.lift_shape_rule(conv_wgrad_ext, monkeypatch)                     # the kernel is under test here, on every shape the entry takes
    tune(monkeypatch, conv_wgrad_wgs=None, conv_taps_f32_rows=None, conv_taps_f32_nb=None)
    calls = X.record_routes(conv_wgrad_ext, monkeypatch)
    return X.through_conv_strided(conv_taps_ext, calls), calls


def _dev():
    return torch.device("cuda", 0)


def _chunks(shape):
    from monodetr_amd import _capi
    B, H, W, C, N = shape
    OH, OW = X.out_hw(H, W)
    return _capi.lib().mdetr_conv_wgrad_s2_f32_chunks(B, H, W, C, OH, OW, N, 3, 2)


CASES = [(s, None) for s in X.SHAPES] + [(X.WRAP_SHAPE, X.WRAP_WGS)]


@pytest.mark.parametrize("shape,wgs", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else "wgs%s" % v)
def test_conv_wgrad_s2_f32_exact_and_random_cases(route, monkeypatch, shape, wgs):
    wgrad, _ = route                                                    # (every call asserts: the entry, once, fp32 -- never the library)
    tune(monkeypatch, conv_wgrad_wgs=wgs)
    if shape == X.WRAP_SHAPE:
        chunks = _chunks(shape)
        assert X.tiles(shape) == 20 and chunks == (1 if wgs else 14) and chunks == X.expected_chunks(shape, wgs)
        assert not wgs or X.tiles(shape) // chunks >= 3                 # the single LDS buffer is reused and the prefetch wraps
    X.check_exact(wgrad, _dev(), shape)
    X.check_small_integers(wgrad, _dev(), shape)
    X.check_random(wgrad, _dev(), shape, twice=True)


def test_conv_wgrad_s2_f32_chunk_counts(route, monkeypatch):
    wgrad, _ = route
    seen = []
    for wgs in (64, None, 8192):
        tune(monkeypatch, conv_wgrad_wgs=wgs)
        seen.append(_chunks(X.WRAP_SHAPE))
        X.check_random(wgrad, _dev(), X.WRAP_SHAPE, "wgs %s" % wgs)
        X.check_exact(wgrad, _dev(), X.WRAP_SHAPE, ("int",), "wgs %s" % wgs)
    assert seen == [1, 14, 20], seen                                    # one chunk of 20 tiles; 14 chunks of 1 - 2; one tile per chunk


@pytest.mark.parametrize("shape", BIG_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv_wgrad_s2_f32_launch_geometry_of_large_shapes(route, shape):
    """The random case only, fp64 on the GPU; a second call returns the same bits (no atomics)."""
    wgrad, _ = route
    X.check_random(wgrad, _dev(), shape, twice=True)


def test_conv_wgrad_s2_f32_precision_class_relative_to_the_library(route):
    """The rule of test_conv_wgrad_f32_precision_class_relative_to_the_library: against product_bound(c = 1, K = B OH OW) the worst
    error / bound ratio of the kernel may be at most max(1, 2 x the ratio of aten.convolution_backward at stride 2 on the same fp32
    operands)."""
    wgrad, calls = route
    dev = _dev()
    for shape in (X.SHAPES[0], X.SHAPES[1], X.SHAPES[3]):
        B, H, W, C, N = shape
        OH, OW = X.out_hw(H, W)
        x, dy = X.random_operands(shape, dev)
        ref, mag = X.random_reference(shape, dev)
        bound = product_bound(ref, mag, B * OH * OW, torch.float32, c=1.0)
        mine = float(((wgrad(x, dy).double() - ref).abs() / bound).max())
        w = torch.zeros(N, C, 3, 3, device=dev).contiguous(memory_format=torch.channels_last)
        del calls[:]
        lib_dw = torch.ops.aten.convolution_backward(dy, x, w, None, (2, 2), (1, 1), (1, 1), False, (0, 0), 1, (False, True, False))[1]
        assert calls == [("library", (False, True, False))]
        lib = float(((lib_dw.double() - ref).abs() / bound).max())
        print("precision class %s: kernel %.3f library %.3f of the c = 1 bound" % (shape, mine, lib))
        assert mine <= max(1.0, 2.0 * lib), (shape, mine, lib)


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def test_fp32_stage_with_the_conv_wgrad_s2_switch_against_fp64(monkeypatch):
    """The fp32 ResNet stage of test_conv_strided_f32_gpu.py::test_fp32_stage_with_the_conv_strided_switch_against_fp64 (its size too: the
    docstring there explains why the 1e-3 gradient floor needs the 96 x 320 input) with MDETR_TGEMM_F32, MDETR_TWGRAD_F32,
    MDETR_CONV3X3_F32, MDETR_CONV_WGRAD_F32 and MDETR_CONV_STRIDED_F32 on in both runs, MDETR_CONV_WGRAD_S2_F32 on against off, each
    against the stage in fp64.  That test's bars: per tensor the switched route's relative error may be at most twice the other route's,
    with floors of 2^-22 for the output and 1e-3 for the gradients.  With the switch on 0.conv2.weight (3x3 / stride 2) comes from the
    new entry and the library is asked for no weight gradient of a stride-2 problem; with it off the library computes it."""
    import copy
    from monodetr_amd import conv3x3_ext, conv_taps_ext, conv_wgrad_ext
    from monodetr_amd.monodetr import backbone, linear
    dev = _dev()
    torch.manual_seed(2)
    down = torch.nn.Sequential(torch.nn.Conv2d(256, 512, 1, 2, bias=False), backbone.FrozenBatchNorm2d(512))
    stage = torch.nn.Sequential(backbone.Bottleneck(256, 128, 2, down), backbone.Bottleneck(512, 128)).to(dev).to(memory_format=torch.channels_last)
    for m in stage.modules():
        if isinstance(m, backbone.FrozenBatchNorm2d):
            m.weight.uniform_(0.5, 1.5); m.bias.normal_(0, 0.2); m.running_mean.normal_(0, 0.2); m.running_var.uniform_(0.5, 1.5)
    x = (torch.randn(4, 256, 96, 320, device=dev) * 0.5).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    proj = torch.linspace(-1, 1, 4 * 512 * 48 * 160, device=dev).view(4, 48, 160, 512).permute(0, 3, 1, 2)
    calls, real_w, real_c = [], conv_wgrad_ext.weight_gradient, torch.ops.aten.convolution_backward

    def weight_gradient(xx, dy, k, stride, *a, **kw):
        calls.append(("entry", xx.dtype, dy.dtype, k, stride, tuple(dy.shape[1:2]) + tuple(xx.shape[1:2])))
        return real_w(xx, dy, k, stride, *a, **kw)

    def convolution_backward(*a):
        calls.append(("library", tuple(a[-1]), tuple(a[4])))           # (output mask, stride)
        return real_c(*a)
    monkeypatch.setattr(conv_wgrad_ext, "weight_gradient", weight_gradient)
    monkeypatch.setattr(torch.ops.aten, "convolution_backward", convolution_backward)
    five = ((linear, "_TGEMM_F32"), (conv_wgrad_ext, "ENABLED_F32"), (conv3x3_ext, "ENABLED_F32"), (conv_wgrad_ext, "ENABLED_CONV_F32"),
            (conv_taps_ext, "ENABLED_F32"))
    for mod, name in five:
        monkeypatch.setattr(mod, name, True)
    X.lift_shape_rule(conv_wgrad_ext, monkeypatch)
    tune(monkeypatch, conv_wgrad_wgs=None, conv3x3_f32_tile=None, conv3x3_f32_nb=None, conv_taps_f32_rows=None, conv_taps_f32_nb=None)
    res = {}
    for on in (False, True):
        monkeypatch.setattr(conv_wgrad_ext, "ENABLED_CONV_S2_F32", on)
        del calls[:]
        stage.zero_grad(set_to_none=True)
        x.grad = None
        y = stage(x)
        (y * proj).sum().backward()
        res[on] = dict({"output": y.detach().clone(), "input gradient": x.grad.clone()},
                       **{n: p.grad.clone() for n, p in stage.named_parameters() if p.grad is not None})
        strided_entry = [c for c in calls if c[0] == "entry" and c[3:5] == (3, 2)]
        strided_library_dw = [c for c in calls if c[0] == "library" and c[1] == (False, True, False) and c[2] == (2, 2)]
        if on:
            assert strided_entry == [("entry", torch.float32, torch.float32, 3, 2, (128, 128))] and strided_library_dw == [], calls
        else:
            assert strided_entry == [] and len(strided_library_dw) == 1, calls
    for mod, name in five + ((conv_wgrad_ext, "ENABLED_CONV_S2_F32"),):
        monkeypatch.setattr(mod, name, False)
    ref = copy.deepcopy(stage).double()
    x64 = x.detach().double().requires_grad_(True)
    y64 = ref(x64)
    (y64 * proj.double()).sum().backward()
    want = dict({"output": y64.detach(), "input gradient": x64.grad}, **{n: p.grad for n, p in ref.named_parameters() if p.grad is not None})
    bad = []                                                            # (every figure is printed before the assertion)
    for name, w64 in want.items():
        e_on, e_off = _rel(res[True][name], w64), _rel(res[False][name], w64)
        print("stage %-28s relative error: conv_wgrad_s2_f32 on %.3e, off %.3e" % (name, e_on, e_off))
        if not e_on <= max(2.0 * e_off, 2.0 ** -22 if name == "output" else 1e-3):
            bad.append((name, e_on, e_off))
    assert not bad, bad
