"""The fp32 form of csrc/conv3x3.hip (mdetr_conv3x3_f32; family MDETR_CONV3X3_F32) on the GPU: the exact cases of
tests/conv3x3_f32_cases.py bit for bit and the random case element-wise against fp64 within the fp32-accumulation bound
(tests/gemm_bounds.py), on every shape and for every (tile, width) the launcher builds; launch geometries only large shapes reach,
deterministic; the library's precision class; and an fp32 ResNet stage with the three fp32 switches on."""
import pytest
import torch
import torch.nn.functional as F

import conv3x3_f32_cases as X
from conftest import tune
from gemm_bounds import conv2d_f64, product_bound

pytestmark = pytest.mark.gpu

# launch geometry the small shapes cannot reach: layer3 (the fewest rounds), 16 slabs with 8+ channel groups, thousands of tiles
BIG_SHAPES = [(8, 24, 80, 256, 256), (8, 12, 40, 512, 512), (2, 96, 320, 64, 64)]


@pytest.fixture
def ext(monkeypatch):
    from monodetr_amd import conv3x3_ext
    monkeypatch.setattr(conv3x3_ext, "ENABLED_F32", True)
    tune(monkeypatch, conv3x3_f32_tile=None, conv3x3_f32_nb=None)
    return conv3x3_ext


def _dev():
    return torch.device("cuda", 0)


@pytest.mark.parametrize("shape", X.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv3x3_f32_exact_and_random_cases(ext, monkeypatch, shape):
    calls = X.record_launches(ext, monkeypatch)
    X.check_exact(ext, _dev(), shape)
    assert all(c[0] == torch.float32 for c in calls) and len(calls) == (9 if X.dx_on_kernel(shape[3], shape[4]) else 3), calls
    X.check_small_integers(ext, _dev(), shape, calls)
    X.check_random(ext, _dev(), shape, twice=True)


@pytest.mark.parametrize("nb", X.NBS)
@pytest.mark.parametrize("tile", X.TILES)
def test_conv3x3_f32_every_tile_and_width(ext, monkeypatch, tile, nb):
    from monodetr_amd import _capi
    tune(monkeypatch, conv3x3_f32_tile=tile, conv3x3_f32_nb=nb)
    B, H, W, C, N = X.SWEEP_SHAPE
    assert _capi.lib().mdetr_conv3x3_f32_plan(B, H, W, N) == 10 * tile + nb
    tag = "tile %d nb %d" % (tile, nb)
    X.check_random(ext, _dev(), X.SWEEP_SHAPE, tag)
    X.check_exact(ext, _dev(), X.SWEEP_SHAPE, ("int", "x"), tag)


@pytest.mark.parametrize("shape", BIG_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv3x3_f32_launch_geometry_of_large_shapes(ext, shape):
    """The random case only, fp64 on the GPU; a second call returns the same bits (no atomics)."""
    X.check_random(ext, _dev(), shape, twice=True)


def test_conv3x3_f32_precision_class_relative_to_the_library(ext):
    """The rule of test_tgemm_f32_precision_class_relative_to_the_library: against product_bound(c = 1, K = 9 C) the worst error / bound
    ratio of the kernel may be at most max(1, 2 x the ratio of F.conv2d on the same fp32 operands)."""
    dev = _dev()
    for shape in ((3, 3, 3, 64, 32), (2, 5, 37, 64, 64), (2, 7, 43, 128, 128)):
        B, H, W, C, N = shape
        x, w, shift, _ = X.random_operands(shape, dev)
        ref = conv2d_f64(x.double(), w.double(), shift.double(), padding=1)
        mag = conv2d_f64(x.double().abs(), w.double().abs(), shift.double().abs(), padding=1)
        bound = product_bound(ref, mag, 9 * C, torch.float32, c=1.0)
        mine = float(((ext.conv3x3(x, w, shift, relu=False).double() - ref).abs() / bound).max())
        lib = float(((F.conv2d(x, w, shift, padding=1).double() - ref).abs() / bound).max())
        print("precision class %s: kernel %.3f library %.3f of the c = 1 bound" % (shape, mine, lib))
        assert mine <= max(1.0, 2.0 * lib), (shape, mine, lib)


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def test_fp32_stage_with_the_conv3x3_switch_against_fp64(monkeypatch):
    """The fp32 ResNet stage of test_twgrad_f32_gpu.py::test_fp32_stage_with_both_switches_against_fp64 with MDETR_TGEMM_F32 +
    MDETR_TWGRAD_F32 on in both runs, MDETR_CONV3X3_F32 on against off, each against the stage in fp64.  That test's bars: per tensor the
    switched route's relative error may be at most twice the other route's, with floors of 2^-22 for the output and 1e-3 for the gradients.
    Both conv2 calls must take the entry, forward and for the input gradient."""
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
    calls = X.record_launches(conv3x3_ext, monkeypatch)
    monkeypatch.setattr(linear, "_TGEMM_F32", True)
    monkeypatch.setattr(conv_wgrad_ext, "ENABLED_F32", True)
    tune(monkeypatch, conv3x3_f32_tile=None, conv3x3_f32_nb=None)
    res = {}
    for on in (False, True):
        monkeypatch.setattr(conv3x3_ext, "ENABLED_F32", on)
        del calls[:]
        stage.zero_grad(set_to_none=True)
        x.grad = None
        y = stage(x)
        (y * proj).sum().backward()
        res[on] = (y.detach().clone(), x.grad.clone(), {n: p.grad.clone() for n, p in stage.named_parameters() if p.grad is not None})
        if on:
            assert sorted(c[1] for c in calls) == [False, False, True, True] and all(c[0] == torch.float32 for c in calls), calls
        else:
            assert calls == [], calls
    monkeypatch.setattr(conv3x3_ext, "ENABLED_F32", False)
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
        print("stage %-28s relative error: conv3x3_f32 on %.3e, off %.3e" % (name, e_on, e_off))
        assert e_on <= max(2.0 * e_off, 2.0 ** -22 if name == "output" else 1e-3), (name, e_on, e_off)
