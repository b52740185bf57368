"""The fp32 form of csrc/conv_stem.hip (conv_stem_f32_kernel, mdetr_conv_stem_f32; family MDETR_CONV_STEM_F32) on the GPU: the exact cases
of tests/conv_stem_f32_cases.py bit for bit, the random case element-wise against fp64 within the fp32-accumulation bound
(tests/gemm_bounds.py) and the non-finite case on every shape; the launch geometry of the real image sizes; the library's precision
class; and the stem module (conv1 -> frozen bn1 -> ReLU through backbone.conv_bn) with the committed fp32 families on."""
import pytest
import torch
import torch.nn.functional as F

import conv_stem_f32_cases as X
from gemm_bounds import conv2d_f64, product_bound

pytestmark = pytest.mark.gpu


@pytest.fixture
def ext(monkeypatch):
    from monodetr_amd import conv_stem_ext
    monkeypatch.setattr(conv_stem_ext, "ENABLED_F32", True)
    return conv_stem_ext


def _dev():
    return torch.device("cuda", 0)


@pytest.mark.parametrize("shape", X.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv_stem_f32_exact_and_random_cases(ext, monkeypatch, shape):
    calls = X.record_launches(ext, monkeypatch)
    X.check_exact(ext, _dev(), shape)
    X.check_small_integers(ext, _dev(), shape)
    X.check_random(ext, _dev(), shape, twice=True)
    assert calls == [torch.float32] * 7, calls


@pytest.mark.parametrize("shape", X.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv_stem_f32_nonfinite_pixel(ext, shape):
    X.check_nonfinite(ext, _dev(), shape)


def test_conv_stem_f32_packed_planes(ext):
    X.check_packed_planes(ext, _dev())


# launch geometry the small shapes cannot reach: 8 x 24 x 4 = 768 workgroups of five full tiles (the benchmark's image), and 2 x 32 x 6
# with a half-empty 28th column tile in a ragged sixth group (the larger configuration's)
BIG_SHAPES = [(8, 384, 1280), (2, 512, 1760)]


@pytest.mark.parametrize("shape", BIG_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv_stem_f32_launch_geometry_of_the_real_shapes(ext, shape):
    """The random case only, fp64 on the GPU; a second call returns the same bits (no atomics)."""
    X.check_random(ext, _dev(), shape, twice=True)
    X.random_reference.cache_clear()                                    # (gigabytes of fp64 on the device)


def test_conv_stem_f32_precision_class_relative_to_the_library(ext):
    """The rule of test_conv_strided_f32_precision_class_relative_to_the_library: against product_bound(c = 1) at K = 147 the worst
    error / bound ratio of the kernel may be at most max(1, 2 x the ratio of F.conv2d (+ shift, ReLU) on the same fp32 operands)."""
    dev = _dev()
    for shape in ((2, 5, 7), (3, 16, 64), (1, 37, 75)):
        x, w, shift, ref, mag = X.random_reference(shape, str(dev))
        bound = product_bound(ref, mag, X.K, torch.float32, c=1.0)
        y = ext.conv_stem(x, w, shift)
        mine = float(((y.double() - ref).abs() / bound).max())
        lib = float(((F.relu(F.conv2d(x, w, shift, stride=2, padding=3)).double() - ref).abs() / bound).max())
        print("precision class %s: kernel %.3f library %.3f of the c = 1 bound" % (shape, mine, lib))
        assert mine <= max(1.0, 2.0 * lib), (shape, mine, lib)


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def test_fp32_stem_with_the_switch_against_fp64(monkeypatch):
    """The stem through backbone.conv_bn (conv1 -> frozen bn1 -> ReLU) on a (2, 3, 96, 320) channels_last fp32 image with the committed fp32
    families applied, MDETR_CONV_STEM_F32 on against off, each against the module in fp64.  The stage tests' bar for outputs: the relative
    error with the switch may be at most max(2 x the other route's, 2^-22).  One recorded launch with the switch on, none with it off."""
    from monodetr_amd import conv_stem_ext, kernel_families as kf
    from monodetr_amd.monodetr import backbone
    dev = _dev()
    torch.manual_seed(4)
    conv = torch.nn.Conv2d(3, 64, 7, 2, 3, bias=False).to(dev).requires_grad_(False)
    bn = backbone.FrozenBatchNorm2d(64).to(dev)
    bn.weight.uniform_(0.5, 1.5); bn.bias.normal_(0, 0.2); bn.running_mean.normal_(0, 0.2); bn.running_var.uniform_(0.5, 1.5)
    x = torch.randn(2, 3, 96, 320, device=dev).contiguous(memory_format=torch.channels_last)
    calls = X.record_launches(conv_stem_ext, monkeypatch)
    committed = set(kf.COMMITTED_SWITCHES["fp32"])
    res = {}
    try:
        for on in (False, True):
            kf.apply_switches(committed | ({"MDETR_CONV_STEM_F32"} if on else set()))
            del calls[:]
            res[on] = backbone.conv_bn(x, conv, bn, True).clone()
            assert calls == ([torch.float32] if on else []), calls
    finally:
        kf.apply_switches(set())
    var64 = bn.running_var.double() + bn.eps
    pre = conv2d_f64(x.double(), conv.weight.double(), stride=2, padding=3)
    want = ((pre - bn.running_mean.double().view(1, -1, 1, 1)) * (bn.weight.double() * var64.rsqrt()).view(1, -1, 1, 1)
            + bn.bias.double().view(1, -1, 1, 1)).clamp(min=0)
    e_on, e_off = _rel(res[True], want), _rel(res[False], want)
    print("stem output relative error: conv_stem_f32 on %.3e, off %.3e" % (e_on, e_off))
    assert res[True].dtype == torch.float32 and res[True].shape == want.shape
    assert e_on <= max(2.0 * e_off, 2.0 ** -22), (e_on, e_off)
