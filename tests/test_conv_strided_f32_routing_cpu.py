"""MDETR_CONV_STRIDED_F32 routing (conv_taps_ext.py, monodetr/backbone.py, kernel_families.py) with the fp32 form of csrc/conv_taps.hip
running on the CPU shim: with the switch off fp32 tensors behave as before (no module reaches an entry); with it on an fp32 Bottleneck
whose conv2 strides and an fp32 ConvStrided module take the entries once forward and once for the input gradient, NCHW-contiguous and
autocast calls stay on the library, and both routes lie within the fp32-accumulation bound of the fp64 value."""
import copy
import os

import pytest
import torch

import native_emul
from conftest import tune
from gemm_bounds import assert_product_close, conv2d_f64


class Counting:
    """The emulated library with its conv_taps / conv_dgrad_s2 launches counted."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith(("mdetr_conv_taps", "mdetr_conv_dgrad_s2")):
            return fn

        def counted(*a):
            self.calls.append(name)
            return fn(*a)
        return counted


@pytest.fixture
def backend(monkeypatch):
    from monodetr_amd import conv_taps_ext
    raw = native_emul.lib()
    raw.mdetr_conv_taps_f32                                             # (AttributeError without the feature)
    L = Counting(raw)
    monkeypatch.setattr(conv_taps_ext, "_backend", L)
    monkeypatch.setattr(conv_taps_ext, "ENABLED", False)
    monkeypatch.setattr(conv_taps_ext, "ENABLED_F32", False)
    tune(monkeypatch, conv_taps_f32_rows=None, conv_taps_f32_nb=None, conv_taps_split=None)
    return L


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def test_switch_off_fp32_tensors_behave_as_before(backend):
    from monodetr_amd import conv_taps_ext as ext
    from monodetr_amd.monodetr.backbone import Bottleneck, FrozenBatchNorm2d
    x, w = _cl(torch.randn(1, 64, 4, 4)), torch.randn(64, 64, 3, 3)
    assert not ext.ENABLED_F32 and not ext.supported(x, w) and not ext.supported_f32(x, w)
    with pytest.raises(RuntimeError):
        ext.conv_strided(x, w)
    assert ext.supported(x.bfloat16(), w.bfloat16())
    conv = ext.ConvStrided(64, 64, kernel_size=(3, 3), stride=2, padding=1).to(memory_format=torch.channels_last)
    assert type(conv(x).grad_fn).__name__ != "_ConvStridedBackward"
    block = Bottleneck(64, 64, 2, torch.nn.Sequential(torch.nn.Conv2d(64, 256, 1, 2, bias=False), FrozenBatchNorm2d(256)))
    block.to(memory_format=torch.channels_last)(x)
    assert backend.calls == []


def test_supported_f32_mirrors_supported(backend, monkeypatch):
    from monodetr_amd import conv_taps_ext as ext
    monkeypatch.setattr(ext, "ENABLED_F32", True)
    x, w = _cl(torch.randn(1, 64, 4, 4)), torch.randn(64, 64, 3, 3)
    assert ext.supported_f32(x, w) and not ext.supported(x, w)                     # the bf16 predicate keeps its meaning
    assert not ext.supported_f32(x.bfloat16(), w.bfloat16()) and not ext.supported_f32(x, w.bfloat16()) and not ext.supported_f32(x.double(), w.double())
    assert not ext.supported_f32(x, w, stride=(1, 1)) and not ext.supported_f32(x, w, padding=(0, 0)) and not ext.supported_f32(x, w, dilation=(2, 2))
    assert not ext.supported_f32(x, w, groups=2) and not ext.supported_f32(x.contiguous(), w)
    assert not ext.supported_f32(_cl(torch.randn(1, 48, 4, 4)), w[:, :48].contiguous()) and not ext.supported_f32(x, torch.randn(40, 64, 3, 3))
    assert not ext.supported_f32(_cl(torch.randn(0, 64, 4, 4)), w)
    # 3x3 only: the 1x1 / stride-2 shortcut (which `supported` takes in bf16) is a gather and a token GEMM in fp32
    w1 = torch.randn(64, 64, 1, 1)
    assert ext.supported(x.bfloat16(), w1.bfloat16(), padding=(0, 0)) and not ext.supported_f32(x, w1, padding=(0, 0))
    # the forward pass takes N % 32 == 0; the input gradient then stays on the library (N % 64 != 0)
    assert ext.supported_f32(x, torch.randn(96, 64, 3, 3)) and not ext._dx_on_kernel(torch.empty(1, 96, 2, 2), 64) and ext._dx_on_kernel(torch.empty(1, 64, 2, 2), 64)
    assert ext._dx_on_kernel(torch.empty(1, 96, 2, 2, dtype=torch.bfloat16), 64)
    # the entry's 32-bit byte offsets: fewer than 2^29 elements of x (a meta tensor: no memory behind it)
    big = torch.empty((8, 64, 1024, 1024), device="meta").contiguous(memory_format=torch.channels_last)
    assert big.numel() == 1 << 29 and not ext.supported_f32(big, w)


def _randomise(module):
    from monodetr_amd.monodetr.backbone import FrozenBatchNorm2d
    for m in module.modules():
        if isinstance(m, FrozenBatchNorm2d):
            m.weight.uniform_(0.5, 1.5); m.bias.normal_(0, 0.3); m.running_mean.normal_(0, 0.3); m.running_var.uniform_(0.5, 2.0)


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def test_fp32_strided_bottleneck_takes_the_entries_with_the_switch_only(backend, monkeypatch):
    """backbone.conv_bn: conv2 (3x3 / stride 2) of an fp32 channels_last bottleneck -- one forward and one input-gradient entry call
    with the switch on, none without; the block's output and all gradients of both routes against the block in fp64, at the stage
    tests' bars (ReLU masks within rounding of zero may flip on either route)."""
    from monodetr_amd import conv_taps_ext as ext
    from monodetr_amd.monodetr.backbone import Bottleneck, FrozenBatchNorm2d, conv_bn
    torch.manual_seed(5)
    down = torch.nn.Sequential(torch.nn.Conv2d(256, 256, 1, 2, bias=False), FrozenBatchNorm2d(256))
    block = Bottleneck(256, 64, 2, down).to(memory_format=torch.channels_last)
    _randomise(block)
    x = _cl(torch.randn(2, 256, 7, 41))
    dy = _cl(torch.randn(2, 256, 4, 21))
    res = {}
    for on in (False, True):
        monkeypatch.setattr(ext, "ENABLED_F32", on)
        del backend.calls[:]
        xi = x.clone().requires_grad_(True)
        block.zero_grad(set_to_none=True)
        y = block(xi)
        y.backward(dy)
        assert backend.calls == (["mdetr_conv_taps_f32", "mdetr_conv_dgrad_s2_f32"] if on else []), backend.calls
        res[on] = [y.detach(), xi.grad] + [p.grad.clone() for p in block.parameters()]
    monkeypatch.setattr(ext, "ENABLED_F32", True)
    del backend.calls[:]
    mid = torch.randn(2, 64, 7, 41)                                                # conv2's input, NCHW-contiguous: the library
    assert conv_bn(mid, block.conv2, block.bn2, True).shape == (2, 64, 4, 21) and backend.calls == []
    assert conv_bn(_cl(mid), block.conv2, block.bn2, True).shape == (2, 64, 4, 21) and backend.calls == ["mdetr_conv_taps_f32"]
    del backend.calls[:]
    with torch.autocast("cpu", dtype=torch.bfloat16):
        block(x)
    assert backend.calls == []                                                     # autocast: the library
    monkeypatch.setattr(ext, "ENABLED_F32", False)
    ref = copy.deepcopy(block).double()
    x64 = x.double().requires_grad_(True)
    y64 = ref(x64)
    y64.backward(dy.double())
    want = [y64.detach(), x64.grad] + [p.grad for p in ref.parameters()]
    for i, (a, b, w64) in enumerate(zip(res[True], res[False], want)):
        e_on, e_off = _rel(a, w64), _rel(b, w64)
        assert e_on <= max(2.0 * e_off, 2.0 ** -22 if i == 0 else 1e-3), (i, e_on, e_off)


def test_fp32_conv_module_takes_the_entries_with_the_switch_only(backend, monkeypatch):
    """conv_taps_ext.ConvStrided (the fourth pyramid level, the depth predictor's downsample: a trainable bias) in fp32: entry calls,
    and y / dx of the kernel route element-wise within the random-case bound of fp64; dw and db (the library's / a column sum) agree
    with the library route."""
    from monodetr_amd import conv_taps_ext as ext
    torch.manual_seed(2)
    conv = ext.ConvStrided(64, 64, kernel_size=(3, 3), stride=2, padding=1).to(memory_format=torch.channels_last)
    x, dy = _cl(torch.randn(2, 64, 7, 33) * 0.5), _cl(torch.randn(2, 64, 4, 17))
    res = {}
    for on in (False, True):
        monkeypatch.setattr(ext, "ENABLED_F32", on)
        del backend.calls[:]
        xi = x.clone().requires_grad_(True)
        conv.zero_grad(set_to_none=True)
        y = conv(xi)
        assert (type(y.grad_fn).__name__ == "_ConvStridedBackward") == on
        y.backward(dy)
        assert backend.calls == (["mdetr_conv_taps_f32", "mdetr_conv_dgrad_s2_f32"] if on else []), backend.calls
        res[on] = (y.detach(), xi.grad, conv.weight.grad.clone(), conv.bias.grad.clone())
    monkeypatch.setattr(ext, "ENABLED_F32", True)
    del backend.calls[:]
    assert type(conv(x.contiguous()).grad_fn).__name__ != "_ConvStridedBackward"      # NCHW-contiguous input
    with torch.autocast("cpu", dtype=torch.bfloat16):
        assert type(conv(x).grad_fn).__name__ != "_ConvStridedBackward"
    assert type(copy.deepcopy(conv).bfloat16()(x.bfloat16()).grad_fn).__name__ != "_ConvStridedBackward" and backend.calls == []      # bf16 needs ITS switch
    x64, w64 = x.double().requires_grad_(True), conv.weight.detach().double().requires_grad_(True)
    ref = conv2d_f64(x64, w64, conv.bias.detach().double(), stride=2, padding=1)
    xa, wa = x.double().abs().requires_grad_(True), w64.detach().abs().requires_grad_(True)
    mag = conv2d_f64(xa, wa, conv.bias.detach().double().abs(), stride=2, padding=1)
    gx, gw = torch.autograd.grad(ref, (x64, w64), dy.double())
    mx, mw = torch.autograd.grad(mag, (xa, wa), dy.double().abs())
    for on in (False, True):
        assert_product_close(res[on][0], ref.detach(), mag.detach(), 9 * 64, "y on=%s" % on)
        assert_product_close(res[on][1], gx, mx, 4 * 64, "dx on=%s" % on)
        assert_product_close(res[on][2], gw, mw, 2 * 4 * 17, "dw on=%s" % on)
    assert torch.equal(res[True][2], res[False][2]) or _rel(res[True][2], res[False][2]) < 1e-6      # the same library call on the same operands
    assert _rel(res[True][3], res[False][3]) < 1e-6


def test_measured_shape_rule_routes_each_class_on_its_own(backend, monkeypatch):
    """The table at conv_taps_ext._F32_FWD_MAX_C: the forward pass takes the kernel up to 128 input channels (layer2), the input gradient
    up to 512 (layer2 / 3 / 4, the depth predictor's downsample); the fourth pyramid level (2048 channels) stays on the library as a
    whole, and so does a wide layer whose N % 64 != 0 keeps the input gradient off the kernel.  At 256 channels the forward pass is the
    library's INSIDE the same autograd node and the input gradient the kernel's: y and dx agree with the all-kernel route."""
    from monodetr_amd import conv_taps_ext as ext
    assert (ext._F32_FWD_MAX_C, ext._F32_DX_MAX_C) == (128, 512)
    monkeypatch.setattr(ext, "ENABLED_F32", True)
    mk = lambda C, N: (_cl(torch.randn(1, C, 5, 6) * 0.5), torch.randn(N, C, 3, 3) / (3.0 * C ** 0.5))          # noqa: E731
    for C, N, sup, fwd, dx in ((128, 128, True, True, True), (128, 96, True, True, False), (256, 256, True, False, True), (512, 64, True, False, True),
                               (256, 96, False, False, False), (576, 64, False, False, False), (2048, 256, False, False, False)):
        x, w = mk(C, N)
        assert ext.supported_f32(x, w) == sup and ext._fwd_on_kernel(x) == fwd and ext._dx_on_kernel(torch.empty(1, N, 3, 3), C) == dx, (C, N)
    assert ext._fwd_on_kernel(x.bfloat16()) and ext._dx_on_kernel(torch.empty(1, 256, 3, 3, dtype=torch.bfloat16), 2048)      # bf16: no rule
    torch.manual_seed(4)
    x, w = mk(256, 64)
    shift, dy = torch.randn(64), _cl(torch.randn(1, 64, 3, 3))
    res = {}
    for lifted in (False, True):
        if lifted:
            monkeypatch.setattr(ext, "_F32_FWD_MAX_C", 1 << 30)
        del backend.calls[:]
        xi = x.clone().requires_grad_(True)
        y = ext.conv_strided(xi, w, shift, relu=True)
        y.backward(dy)
        assert backend.calls == (["mdetr_conv_taps_f32"] if lifted else []) + ["mdetr_conv_dgrad_s2_f32"], backend.calls
        res[lifted] = (y.detach(), xi.grad)
    assert _rel(res[False][0], res[True][0]) < 1e-6 and _rel(res[False][1], res[True][1]) < 1e-6


def test_fp32_pointwise_conv_module_with_3x3_stride_2_takes_the_entry_with_the_switch_only(backend, monkeypatch):
    """linear.PointwiseConv2d is the class of the fourth pyramid level's and the depth predictor's 3x3 / stride-2 convolutions in the
    model: its fall-through to conv_taps_ext has the fp32 branch too."""
    from monodetr_amd import conv_taps_ext as ext
    from monodetr_amd.monodetr.linear import PointwiseConv2d
    torch.manual_seed(3)
    conv = PointwiseConv2d(64, 32, kernel_size=3, stride=2, padding=1).to(memory_format=torch.channels_last)
    x = _cl(torch.randn(1, 64, 5, 9))
    want = torch.nn.functional.conv2d(x, conv.weight, conv.bias, stride=2, padding=1)
    assert type(conv(x).grad_fn).__name__ != "_ConvStridedBackward" and backend.calls == []
    monkeypatch.setattr(ext, "ENABLED_F32", True)
    y = conv(x)
    assert type(y.grad_fn).__name__ == "_ConvStridedBackward" and backend.calls == ["mdetr_conv_taps_f32"]
    assert _rel(y, want) < 1e-6
    with torch.autocast("cpu", dtype=torch.bfloat16):
        assert type(conv(x).grad_fn).__name__ != "_ConvStridedBackward"


def test_switch_is_listed_applied_and_not_committed(monkeypatch):
    from monodetr_amd import conv3x3_ext, conv_taps_ext, kernel_families as kf
    name_ = "MDETR_CONV_STRIDED_F32"
    assert name_ in kf.ALL_SWITCHES and name_ in kf.AUTOTUNE_SWITCHES and name_ in kf.SWITCH_TESTS
    assert all(name_ not in fams for fams in kf.COMMITTED_SWITCHES.values())
    for pat in kf.SWITCH_TESTS[name_].split(","):
        name, stem = pat.strip().split("::")                            # every pattern names its file, and a test of that file
        assert name == "test_conv_strided_f32_gpu.py", pat
        assert "def " + stem.rstrip("*") in open(os.path.join(os.path.dirname(__file__), name)).read(), pat
    try:
        kf.apply_switches({name_})
        assert conv_taps_ext.ENABLED_F32 and not conv_taps_ext.ENABLED and not conv3x3_ext.ENABLED_F32
        kf.apply_switches({"MDETR_CONV_STRIDED", "MDETR_CONV3X3_F32"})
        assert not conv_taps_ext.ENABLED_F32 and conv_taps_ext.ENABLED and conv3x3_ext.ENABLED_F32
    finally:
        kf.apply_switches(set())
    assert not conv_taps_ext.ENABLED_F32 and not conv_taps_ext.ENABLED
    monkeypatch.setenv(name_, "1")
    assert name_ in kf.env_switches()
