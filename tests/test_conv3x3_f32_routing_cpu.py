"""MDETR_CONV3X3_F32 routing (conv3x3_ext.py, monodetr/backbone.py, kernel_families.py) with the fp32 form of csrc/conv3x3.hip running
on the CPU shim: with the switch off fp32 tensors behave as before (`supported` false, `conv3x3` raises, no module reaches the entry);
with it on an fp32 Bottleneck and an fp32 Conv3x3 module take the entry once forward and once for the input gradient, NCHW-contiguous
and autocast calls stay on the library, and both routes lie within the fp32-accumulation bound of the fp64 value."""
import copy
import os

import pytest
import torch

import native_emul
from conftest import tune
from gemm_bounds import assert_product_close, conv2d_f64


# mdetr_conv3x3_f32_plan at B = 8: 32 output channels per workgroup everywhere (two workgroups per CU: 512 places)
PLAN_LAYER1, PLAN_LAYER2, PLAN_LAYER3, PLAN_LAYER4 = 3211, 3211, 1611, 821


class Counting:
    """The emulated library with its conv3x3 launches counted (the planners are not launches)."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("mdetr_conv3x3") or name.endswith("_plan"):
            return fn

        def counted(*a):
            self.calls.append((name, a[-3]))                            # (entry, flags)
            return fn(*a)
        return counted


@pytest.fixture
def backend(monkeypatch):
    from monodetr_amd import conv3x3_ext
    raw = native_emul.lib()
    raw.mdetr_conv3x3_f32                                               # (AttributeError without the feature)
    L = Counting(raw)
    monkeypatch.setattr(conv3x3_ext, "_backend", L)
    monkeypatch.setattr(conv3x3_ext, "ENABLED", False)
    monkeypatch.setattr(conv3x3_ext, "ENABLED_F32", False)
    tune(monkeypatch, conv3x3_f32_tile=None, conv3x3_f32_nb=None)
    return L


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def test_switch_off_fp32_tensors_behave_as_before(backend):
    from monodetr_amd import conv3x3_ext as ext
    x, w = _cl(torch.randn(1, 64, 4, 4)), torch.randn(32, 64, 3, 3)
    assert not ext.ENABLED_F32 and not ext.supported(x, w) and not ext.supported_f32(x, w)
    with pytest.raises(RuntimeError):
        ext.conv3x3(x, w)
    assert ext.supported(x.bfloat16(), w.bfloat16())
    assert backend.calls == []


def test_supported_f32_mirrors_supported(backend, monkeypatch):
    from monodetr_amd import conv3x3_ext as ext
    monkeypatch.setattr(ext, "ENABLED_F32", True)
    x, w = _cl(torch.randn(1, 64, 4, 4)), torch.randn(32, 64, 3, 3)
    assert ext.supported_f32(x, w) and not ext.supported(x, w)                     # the bf16 predicate keeps its meaning
    assert not ext.supported_f32(x.bfloat16(), w.bfloat16()) and not ext.supported_f32(x, w.bfloat16()) and not ext.supported_f32(x.double(), w.double())
    assert not ext.supported_f32(x, w, stride=(2, 2)) and not ext.supported_f32(x, w, padding=(0, 0)) and not ext.supported_f32(x, w, dilation=(2, 2))
    assert not ext.supported_f32(x, w, groups=2) and not ext.supported_f32(x.contiguous(), w)
    assert not ext.supported_f32(_cl(torch.randn(1, 48, 4, 4)), w[:, :48].contiguous()) and not ext.supported_f32(x, torch.randn(40, 64, 3, 3))
    assert not ext.supported_f32(_cl(torch.randn(0, 64, 4, 4)), w)


def _randomise(module):
    from monodetr_amd.monodetr.backbone import FrozenBatchNorm2d
    for m in module.modules():
        if isinstance(m, FrozenBatchNorm2d):
            m.weight.uniform_(0.5, 1.5); m.bias.normal_(0, 0.3); m.running_mean.normal_(0, 0.3); m.running_var.uniform_(0.5, 2.0)


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def test_fp32_bottleneck_takes_the_entry_with_the_switch_only(backend, monkeypatch):
    """backbone.conv_bn: conv2 of an fp32 channels_last bottleneck -- one launch forward, one (mirrored) for the input gradient with the
    switch on, none without; the block's output and all gradients of both routes against the block in fp64, at the stage test's bars
    (ReLU masks within rounding of zero may flip on either route)."""
    from monodetr_amd import conv3x3_ext as ext
    from monodetr_amd.monodetr.backbone import Bottleneck
    torch.manual_seed(5)
    block = Bottleneck(256, 64).to(memory_format=torch.channels_last)
    _randomise(block)
    x = _cl(torch.randn(2, 256, 6, 40))
    dy = _cl(torch.randn(2, 256, 6, 40))
    res = {}
    for on in (False, True):
        monkeypatch.setattr(ext, "ENABLED_F32", on)
        del backend.calls[:]
        xi = x.clone().requires_grad_(True)
        block.zero_grad(set_to_none=True)
        y = block(xi)
        y.backward(dy)
        assert backend.calls == ([("mdetr_conv3x3_f32", 1), ("mdetr_conv3x3_f32", 2)] if on else []), backend.calls     # ReLU forward; mirrored dx
        res[on] = [y.detach(), xi.grad] + [p.grad.clone() for p in block.parameters()]
    monkeypatch.setattr(ext, "ENABLED_F32", True)
    del backend.calls[:]
    from monodetr_amd.monodetr.backbone import conv_bn
    mid = torch.randn(2, 64, 6, 40)                                                # conv2's input, NCHW-contiguous: the library
    assert conv_bn(mid, block.conv2, block.bn2, True).shape == mid.shape and backend.calls == []
    assert conv_bn(_cl(mid), block.conv2, block.bn2, True).shape == mid.shape and backend.calls == [("mdetr_conv3x3_f32", 1)]
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


def test_fp32_conv_module_takes_the_entry_with_the_switch_only(backend, monkeypatch):
    """conv3x3_ext.Conv3x3 (the depth head's convolutions: a trainable bias) in fp32: entry calls, and y / dx of the kernel route
    element-wise within the random-case bound of fp64; dw and db (the library's / a column sum) agree with the library route."""
    from monodetr_amd import conv3x3_ext as ext
    torch.manual_seed(2)
    conv = ext.Conv3x3(64, 64, kernel_size=(3, 3), padding=1).to(memory_format=torch.channels_last)
    x, dy = _cl(torch.randn(2, 64, 7, 33) * 0.5), _cl(torch.randn(2, 64, 7, 33))
    res = {}
    for on in (False, True):
        monkeypatch.setattr(ext, "ENABLED_F32", on)
        del backend.calls[:]
        xi = x.clone().requires_grad_(True)
        conv.zero_grad(set_to_none=True)
        y = conv(xi)
        assert (type(y.grad_fn).__name__ == "_Conv3x3Backward") == on
        y.backward(dy)
        assert backend.calls == ([("mdetr_conv3x3_f32", 0), ("mdetr_conv3x3_f32", 2)] if on else []), backend.calls
        res[on] = (y.detach(), xi.grad, conv.weight.grad.clone(), conv.bias.grad.clone())
    monkeypatch.setattr(ext, "ENABLED_F32", True)
    del backend.calls[:]
    assert type(conv(x.contiguous()).grad_fn).__name__ != "_Conv3x3Backward"      # NCHW-contiguous input
    with torch.autocast("cpu", dtype=torch.bfloat16):
        assert type(conv(x).grad_fn).__name__ != "_Conv3x3Backward"
    assert type(copy.deepcopy(conv).bfloat16()(x.bfloat16()).grad_fn).__name__ != "_Conv3x3Backward" and backend.calls == []      # bf16 needs ITS switch
    x64, w64 = x.double().requires_grad_(True), conv.weight.detach().double().requires_grad_(True)
    ref = conv2d_f64(x64, w64, conv.bias.detach().double(), padding=1)
    xa, wa = x.double().abs().requires_grad_(True), w64.detach().abs().requires_grad_(True)
    mag = conv2d_f64(xa, wa, conv.bias.detach().double().abs(), padding=1)
    gx, gw = torch.autograd.grad(ref, (x64, w64), dy.double())
    mx, mw = torch.autograd.grad(mag, (xa, wa), dy.double().abs())
    for on in (False, True):
        assert_product_close(res[on][0], ref.detach(), mag.detach(), 9 * 64, "y on=%s" % on)
        assert_product_close(res[on][1], gx, mx, 9 * 64, "dx on=%s" % on)
        assert_product_close(res[on][2], gw, mw, 2 * 7 * 33, "dw on=%s" % on)
    assert torch.equal(res[True][2], res[False][2]) or _rel(res[True][2], res[False][2]) < 1e-6      # the same library call on the same operands
    assert _rel(res[True][3], res[False][3]) < 1e-6


def test_switch_is_listed_applied_and_not_committed(monkeypatch):
    from monodetr_amd import conv3x3_ext, conv_wgrad_ext, kernel_families as kf
    from monodetr_amd.monodetr import linear
    assert "MDETR_CONV3X3_F32" in kf.ALL_SWITCHES and "MDETR_CONV3X3_F32" in kf.SWITCH_TESTS
    assert all("MDETR_CONV3X3_F32" not in fams for fams in kf.COMMITTED_SWITCHES.values())
    for pat in kf.SWITCH_TESTS["MDETR_CONV3X3_F32"].split(","):
        name, stem = pat.strip().split("::")                            # every pattern names its file, and a test of that file
        assert name == "test_conv3x3_f32_gpu.py", pat
        assert "def " + stem.rstrip("*") in open(os.path.join(os.path.dirname(__file__), name)).read(), pat
    try:
        kf.apply_switches({"MDETR_CONV3X3_F32"})
        assert conv3x3_ext.ENABLED_F32 and not conv3x3_ext.ENABLED and not linear._TGEMM_F32 and not conv_wgrad_ext.ENABLED_F32
        kf.apply_switches({"MDETR_CONV3X3", "MDETR_TGEMM_F32", "MDETR_TWGRAD_F32"})
        assert not conv3x3_ext.ENABLED_F32 and conv3x3_ext.ENABLED and linear._TGEMM_F32 and conv_wgrad_ext.ENABLED_F32
    finally:
        kf.apply_switches(set())
    assert not conv3x3_ext.ENABLED_F32 and not conv3x3_ext.ENABLED
    monkeypatch.setenv("MDETR_CONV3X3_F32", "1")
    assert "MDETR_CONV3X3_F32" in kf.env_switches()


def test_conv3x3_f32_launch_geometry_for_the_resnet_stages(monkeypatch):
    """mdetr_conv3x3_f32_plan (host only) at B = 8, 384 x 1280, pinned to what choose_f32 returns: 512 places at 32 output channels per
    workgroup, 256 at 64.  100 WC + 10 GC + NB.  The bf16 kernel's MDETR_TUNE keys do not move it, and its own keys do not move the
    bf16 plan."""
    lib = native_emul.lib()
    tune(monkeypatch, conv3x3_f32_tile=None, conv3x3_f32_nb=None, conv3x3_tile=None, conv3x3_nb=None)
    plan = lambda H, W, N, B=8: lib.mdetr_conv3x3_f32_plan(B, H, W, N)       # noqa: E731
    want = {(96, 320, 64): PLAN_LAYER1, (48, 160, 128): PLAN_LAYER2, (24, 80, 256): PLAN_LAYER3, (12, 40, 512): PLAN_LAYER4}
    for (H, W, N), p in want.items():
        assert plan(H, W, N) == p, (H, W, N, plan(H, W, N))
        assert p % 10 in (1, 2) and p // 10 in (321, 161, 162, 84, 82)
    bf16 = lib.mdetr_conv3x3_plan(8, 24, 80, 256)
    tune(monkeypatch, conv3x3_tile=84, conv3x3_nb=1)
    assert plan(24, 80, 256) == PLAN_LAYER3 and lib.mdetr_conv3x3_plan(8, 24, 80, 256) == 841
    tune(monkeypatch, conv3x3_tile=None, conv3x3_nb=None, conv3x3_f32_tile=82, conv3x3_f32_nb=2)
    assert plan(24, 80, 256) == 822 and lib.mdetr_conv3x3_plan(8, 24, 80, 256) == bf16
    assert plan(24, 80, 32) == 821                                           # a forced width beyond the cap: the cap
    assert plan(0, 1, 32) < 0

