"""MDETR_CONV_STEM_F32 routing (conv_stem_ext.py, monodetr/backbone.py, kernel_families.py) with both forms of csrc/conv_stem.hip running
on the CPU shim: with the switch off an fp32 stem behaves as before (no entry is reached); with it on conv_bn on a frozen fp32 stem takes
mdetr_conv_stem_f32 exactly once; autocast, an NCHW-contiguous image, a trainable weight, another stride or padding and relu=False stay
on the library; bf16 operands keep the bf16 entry, and the two forms' packed weights do not evict each other."""
import os

import pytest
import torch

import conv_stem_f32_cases as X
import native_emul
from gemm_bounds import assert_product_close, conv2d_f64


@pytest.fixture
def ext(monkeypatch):
    from monodetr_amd import conv_stem_ext
    raw = native_emul.lib()
    raw.mdetr_conv_stem_f32                                             # (AttributeError without the feature)
    monkeypatch.setattr(conv_stem_ext, "_backend", raw)
    monkeypatch.setattr(conv_stem_ext, "ENABLED", False)
    monkeypatch.setattr(conv_stem_ext, "ENABLED_F32", False)
    monkeypatch.setattr(conv_stem_ext, "_packed", {})
    return conv_stem_ext


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _stem(stride=2, padding=3, frozen=True):
    from monodetr_amd.monodetr.backbone import FrozenBatchNorm2d
    torch.manual_seed(3)
    conv = torch.nn.Conv2d(3, 64, 7, stride, padding, bias=False)
    with torch.no_grad():
        conv.weight.mul_(3.0)
    conv.weight.requires_grad_(not frozen)
    bn = FrozenBatchNorm2d(64)
    bn.weight.uniform_(0.5, 1.5); bn.bias.normal_(0, 0.3); bn.running_mean.normal_(0, 0.3); bn.running_var.uniform_(0.5, 2.0)
    return conv, bn


def test_supported_f32_asks_for_the_family_and_the_stem(ext, monkeypatch):
    x, w = _cl(torch.randn(1, 3, 6, 8)), torch.randn(64, 3, 7, 7)
    assert not ext.supported_f32(x, w) and not ext.supported(x, w)      # the family alone decides, also under the emulated kernel
    with pytest.raises(RuntimeError):
        ext.conv_stem(x, w, None)
    monkeypatch.setattr(ext, "ENABLED_F32", True)
    assert ext.supported_f32(x, w) and not ext.supported(x, w)          # the bf16 predicate keeps its meaning
    assert not ext.supported_f32(x.bfloat16(), w.bfloat16()) and not ext.supported_f32(x, w.bfloat16()) and not ext.supported_f32(x.double(), w.double())
    assert not ext.supported_f32(x, w, stride=(1, 1)) and not ext.supported_f32(x, w, padding=(2, 2)) and not ext.supported_f32(x, w, dilation=(2, 2))
    assert not ext.supported_f32(x, w, groups=3) and not ext.supported_f32(torch.randn(2, 3, 6, 8), w)                 # NCHW-contiguous
    assert not ext.supported_f32(_cl(torch.randn(1, 4, 6, 8)), torch.randn(64, 4, 7, 7)) and not ext.supported_f32(x, torch.randn(32, 3, 7, 7))
    assert not ext.supported_f32(x, torch.randn(64, 3, 5, 5), padding=(2, 2)) and not ext.supported_f32(_cl(torch.randn(0, 3, 6, 8)), w)
    assert not ext.supported_f32(x, w.clone().requires_grad_(True)) and not ext.supported_f32(x.clone().requires_grad_(True), w)
    # the entry's 32-bit byte offsets: B H W 12 < 2^31 (meta tensors: no memory behind them)
    meta = lambda W_: torch.empty((256, 3, 1024, W_), device="meta").contiguous(memory_format=torch.channels_last)      # noqa: E731
    monkeypatch.setattr(ext, "_backend", object())
    assert ext.supported_f32(meta(682), w) and not ext.supported_f32(meta(683), w)


def test_fp32_stem_takes_the_entry_once_with_the_switch_only(ext, monkeypatch):
    """backbone.conv_bn on a frozen fp32 conv1 + FrozenBatchNorm2d: one launch of the fp32 form with the switch on, none without; both
    routes within the fp32-accumulation bound of the folded convolution in fp64."""
    from monodetr_amd.monodetr.backbone import conv_bn
    conv, bn = _stem()
    x = _cl(torch.randn(2, 3, 9, 37) * 0.5)
    calls = X.record_launches(ext, monkeypatch)
    res = {}
    for on in (False, True):
        monkeypatch.setattr(ext, "ENABLED_F32", on)
        del calls[:]
        res[on] = conv_bn(x, conv, bn, True)
        assert calls == ([torch.float32] if on else []), calls
        assert res[on].dtype == torch.float32 and tuple(res[on].shape) == (2, 64, 5, 19)
    scale, shift = bn.affine()
    w64 = conv.weight.detach().double() * scale.double().view(-1, 1, 1, 1)
    ref = conv2d_f64(x.double(), w64, shift.double(), stride=2, padding=3).clamp(min=0)
    mag = conv2d_f64(x.double().abs(), w64.abs(), shift.double().abs(), stride=2, padding=3)
    for on in (False, True):
        # (the folded fp32 weight is one rounding of w64: 2^-24 |x||w| per product, inside the bound at K = 147)
        assert_product_close(res[on], ref, mag, X.K, "stem through conv_bn, switch %s" % on)
    assert bool((res[True] == 0).any()) and bool((res[True] > 0).any())


def test_fp32_stem_refusals_stay_on_the_library(ext, monkeypatch):
    from monodetr_amd.monodetr.backbone import conv_bn
    monkeypatch.setattr(ext, "ENABLED_F32", True)
    calls = X.record_launches(ext, monkeypatch)
    conv, bn = _stem()
    x = _cl(torch.randn(1, 3, 8, 12))
    assert conv_bn(x, conv, bn, True).shape == (1, 64, 4, 6) and calls == [torch.float32]
    del calls[:]
    with torch.autocast("cpu", dtype=torch.bfloat16):
        conv_bn(x, conv, bn, True)
    assert calls == []                                                  # autocast: the library computes in the lower precision
    assert conv_bn(x.contiguous(), conv, bn, True).shape == (1, 64, 4, 6) and calls == []            # an NCHW-contiguous image
    assert conv_bn(x, conv, bn, False).shape == (1, 64, 4, 6) and calls == []                        # relu=False: the epilogue always applies it
    trainable, bn2 = _stem(frozen=False)
    assert conv_bn(x, trainable, bn2, True).requires_grad and calls == []                            # a weight that requires grad
    assert conv_bn(x, *_stem(stride=1), True).shape == (1, 64, 8, 12) and calls == []                # stride != 2
    assert conv_bn(x, *_stem(padding=2), True).shape == (1, 64, 3, 5) and calls == []                # padding != 3
    assert conv_bn(x, conv, bn, True).shape == (1, 64, 4, 6) and calls == [torch.float32]            # ... and the stem still does


def test_bf16_operands_keep_the_bf16_entry_and_each_form_packs_once(ext, monkeypatch):
    from monodetr_amd.monodetr.backbone import conv_bn
    calls = X.record_launches(ext, monkeypatch)
    packs = []
    real, real_f32 = ext.pack_weight, ext.pack_weight_f32
    monkeypatch.setattr(ext, "pack_weight", lambda w: (packs.append("bf16"), real(w))[1])
    monkeypatch.setattr(ext, "pack_weight_f32", lambda w: (packs.append("f32"), real_f32(w))[1])
    conv, bn = _stem()
    x = _cl(torch.randn(1, 3, 8, 12))
    monkeypatch.setattr(ext, "ENABLED_F32", True)
    assert conv_bn(x.bfloat16(), conv, bn, True).dtype == torch.bfloat16 and calls == [] and packs == []        # bf16 needs ITS switch
    monkeypatch.setattr(ext, "ENABLED", True)
    monkeypatch.setattr(ext, "ENABLED_F32", False)
    assert conv_bn(x, conv, bn, True).dtype == torch.float32 and calls == [] and packs == []                    # ... and fp32 its own
    monkeypatch.setattr(ext, "ENABLED_F32", True)
    outs = []
    for _ in range(3):                                                  # alternating: conv_bn caches one folded weight per dtype
        outs.append(conv_bn(x, conv, bn, True))
        outs.append(conv_bn(x.bfloat16(), conv, bn, True))
    assert calls == [torch.float32, torch.bfloat16] * 3, calls
    assert conv.weight.dtype == torch.float32
    # conv_bn's frozen fold keeps ONE folded weight per module (a dtype change refolds), so go below it for the cache itself
    _, shift = bn.affine()
    w32 = (conv.weight.detach() * bn.affine()[0].view(-1, 1, 1, 1)).contiguous()
    w16 = w32.bfloat16()
    del packs[:]
    for _ in range(3):
        a = ext.conv_stem(x, w32, shift)
        b = ext.conv_stem(x.bfloat16(), w16, shift)
    assert packs == ["f32", "bf16"], packs                              # alternating calls do not evict each other
    assert torch.equal(a, outs[0]) and torch.equal(b, outs[1])
    with torch.no_grad():
        w32.mul_(2.0)                                                   # a new version of the same tensor packs again
    ext.conv_stem(x, w32, shift)
    ext.conv_stem(x.bfloat16(), w16, shift)
    assert packs == ["f32", "bf16", "f32"], packs
    ext.conv_stem(x, w32, None)                                         # ... and so does another shift
    assert packs[-1] == "f32" and len(packs) == 4


def test_switch_is_listed_applied_and_not_committed(monkeypatch):
    from monodetr_amd import conv_stem_ext, conv_taps_ext, kernel_families as kf
    name_ = "MDETR_CONV_STEM_F32"
    assert name_ in kf.ALL_SWITCHES and name_ in kf.AUTOTUNE_SWITCHES and name_ in kf.SWITCH_TESTS
    assert all(name_ not in fams for fams in kf.COMMITTED_SWITCHES.values())
    for pat in kf.SWITCH_TESTS[name_].split(","):
        name, stem = pat.strip().split("::")                            # every pattern names its file, and a test of that file
        assert name == "test_conv_stem_f32_gpu.py", pat
        assert "def " + stem.rstrip("*") in open(os.path.join(os.path.dirname(__file__), name)).read(), pat
    try:
        kf.apply_switches({name_})
        assert conv_stem_ext.ENABLED_F32 and not conv_stem_ext.ENABLED and not conv_taps_ext.ENABLED_F32
        kf.apply_switches({"MDETR_CONV_STEM", "MDETR_CONV_STRIDED_F32"})
        assert not conv_stem_ext.ENABLED_F32 and conv_stem_ext.ENABLED and conv_taps_ext.ENABLED_F32
    finally:
        kf.apply_switches(set())
    assert not conv_stem_ext.ENABLED_F32 and not conv_stem_ext.ENABLED
    monkeypatch.setenv(name_, "1")
    assert name_ in kf.env_switches()
