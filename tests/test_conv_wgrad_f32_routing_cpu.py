"""MDETR_CONV_WGRAD_F32 routing (conv_wgrad_ext.py, conv3x3_ext._Conv3x3.backward, kernel_families.py) with the fp32 forms of
csrc/conv3x3.hip and csrc/conv_wgrad.hip running on the CPU shim and MDETR_CONV3X3_F32 on: with the new switch off the weight gradient of
an fp32 conv3x3 is the library's; with it on it is the entry's, once, on fp32 operands; what the predicate refuses falls to the library
without an exception; a leaf weight whose strides differ from the result's gets its sum at once under chunk_sums.deferred()."""
import os
import types

import pytest
import torch

import conv_wgrad_f32_cases as X
import native_emul
from conftest import tune
from gemm_bounds import assert_product_close

WGRAD_ONLY = (False, True, False)


@pytest.fixture
def routes(monkeypatch):
    from monodetr_amd import chunk_sums, conv3x3_ext, conv_wgrad_ext
    L = native_emul.lib()
    L.mdetr_conv_wgrad_f32                                              # (AttributeError without the feature)
    for m in (conv3x3_ext, conv_wgrad_ext, chunk_sums):
        monkeypatch.setattr(m, "_backend", L)
    monkeypatch.setattr(conv3x3_ext, "ENABLED_F32", True)
    monkeypatch.setattr(conv_wgrad_ext, "ENABLED_CONV_F32", False)
    X.lift_shape_rule(conv_wgrad_ext, monkeypatch)                     # the kernel is under test here, on every shape the entry takes
    monkeypatch.setattr(chunk_sums, "ENABLED", True)
    tune(monkeypatch, conv_wgrad_wgs=None, conv3x3_f32_tile=None, conv3x3_f32_nb=None)
    return X.record_routes(conv_wgrad_ext, monkeypatch)


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


SHAPE = (2, 5, 19, 64, 32)


def _operands():
    B, H, W, C, N = SHAPE
    g = torch.Generator().manual_seed(11)
    x = _cl(torch.randn(B, C, H, W, generator=g) * 0.5)
    dy = _cl(torch.randn(B, N, H, W, generator=g))
    w = _cl(torch.randn(N, C, 3, 3, generator=g) / 24.0)
    return x, dy, w


def _backward(x, dy, w):
    from monodetr_amd import conv3x3_ext
    wr = w.clone(memory_format=torch.preserve_format).requires_grad_(True)
    conv3x3_ext.conv3x3(x, wr, None, relu=False).backward(dy)
    return wr.grad


def test_switch_off_the_library_computes_the_fp32_weight_gradient(routes):
    from monodetr_amd import conv_wgrad_ext
    x, dy, w = _operands()
    assert not conv_wgrad_ext.ENABLED_CONV_F32 and not conv_wgrad_ext.supported_f32(x, dy, 3, 1) and not conv_wgrad_ext.supported(x, dy, 3, 1)
    dw = _backward(x, dy, w)
    assert routes == [("library", WGRAD_ONLY)], routes
    B, H, W, C, N = SHAPE
    assert_product_close(dw, X.wgrad_f64(x.double(), dy.double()), X.wgrad_f64(x.double().abs(), dy.double().abs()), B * H * W, "library dW")


def test_switch_on_the_entry_computes_it_once_on_fp32_operands(routes, monkeypatch):
    from monodetr_amd import conv_wgrad_ext
    monkeypatch.setattr(conv_wgrad_ext, "ENABLED_CONV_F32", True)
    x, dy, w = _operands()
    assert conv_wgrad_ext.supported_f32(x, dy, 3, 1) and not conv_wgrad_ext.supported(x, dy, 3, 1)       # the bf16 predicate keeps its meaning
    dw = _backward(x, dy, w)
    assert routes == [("entry", torch.float32, torch.float32)], routes
    B, H, W, C, N = SHAPE
    assert dw.dtype == torch.float32 and tuple(dw.shape) == (N, C, 3, 3) and dw.stride() == (9 * C, 1, 3 * C, C)
    assert_product_close(dw, X.wgrad_f64(x.double(), dy.double()), X.wgrad_f64(x.double().abs(), dy.double().abs()), B * H * W, "entry dW")
    # a dy that arrives NCHW-contiguous is made channels_last by the backward pass before the predicate sees it: still the entry
    del routes[:]
    dw2 = _backward(x, dy.contiguous(), w)
    assert not conv_wgrad_ext.supported_f32(x, dy.contiguous(), 3, 1)
    assert routes == [("entry", torch.float32, torch.float32)] and torch.equal(dw2, dw)


def _bare_backward(x, dy, weight):
    """_Conv3x3.backward on a context of its own (the forward of these operands is not the kernel's): the weight gradient only."""
    from monodetr_amd import conv3x3_ext
    ctx = types.SimpleNamespace(saved_tensors=(x, weight, None), relu=False, relu_token=None, in_token=None, w_ihwo=None, shift_dtype=None,
                                needs_input_grad=(False, True, False, False, False, False))
    return conv3x3_ext._Conv3x3.backward(ctx, dy)[1]


def test_what_the_predicate_refuses_falls_to_the_library(routes, monkeypatch):
    from monodetr_amd import conv_wgrad_ext as ext
    monkeypatch.setattr(ext, "ENABLED_CONV_F32", True)
    x, dy, w = _operands()
    assert ext.supported_f32(x, dy, 3, 1)
    assert not ext.supported_f32(x, dy, 3, 2) and not ext.supported_f32(x, dy, 1, 1)
    assert not ext.supported_f32(x.bfloat16(), dy.bfloat16(), 3, 1) and not ext.supported_f32(x, dy.bfloat16(), 3, 1) and not ext.supported_f32(x.double(), dy.double(), 3, 1)
    assert not ext.supported_f32(x.contiguous(), dy, 3, 1) and not ext.supported_f32(x, dy.contiguous(), 3, 1)
    assert not ext.supported_f32(x[:, :32].contiguous(memory_format=torch.channels_last), dy, 3, 1)
    assert not ext.supported_f32(x, _cl(torch.randn(2, 40, 5, 19)), 3, 1) and not ext.supported_f32(x, dy[:, :, :4], 3, 1)
    # C = 32: the library, no exception
    x32 = _cl(x[:, :32])
    dw = _bare_backward(x32, dy, w[:, :32])
    assert routes == [("library", WGRAD_ONLY)] and tuple(dw.shape) == (32, 32, 3, 3)
    # a bf16 weight with fp32 activations: the entry is not asked (the library decides what it does with such operands -- here a stand-in
    # that records the call, since the CPU library raises for mixed dtypes as it would without this change)
    del routes[:]
    seen = []
    monkeypatch.setattr(torch.ops.aten, "convolution_backward", lambda *a: (seen.append(tuple(a[-1])), (None, torch.zeros_like(a[2]), None))[1])
    dw = _bare_backward(x, dy, w.bfloat16())
    assert seen == [WGRAD_ONLY] and routes == [] and dw.dtype == torch.bfloat16


def test_the_shape_rule_sends_the_measured_slower_classes_to_the_library(monkeypatch):
    """Without the tests' lift: fewer than 128 output channels (layer1) and more than 8 weight blocks (layer4) stay on the library,
    layer2's and layer3's widths take the kernel (the table at conv_wgrad_ext._F32_MIN_N)."""
    from monodetr_amd import conv_wgrad_ext as ext
    monkeypatch.setattr(ext, "_backend", native_emul.lib())
    monkeypatch.setattr(ext, "ENABLED_CONV_F32", True)
    assert (ext._F32_MIN_N, ext._F32_MAX_BLOCKS) == (128, 8)
    ok = lambda C, N: ext.supported_f32(_cl(torch.zeros(1, C, 2, 2)), _cl(torch.zeros(1, N, 2, 2)), 3, 1)       # noqa: E731
    assert not ok(64, 64) and not ok(64, 96) and ok(128, 128) and ok(256, 256) and ok(64, 1024)
    assert not ok(512, 512) and not ok(576, 256) and not ok(320, 384)


def test_a_leaf_weight_with_standard_strides_gets_its_sum_at_once(routes, monkeypatch):
    """chunk_sums.deferred(): the channels_last weight's sum is registered (AccumulateGrad keeps the tensor as it is), the NCHW-contiguous
    leaf's is computed at once (`_stolen` is false: AccumulateGrad would read it); both equal the non-deferred gradient bit for bit."""
    from monodetr_amd import chunk_sums, conv_wgrad_ext
    monkeypatch.setattr(conv_wgrad_ext, "ENABLED_CONV_F32", True)
    monkeypatch.setattr(chunk_sums, "POISON", True)
    x, dy, w = _operands()
    plain = _backward(x, dy, w)
    for weight, registered in ((w, 1), (w.contiguous(), 0)):
        assert weight.is_contiguous(memory_format=torch.channels_last) == bool(registered)
        from monodetr_amd import conv3x3_ext
        wr = weight.clone(memory_format=torch.preserve_format).requires_grad_(True)
        assert conv_wgrad_ext._stolen(wr, SHAPE[4], SHAPE[3], 3) == bool(registered)
        del routes[:]
        with chunk_sums.deferred():
            conv3x3_ext.conv3x3(x, wr, None, relu=False).backward(dy)
            assert len(chunk_sums._pending) == registered
            if not registered:
                assert not bool(wr.grad.isnan().any())
        assert routes == [("entry", torch.float32, torch.float32)] and chunk_sums._pending == []
        assert wr.grad.stride() == wr.stride() and torch.equal(wr.grad, plain)


def test_switch_is_listed_applied_and_not_committed(monkeypatch):
    from monodetr_amd import conv3x3_ext, conv_wgrad_ext, kernel_families as kf
    from monodetr_amd.monodetr import linear
    name = "MDETR_CONV_WGRAD_F32"
    assert name in kf.ALL_SWITCHES and name in kf.SWITCH_TESTS
    assert all(name not in fams for fams in kf.COMMITTED_SWITCHES.values())
    for pat in kf.SWITCH_TESTS[name].split(","):
        fname, stem = pat.strip().split("::")                           # every pattern names its file, and a test of that file
        assert fname == "test_conv_wgrad_f32_gpu.py", pat
        assert "def " + stem.rstrip("*") in open(os.path.join(os.path.dirname(__file__), fname)).read(), pat
    try:
        kf.apply_switches({name})
        assert conv_wgrad_ext.ENABLED_CONV_F32
        assert not conv_wgrad_ext.ENABLED and not conv_wgrad_ext.ENABLED_F32 and not conv3x3_ext.ENABLED_F32 and not conv3x3_ext.ENABLED and not linear._TGEMM_F32
        kf.apply_switches({"MDETR_CONV_WGRAD", "MDETR_TWGRAD_F32", "MDETR_CONV3X3_F32"})
        assert not conv_wgrad_ext.ENABLED_CONV_F32 and conv_wgrad_ext.ENABLED and conv_wgrad_ext.ENABLED_F32 and conv3x3_ext.ENABLED_F32
    finally:
        kf.apply_switches(set())
    assert not conv_wgrad_ext.ENABLED_CONV_F32 and not conv_wgrad_ext.ENABLED and not conv_wgrad_ext.ENABLED_F32 and not conv3x3_ext.ENABLED_F32
    monkeypatch.setenv(name, "1")
    assert name in kf.env_switches()
