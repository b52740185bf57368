"""MDETR_CONV_WGRAD_S2_F32 routing (conv_wgrad_ext.py, conv_taps_ext._ConvStrided.backward, kernel_families.py) with the fp32 forms of
csrc/conv_taps.hip and csrc/conv_wgrad.hip running on the CPU shim and MDETR_CONV_STRIDED_F32 on: with the new switch off the weight
gradient of an fp32 conv_strided is the library's; with it on it is the entry's, once, on fp32 operands; what the predicate refuses falls
to the library without an exception; a leaf weight whose strides differ from the result's gets its sum at once under
chunk_sums.deferred(); the shape rule without the tests' lift."""
import os
import types

import pytest
import torch

import conv_wgrad_s2_f32_cases as X
import native_emul
from conftest import tune
from gemm_bounds import assert_product_close

WGRAD_ONLY = (False, True, False)
F32 = torch.float32


@pytest.fixture
def routes(monkeypatch):
    from monodetr_amd import chunk_sums, conv_taps_ext, conv_wgrad_ext
    L = native_emul.lib()
    L.mdetr_conv_wgrad_s2_f32                                           # (AttributeError without the feature)
    for m in (conv_taps_ext, conv_wgrad_ext, chunk_sums):
        monkeypatch.setattr(m, "_backend", L)
    monkeypatch.setattr(conv_taps_ext, "ENABLED_F32", True)
    monkeypatch.setattr(conv_wgrad_ext, "ENABLED_CONV_S2_F32", False)
    monkeypatch.setattr(conv_wgrad_ext, "ENABLED_CONV_F32", False)
    X.lift_shape_rule(conv_wgrad_ext, monkeypatch)                     # the kernel is under test here, on every shape the entry takes
    monkeypatch.setattr(chunk_sums, "ENABLED", True)
    tune(monkeypatch, conv_wgrad_wgs=None, conv_taps_f32_rows=None, conv_taps_f32_nb=None, conv_taps_split=None)
    return X.record_routes(conv_wgrad_ext, monkeypatch)


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


SHAPE = (2, 6, 19, 64, 32)                                             # (B, H, W, C, N): a 3 x 10 output map


def _operands():
    B, H, W, C, N = SHAPE
    OH, OW = X.out_hw(H, W)
    g = torch.Generator().manual_seed(13)
    x = _cl(torch.randn(B, C, H, W, generator=g) * 0.5)
    dy = _cl(torch.randn(B, N, OH, OW, generator=g))
    w = _cl(torch.randn(N, C, 3, 3, generator=g) / 24.0)
    return x, dy, w


def _backward(x, dy, w):
    from monodetr_amd import conv_taps_ext
    wr = w.clone(memory_format=torch.preserve_format).requires_grad_(True)
    conv_taps_ext.conv_strided(x, wr, None, relu=False).backward(dy)
    return wr.grad


def _close(dw, x, dy, what):
    B, H, W, C, N = SHAPE
    OH, OW = X.out_hw(H, W)
    assert_product_close(dw, X.wgrad_f64(x.double(), dy.double()), X.wgrad_f64(x.double().abs(), dy.double().abs()), B * OH * OW, what)


def test_switch_off_the_library_computes_the_fp32_strided_weight_gradient(routes):
    from monodetr_amd import conv_wgrad_ext as ext
    x, dy, w = _operands()
    assert not ext.ENABLED_CONV_S2_F32 and not ext.supported_f32_s2(x, dy) and not ext.supported_f32(x, dy, 3, 2) and not ext.supported(x, dy, 3, 2)
    dw = _backward(x, dy, w)
    assert routes == [("library", WGRAD_ONLY)], routes
    _close(dw, x, dy, "library dW")


def test_switch_on_the_entry_computes_it_once_on_fp32_operands(routes, monkeypatch):
    from monodetr_amd import conv_wgrad_ext as ext
    monkeypatch.setattr(ext, "ENABLED_CONV_S2_F32", True)
    x, dy, w = _operands()
    assert ext.supported_f32_s2(x, dy) and not ext.supported_f32(x, dy, 3, 2) and not ext.supported(x, dy, 3, 2)     # the other predicates keep their meaning
    dw = _backward(x, dy, w)
    assert routes == [("entry", F32, F32)], routes
    B, H, W, C, N = SHAPE
    assert dw.dtype == F32 and tuple(dw.shape) == (N, C, 3, 3) and dw.stride() == (9 * C, 1, 3 * C, C)
    _close(dw, x, dy, "entry dW")
    # a dy that arrives NCHW-contiguous is made channels_last by the backward pass before the predicate sees it: still the entry
    del routes[:]
    dw2 = _backward(x, dy.contiguous(), w)
    assert not ext.supported_f32_s2(x, dy.contiguous())
    assert routes == [("entry", F32, F32)] and torch.equal(dw2, dw)
    # the stride-1 family alone does not reach the strided convolutions
    monkeypatch.setattr(ext, "ENABLED_CONV_S2_F32", False)
    monkeypatch.setattr(ext, "ENABLED_CONV_F32", True)
    del routes[:]
    _backward(x, dy, w)
    assert routes == [("library", WGRAD_ONLY)], routes


def test_a_convolution_whose_forward_stays_on_the_library_still_takes_the_entry(routes, monkeypatch):
    """layer3.0.conv2's class: C = 256 is beyond conv_taps_ext._F32_FWD_MAX_C, so the forward pass inside _ConvStrided is the library's
    (no entry of csrc/conv_taps.hip runs forward); the weight gradient is the kernel's all the same."""
    from monodetr_amd import conv_taps_ext, conv_wgrad_ext as ext
    monkeypatch.setattr(ext, "ENABLED_CONV_S2_F32", True)
    g = torch.Generator().manual_seed(14)
    x = _cl(torch.randn(1, 256, 4, 5, generator=g) * 0.5)
    dy = _cl(torch.randn(1, 64, 2, 3, generator=g))
    w = _cl(torch.randn(64, 256, 3, 3, generator=g) / 48.0)
    assert conv_taps_ext.supported_f32(x, w) and not conv_taps_ext._fwd_on_kernel(x)
    dw = _backward(x, dy, w)
    assert routes == [("entry", F32, F32)], routes
    assert_product_close(dw, X.wgrad_f64(x.double(), dy.double()), X.wgrad_f64(x.double().abs(), dy.double().abs()), 6, "entry dW behind a library forward")


def _bare_backward(x, dy, weight):
    """_ConvStrided.backward on a context of its own (the forward of these operands is not the kernel's): the weight gradient only."""
    from monodetr_amd import conv_taps_ext
    ctx = types.SimpleNamespace(saved_tensors=(x, weight, None), relu=False, relu_token=None, w_ihwo=None, shift_dtype=None,
                                needs_input_grad=(False, True, False, False, False))
    return conv_taps_ext._ConvStrided.backward(ctx, dy)[1]


def test_what_the_predicate_refuses_falls_to_the_library(routes, monkeypatch):
    from monodetr_amd import conv_wgrad_ext as ext
    monkeypatch.setattr(ext, "ENABLED_CONV_S2_F32", True)
    x, dy, w = _operands()
    B, H, W, C, N = SHAPE
    assert ext.supported_f32_s2(x, dy)
    assert not ext.supported_f32_s2(x.bfloat16(), dy.bfloat16()) and not ext.supported_f32_s2(x, dy.bfloat16()) and not ext.supported_f32_s2(x.double(), dy.double())
    assert not ext.supported_f32_s2(x.contiguous(), dy) and not ext.supported_f32_s2(x, dy.contiguous())
    assert not ext.supported_f32_s2(_cl(x[:, :32]), dy) and not ext.supported_f32_s2(x, _cl(torch.randn(2, 40, 3, 10)))
    assert not ext.supported_f32_s2(x, _cl(dy[:, :, :2])) and not ext.supported_f32_s2(x, _cl(torch.randn(2, 32, 6, 19))) and not ext.supported_f32_s2(x, _cl(dy[:1]))
    big = torch.empty((8, 64, 1024, 1024), device="meta").contiguous(memory_format=torch.channels_last)
    assert big.numel() == 1 << 29 and not ext.supported_f32_s2(big, torch.empty((8, 32, 512, 512), device="meta").contiguous(memory_format=torch.channels_last))
    # C = 32: the library, no exception
    dw = _bare_backward(_cl(x[:, :32]), dy, _cl(w[:, :32]))
    assert routes == [("library", WGRAD_ONLY)] and tuple(dw.shape) == (N, 32, 3, 3)
    # an NCHW-contiguous x (the forward pass would not have taken it; a context of its own): the library
    del routes[:]
    dw = _bare_backward(x.contiguous(), dy, w)
    assert routes == [("library", WGRAD_ONLY)]
    _close(dw, x, dy, "library dW of an NCHW-contiguous x")
    # the remaining cases through a stand-in that records the call (the CPU library raises for what it is handed here, as it would
    # without this change): an output map that does not belong to the input, bf16 operands, a bf16 weight with fp32 activations
    # (the bf16 predicate is held off: under the emulated library it would hand bf16 operands to the bf16 kernel, which is not the question here)
    seen = []
    monkeypatch.setattr(ext, "supported", lambda *a: False)
    monkeypatch.setattr(torch.ops.aten, "convolution_backward", lambda *a: (seen.append(tuple(a[-1])), (None, torch.zeros_like(a[2]), None))[1])
    for xx, dd, ww in ((x, _cl(dy[:, :, :2]), w), (x.bfloat16(), dy.bfloat16(), w.bfloat16()), (x, dy, w.bfloat16())):
        del routes[:], seen[:]
        dw = _bare_backward(xx, dd, ww)
        assert seen == [WGRAD_ONLY] and routes == [] and dw.dtype == ww.dtype


def test_the_shape_rule_has_the_values_written_in_conv_wgrad_ext(monkeypatch):
    """Without the tests' lift (the table at conv_wgrad_ext._F32_S2_MIN_N): fewer than 128 output channels stay on the library; the
    128 -> 128 and 256 -> 256 sites (4 and 16 blocks of 64 n x 64 c) take the kernel; 512 -> 512 (64 blocks) stays on the library."""
    from monodetr_amd import conv_wgrad_ext as ext
    monkeypatch.setattr(ext, "_backend", native_emul.lib())
    monkeypatch.setattr(ext, "ENABLED_CONV_S2_F32", True)
    assert (ext._F32_S2_MIN_N, ext._F32_S2_MAX_BLOCKS) == (128, 16)
    ok = lambda C, N: ext.supported_f32_s2(_cl(torch.zeros(1, C, 4, 4)), _cl(torch.zeros(1, N, 2, 2)))       # noqa: E731
    assert not ok(64, 64) and not ok(64, 96) and ok(128, 128) and ok(256, 256) and ok(64, 1024)
    assert not ok(512, 512) and not ok(320, 256) and not ok(256, 320)


def test_a_leaf_weight_with_standard_strides_gets_its_sum_at_once(routes, monkeypatch):
    """chunk_sums.deferred(): the channels_last weight's sum is registered (AccumulateGrad keeps the tensor as it is), the NCHW-contiguous
    leaf's is computed at once (`_stolen` is false: AccumulateGrad would read it); both equal the non-deferred gradient bit for bit."""
    from monodetr_amd import chunk_sums, conv_taps_ext, conv_wgrad_ext
    monkeypatch.setattr(conv_wgrad_ext, "ENABLED_CONV_S2_F32", True)
    monkeypatch.setattr(chunk_sums, "POISON", True)
    x, dy, w = _operands()
    plain = _backward(x, dy, w)
    for weight, registered in ((w, 1), (w.contiguous(), 0)):
        assert weight.is_contiguous(memory_format=torch.channels_last) == bool(registered)
        wr = weight.clone(memory_format=torch.preserve_format).requires_grad_(True)
        assert conv_wgrad_ext._stolen(wr, SHAPE[4], SHAPE[3], 3) == bool(registered)
        del routes[:]
        with chunk_sums.deferred():
            conv_taps_ext.conv_strided(x, wr, None, relu=False).backward(dy)
            assert len(chunk_sums._pending) == registered
            if not registered:
                assert not bool(wr.grad.isnan().any())
        assert routes == [("entry", F32, F32)] and chunk_sums._pending == []
        assert wr.grad.stride() == wr.stride() and torch.equal(wr.grad, plain)


def test_switch_is_listed_applied_and_not_committed(monkeypatch):
    from monodetr_amd import conv_taps_ext, conv_wgrad_ext, kernel_families as kf
    name = "MDETR_CONV_WGRAD_S2_F32"
    assert name in kf.ALL_SWITCHES and name == kf.AUTOTUNE_SWITCHES[-1] and name in kf.SWITCH_TESTS
    assert all(name not in fams for fams in kf.COMMITTED_SWITCHES.values())
    for pat in kf.SWITCH_TESTS[name].split(","):
        fname, stem = pat.strip().split("::")                           # every pattern names its file, and a test of that file
        assert fname == "test_conv_wgrad_s2_f32_gpu.py", pat
        assert "def " + stem.rstrip("*") in open(os.path.join(os.path.dirname(__file__), fname)).read(), pat
    try:
        kf.apply_switches({name})
        assert conv_wgrad_ext.ENABLED_CONV_S2_F32
        assert not conv_wgrad_ext.ENABLED and not conv_wgrad_ext.ENABLED_F32 and not conv_wgrad_ext.ENABLED_CONV_F32 and not conv_taps_ext.ENABLED_F32
        kf.apply_switches({"MDETR_CONV_WGRAD", "MDETR_CONV_WGRAD_F32", "MDETR_CONV_STRIDED_F32"})
        assert not conv_wgrad_ext.ENABLED_CONV_S2_F32 and conv_wgrad_ext.ENABLED and conv_wgrad_ext.ENABLED_CONV_F32 and conv_taps_ext.ENABLED_F32
    finally:
        kf.apply_switches(set())
    assert not conv_wgrad_ext.ENABLED_CONV_S2_F32 and not conv_wgrad_ext.ENABLED_CONV_F32 and not conv_taps_ext.ENABLED_F32
    monkeypatch.setenv(name, "1")
    assert name in kf.env_switches()
