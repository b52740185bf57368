"""MDETR_TWGRAD_F32 routing (monodetr/linear.py, conv_wgrad_ext.py, kernel_families.py) with the fp32 form of csrc/twgrad.hip running on
the CPU shim: fp32 layers above small_wgrad's rows take mdetr_token_wgrad_f32 for their weight + bias gradient with the switch on
(calls counted on the backend) and the library route with it off; both routes lie within the fp32-accumulation bound
(tests/gemm_bounds.py) of the fp64 value; bf16 layers, MDETR_TGEMM_F32 alone, short rows and the deferred chunk sums behave as
before."""
import os

import pytest
import torch

import native_emul
from gemm_bounds import assert_product_close


class Counting:
    """The emulated library with its token-GEMM and token weight-gradient entries counted (the *_chunks planners are not launches)."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not (name.startswith("mdetr_tgemm") or name.startswith("mdetr_token_wgrad")) or name.endswith("_chunks"):
            return fn

        def counted(*a):
            self.calls.append(name)
            return fn(*a)
        return counted

    def count(self, name):
        return sum(1 for c in self.calls if c == name)


@pytest.fixture
def backend(monkeypatch):
    from monodetr_amd import bias_act_ext, chunk_sums, conv_wgrad_ext, small_wgrad_ext, tgemm_ext
    from monodetr_amd.monodetr import linear
    raw = native_emul.lib()
    raw.mdetr_token_wgrad_f32                                           # (AttributeError without the feature)
    L = Counting(raw)
    monkeypatch.setattr(tgemm_ext, "_backend", L)
    monkeypatch.setattr(conv_wgrad_ext, "_backend", L)
    monkeypatch.setattr(bias_act_ext, "_backend", raw)
    monkeypatch.setattr(small_wgrad_ext, "ENABLED", False)
    monkeypatch.setattr(chunk_sums, "ENABLED", False)
    monkeypatch.setattr(conv_wgrad_ext, "ENABLED", False)
    monkeypatch.setattr(conv_wgrad_ext, "ENABLED_F32", False)
    for flag in ("_TGEMM", "_TGEMM_F32", "_PREMASK", "_GEMM_RELU"):
        monkeypatch.setattr(linear, flag, False)
    return L


def _switch(monkeypatch, on):
    from monodetr_amd import conv_wgrad_ext
    monkeypatch.setattr(conv_wgrad_ext, "ENABLED_F32", on)


def _check_grads(dw, db, x2, dy2, what):
    x64, dy64 = x2.double(), dy2.double()
    T = x2.shape[0]
    assert dw.dtype == torch.float32 and db.dtype == torch.float32
    assert_product_close(dw.reshape(dy2.shape[1], x2.shape[1]), dy64.t() @ x64, dy64.abs().t() @ x64.abs(), T, what + " dW")
    assert_product_close(db, dy64.sum(0), dy64.abs().sum(0), T, what + " db")


T, K, N = 8400, 64, 72                                                  # above small_wgrad_ext.MAX_ROWS, N > 64


def test_linear_takes_the_kernel_with_the_switch_and_the_library_without(backend, monkeypatch):
    from monodetr_amd.monodetr import linear
    torch.manual_seed(3)
    lin = linear.Linear(K, N)
    x = (torch.randn(3, T // 3, K) * 0.5).requires_grad_(True)
    proj = torch.randn(3, T // 3, N)
    for on in (False, True):
        _switch(monkeypatch, on)
        backend.calls.clear()
        x.grad = lin.weight.grad = lin.bias.grad = None
        (lin(x) * proj).sum().backward()
        assert backend.calls == (["mdetr_token_wgrad_f32"] if on else []), backend.calls      # ONE launch for dW and db; never without
        _check_grads(lin.weight.grad, lin.bias.grad, x.detach().view(T, K), proj.view(T, N), "Linear on=%s" % on)


def test_pointwise_conv_takes_the_kernel_with_the_switch(backend, monkeypatch):
    from monodetr_amd.monodetr import linear
    torch.manual_seed(4)
    B, H, W = 2, 60, 70                                                  # 8 400 tokens
    conv = linear.PointwiseConv2d(K, N, 1).to(memory_format=torch.channels_last)
    x = (torch.randn(B, K, H, W) * 0.5).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    proj = torch.randn(B, N, H, W).contiguous(memory_format=torch.channels_last)
    for on in (False, True):
        _switch(monkeypatch, on)
        backend.calls.clear()
        x.grad = conv.weight.grad = conv.bias.grad = None
        (conv(x) * proj).sum().backward()
        assert backend.calls == (["mdetr_token_wgrad_f32"] if on else []), backend.calls
        _check_grads(conv.weight.grad, conv.bias.grad, x.detach().permute(0, 2, 3, 1).reshape(-1, K), proj.permute(0, 2, 3, 1).reshape(-1, N),
                     "PointwiseConv2d on=%s" % on)


def test_bf16_modules_and_the_other_switches_make_the_calls_they_made(backend, monkeypatch):
    """bf16 layers never reach the fp32 entry (and reach the bf16 one exactly as before: with the emulated backend in place);
    MDETR_TGEMM_F32 alone makes no token_wgrad_f32 call; both fp32 switches together make three kernel calls per layer."""
    from monodetr_amd.monodetr import linear
    torch.manual_seed(7)
    lin16, lin32 = linear.Linear(K, N).to(torch.bfloat16), linear.Linear(K, N)
    x16 = (torch.randn(T, K) * 0.5).to(torch.bfloat16).requires_grad_(True)
    x32 = (torch.randn(T, K) * 0.5).requires_grad_(True)
    for tgemm_on, twgrad_on in ((False, False), (True, False), (False, True), (True, True)):
        monkeypatch.setattr(linear, "_TGEMM_F32", tgemm_on)
        _switch(monkeypatch, twgrad_on)
        backend.calls.clear()
        (lin16(x16).float() * 2.0).sum().backward()
        assert backend.calls == ["mdetr_token_wgrad"], backend.calls                            # (the emulated backend stands for MDETR_CONV_WGRAD)
        backend.calls.clear()
        (lin32(x32) * 2.0).sum().backward()
        want = (["mdetr_tgemm_f32", "mdetr_tgemm_f32"] if tgemm_on else []) + (["mdetr_token_wgrad_f32"] if twgrad_on else [])
        assert backend.calls == want, (tgemm_on, twgrad_on, backend.calls)


def test_mixed_dtypes_keep_the_library_route(backend, monkeypatch):
    from monodetr_amd import conv_wgrad_ext
    from monodetr_amd.monodetr import linear
    _switch(monkeypatch, True)
    x, dy = torch.randn(T, K), torch.randn(T, N)
    assert conv_wgrad_ext.token_supported_f32(x, dy)
    assert not conv_wgrad_ext.token_supported_f32(x.bfloat16(), dy) and not conv_wgrad_ext.token_supported_f32(x, dy.bfloat16())
    assert not conv_wgrad_ext.token_supported_f32(x[:, :60], dy) and not conv_wgrad_ext.token_supported_f32(x[:, 8:], dy)      # width, contiguity
    w16 = torch.zeros(N, K, dtype=torch.bfloat16)
    backend.calls.clear()
    dw, db = linear._weight_bias_grads(x, dy, w16, True, True)           # fp32 operands, a bf16 weight (autocast's pairing): the library
    assert backend.calls == [] and dw.dtype == torch.bfloat16
    _switch(monkeypatch, False)
    assert not conv_wgrad_ext.token_supported_f32(x, dy)


def test_rows_up_to_the_recorded_threshold_keep_small_wgrad(backend, monkeypatch):
    """`linear._TWGRAD_F32_MIN_ROWS`: the decoder's 4 400 rows and small_wgrad's last row count stay with csrc/small_wgrad.hip; the
    first row count above takes the kernel; narrow outputs (N <= 64) keep small_wgrad's precedence at any row count it takes."""
    from monodetr_amd import small_wgrad_ext
    from monodetr_amd.monodetr import linear
    assert linear._TWGRAD_F32_MIN_ROWS == small_wgrad_ext.MAX_ROWS + 1 == 8193
    _switch(monkeypatch, True)
    monkeypatch.setattr(small_wgrad_ext, "ENABLED", True)
    monkeypatch.setattr(small_wgrad_ext, "_backend", native_emul.lib())
    small = []
    real = small_wgrad_ext.small_wgrad
    monkeypatch.setattr(small_wgrad_ext, "small_wgrad", lambda *a, **k: (small.append(a[0].shape[0]), real(*a, **k))[1])
    g = torch.Generator().manual_seed(5)
    for rows, n, kernel in ((4400, 72, False), (8192, 72, False), (8193, 72, True), (8400, 64, False)):
        x, dy = torch.randn(rows, 64, generator=g) * 0.5, torch.randn(rows, n, generator=g)
        backend.calls.clear()
        del small[:]
        dw, db = linear._weight_bias_grads(x, dy, torch.zeros(n, 64), True, True)
        assert backend.calls == (["mdetr_token_wgrad_f32"] if kernel else []), (rows, n, backend.calls)
        assert small == ([] if kernel else [rows]), (rows, n, small)
        _check_grads(dw, db, x, dy, "rows=%d N=%d" % (rows, n))


def test_deferred_chunk_sums_give_the_same_bits(backend, monkeypatch):
    """Inside chunk_sums.deferred() (the emulated chunk-sum kernel substituted) the fp32 gradients are registered and arrive with the
    flush: bit for bit the sums launched at once."""
    from monodetr_amd import chunk_sums
    from monodetr_amd.monodetr import linear
    _switch(monkeypatch, True)
    monkeypatch.setattr(chunk_sums, "_backend", native_emul.lib())
    monkeypatch.setattr(chunk_sums, "ENABLED", True)
    torch.manual_seed(9)
    lin = linear.Linear(K, N)
    x = (torch.randn(T, K) * 0.5).requires_grad_(True)
    proj = torch.randn(T, N)
    got = {}
    for deferred in (False, True):
        lin.weight.grad = lin.bias.grad = x.grad = None
        backend.calls.clear()
        if deferred:
            with chunk_sums.deferred(lin):
                (lin(x) * proj).sum().backward()
                assert len(chunk_sums._pending) == 1                      # dW and db: one registered sum
        else:
            (lin(x) * proj).sum().backward()
            assert not chunk_sums._pending
        assert backend.calls == ["mdetr_token_wgrad_f32"]
        got[deferred] = (lin.weight.grad.clone(), lin.bias.grad.clone())
    assert torch.equal(got[True][0], got[False][0]) and torch.equal(got[True][1], got[False][1])
    _check_grads(got[True][0], got[True][1], x.detach(), proj, "deferred")


def test_switch_is_listed_applied_and_not_committed(monkeypatch):
    from monodetr_amd import conv_wgrad_ext, kernel_families as kf
    from monodetr_amd.monodetr import linear
    assert "MDETR_TWGRAD_F32" in kf.ALL_SWITCHES and "MDETR_TWGRAD_F32" in kf.SWITCH_TESTS
    assert all("MDETR_TWGRAD_F32" not in fams for fams in kf.COMMITTED_SWITCHES.values())
    for pat in kf.SWITCH_TESTS["MDETR_TWGRAD_F32"].split(","):
        name, stem = pat.strip().split("::")                            # every pattern names its file, and a test of that file
        assert name == "test_twgrad_f32_gpu.py", pat
        assert "def " + stem.rstrip("*") in open(os.path.join(os.path.dirname(__file__), name)).read(), pat
    try:
        kf.apply_switches({"MDETR_TWGRAD_F32"})
        assert conv_wgrad_ext.ENABLED_F32 and not conv_wgrad_ext.ENABLED and not linear._TGEMM_F32
        kf.apply_switches({"MDETR_TGEMM_F32", "MDETR_CONV_WGRAD"})
        assert not conv_wgrad_ext.ENABLED_F32 and conv_wgrad_ext.ENABLED and linear._TGEMM_F32
    finally:
        kf.apply_switches(set())
    assert not conv_wgrad_ext.ENABLED_F32 and not conv_wgrad_ext.ENABLED and not linear._TGEMM_F32
    monkeypatch.setenv("MDETR_TWGRAD_F32", "1")
    assert "MDETR_TWGRAD_F32" in kf.env_switches()
