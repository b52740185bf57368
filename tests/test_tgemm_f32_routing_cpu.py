"""MDETR_TGEMM_F32 routing (monodetr/linear.py, kernel_families.py) with csrc/tgemm.hip's fp32 form running on the CPU shim: fp32
modules take the kernel with the switch on (calls counted on the backend) and the library with it off; outputs and input gradients
of both routes lie within the fp32-accumulation bound (tests/gemm_bounds.py) of the fp64 value of the same fp32 operands; bf16 modules
and the other switches are untouched."""
import pytest
import torch
import torch.nn.functional as F

import native_emul
from gemm_bounds import assert_product_close


class Counting:
    """The emulated library with its token-GEMM entries counted."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("mdetr_tgemm"):
            return fn

        def counted(*a):
            self.calls.append(name)
            return fn(*a)
        return counted

    def count(self, name):
        return sum(1 for c in self.calls if c == name)


@pytest.fixture
def backend(monkeypatch):
    from monodetr_amd import bias_act_ext, small_wgrad_ext, tgemm_ext
    from monodetr_amd.monodetr import linear
    L = Counting(native_emul.lib())
    monkeypatch.setattr(tgemm_ext, "_backend", L)
    monkeypatch.setattr(bias_act_ext, "_backend", native_emul.lib())
    monkeypatch.setattr(small_wgrad_ext, "ENABLED", False)            # (weight gradients: their present route, the plain products here)
    for flag in ("_TGEMM", "_TGEMM_F32", "_PREMASK", "_GEMM_RELU"):
        monkeypatch.setattr(linear, flag, False)
    monkeypatch.setattr(linear, "_F32_NN_MIN_TOKENS", 0)              # (the row rule of the fp32 input gradients has a test of its own below)
    return L


def _switch(monkeypatch, on):
    from monodetr_amd.monodetr import linear
    monkeypatch.setattr(linear, "_TGEMM_F32", on)


def _close(got, a64, w64_kn, K, bias=None, res=None, relu=False, scale=1.0, keep=None, what=""):
    """got against the fp64 value scale * [keep] relu(a w + bias + res), within assert_product_close's bound (scaled alike)."""
    ref = a64 @ w64_kn
    mag = a64.abs() @ w64_kn.abs()
    if bias is not None:
        ref, mag = ref + bias.double(), mag + bias.double().abs()
    if res is not None:
        ref, mag = ref + res.double(), mag + res.double().abs()
    if relu:
        ref = ref.clamp(min=0)
    if keep is not None:
        ref, mag = ref * keep, mag * keep
    assert_product_close(got.reshape(ref.shape), ref * scale, mag * scale, K, what)


def test_linear_takes_the_kernel_with_the_switch_and_the_library_without(backend, monkeypatch):
    from monodetr_amd.monodetr import linear
    torch.manual_seed(3)
    T, K, N = 4200, 64, 72
    lin = linear.Linear(K, N)
    x = (torch.randn(3, T // 3, K) * 0.5).requires_grad_(True)
    proj = torch.randn(3, T // 3, N)
    grads = {}
    for on in (False, True):
        _switch(monkeypatch, on)
        backend.calls.clear()
        x.grad = lin.weight.grad = lin.bias.grad = None
        y = lin(x)
        (y * proj).sum().backward()
        assert y.dtype == torch.float32
        # forward NT + input gradient NN through the kernel; the weight / bias gradients keep their route
        assert backend.calls == (["mdetr_tgemm_f32", "mdetr_tgemm_f32"] if on else []), backend.calls
        _close(y.detach(), x.detach().double().view(T, K), lin.weight.detach().double().t(), K, lin.bias.detach(), what="forward on=%s" % on)
        _close(x.grad, proj.double().view(T, N), lin.weight.detach().double(), N, what="input gradient on=%s" % on)
        grads[on] = (lin.weight.grad.clone(), lin.bias.grad.clone())
    assert torch.equal(grads[True][0], grads[False][0]) and torch.equal(grads[True][1], grads[False][1])     # same operands, same route


def test_pointwise_conv_takes_the_kernel_with_the_switch(backend, monkeypatch):
    from monodetr_amd.monodetr import linear
    torch.manual_seed(4)
    B, C, H, W, N = 2, 64, 48, 48, 72
    conv = linear.PointwiseConv2d(C, N, 1).to(memory_format=torch.channels_last)
    x = (torch.randn(B, C, H, W) * 0.5).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    proj = torch.randn(B, N, H, W).contiguous(memory_format=torch.channels_last)
    x2 = x.detach().permute(0, 2, 3, 1).reshape(-1, C).double()
    w2 = conv.weight.detach().reshape(N, C).double()
    for on in (False, True):
        _switch(monkeypatch, on)
        backend.calls.clear()
        x.grad = None
        y = conv(x)
        (y * proj).sum().backward()
        assert backend.count("mdetr_tgemm_f32") == (2 if on else 0), backend.calls
        _close(y.detach().permute(0, 2, 3, 1), x2, w2.t(), C, conv.bias.detach(), what="forward on=%s" % on)
        _close(x.grad.permute(0, 2, 3, 1), proj.permute(0, 2, 3, 1).reshape(-1, N).double(), w2, N, what="input gradient on=%s" % on)


def test_ffn_hidden_runs_relu_and_dropout_in_the_fp32_epilogue(backend, monkeypatch):
    """The two routes draw different dropout decisions (the framework's generator against the kernel's stateless hash), so each is
    held to the fp64 value under ITS OWN decisions (read off its output), and the routes to each other with the dropout off."""
    from monodetr_amd.monodetr import linear
    torch.manual_seed(0)
    K, N = 64, 72
    lin = linear.Linear(K, N)
    x = (torch.randn(2, 2100, K) * 0.5).requires_grad_(True)
    a64, w64 = x.detach().double().view(-1, K), lin.weight.detach().double()
    for training in (True, False):
        drop = torch.nn.Dropout(0.25).train(training)
        scale = 1.0 / 0.75 if training else 1.0
        for skip in (False, True):
            for on in (False, True):
                _switch(monkeypatch, on)
                backend.calls.clear()
                out = linear.ffn_hidden(x, lin, drop, skip=skip)
                h = out[0] if skip else out
                assert backend.count("mdetr_tgemm_f32") == (1 if on else 0), backend.calls     # ONE launch: bias + ReLU (+ Dropout)
                pre = a64 @ w64.t() + lin.bias.detach().double()
                keep = (h.detach().view(-1, N) != 0).double()
                # (an element is zero because it was dropped or because it was not positive: `keep` zeroes the fp64 value for both)
                assert bool((pre[keep == 0] <= 1e-5).all()) or training
                frac = (h != 0).float().mean().item()
                assert (0.3 < frac < 0.45) if training else (0.4 < frac < 0.6)
                _close(h.detach(), a64, w64.t(), K, lin.bias.detach(), relu=True, scale=scale, keep=keep, what="hidden on=%s skip=%s" % (on, skip))
                dy = torch.linspace(-1, 1, h.numel()).view_as(h)
                gx = torch.autograd.grad((h * dy).sum() + ((out[1] * 2.0).sum() if skip else 0.0), x)[0]
                act = (h.detach().view(-1, N) > 0).double() * scale                             # the route's own mask
                _close(gx, dy.double().view(-1, N) * act, w64, N, res=(torch.full_like(a64, 2.0) if skip else None),
                       what="input gradient on=%s skip=%s" % (on, skip))
                if on:
                    assert backend.count("mdetr_tgemm_f32") == 2                                  # ... and the input gradient (the skip's gradient inside)


def test_pointwise_conv_residual_relu_in_fp32(backend, monkeypatch):
    from monodetr_amd.monodetr import linear
    torch.manual_seed(5)
    B, C, H, W, N = 2, 16, 48, 48, 64
    w = (torch.randn(N, C, 1, 1) * 0.1).requires_grad_(True)
    b = torch.randn(N)
    x = (torch.randn(B, C, H, W) * 0.5).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    idn = torch.randn(B, N, H, W).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    dy = torch.randn(B, N, H, W).contiguous(memory_format=torch.channels_last)
    x2, r2, w2 = x.detach().permute(0, 2, 3, 1).reshape(-1, C).double(), idn.detach().permute(0, 2, 3, 1).reshape(-1, N).double(), w.detach().view(N, C).double()
    _switch(monkeypatch, False)
    assert not linear.pointwise_residual_relu_eligible(x, w, b, idn)                           # the library route: conv, add, ReLU
    outs = {}
    for on in (False, True):
        _switch(monkeypatch, on)
        backend.calls.clear()
        x.grad = idn.grad = w.grad = None
        if on:
            assert linear.pointwise_residual_relu_eligible(x, w, b, idn)
            assert not linear.pointwise_residual_relu_eligible(x, w.bfloat16(), b, idn)       # one dtype throughout
            y = linear.pointwise_conv_residual_relu(x, w, b, idn)
        else:
            y = F.relu(F.conv2d(x, w, b) + idn)
        (y * dy).sum().backward()
        assert backend.calls == (["mdetr_tgemm_f32", "mdetr_tgemm_f32"] if on else []), backend.calls
        _close(y.detach().permute(0, 2, 3, 1), x2, w2.t(), C, b, r2, relu=True, what="forward on=%s" % on)
        g = (dy * (y.detach() > 0)).permute(0, 2, 3, 1).reshape(-1, N).double()              # the route's own mask
        _close(x.grad.permute(0, 2, 3, 1), g, w2, N, what="input gradient on=%s" % on)
        assert torch.equal(idn.grad, dy * (y.detach() > 0))
        outs[on] = w.grad.clone()
    assert float((outs[True] - outs[False]).abs().max()) <= 1e-4 * float(outs[False].abs().max())     # (masks may differ where y ~ 0)


def test_premask_with_fp32_operands_takes_the_fp32_masked_form(backend, monkeypatch):
    """MDETR_RELU_PREMASK + MDETR_TGEMM_F32: the consumer's input gradient applies the producer's ReLU mask inside
    mdetr_tgemm_f32_masked; without the fp32 switch the producer keeps its own pass and nothing is premasked."""
    from monodetr_amd.monodetr import linear
    torch.manual_seed(6)
    T, K, N = 4200, 64, 72
    w = (torch.randn(N, K) * 0.1).requires_grad_(True)
    src = torch.randn(T, K)
    dy = torch.randn(T, N)
    monkeypatch.setattr(linear, "_PREMASK", True)
    res = {}
    for on in (False, True):
        _switch(monkeypatch, on)
        backend.calls.clear()
        x = F.relu(src).requires_grad_(True)                                                    # a ReLU output (zeros and positives)
        token = linear.ReluToken()
        y, xs = linear.token_linear_skip(x, w, None, relu_token=token)
        ((y * dy).sum() + (xs * 2.0).sum()).backward()
        assert token.premasked == on
        assert backend.count("mdetr_tgemm_f32_masked") == (1 if on else 0), backend.calls
        res[on] = x.grad.clone()
    full = dy.double() @ w.detach().double() + 2.0
    keep = (src > 0).double()
    assert bool((res[True][src <= 0] == 0).all())
    assert_product_close(res[True], full * keep, (dy.double().abs() @ w.detach().double().abs() + 2.0) * keep, N, "premasked input gradient")
    assert_product_close(res[False], full, dy.double().abs() @ w.detach().double().abs() + 2.0, N, "unmasked route (the producer masks)")


def test_switch_is_listed_applied_and_not_committed(monkeypatch):
    from monodetr_amd import kernel_families as kf
    from monodetr_amd.monodetr import linear
    assert "MDETR_TGEMM_F32" in kf.ALL_SWITCHES and "MDETR_TGEMM_F32" in kf.SWITCH_TESTS
    assert all("MDETR_TGEMM_F32" not in fams for fams in kf.COMMITTED_SWITCHES.values())
    import os
    for pat in kf.SWITCH_TESTS["MDETR_TGEMM_F32"].split(","):
        name, stem = pat.strip().split("::")                         # every pattern names its file, and a test of that file
        assert name in ("test_tgemm_f32_gpu.py", "test_exact_products_gpu.py"), pat
        assert "def " + stem.rstrip("*") in open(os.path.join(os.path.dirname(__file__), name)).read(), pat
    try:
        kf.apply_switches({"MDETR_TGEMM_F32"})
        assert linear._TGEMM_F32 and not linear._TGEMM
        kf.apply_switches({"MDETR_TGEMM"})
        assert linear._TGEMM and not linear._TGEMM_F32
    finally:
        kf.apply_switches(set())
    assert not linear._TGEMM_F32 and not linear._TGEMM
    monkeypatch.setenv("MDETR_TGEMM_F32", "1")
    assert kf.env_switches() == {"MDETR_TGEMM_F32"}


def test_bf16_module_under_the_bf16_switch_alone_makes_the_calls_it_made(backend, monkeypatch):
    """MDETR_TGEMM alone: bf16 layers call mdetr_tgemm exactly as before (forward + input gradient), fp32 layers call nothing;
    MDETR_TGEMM_F32 alone: the reverse."""
    from monodetr_amd.monodetr import linear
    torch.manual_seed(7)
    lin16, lin32 = linear.Linear(64, 72).to(torch.bfloat16), linear.Linear(64, 72)
    x16 = (torch.randn(4200, 64) * 0.5).to(torch.bfloat16).requires_grad_(True)
    x32 = (torch.randn(4200, 64) * 0.5).requires_grad_(True)
    for bf16_on, f32_on in ((True, False), (False, True), (False, False), (True, True)):
        monkeypatch.setattr(linear, "_TGEMM", bf16_on)
        monkeypatch.setattr(linear, "_TGEMM_F32", f32_on)
        backend.calls.clear()
        y = lin16(x16)
        y.float().sum().backward()
        assert y.dtype == torch.bfloat16 and backend.calls == (["mdetr_tgemm", "mdetr_tgemm"] if bf16_on else []), backend.calls
        backend.calls.clear()
        y = lin32(x32)
        (y * 2.0).sum().backward()                                                              # (a materialised gradient: a broadcast one goes to the library)
        assert y.dtype == torch.float32 and backend.calls == (["mdetr_tgemm_f32", "mdetr_tgemm_f32"] if f32_on else []), backend.calls
        assert not linear.pointwise_relu_fusable(torch.zeros(1, 64, 80, 80), lin16.weight.view(72, 64, 1, 1), lin16.bias)     # mixed dtypes: never


def test_short_fp32_input_gradients_stay_with_the_library(backend, monkeypatch):
    """`linear._F32_NN_MIN_TOKENS`: below 8 192 rows the fp32 input gradient takes the library (measured slower on the kernel at the
    decoder's 4 400 rows), the forward product the kernel; from 8 192 rows on both take the kernel."""
    from monodetr_amd.monodetr import linear
    monkeypatch.undo()
    from monodetr_amd import tgemm_ext
    monkeypatch.setattr(tgemm_ext, "_backend", backend)
    monkeypatch.setattr(linear, "_TGEMM_F32", True)
    assert linear._F32_NN_MIN_TOKENS == 8192
    torch.manual_seed(8)
    lin = linear.Linear(64, 72)
    for T, want in ((4400, ["mdetr_tgemm_f32"]), (8192, ["mdetr_tgemm_f32", "mdetr_tgemm_f32"])):
        x = (torch.randn(T, 64) * 0.5).requires_grad_(True)
        backend.calls.clear()
        (lin(x) * 2.0).sum().backward()
        assert backend.calls == want, (T, backend.calls)
        _close(x.grad, torch.full((T, 72), 2.0, dtype=torch.float64), lin.weight.detach().double(), 72, what="T=%d" % T)
