"""The hand-over of the decoder's value gradient (monodetr/linear.py WideGradToken): the value projection with an fp32 ("wide")
result -> view -> MSDeformAttnFunction, whose backward has the kernel write grad_value in bf16 (mdetr_msda_backward_to, here on the
HIP-on-CPU shim), leaves it in the projection's token and returns no gradient for the value.  The projection's GEMM kernel exists
on the GPU only: its forward product is stood in for by the same arithmetic in torch (bf16 operands, fp32 result) -- what is under
test is the autograd plumbing and the operator, and that every gradient keeps its bits against the fp32 gradient + rounding."""
import pytest
import torch

import msda_grad_value_cases as C
import native_emul
from test_msda_emulated_cpu import _check, bwd, fwd
from test_msda_bf16_grad_value_emulated_cpu import TINY

asked = []


class _EmulModule:
    """The extension-module object as MSDeformAttnFunction sees it, backed by the emulated C ABI (fp32 tensors)."""
    GRAD_VALUE_DTYPE = True

    @staticmethod
    def bf16_supported(value, loc):
        return False

    @staticmethod
    def ms_deform_attn_forward(value, shapes, start, loc, attn, im2col_step):
        return fwd(dict(value=value, shapes=shapes, level_start=start, loc=loc, attn=attn))

    @staticmethod
    def ms_deform_attn_backward(value, shapes, start, loc, attn, grad_out, im2col_step, grad_value_dtype=None):
        asked.append(grad_value_dtype)
        p = dict(value=value, shapes=shapes, level_start=start, loc=loc, attn=attn, grad_out=grad_out)
        if grad_value_dtype is None:
            return list(bwd(p, path="fused"))
        L = native_emul.lib()
        B, S, M, D = value.shape
        Lq = loc.shape[1]
        gv, gl, ga = torch.empty(value.shape, dtype=grad_value_dtype), torch.empty_like(loc), torch.empty_like(attn)
        n = L.mdetr_msda_backward_workspace_bytes(0, shapes.data_ptr(), start.data_ptr(), B, S, M, D, 4, Lq, 4)
        ws = torch.randint(0, 255, (n,), dtype=torch.uint8)
        _check(L.mdetr_msda_backward_to(0, 2, value.data_ptr(), loc.data_ptr(), attn.data_ptr(), grad_out.data_ptr(), gv.data_ptr(), gl.data_ptr(),
                                        ga.data_ptr(), B, S, M, D, 4, Lq, 4, shapes.data_ptr(), start.data_ptr(), ws.data_ptr(), n, 0, None))
        return [gv, gl, ga]


@pytest.mark.parametrize("form", ["plain", "skip", "unused"])
def test_the_value_gradient_travels_in_the_token_and_no_gradient_changes(monkeypatch, form):
    from monodetr_amd.monodetr import linear
    from monodetr_amd.monodetr.ops.functions import ms_deform_attn_func as F
    monkeypatch.setattr(F, "MSDA", _EmulModule)
    monkeypatch.setattr(linear, "_tgemm_ok", lambda x2, weight, bias=None, res2=None, nn=False: not nn)
    monkeypatch.setattr(linear, "_fwd_product", lambda x2, w, b, relu=False, res2=None, dropout_p=0.0, seed=0, seed_dev=None, out_dtype=None:
                        (x2.float() @ w.float().t() + b.float()).to(out_dtype))
    p = C.near_problem(1, 2, 9, TINY, 1.4, seed=31)
    S, M = p["value"].shape[1], 2
    g = torch.Generator().manual_seed(3)
    x0 = torch.randn(1, S, 48, generator=g).to(torch.bfloat16)
    w0 = (torch.randn(M * 32, 48, generator=g) * 0.1).to(torch.bfloat16)
    b0 = (torch.randn(M * 32, generator=g) * 0.1).to(torch.bfloat16)
    res = {}
    for on in (True, False):
        monkeypatch.setattr(F, "_BF16_GRAD_VALUE", on)
        del asked[:]
        x, w, b = (t.clone().requires_grad_(True) for t in (x0, w0, b0))
        loc, attn = p["loc"].clone().requires_grad_(True), p["attn"].clone().requires_grad_(True)
        if form == "skip":
            value, nxt = linear._TokenLinearSkip.apply(x, w, b, None, False, 0.0, False, True, None)
        else:
            value, nxt = linear._TokenLinear.apply(x, w, b, False, True), None
        assert value.dtype == torch.float32 and isinstance(value._mdetr_wide_token, linear.WideGradToken)
        if form == "unused":                                   # the projection's result is not used at all: no gradient arrives, none is invented
            (x.float().sum() * 0.5).backward()
            assert w.grad is None and b.grad is None and asked == []
            continue
        tok = value._mdetr_wide_token
        out = F.MSDeformAttnFunction.apply(value.view(1, S, M, 32), p["shapes"], p["level_start"], loc, attn, 64, tok)
        loss = (out * p["grad_out"]).sum() + (nxt.float().sum() * 0.25 if nxt is not None else 0.0)
        loss.backward()
        assert asked == ([torch.bfloat16] if on else [None]) and tok.grad is None
        res[on] = (x.grad, w.grad, b.grad, loc.grad, attn.grad)
    if form != "unused":
        for a, c in zip(res[True], res[False]):
            assert a is not None and float(a.float().abs().max()) > 0 and torch.equal(a, c)
