"""The MSDA backward writing grad_value in bf16 (csrc/msda_fused.hip behind mdetr_msda_backward_to, ``grad_value_dtype`` of
monodetr_amd/msda_ext.py): D = 32, L = P = 4, B = 2, M = 2 over the pyramid (26, 34) (13, 17) (6, 8) (3, 4), S = 1165 -- level 0
splits into ragged core tiles, the other levels are whole-level chunked in self-attention -- as self-attention (Lq = S) and as
cross-attention (Lq = 50), for bf16 and fp32 value / grad_out.

* sampling offsets within 2 px: no corner leaves a block's reach (the workspace header's `far` word stays 0, asserted), and the bf16
  grad_value is the fp32 grad_value of the same call rounded once -- torch.equal; grad_loc / grad_attn are the same bits.
* uniformly random locations: in self-attention the `far` word is set (asserted) and the finalize pass adds the fp32 side buffer to
  the ALREADY ROUNDED core value and rounds again.  With output gradients of one sign that is at most one bf16 ulp from the fp32
  result rounded once (asserted element-wise).  With both signs the core value's rounding, 2^-8 |c|, can be many ulps of a sum that
  cancels: held to 2^-8 (A + |result|), A = the same sum over |grad_out| (msda_grad_value_cases.assert_far_path_bound; the CPU
  emulation of the same kernels measures 0.64 - 0.75 of it).  Cross-attention blocks scan every query: no side buffer, equal bits.
  Both against the C oracle within the fp32 operator's bar (1e-5 of scale, tests/test_msda_gpu.py) plus these roundings.
* an MSDeformAttn module in bf16, forward and backward, with and without the bf16 grad_value: every gradient torch.equal."""
import pytest
import torch

import msda_grad_value_cases as C

pytestmark = pytest.mark.gpu

PYRAMID = [(26, 34), (13, 17), (6, 8), (3, 4)]
B, M = 2, 2


@pytest.fixture()
def far_flags(monkeypatch):
    """The `far` word of the workspace header after each backward call made through msda_ext (read when asked: synchronises)."""
    from monodetr_amd import msda_ext
    seen, orig = [], msda_ext._workspace

    def spy(device, nbytes):
        ws = orig(device, nbytes)
        seen.append(ws)
        return ws

    monkeypatch.setattr(msda_ext, "_workspace", spy)

    def take():
        torch.cuda.synchronize()
        flag = int(seen[-1].view(torch.int32)[2].item())
        del seen[:]
        return flag
    return take


def backward(p, elem, gv_dtype, far_flags):
    from monodetr_amd import msda_ext
    d = {k: v.cuda() for k, v in p.items()}
    if elem == torch.bfloat16:
        got = msda_ext.ms_deform_attn_backward_bf16(d["value"].to(elem), d["shapes"], d["level_start"], d["loc"], d["attn"], d["grad_out"].to(elem),
                                                    grad_value_dtype=gv_dtype)
    else:
        got = msda_ext.ms_deform_attn_backward(d["value"], d["shapes"], d["level_start"], d["loc"], d["attn"], d["grad_out"], 64,
                                               grad_value_dtype=None if gv_dtype == torch.float32 else gv_dtype)
    flag = far_flags()
    assert got[0].dtype == gv_dtype and got[1].dtype == got[2].dtype == torch.float32
    return got, flag


def oracle_grad_value(oracle, p, elem):
    c = (lambda t: t.to(elem).double()) if elem == torch.bfloat16 else (lambda t: t.double())
    return oracle.backward(c(p["value"]), p["shapes"], p["level_start"], p["loc"].double(), p["attn"].double(), c(p["grad_out"]))[0]


@pytest.mark.parametrize("elem", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("Lq", [None, 50])
def test_msda_bf16_grad_value_is_the_fp32_one_rounded_once(oracle, far_flags, elem, Lq):
    p = C.near_problem(B, M, Lq, PYRAMID, 2.0, seed=21)
    (gv32, gl32, ga32), far32 = backward(p, elem, torch.float32, far_flags)
    (gv16, gl16, ga16), far16 = backward(p, elem, torch.bfloat16, far_flags)
    assert far32 == 0 and far16 == 0
    assert torch.equal(gv16, gv32.to(torch.bfloat16))
    assert torch.equal(gl16, gl32) and torch.equal(ga16, ga32)
    assert float(gv32.abs().max()) > 0
    C.assert_within_oracle(gv16, oracle_grad_value(oracle, p, elem))


@pytest.mark.parametrize("elem", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("Lq", [None, 50])
def test_msda_bf16_grad_value_with_uniform_locations(oracle, far_flags, elem, Lq):
    p = C.uniform_problem(B, M, Lq, PYRAMID, seed=22, positive=True)
    q = C.uniform_problem(B, M, Lq, PYRAMID, seed=22)
    (gv32, gl32, ga32), far32 = backward(p, elem, torch.float32, far_flags)
    (gv16, gl16, ga16), far16 = backward(p, elem, torch.bfloat16, far_flags)
    (mv32, ml32, ma32), mfar32 = backward(q, elem, torch.float32, far_flags)
    (mv16, ml16, ma16), mfar16 = backward(q, elem, torch.bfloat16, far_flags)
    assert torch.equal(gl16, gl32) and torch.equal(ga16, ga32) and torch.equal(ml16, ml32) and torch.equal(ma16, ma32)
    if Lq is None:
        assert far32 == far16 == mfar32 == mfar16 == 1                      # the side buffer was used: the case is what it claims to be
        print("one sign: %d bf16 ulps from the fp32 result rounded once" % C.ulps_apart(gv16, gv32.to(torch.bfloat16)))
        assert C.ulps_apart(gv16, gv32.to(torch.bfloat16)) <= 1
        C.assert_far_path_bound(mv16, mv32, gv32)                           # (p is q with |grad_out|)
        C.assert_within_oracle(gv16, oracle_grad_value(oracle, p, elem), gv32)
        C.assert_within_oracle(mv16, oracle_grad_value(oracle, q, elem), gv32)
    else:
        assert far32 == far16 == mfar32 == mfar16 == 0                      # every block scans every query: nothing leaves its reach
        assert torch.equal(gv16, gv32.to(torch.bfloat16)) and torch.equal(mv16, mv32.to(torch.bfloat16))
        C.assert_within_oracle(mv16, oracle_grad_value(oracle, q, elem))


def test_msda_bf16_module_gradients_do_not_change_with_the_bf16_grad_value(monkeypatch, far_flags):
    """MSDeformAttn (256 wide: 8 heads of 32) in bf16 as the encoder calls it -- self-attention over the pyramid, the bf16-native
    operator -- forward and backward with the value gradient written in bf16 by the kernel, and with the fp32 value gradient and
    its conversion: the rounding is the same one, moved, so every parameter's and input's gradient has the same bits."""
    from monodetr_amd.monodetr.ops.functions import ms_deform_attn_func
    from monodetr_amd.monodetr.ops.modules import MSDeformAttn
    monkeypatch.setattr(ms_deform_attn_func, "_NATIVE_BF16", True)
    S = sum(h * w for h, w in PYRAMID)
    g = torch.Generator().manual_seed(5)
    m = MSDeformAttn(256, 4, 8, 4)
    with torch.no_grad():
        m.sampling_offsets.weight.normal_(0, 0.002, generator=g)
        m.attention_weights.weight.normal_(0, 0.05, generator=g)
    m = m.to(torch.bfloat16).cuda()
    shapes = torch.tensor(PYRAMID, dtype=torch.int64, device="cuda")
    start = torch.cat((shapes.new_zeros(1), shapes.prod(1).cumsum(0)[:-1]))
    ref = torch.cat([torch.stack(torch.meshgrid((torch.arange(h) + 0.5) / h, (torch.arange(w) + 0.5) / w, indexing="ij"), -1).reshape(-1, 2)
                     for h, w in PYRAMID])[:, [1, 0]]
    ref = ref.view(1, S, 1, 2).expand(B, S, 4, 2).contiguous().cuda()
    src0 = torch.randn(B, S, 256, generator=g).to(torch.bfloat16).cuda()
    qry0 = torch.randn(B, S, 256, generator=g).to(torch.bfloat16).cuda()
    dy = torch.randn(B, S, 256, generator=g).to(torch.bfloat16).cuda()
    grads = {}
    for on in (True, False):
        monkeypatch.setattr(ms_deform_attn_func, "_BF16_GRAD_VALUE", on)
        src, qry = src0.clone().requires_grad_(True), qry0.clone().requires_grad_(True)
        for prm in m.parameters():
            prm.grad = None
        m(qry, ref, src, shapes, start).backward(dy)
        assert far_flags() == 0
        grads[on] = dict({n: prm.grad.clone() for n, prm in m.named_parameters()}, src=src.grad.clone(), query=qry.grad.clone())
    assert set(grads[True]) == set(grads[False]) and len(grads[True]) == 10
    for n in grads[True]:
        assert grads[True][n].dtype == torch.bfloat16 and float(grads[True][n].float().abs().max()) > 0, n
        assert torch.equal(grads[True][n], grads[False][n]), n


@pytest.mark.parametrize("chain", [False, True])
def test_msda_bf16_wide_cross_attention_takes_its_value_gradient_from_the_kernel(monkeypatch, far_flags, chain):
    """The decoder's call: 50 queries into the pyramid, bf16 model, fp32 ("wide") values from the value projection's token GEMM.  The
    operator's kernel writes the value gradient in bf16 and hands it to the projection's backward (linear.WideGradToken) instead
    of an fp32 tensor that the projection rounds: asked for (asserted), and every gradient has the same bits as without."""
    from monodetr_amd import msda_ext
    from monodetr_amd.monodetr import linear
    from monodetr_amd.monodetr.ops.functions import ms_deform_attn_func
    from monodetr_amd.monodetr.ops.modules import MSDeformAttn
    monkeypatch.setattr(linear, "_TGEMM", True)
    monkeypatch.setattr(linear, "_MIN_TOKENS", 1024)                           # (the 2 330 token rows here take the kernels' route, chained or not)
    S, Lq = sum(h * w for h, w in PYRAMID), 50
    g = torch.Generator().manual_seed(6)
    m = MSDeformAttn(256, 4, 8, 4)
    with torch.no_grad():
        m.sampling_offsets.weight.normal_(0, 0.002, generator=g)
        m.attention_weights.weight.normal_(0, 0.05, generator=g)
    m = m.to(torch.bfloat16).cuda()
    shapes = torch.tensor(PYRAMID, dtype=torch.int64, device="cuda")
    start = torch.cat((shapes.new_zeros(1), shapes.prod(1).cumsum(0)[:-1]))
    ref = torch.rand(B, Lq, 1, 2, generator=g).expand(B, Lq, 4, 2).contiguous().cuda()
    src0 = torch.randn(B, S, 256, generator=g).to(torch.bfloat16).cuda()
    qry0 = torch.randn(B, Lq, 256, generator=g).to(torch.bfloat16).cuda()
    dy = torch.randn(B, Lq, 256, generator=g).to(torch.bfloat16).cuda()
    asked, real = [], msda_ext.ms_deform_attn_backward

    def spy(*a, **kw):
        asked.append((a[0].dtype, kw.get("grad_value_dtype")))
        return real(*a, **kw)

    monkeypatch.setattr(msda_ext, "ms_deform_attn_backward", spy)
    grads = {}
    for on in (True, False):
        monkeypatch.setattr(ms_deform_attn_func, "_BF16_GRAD_VALUE", on)
        src, qry = src0.clone().requires_grad_(True), qry0.clone().requires_grad_(True)
        for prm in m.parameters():
            prm.grad = None
        if chain:
            out, nxt = m(qry, ref, src, shapes, start, chain_input=True)
            (out.float().mul(dy.float()).sum() + nxt.float().sum() * 0.25).backward()
        else:
            m(qry, ref, src, shapes, start).backward(dy)
        assert far_flags() == 0
        grads[on] = dict({n: prm.grad.clone() for n, prm in m.named_parameters()}, src=src.grad.clone(), query=qry.grad.clone())
    assert asked == [(torch.float32, torch.bfloat16), (torch.float32, None)], asked
    for n in grads[True]:
        assert float(grads[True][n].float().abs().max()) > 0, n
        assert torch.equal(grads[True][n], grads[False][n]), n
