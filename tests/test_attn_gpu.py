"""Fused attention kernels (monodetr_amd/csrc/attn.hip) vs a plain fp64 PyTorch evaluation of
softmax(q k^T / sqrt(d) + mask) v and its autograd gradients, at the three hot-path shapes
(depth encoder 1920x1920, depth cross-attention 550x1920, grouped self-attention 50x50) and on
ragged sizes.  The kernels multiply in bf16 on the matrix cores (fp32 accumulate), so the
tolerance is bf16-level: 2e-2 of the output scale (inputs ~ N(0,1)); with bf16 inputs the reference
is evaluated on the same rounded inputs."""
import pytest
import torch

from attn_cases import keep_mask, reference       # noqa: F401  (tests/test_attn_emulated_cpu.py imports them from here)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B,H,Lq,Lk,dtype", [
    (2, 8, 1920, 1920, torch.float32),     # depth encoder
    (2, 8, 550, 1920, torch.float32),      # depth cross-attention (train)
    (22, 8, 50, 50, torch.float32),        # grouped self-attention: B*11 folded batches
    (3, 2, 33, 65, torch.float32),         # ragged
    (1, 1, 1, 1, torch.float32),
    (2, 8, 550, 1920, torch.bfloat16),
    (3, 4, 129, 200, torch.bfloat16),
])
def test_forward_backward_vs_fp64(B, H, Lq, Lk, dtype):
    from monodetr_amd.attn_ext import fused_attention
    torch.manual_seed(B * 100 + Lq)
    E = H * 32
    q, k, v = (torch.randn(B, L, E, device="cuda").to(dtype).requires_grad_(True) for L in (Lq, Lk, Lk))
    go = torch.randn(B, Lq, E, device="cuda").to(dtype)
    out = fused_attention(q, k, v, H)
    out.backward(go)
    qd, kd, vd = (t.detach().double().requires_grad_(True) for t in (q, k, v))
    ref = reference(qd, kd, vd, H)
    ref.backward(go.double())
    assert out.dtype == dtype and out.shape == (B, Lq, E)
    # fp32 I/O uses three-part split operands (hi + mid + lo = all 24 significand bits, six MFMA terms: fp32 products; measured
    # 0.7 - 2.7e-6 of scale on the shim); bf16 I/O is bf16-level.  Round 5's two-part split stood at 2e-4 / 5e-4 / 1e-4 here.
    tol, gtol, ftol = (2e-5, 2e-5, 1e-5) if dtype == torch.float32 else (2e-2, 3e-2, 1e-2)
    assert (out.double() - ref).abs().max() < tol * max(1.0, ref.abs().max().item())
    # The max-norm bar has a floor of 1: at Lk = 1920 with these flat softmaxes |out| is 0.02 .. 0.1, far below it.  Relative
    # Frobenius error of the output at the gradients' bar: the output passes through fewer roundings than they do (bf16: q scale,
    # P and the store, against q scale, P, dS, D and the store).
    assert ((out.double() - ref).norm() / ref.norm()) < ftol
    for g, r, name in ((q.grad, qd.grad, "dq"), (k.grad, kd.grad, "dk"), (v.grad, vd.grad, "dv")):
        assert (g.double() - r).abs().max() < gtol * max(1.0, r.abs().max().item()), name
        if r.norm() > 1e-3:       # (degenerate single-key problems have exactly zero dq / dk)
            assert ((g.double() - r).norm() / r.norm()) < ftol, name      # relative Frobenius error


def test_strided_inputs_from_packed_projection():
    """q, k, v as slices of one [B, L, 3E] in-projection output (no copies)."""
    from monodetr_amd.attn_ext import fused_attention
    torch.manual_seed(0)
    B, L, H = 2, 77, 8
    E = H * 32
    packed = torch.randn(B, L, 3 * E, device="cuda", requires_grad=True)
    q, k, v = packed.split(E, -1)
    go = torch.randn(B, L, E, device="cuda")
    out = fused_attention(q, k, v, H)
    out.backward(go)
    pd = packed.detach().double().requires_grad_(True)
    ref = reference(*pd.split(E, -1), H)
    ref.backward(go.double())
    assert (out.double() - ref).abs().max() < 2e-2 * max(1.0, ref.abs().max().item())
    # fp32 I/O: the bars of test_forward_backward_vs_fp64, on the output and on each third of the packed gradient
    assert ((out.double() - ref).norm() / ref.norm()) < 1e-5
    assert packed.grad.shape == packed.shape
    for g, r, name in zip(packed.grad.split(E, -1), pd.grad.split(E, -1), ("dq", "dk", "dv")):
        assert (g.double() - r).abs().max() < 2e-5 * max(1.0, r.abs().max().item()), name
        assert ((g.double() - r).norm() / r.norm()) < 1e-5, name


def test_key_padding_mask_and_fully_masked_rows():
    from monodetr_amd.attn_ext import fused_attention
    torch.manual_seed(1)
    B, H, Lq, Lk = 3, 4, 40, 100
    E = H * 32
    q, k, v = (torch.randn(B, L, E, device="cuda", requires_grad=True) for L in (Lq, Lk, Lk))
    kpm = torch.rand(B, Lk, device="cuda") < 0.3
    kpm[2] = True                                     # every key of batch 2 masked -> zeros, no NaN
    out = fused_attention(q, k, v, H, key_padding_mask=kpm)
    out.sum().backward()
    ref = reference(q.detach(), k.detach(), v.detach(), H, kpm)
    assert torch.isfinite(out).all() and torch.isfinite(q.grad).all() and torch.isfinite(k.grad).all()
    assert (out[2] == 0).all()
    assert (out.double() - ref).abs().max() < 2e-2 * max(1.0, ref.abs().max().item())
    assert (k.grad[kpm] == 0).all() and (v.grad[kpm] == 0).all()
    # the gradients against fp64 (fp32 I/O: the bars of test_forward_backward_vs_fp64); the fully masked image has none
    qd, kd, vd = (t.detach().double().requires_grad_(True) for t in (q, k, v))
    reference(qd, kd, vd, H, kpm).sum().backward()
    assert ((out.double() - ref).norm() / ref.norm()) < 1e-5
    for g, r, name in ((q.grad, qd.grad, "dq"), (k.grad, kd.grad, "dk"), (v.grad, vd.grad, "dv")):
        assert (g.double() - r).abs().max() < 2e-5 * max(1.0, r.abs().max().item()), name
        assert ((g.double() - r).norm() / r.norm()) < 1e-5, name
        assert (g[2] == 0).all(), name


def test_dropout_mask_is_consistent_between_forward_and_backward():
    from monodetr_amd.attn_ext import fused_attention
    torch.manual_seed(2)
    B, H, Lq, Lk, p, seed = 2, 4, 70, 90, 0.1, 0x1234567890ABCDEF
    E = H * 32
    q, k, v = (torch.randn(B, L, E, device="cuda", requires_grad=True) for L in (Lq, Lk, Lk))
    go = torch.randn(B, Lq, E, device="cuda")
    out = fused_attention(q, k, v, H, dropout_p=p, seed=seed)
    out.backward(go)
    keep = keep_mask(seed, B, H, Lq, Lk, p).cuda()
    assert abs(keep.float().mean().item() - (1 - p)) < 0.01
    qd, kd, vd = (t.detach().double().requires_grad_(True) for t in (q, k, v))
    ref = reference(qd, kd, vd, H, keep=keep, p=p)
    ref.backward(go.double())
    assert (out.double() - ref).abs().max() < 2e-2 * max(1.0, ref.abs().max().item())
    for g, r in ((q.grad, qd.grad), (k.grad, kd.grad), (v.grad, vd.grad)):
        assert ((g.double() - r).norm() / r.norm()) < 1e-2
    # a different seed gives a different mask, the same seed the same output
    assert torch.equal(out, fused_attention(q, k, v, H, dropout_p=p, seed=seed))
    assert not torch.equal(out, fused_attention(q, k, v, H, dropout_p=p, seed=seed + 1))
