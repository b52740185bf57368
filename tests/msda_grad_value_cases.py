"""Shared by tests/test_msda_bf16_grad_value_gpu.py and tests/test_msda_bf16_grad_value_emulated_cpu.py: problems for the one-pass
MSDA backward (csrc/msda_fused.hip) writing grad_value in bf16, and the comparisons of that result with the fp32 one."""
import torch

from conftest import make_problem


def near_problem(B, M, Lq, shapes, max_px, seed):
    """Self-attention (Lq = None: one query per cell, reference point = its centre) or cross-attention (Lq queries at random
    reference points) with sampling offsets of at most `max_px` cells on every level: nothing leaves a block's reach."""
    S = sum(h * w for h, w in shapes)
    p = make_problem(B, M, 32, S if Lq is None else Lq, shapes, 4, torch.float32, seed=seed)
    g = torch.Generator().manual_seed(seed + 100)
    if Lq is None:
        ref = torch.cat([torch.stack(torch.meshgrid((torch.arange(h) + 0.5) / h, (torch.arange(w) + 0.5) / w, indexing="ij"), -1).reshape(-1, 2)
                         for h, w in shapes])[:, [1, 0]]                     # (x, y) of every query
        ref = ref.view(1, S, 1, 1, 1, 2)
    else:
        ref = torch.rand(B, Lq, 1, 1, 1, 2, generator=g)
    off = (torch.rand(p["loc"].shape, generator=g) * 2 - 1) * max_px
    sizes = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float32).view(1, 1, 1, len(shapes), 1, 2)
    p["loc"] = (ref + off / sizes).contiguous()
    return p


def uniform_problem(B, M, Lq, shapes, seed, positive=False):
    """Sampling locations anywhere in (and a little outside) the maps: in self-attention most corners leave every block's reach.
    positive: every output gradient >= 0, so that every contribution to grad_value is (weights are positive) and nothing cancels."""
    S = sum(h * w for h, w in shapes)
    p = make_problem(B, M, 32, S if Lq is None else Lq, shapes, 4, torch.float32, seed=seed, lo=-0.05, hi=1.05)
    if positive:
        p["grad_out"] = p["grad_out"].abs()
    return p


def ordered(t):
    """bf16 bit patterns as integers in the order of the values they stand for (adjacent values differ by one)."""
    i = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


def ulps_apart(a, b):
    return int((ordered(a) - ordered(b)).abs().max())


def assert_far_path_bound(gv16, gv32, gv_abs):
    """The side-buffer path with gradients of both signs.  The finalize pass adds the fp32 side buffer f to the core tile's value c
    AFTER c was rounded to bf16: result = bf16(bf16(c) + f) where the fp32 call gives c + f.  The first rounding moves c by at most
    2^-8 |c|, the second the sum by at most 2^-8 of its size; |c| <= A, the same sum over the gradients' magnitudes (`gv_abs`, from
    a call with |grad_out|: every weight is positive).  Where c and f cancel, 2^-8 |c| is many ulps of the small result -- the
    reason the one-ulp statement is made for gradients of one sign only.  (1e-6 A: the side buffer's fp32 atomics arrive in
    another order in every call.)"""
    A = gv_abs.double().abs()
    allowed = 2.0 ** -8 * (A + gv32.double().abs()) * (1 + 2.0 ** -8) + 1e-6 * A
    err = (gv16.double() - gv32.double()).abs()
    print("far path, both signs: worst error / bound %.3g, worst distance from the fp32 result rounded once: %d bf16 ulps"
          % (float((err / allowed.clamp_min(1e-30)).max()), ulps_apart(gv16, gv32.to(torch.bfloat16))))
    assert bool((err <= allowed).all()), float((err / allowed.clamp_min(1e-30)).max())


def assert_within_oracle(gv16, rv, gv_abs=None):
    """The fp32 grad_value is held to 1e-5 of the oracle's scale (tests/test_msda_gpu.py); rounding it to bf16 moves it by at most
    2^-8 of its size.  gv_abs (side-buffer path, see assert_far_path_bound): the core value's own rounding, 2^-8 A, on top."""
    scale = max(1.0, float(rv.abs().max()))
    allowed = 1e-5 * scale + 2.0 ** -8 * (rv.abs().double() + 1e-5 * scale) * (1 + 2.0 ** -8)
    if gv_abs is not None:
        allowed = allowed + 2.0 ** -8 * gv_abs.double().abs().cpu() * (1 + 2.0 ** -8)
    err = (gv16.double().cpu() - rv.double()).abs()
    assert bool((err <= allowed).all()), float((err / allowed).max())
