"""Cases, references and bounds for the fused attention kernels (csrc/attn.hip).  Test infrastructure: plain torch in fp64, no kernel
code; tests/test_attn_cases_gpu.py runs the cases on the device, tests/test_attn_cases_emulated_cpu.py through tests/native_emul.py.

(a) INTEGER-SCORE CASES: the forward to the bit.
The caller passes scale = float32(ln 2 / 4); the kernels multiply q by fl32(scale * log2e), which is 0.25 exactly.  q has one
non-zero entry per head, 4 n with n in 1..3; k holds integers in -6..-1 (a narrower range in the first 32-key sub-tiles, so that the
running maximum moves several times) and one planted all-zero key per (image, head): every log2-domain score is an integer in
-18..0 in every kernel and both dtypes, the planted key is the row maximum, every probability is a power of two.  v holds integers
in -4..4.  Every partial sum of l = sum_j e_j and of the numerator sum_j e_j v_j, in ANY order and at any intermediate running
maximum (a rescale by a power of two is exact), is a multiple of 2^-spread (spread = row maximum - smallest live score) of magnitude
<= sum_j e_j |v_j| resp. l: it is exact in fp32 if those are < 2^24 2^-spread.  `budget` checks that per row; it follows from
spread + log2 max|v| + log2 Lk <= 23 and is sharper (most probabilities of a row are tiny).  What remains in the kernel is
inv = fl(rinv / l) and one product by it, two roundings of 2^-24:
    fp32:  |out - ref| <= 2^-23 |ref|
    bf16:  out == bf16(ref) wherever ref is further than 2^-22 |ref| from the midpoint of two neighbouring bf16 numbers (the fp32
           value before the store is within 2^-23 |ref| of ref, so it lies on the same side of the midpoint).
This takes exp2 to be exact at integer arguments.
Premises, checked from the operands and the fp64 reference before any kernel runs (`PremiseError`): the scores are integers, the
budget holds, <= 1 % of the elements are excluded as near a midpoint and >= 10 % of the bf16 results are no bf16 numbers (the store
must round).  The last one cannot hold where one key is live -- the result is that key's v, an integer -- and is not asked there.

(b) RANDOM AND PEAKED CASES: forward and backward against fp64.
q, k, v, dO ~ N(0, 1), q scaled so that the logits q k scale have standard deviation 1, 8 or 30.  `truth` evaluates, in fp64 and
in closed form (tests/test_attn_cases_emulated_cpu.py checks it against autograd once), with Pd = P keep / (1 - p):
    out = Pd v,  D_i = sum_c dO_ic out_ic,  dPd = (dO v^T) keep / (1 - p),  dS = P (dPd - D),
    dQ = scale dS k,  dK = scale dS^T q,  dV = Pd^T dO.

bf16 I/O -- `model` is that evaluation with the kernels' roundings put in (bf16: 8 significand bits, round to nearest even -- a
rounding errs by at most half an ulp, 2^-9 of the binade's power of two, i.e. 2^-9 .. 2^-8 of the value):
    q' = bf16(fl32(q c)), c = fl32(scale log2e): ONE rounded operand for all three kernels; scores s = q' k; the backward's
    P = exp2(s - lse) with lse = fl32(max + log2 l), as the forward stores it in its float32 buffer;
    forward: e = exp2(s - max) is rounded to bf16 (after the drop) before the product with v; l sums the unrounded e;
    out = bf16(rinv (bf16(e keep) v) / l);  D from that ROUNDED out;  dS and P keep are rounded to bf16 before their products;
    dQ = bf16(scale bf16(dS) k),  dK = bf16(bf16(dS)^T q' / log2e),  dV = bf16(rinv bf16(P keep)^T dO).
The per-element bound is |kernel - model| <= 2^-7 A, A the same contraction on absolute values:
    A_out = Pd |v|,  A_D_i = sum_c |dO_ic| A_out_ic  (>= |D_i|),  W = P (|dPd| + A_D)  (>= |dS|),
    A_dQ = scale W |k|,  A_dK = W^T |q'| / log2e,  A_dV = Pd^T |dO|.
Derivation.  Kernel and model round the same quantities at the same places, but not the same bits: the kernel rounds e relative to
the RUNNING maximum (the model relative to the final one), its scores and exp2 carry fp32 errors (<= ~40 2^-24 sum|q'||k| in the
exponent, 1 ulp of exp2, lse stored in fp32: below 2^-11 relative in P at logit std 30), and two values that differ in their last
fp32 bits can lie on either side of a bf16 midpoint and round one ulp apart.  2^-7 A is room for three half-ulp rounding errors
(3 x 2^-9 at the bottom of a binade ... 3 x 2^-8 at its top would already be 1.5 x 2^-7) plus the fp32 terms.  What it covers:
  * out: the kernel's and the model's e carry INDEPENDENT rounding errors (different reference maximum), <= 2^-8 e each, which add up
    over a row far below 2^-8 A_out; the store then rounds two slightly different values, often one ulp apart: <= 2^-7 |out|.  In a
    peaked row A_out ~ |out|, so the measured worst ratio sits just below 1 in every peaked case (0.89 .. 0.996 on the emulation).
  * dV: P keep and the store are rounded at the same scale by kernel and model, so they agree to the bit (ratio 0.000 in half of the
    cases) unless a P straddles a midpoint (about 1 in 400: 2^-17 relative fp32 error against 2^-8 spacing); one flipped P is one
    ulp of P in dV of that key, <= 2^-7 of its term.
  * dQ / dK: the same for dS, and the kernel's D comes from the KERNEL's rounded out, the model's from the model's:
    |D_k - D_m| <= sum_c |dO| |out_k - out_m| <= 2^-7 A_D, which enters dS as P 2^-7 A_D <= 2^-7 W.
The bound is the one the issue set and is NOT a worst case: a flipped P (or dS) under a flipped store is two ulps, up to 2^-6 of
a result that has one dominant term (A ~ |result|), and the kernel is right when that happens.  That is why the model rounds lse to
fp32 as the forward's store does: without it, `scale` bf16 on the emulation had one P (0.01715, 97 % of key 140's column, 2 10^-7
relative from a bf16 midpoint) on the other side of the midpoint, moved there by the 5 10^-7 that the stored lse differs from the
fp64 one, and 12 of that key's 32 dV channels beyond the bound (worst 1.718).  With it every tensor of every case is within the bound
on the emulation (worst 0.996, dV agrees to the bit in most cases; profiles/attn_cases_ratios_emulated.txt).  A ratio above 1 is a
finding to be traced to its element like that one, not a reason to widen the bound.
Beside that bound, ||kernel - fp64|| <= 2 ||model - fp64|| + 2^-7 ||A|| (Frobenius): model - fp64 is the inherent cost of the bf16
roundings (dominated by q' at peaked logits: up to 2^-8 sum|q c||k| in the exponent); a kernel that rounds more than the model says
fails -- the dK/dV kernel that rounded k c instead of reading q' gave 0.0217 against the model's 0.0075 for dK at std 8.

fp32 I/O -- against fp64 directly.  With T_ij = sum_c |q_ic c| |k_jc| (log2 domain) a kernel score errs by <= eps_s T_ij,
    eps_s = 2^-23 (dropped mid*lo, lo*mid, lo*lo terms of the three-way bf16 split) + 2^-24 (fl32(q c)) + 2^-23 (c itself: the
            rounded product of two rounded factors) + 40 2^-24 (fp32 accumulation over d = 32 in six passes)  <= 48 2^-24.
It enters the exponent: P errs relatively by ln2 eps_s (T_ij + Tbar_i), Tbar_i = sum_j P_ij T_ij (the normaliser moves by the
P-weighted mean of the score errors), plus eta_L = (2 L + 64) 2^-24 for a sum of L terms accumulated in fp32, once for l and once
for the product itself, exp2 at 1 ulp (2^-23), the subtraction, fl(rinv / l), the final scale and the split of P (2^-23):
    relP(L) = ln2 eps_s (T + Tbar) + eta_L
    B_out = (Pd relP(Lk)) |v|
    B_D   = sum_c |dO| B_out + 40 2^-24 A_D,   B_dP = 40 2^-24 (|dO| |v|^T) keep / (1 - p)
    B_dS  = P relP(Lk) (|dPd| + |D|) + P (B_dP + B_D) + 2^-23 |dS|
    B_dQ  = scale (B_dS |k| + eta_Lk |dS| |k|),   B_dK = scale (B_dS^T |q| + eta_Lq |dS|^T |q|),   B_dV = (Pd relP(Lk + Lq))^T |dO|.
These are worst-case constants (every accumulation error aligned): measured ratios are a few per cent.

In both modes a bound of exactly 0 -- a masked key's dK and dV, every result of a fully masked row -- asks for an exact 0."""
import functools
import math

import numpy as np
import torch

BF16, F32 = torch.bfloat16, torch.float32
LOG2E = 1.4426950408889634
LOG2E32 = float(np.float32(LOG2E))
INVLOG2E32 = float(np.float32(0.6931471805599453))
EPS_S = 48.0 * 2.0 ** -24
D = 32


class PremiseError(AssertionError):
    """The operands do not have the property the case was built for (a fault of the test, not of a kernel)."""


def gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * (int(k) if not isinstance(k, str) else sum(map(ord, k)))
                                             for i, k in enumerate(key)) % (2 ** 31))


# ---- the operation, restated ---------------------------------------------------------------------------------------------------------
def keep_mask(seed, B, H, Lq, Lk, p):
    """The kernels' stateless dropout decision (attn.hip keep_elem: the low 32 bits of the product of the low 24 bits of two
    finalised hashes, one of the query, one of the key), restated with int64 arithmetic.  The threshold is the kernels':
    unsigned(float32(p) * 2^32) -- p arrives as a C float (429496736 at p = 0.1; the double 0.1 gives 429496729)."""
    M = 0xFFFFFFFF

    def strong32(v):
        v = v ^ (v >> 16); v = (v * 0x85EBCA6B) & M; v = v ^ (v >> 13); v = (v * 0xC2B2AE35) & M
        return v ^ (v >> 16)

    b = torch.arange(B).view(B, 1, 1, 1)
    h = torch.arange(H).view(1, H, 1, 1)
    q = torch.arange(Lq).view(1, 1, Lq, 1)
    k = torch.arange(Lk).view(1, 1, 1, Lk)
    qconst = (seed & M) ^ ((((seed >> 32) & M) + ((b * 131 + h) * 0xC2B2AE3D & M)) & M)
    qs = strong32(((q * 0x9E3779B1) & M) ^ qconst) | 1
    ks = strong32((((k + 0x7F4A7C15) & M) * 0x85EBCA77) & M)
    x = ((qs & 0xFFFFFF) * (ks & 0xFFFFFF)) & M
    return x >= int(float(np.float32(p)) * 4294967296.0)


def reference(q, k, v, H, kpm=None, keep=None, p=0.0, scale=None):
    """softmax(q k^T scale + mask) v with dropout mask `keep`, in fp64, differentiable."""
    B, Lq, E = q.shape
    d = E // H
    qh, kh, vh = (t.double().view(B, -1, H, d).transpose(1, 2) for t in (q, k, v))
    s = qh @ kh.transpose(-1, -2) * (d ** -0.5 if scale is None else scale)
    if kpm is not None:
        s = s.masked_fill(kpm[:, None, None, :], float("-inf"))
    a = torch.softmax(s, -1)
    a = torch.nan_to_num(a)                       # fully masked rows -> 0
    if keep is not None:
        a = a * keep.double() / (1 - p)
    return (a @ vh).transpose(1, 2).reshape(B, Lq, E)


def key_mask(name, B, Lk):
    """The mask geometries (True = ignore the key)."""
    if name is None:
        return None
    m = torch.zeros(B, Lk, dtype=torch.bool)
    if name == "lead96":              # one image: a whole 64-key tile and a 32-key sub-tile pass with m = -inf
        m[0, :96] = True
    elif name == "inner64_127":       # an inner tile, met while the running maximum is finite
        m[:, 64:128] = True
    elif name == "tail190":           # the ragged tail and two keys before it
        m[:, 190:] = True
    elif name == "one_live_last":
        m[:] = True
        m[:, Lk - 1] = False
    elif name == "one_live_first":
        m[:] = True
        m[:, 0] = False
    elif name == "image_masked":      # every row of the last image is fully masked
        m[B - 1] = True
    else:
        raise KeyError(name)
    return m


def heads(t, H):
    B, L, E = t.shape
    return t.double().view(B, L, H, E // H).transpose(1, 2)


def unheads(t):
    B, H, L, d = t.shape
    return t.transpose(1, 2).reshape(B, L, H * d)


def bf(t):
    return t.to(BF16).double()


# ---- (a) integer scores ----------------------------------------------------------------------------------------------------------------
INT_SCALE = float(np.float32(math.log(2.0) / 4.0))

INTEGER_CASES = {
    #  name               B  H  Lq   Lk   mask              plant          p
    "plain":             (2, 2, 70, 200, None,             None,          0.0),
    "lead96":            (2, 2, 70, 200, "lead96",         None,          0.0),
    "inner64_127":       (2, 2, 70, 200, "inner64_127",    None,          0.0),
    "tail190":           (2, 2, 70, 200, "tail190",        None,          0.0),
    "one_live_last":     (2, 2, 70, 200, "one_live_last",  None,          0.0),
    "one_live_first":    (2, 2, 70, 200, "one_live_first", None,          0.0),
    "image_masked":      (2, 2, 70, 200, "image_masked",   None,          0.0),
    "Lk64":              (2, 2, 70, 64,  None,             None,          0.0),
    "Lk65":              (2, 2, 70, 65,  None,             None,          0.0),
    "Lk33":              (2, 2, 70, 33,  None,             None,          0.0),
    "Lq129":             (2, 2, 129, 200, None,            None,          0.0),
    "Lk330":             (2, 2, 70, 330, None,             None,          0.0),     # >= 256 keys: the key split's shape
    "Lk330_lead96":      (2, 2, 70, 330, "lead96",         None,          0.0),
    "max_in_first_tile": (2, 2, 70, 200, None,             (5,),          0.0),
    "max_in_last_full_tile": (2, 2, 70, 200, None,         (150,),        0.0),
    "max_in_ragged_tail": (2, 2, 70, 200, None,            (197,),        0.0),
    "dropout_half":      (2, 2, 70, 200, None,             None,          0.5),
}
INT_SEED = 0x51ED270B0F1E2D3C


class IntegerCase:
    pass


@functools.lru_cache(maxsize=None)
def integer_case(name):
    B, H, Lq, Lk, mask, plant, p = INTEGER_CASES[name]
    g = gen("int", name)
    if float(np.float32(INT_SCALE) * np.float32(LOG2E)) != 0.25:
        raise PremiseError("fl32(scale * log2e) is not 0.25")
    n = torch.randint(1, 4, (B, H, Lq, 1), generator=g)
    col = torch.randint(0, D, (B, H, Lq, 1), generator=g)
    q = torch.zeros(B, H, Lq, D).scatter_(-1, col, 4.0 * n)
    top = (torch.arange(Lk) // 32 - 4).clamp(max=-1)                       # sub-tile 0: -6..-4, 1: -6..-3, 2: -6..-2, then -6..-1
    k = (-6 + torch.randint(0, 1 << 30, (B, H, Lk, D), generator=g) % (top + 7).view(1, 1, Lk, 1)).float()
    plant = plant or (5, Lk - 1, (Lk // 64) * 64 - 14 if Lk >= 128 else Lk // 2, Lk // 2 + 3)
    for b in range(B):
        for h in range(H):
            k[b, h, plant[(b * H + h) % len(plant)]] = 0.0
    v = torch.randint(-4, 5, (B, H, Lk, D), generator=g).float()
    c = IntegerCase()
    c.name, c.B, c.H, c.Lq, c.Lk, c.p = name, B, H, Lq, Lk, p
    c.q, c.k, c.v = unheads(q), unheads(k), unheads(v)
    c.kpm = key_mask(mask, B, Lk)
    c.keep = keep_mask(INT_SEED, B, H, Lq, Lk, p) if p > 0 else None
    # the reference, exactly
    s = (q.double() * 0.25) @ k.double().transpose(-1, -2)
    if not bool((s == s.round()).all()):
        raise PremiseError("scores are not integers")
    live = torch.ones(B, 1, 1, Lk, dtype=torch.bool) if c.kpm is None else ~c.kpm[:, None, None, :]
    live = live.expand_as(s)
    big = s.abs().max() + 1
    m = torch.where(live, s, -big).amax(-1, keepdim=True)
    lo = torch.where(live, s, big).amin(-1, keepdim=True)
    e = torch.where(live, torch.ldexp(torch.ones_like(s), (s - m).clamp(min=-60).to(torch.int32)), torch.zeros_like(s))
    l = e.sum(-1, keepdim=True)
    any_live = l > 0
    spread = torch.where(any_live, m - lo, torch.zeros_like(m))
    mass = torch.maximum(l, (e @ v.double().abs()).amax(-1, keepdim=True))
    c.budget_bits = float(torch.log2(mass.clamp(min=1.0) * torch.exp2(spread)).max())
    if not c.budget_bits < 24.0:
        raise PremiseError("partial sums need %.2f bits" % c.budget_bits)
    kept = e if c.keep is None else e * c.keep.double()
    rinv = 1.0 / (1.0 - float(np.float32(p)))                              # (p = 0.5: exactly 2)
    ref = torch.where(any_live, rinv * (kept @ v.double()) / l.clamp(min=1.0), torch.zeros(()).double())
    c.ref = unheads(ref)
    c.one_live = mask in ("one_live_last", "one_live_first")
    # bf16: the elements whose rounding the fp32 value before the store cannot decide differently
    r32 = c.ref.float()
    down = (r32.view(torch.int32) & -65536).view(F32).double()
    up = ((r32.view(torch.int32) & -65536) + 65536).view(F32).double()
    c.decided = ((c.ref - (down + up) / 2).abs() > 2.0 ** -22 * c.ref.abs()) | (c.ref == 0)
    c.ref_bf16 = c.ref.to(BF16)
    rounds = c.ref_bf16.double() != c.ref
    if (~c.decided).double().mean() > 0.01:
        raise PremiseError("%.2f %% of the elements are near a bf16 midpoint" % (100 * (~c.decided).double().mean()))
    if not c.one_live and rounds.double().mean() < 0.10:
        raise PremiseError("only %.1f %% of the bf16 results need rounding" % (100 * rounds.double().mean()))
    if c.one_live and not torch.equal(c.ref, unheads(v.double()[:, :, (Lk - 1 if mask == "one_live_last" else 0)][:, :, None].expand(B, H, Lq, D))):
        raise PremiseError("one live key: the result is not that key's v")
    return c


def check_integer_forward(fused_attention, name, dtype, device):
    """Run the forward of integer case `name` and assert it to the bit (see the module docstring)."""
    c = integer_case(name)
    q, k, v = (t.to(dtype).to(device) for t in (c.q, c.k, c.v))
    out = fused_attention(q, k, v, c.H, dropout_p=c.p, key_padding_mask=None if c.kpm is None else c.kpm.to(device),
                          scale=INT_SCALE, seed=INT_SEED if c.p > 0 else None).cpu()
    assert out.dtype == dtype and out.shape == c.ref.shape
    err = (out.double() - c.ref).abs()
    rel = float((err / c.ref.abs().clamp(min=1e-300)).max())
    if dtype == F32:
        print("integer %s fp32: worst error %.3f x 2^-23 |ref| (budget %.2f bits)" % (name, rel * 2.0 ** 23, c.budget_bits))
        assert bool((err <= 2.0 ** -23 * c.ref.abs()).all())
    else:
        same = out[c.decided] == c.ref_bf16[c.decided]
        print("integer %s bf16: %.4f %% of %d decided elements equal bf16(ref)" % (name, 100 * same.double().mean(), same.numel()))
        assert bool(same.all())


# ---- (b) random and peaked -------------------------------------------------------------------------------------------------------------
RANDOM_CASES = {
    #  name              B  H  Lq  Lk   std  mask              p    packed scale
    "std1":             (1, 2, 70, 200, 1,  None,             0.0, False, None),
    "std8":             (1, 2, 70, 200, 8,  None,             0.0, False, None),
    "std30":            (1, 2, 70, 200, 30, None,             0.0, False, None),
    "wide_std8":        (1, 2, 40, 330, 8,  None,             0.0, False, None),     # >= 256 keys: the key split's shape
    "wide_std30":       (1, 2, 40, 330, 30, None,             0.0, False, None),
    "lead96":           (2, 2, 70, 200, 8,  "lead96",         0.0, False, None),
    "inner64_127":      (2, 1, 70, 200, 8,  "inner64_127",    0.0, False, None),
    "tail190":          (2, 1, 70, 200, 8,  "tail190",        0.0, False, None),
    "one_live_last":    (2, 1, 70, 200, 8,  "one_live_last",  0.0, False, None),
    "image_masked":     (2, 2, 70, 200, 8,  "image_masked",   0.0, False, None),
    "wide_lead96":      (2, 1, 40, 330, 8,  "lead96",         0.0, False, None),
    "dropout":          (1, 2, 70, 200, 8,  None,             0.1, False, None),
    "dropout_lead96":   (2, 2, 70, 200, 8,  "lead96",         0.1, False, None),
    "packed":           (2, 2, 77, 77,  8,  None,             0.0, True,  None),
    "scale":            (1, 2, 70, 200, 8,  None,             0.0, False, 0.3),
}
RND_SEED = 0x0FEDCBA987654321


class RandomCase:
    pass


@functools.lru_cache(maxsize=None)
def random_case(name, dtype):
    B, H, Lq, Lk, std, mask, p, packed, scale = RANDOM_CASES[name]
    g = gen("rnd", name)
    E = H * D
    c = RandomCase()
    c.name, c.dtype, c.B, c.H, c.Lq, c.Lk, c.p, c.scale_arg = name, dtype, B, H, Lq, Lk, p, scale
    c.scale = float(np.float32(D ** -0.5 if scale is None else scale))       # what the kernels receive (a C float)
    qmul = std / (c.scale * D ** 0.5)                                        # logits q k scale ~ N(0, std^2)
    if packed:
        x = torch.randn(B, Lq, 3 * E, generator=g)
        x[..., :E] *= qmul
        c.packed = x.to(dtype)
        c.q, c.k, c.v = c.packed.split(E, -1)
    else:
        c.packed = None
        c.q = (torch.randn(B, Lq, E, generator=g) * qmul).to(dtype)
        c.k, c.v = (torch.randn(B, Lk, E, generator=g).to(dtype) for _ in range(2))
    c.go = torch.randn(B, Lq, E, generator=g).to(dtype)
    c.kpm = key_mask(mask, B, Lk)
    c.keep = keep_mask(RND_SEED, B, H, Lq, Lk, p) if p > 0 else None
    _analyse(c)
    return c


def _softmax2(s, live):
    """log2-domain scores -> (e relative to the row maximum, l, P); masked keys and fully masked rows give exact zeros."""
    s = s.masked_fill(~live, float("-inf"))
    m = s.amax(-1, keepdim=True)
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    e = torch.exp2(s - m)
    l = e.sum(-1, keepdim=True)
    return e, l, torch.where(l > 0, e / l.clamp(min=1e-300), torch.zeros_like(e))


def _chain(V, G, P, Kp, out):
    """D from `out`, the dropped and rescaled dP, and dS = P (dPd - D)."""
    Dq = (G * out).sum(-1, keepdim=True)
    dPd = (G @ V.transpose(-1, -2)) * Kp
    dS = P * (dPd - Dq)
    return Dq, dPd, dS


def _analyse(c):
    H, Lq, Lk = c.H, c.Lq, c.Lk
    Q, K, V, G = (heads(t, H) for t in (c.q, c.k, c.v, c.go))
    live = (torch.ones(c.B, Lk, dtype=torch.bool) if c.kpm is None else ~c.kpm)[:, None, None, :].expand(c.B, H, Lq, Lk)
    p32 = float(np.float32(c.p))
    rinv = 1.0 / (1.0 - p32)
    keepf = torch.ones(()).double() if c.keep is None else c.keep.double()
    Kp = keepf * rinv
    scale = c.scale
    T_ = lambda t: t.transpose(-1, -2)

    # fp64 truth
    e, l, P = _softmax2((Q @ T_(K)) * (scale * LOG2E), live)
    Pd = P * Kp
    out = Pd @ V
    Dq, dPd, dS = _chain(V, G, P, Kp, out)
    c.truth = dict(out=out, dq=scale * (dS @ K), dk=scale * (T_(dS) @ Q), dv=T_(Pd) @ G)
    A_out = Pd @ V.abs()
    A_D = (G.abs() * A_out).sum(-1, keepdim=True)

    if c.dtype == BF16:
        c32 = float(np.float32(scale) * np.float32(LOG2E))
        Qs = (Q.float() * c32).to(BF16).double()
        s2 = (Qs @ T_(K)).masked_fill(~live, float("-inf"))
        e, l, P = _softmax2(s2, live)
        out_m = bf(rinv * (bf(e * keepf) @ V) / l.clamp(min=1e-300)) * (l > 0)
        # the backward reads lse from the forward's float32 buffer: a store like the others (half an fp32 ulp of |lse| ~ 30 .. 200 is
        # 2^-20 .. 2^-17 relative in P, the largest fp32 term between kernel and model)
        m = torch.where(l > 0, s2.amax(-1, keepdim=True), torch.zeros_like(l))
        lse32 = (m + torch.log2(l.clamp(min=1e-300))).float().double()
        P = torch.where(l > 0, torch.exp2(s2 - lse32), torch.zeros_like(e))
        Dq, dPd, dS = _chain(V, G, P, Kp, out_m)
        dSb = bf(dS)
        c.model = dict(out=out_m, dq=bf(scale * (dSb @ K)), dk=bf(INVLOG2E32 * (T_(dSb) @ Qs)), dv=bf(rinv * (T_(bf(P * keepf)) @ G)))
        Pd = P * Kp
        A_out = Pd @ V.abs()
        A_D = (G.abs() * A_out).sum(-1, keepdim=True)
        W = P * (dPd.abs() + A_D)
        c.A = dict(out=A_out, dq=scale * (W @ K.abs()), dk=(T_(W) @ Qs.abs()) / LOG2E, dv=T_(Pd) @ G.abs())
        c.bound = {n: 2.0 ** -7 * a for n, a in c.A.items()}
    else:
        T = (Q.abs() @ T_(K.abs())) * (scale * LOG2E)
        Tbar = (P * T).sum(-1, keepdim=True)
        eta = lambda L: (2.0 * L + 64.0) * 2.0 ** -24
        relP = lambda L: math.log(2.0) * EPS_S * (T + Tbar) + eta(L)
        B_out = (Pd * relP(Lk)) @ V.abs()
        B_D = (G.abs() * B_out).sum(-1, keepdim=True) + 40 * 2.0 ** -24 * A_D
        B_dP = 40 * 2.0 ** -24 * (G.abs() @ T_(V.abs())) * Kp
        B_dS = P * relP(Lk) * (dPd.abs() + Dq.abs()) + P * (B_dP + B_D) + 2.0 ** -23 * dS.abs()
        c.bound = dict(out=B_out,
                       dq=scale * (B_dS @ K.abs() + eta(Lk) * (dS.abs() @ K.abs())),
                       dk=scale * (T_(B_dS) @ Q.abs() + eta(Lq) * (T_(dS.abs()) @ Q.abs())),
                       dv=T_(Pd * relP(Lk + Lq)) @ G.abs())
    for d in (c.truth, c.bound) + ((c.model, c.A) if c.dtype == BF16 else ()):
        for n in d:
            d[n] = unheads(d[n])


def run_random(fused_attention, c, device):
    """The kernels on case `c`: dict(out, dq, dk, dv) on the CPU.  A packed case passes the three slices of ONE leaf tensor and
    takes its gradient apart."""
    E = c.H * D
    if c.packed is not None:
        leaf = c.packed.clone().to(device).requires_grad_(True)            # (a copy: the case is shared and stays as it is)
        q, k, v = leaf.split(E, -1)
    else:
        q, k, v = (t.clone().to(device).requires_grad_(True) for t in (c.q, c.k, c.v))
    out = fused_attention(q, k, v, c.H, dropout_p=c.p, key_padding_mask=None if c.kpm is None else c.kpm.to(device),
                          scale=c.scale_arg, seed=RND_SEED if c.p > 0 else None)
    out.backward(c.go.to(device))
    dq, dk, dv = leaf.grad.split(E, -1) if c.packed is not None else (q.grad, k.grad, v.grad)
    got = dict(out=out.detach(), dq=dq, dk=dk, dv=dv)
    for n, t in got.items():
        assert t.dtype == c.dtype, n
    return {n: t.cpu() for n, t in got.items()}


def random_ratios(c, got):
    """Per tensor: (worst |error| / bound over the elements with a non-zero bound, are the zero-bound elements exact zeros, and for
    bf16 the Frobenius figures (||kernel - fp64||, ||model - fp64||, ||A||))."""
    res = {}
    centre = c.model if c.dtype == BF16 else c.truth
    for n in ("out", "dq", "dk", "dv"):
        g, bound = got[n].double(), c.bound[n]
        err = (g - centre[n]).abs()
        pos = bound > 0
        ratio = float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0
        zeros_exact = bool((g[~pos] == 0).all())
        fro = None
        if c.dtype == BF16:
            fro = (float((g - c.truth[n]).norm()), float((c.model[n] - c.truth[n]).norm()), float(c.A[n].norm()))
        res[n] = (ratio, zeros_exact, fro)
    return res


def check_random(fused_attention, name, dtype, device):
    c = random_case(name, dtype)
    res = random_ratios(c, run_random(fused_attention, c, device))
    line = "random %s %s:" % (name, "bf16" if dtype == BF16 else "fp32")
    for n, (ratio, zeros_exact, fro) in res.items():
        line += " %s %.3f" % (n, ratio)
        if fro:
            line += " (fro %.3g vs model %.3g)" % (fro[0] / max(c.truth[n].norm().item(), 1e-300), fro[1] / max(c.truth[n].norm().item(), 1e-300))
    print(line)
    for n, (ratio, zeros_exact, fro) in res.items():
        assert zeros_exact, "%s: an element that must be exactly 0 is not" % n
        assert ratio <= 1.0, "%s: error / bound = %.3f" % (n, ratio)
        if fro:
            assert fro[0] <= 2.0 * fro[1] + 2.0 ** -7 * fro[2], "%s: %.4g > 2 x %.4g + 2^-7 x %.4g" % ((n,) + fro)
    # the masked keys and the fully masked rows that the case is about are there
    if c.kpm is not None:
        assert bool((c.bound["dk"][c.kpm] == 0).all()) and bool((c.bound["dv"][c.kpm] == 0).all())
        dead = c.kpm.all(1)
        assert bool((c.bound["out"][dead] == 0).all()) and bool((c.bound["dq"][dead] == 0).all())
    return res
