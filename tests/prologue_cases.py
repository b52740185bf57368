"""Cases, references and checks for csrc/msda_prologue.hip: the softmax over a head's L P attention logits and the sampling
locations of MSDeformAttn.forward, forward and backward, in the two-tensor form, the packed form (one projection output holding
offsets | logits per query: what the model calls) and on views at an odd storage offset (the element-wise kernels).  Test
infrastructure: plain torch in fp64, no kernel code; tests/test_prologue_cases_gpu.py runs the cases on the device,
tests/test_prologue_cases_emulated_cpu.py through tests/native_emul.py.

REFERENCE.  `reference` writes the operator out in fp64 with x_i = logit_i - max(logit):
    attn_i = exp(x_i) / sum_j exp(x_j)                          g_logit_i = attn_i (g_attn_i - sum_j attn_j g_attn_j)
    loc    = ref_c + off / (W_l, H_l)_c            (R = 2)      g_off = g_loc / (W_l, H_l)_c      g_ref_c = sum_{m,p} g_loc
    loc    = ref_c + off / P (ref_2+2c + ref_3+2c) 0.5  (R = 6) g_off = g_loc / P extent 0.5      g_ref_c = sum g_loc,
                                                                g_ref_{2+2c} = g_ref_{3+2c} = sum_{m,p} g_loc (off / P) 0.5
together with the NATURAL MAGNITUDE of every result -- the same expression with every term replaced by its absolute value -- plus
the amplification of an input's own fp32 rounding where it feeds the exponential: x_i is an fp32 difference (2^-24 |x_i| off), so
    n_i = attn_i (1 + |x_i|),   scale(attn) = max_i n_i over the (b, q, m) row,
    scale(g_logits) = max_i n_i (|g_attn_i| + sum_j n_j |g_attn_j|) over the row
(the row's largest: an underflowed weight is not asked for a relative accuracy it cannot have),
    scale(g_off) = |g_loc| / (W, H)  or  |g_loc| / P (|ref_2+2c| + |ref_3+2c|) 0.5          per element,
    scale(g_ref) = the largest over the (b, q, l) row of  sum |g_loc|  /  sum |g_loc| |off| / P 0.5.
`anchor` shows once that the reference is the module's formulation (tests/test_msda_prologue_cpu.py `torch_prologue`) with autograd
in float64, to 1e-12.

BOUND (the project's rule, criterion_cases.py; no new number).  Per element
    B = max(8 x the error of `torch_prologue` in fp32 on the same device and inputs within the element's row, 64 x 2^-24 x scale),
row = one (b, q, m) for attn, g_logits and g_offsets, one (b, q, l) for g_ref.  The fp32-I/O kernel carries the comparison with
fp64.  The bf16-I/O instantiations get no tolerance: on the same bf16-representable inputs `loc` and `attn` must equal the fp32-I/O
kernel's bit for bit, g_offsets / g_logits must equal `.to(bfloat16)` of the fp32-I/O kernel's, g_ref (fp32 atomics over the heads, in
any order) must lie within B.  Where the reference points are bf16 the function returns g_ref rounded to bf16: the value may then be
half a bf16 step (of |v| + B) further off, the one rounding of the number format.
The packed form must give the bits of the two-tensor form on the same data (g_ref within B).
`loc` is asserted bit for bit against the module's fp32 formula evaluated on the CPU: pro_location has contraction off and every
operation (add, divide, multiply) is correctly rounded, so there is one fp32 answer.

EXACT CASES (equality; premises raise `PremiseError` from the operands and the reference alone).  Every row's logits are equal (an
integer in -3 .. 3 that varies by row), g_attn and g_loc are integers in +-64, offsets integers in +-8, reference points multiples of
1 / 64, level sizes powers of two.  Then attn == fp32(1 / LP) for any LP; for LP a power of two g_logits == (g - sum g / LP) / LP, the
fp64 value rounded once to the I/O type; g_offsets and g_ref are dyadic rationals that fp32 holds in any order of the atomics: the
fp64 value (rounded once where the type is bf16).  Premise for LP >= 16 with bf16 I/O: >= 10 % of the g_logits are no bf16 numbers
and >= 1 % are exact ties.
FACTS asserted in every bounded case, on the elements that the inputs and the fp64 reference single out: LP = 1: attn == 1 and
g_logits == 0; a weight that is 0 in fp64 (a logit 10^4 below the row's maximum) is 0 and so is its gradient; logits that tie for the
row's maximum get equal weights; R = 6 with a zero extent: loc == ref[..., :2] and g_offsets == 0.  The "edges" kind builds such rows
(premises: they exist wherever LP >= 2).

Every check prints its figures ("prologue_case ..." lines: worst error / bound per tensor, and the framework's own error over the
floor) before it asserts; the device's are in profiles/pointwise_cases_measured.txt.  No share of elements is left out.  No bound was
widened.  The closest figure, on the device and the emulation alike, is attn at LP = 64 with one logit 12 above the rest (0.143 of B;
g_logits 0.108 there): 63 weights of e^-12 whose exponential's argument carries 12 x 2^-24.
DEFECT FOUND on the device by the bf16-against-fp32 equality (peaked rows, L P = 16; 1 - 11 g_logits per case): the compiler contracted
the sum of pro_softmax_backward differently in every instantiation of the unrolled kernels, and where g_attn - dot cancels the last bit
of dot decided a bf16 rounding.  Fixed in csrc/msda_prologue_math.h (a chain of explicit fmaf, contraction off)."""
import contextlib
import functools
import math
import zlib

import torch

from exact_cases import PremiseError, _need, assert_bits_equal, bf16_rounding_shares
from test_msda_prologue_cpu import torch_prologue

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
FLOOR = 64.0 * 2.0 ** -24
MARGIN = 8.0

#           (B, Lq, M, L, P)
SHAPES = {
    "unit":     (1, 1, 1, 4, 4),        # one unit
    "ragged":   (2, 37, 8, 4, 4),       # 592 units: two blocks and a ragged third
    "m5":       (1, 33, 5, 4, 4),       # M = 5: packed pitch 240
    "lp16":     (2, 19, 8, 2, 8),       # LP = 16 without L = P = 4: prologue_*_kernel<.., 16>
    "generic":  (2, 9, 8, 3, 2),        # the generic path, LP = 6
    "cap":      (1, 5, 3, 8, 8),        # LP = 64 = kPrologueMaxLP
    "lp1":      (1, 7, 2, 1, 1),        # LP = 1
}
LEVELS = ((48, 160), (24, 80), (12, 40), (6, 20), (3, 10), (2, 5), (1, 3), (1, 1))
EXACT_LEVELS = ((16, 64), (8, 32), (4, 16), (2, 8), (1, 4), (1, 2), (1, 1), (2, 2))
KINDS = ("benign", "peak12", "peak30", "peak100", "shift80", "offsets1e3", "extents", "edges")
FP32_ONLY = ("peak100", "shift80")      # (bf16 logits of 80 + N(0, 1) or 100 + N(0, 1) hold steps of 0.5: nothing left of the row)


def forms(shape):
    """two-tensor always; L = P = 4 also the packed form and views at an odd storage offset (the element-wise <.., 16> kernels)."""
    return ("two", "packed", "odd") if shape[3:] == (4, 4) else ("two",)


def kinds(R, io):
    return tuple(k for k in KINDS if not (k == "extents" and R == 2) and not (k in FP32_ONLY and io == BF16))


def thinned(name, R, io):
    """(kind, expanded, ref dtype, form) of one shape, R and I/O type: the benign and the edge rows with every combination of
    reference-point layout and type, the other kinds with one each in turn; every form throughout."""
    out = []
    for i, kind in enumerate(kinds(R, io)):
        for e, (expanded, rdt) in enumerate(((False, F32), (True, F32), (False, BF16), (True, BF16))):
            if kind in ("benign", "edges") or e == (i + R // 6 + (io == BF16)) % 4:
                out += [(kind, expanded, rdt, form) for form in forms(SHAPES[name])]
    return out


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


@contextlib.contextmanager
def kernels_on(backend=None):
    """Route the extension to `backend` (the emulated library) for the duration; None: the device library."""
    from monodetr_amd import msda_prologue_ext
    saved = msda_prologue_ext._backend
    if backend is not None:
        msda_prologue_ext._backend = backend
    try:
        yield msda_prologue_ext
    finally:
        msda_prologue_ext._backend = saved


# ---- reference -------------------------------------------------------------------------------------------------------------------------
def reference(off, lg, ref, shapes, g_loc, g_attn):
    """fp64.  off [B,Lq,M,L,P,2], lg [B,Lq,M,LP], ref [B,Lq,L,R] (full), shapes [L,2] (H, W), g_loc like off, g_attn [B,Lq,M,L,P]."""
    B, Lq, M, L, P, _ = off.shape
    R = ref.shape[-1]
    ga = g_attn.reshape(B, Lq, M, L * P)
    x = lg - lg.amax(-1, keepdim=True)
    e = torch.exp(x)
    attn = e / e.sum(-1, keepdim=True)
    g_lg = attn * (ga - (attn * ga).sum(-1, keepdim=True))
    n = attn * (1 + x.abs())
    s_attn = n.amax(-1, keepdim=True).expand_as(attn)
    s_glg = (n * (ga.abs() + (n * ga.abs()).sum(-1, keepdim=True))).amax(-1, keepdim=True).expand_as(attn)
    r = ref[:, :, None, :, None, :]                                            # [B,Lq,1,L,1,R]
    if R == 2:
        wh = shapes.flip(-1).double()[None, None, None, :, None, :]
        loc = r + off / wh
        g_off, s_goff = g_loc / wh, g_loc.abs() / wh
        g_ref, s_gref = g_loc.sum((2, 4)), g_loc.abs().sum((2, 4))
    else:
        extent = r[..., 2::2] + r[..., 3::2]                                   # [B,Lq,1,L,1,2]
        loc = r[..., :2] + off / P * extent * 0.5
        g_off, s_goff = g_loc / P * extent * 0.5, g_loc.abs() / P * (r[..., 2::2].abs() + r[..., 3::2].abs()) * 0.5
        ge, sge = (g_loc * (off / P) * 0.5).sum((2, 4)), (g_loc.abs() * (off.abs() / P) * 0.5).sum((2, 4))     # [B,Lq,L,2]
        g_ref = torch.cat((g_loc.sum((2, 4)), ge[..., :1], ge[..., :1], ge[..., 1:], ge[..., 1:]), -1)
        s_gref = torch.cat((g_loc.abs().sum((2, 4)), sge[..., :1], sge[..., :1], sge[..., 1:], sge[..., 1:]), -1)
    s_gref = s_gref.amax(-1, keepdim=True).expand_as(g_ref)
    return dict(attn=attn.view(B, Lq, M, L, P), loc=loc, g_lg=g_lg, g_off=g_off, g_ref=g_ref, x=x,
                scale=dict(attn=s_attn.reshape(B, Lq, M, L, P), g_lg=s_glg, g_off=s_goff, g_ref=s_gref.contiguous()))


def anchor():
    """`reference` is the module's formulation with autograd in float64 (1e-12 of each tensor's largest entry), both R forms."""
    for R, (L, P) in ((2, (4, 4)), (6, (3, 2))):
        g = gen("anchor", R)
        B, Lq, M = 2, 5, 3
        shapes = torch.tensor(LEVELS[:L])
        off = (3 * torch.randn(B, Lq, M, L, P, 2, generator=g, dtype=F64)).requires_grad_(True)
        lg = torch.randn(B, Lq, M, L * P, generator=g, dtype=F64).requires_grad_(True)
        ref = torch.rand(B, Lq, L, R, generator=g, dtype=F64).requires_grad_(True)
        g_loc, g_attn = torch.randn(B, Lq, M, L, P, 2, generator=g, dtype=F64), torch.randn(B, Lq, M, L, P, generator=g, dtype=F64)
        r = ref[:, :, None, :, None, :]
        w = torch.softmax(lg, -1).view(B, Lq, M, L, P)
        loc = r + off / shapes.flip(-1).double()[None, None, None, :, None, :] if R == 2 else r[..., :2] + off / P * (r[..., 2::2] + r[..., 3::2]) * 0.5
        grads = torch.autograd.grad([loc, w], [off, lg, ref], [g_loc, g_attn])
        want = reference(off.detach(), lg.detach(), ref.detach(), shapes, g_loc, g_attn)
        for name, t in (("loc", loc.detach()), ("attn", w.detach()), ("g_off", grads[0]), ("g_lg", grads[1]), ("g_ref", grads[2])):
            assert float((t - want[name]).abs().max()) <= 1e-12 * float(want[name].abs().max()), (R, name)


# ---- running the kernel and the framework path ------------------------------------------------------------------------------------------
def _full_ref(base, expanded, L):
    return base[:, :, None].expand(-1, -1, L, -1) if expanded else base


def _odd(t, device):
    """A contiguous view one element into its storage: not 16-byte aligned."""
    buf = torch.zeros(t.numel() + 1, dtype=t.dtype)
    buf[1:] = t.reshape(-1)
    view = buf.to(device)[1:].view(t.shape)
    if view.data_ptr() % 16 == 0:
        raise PremiseError("the view is 16-byte aligned: the element-wise kernel is not taken")
    return view.requires_grad_(True)


def run(c, io, form, device, backend=None):
    """The kernel through the product's autograd functions, inputs widened / kept at `io` -> CPU tensors loc, attn, g_off, g_lg,
    g_ref [B,Lq,L,R] (the gradient arriving at the reference-point tensor the call was given, expanded or not)."""
    B, Lq, M, L, P = c.shape
    off, lg = c.off.to(io), c.lg.to(io)
    base = c.base.to(device).requires_grad_(True)
    ref = _full_ref(base, c.expanded, L)
    shapes, g_loc, g_attn = c.shapes.to(device), c.g_loc.to(device), c.g_attn.to(device)
    with kernels_on(backend) as ext:
        if form == "packed":
            packed = torch.cat((off.reshape(B, Lq, -1), lg.reshape(B, Lq, -1)), -1).to(device).requires_grad_(True)
            if not ext.packed_supported(packed, ref, L, P):
                raise PremiseError("the packed form does not take this call")
            loc, attn = ext.msda_prologue_packed(packed, ref, shapes, M, L, P)
            g_packed, g_ref = torch.autograd.grad([loc, attn], [packed, ref], [g_loc, g_attn])
            assert g_packed.dtype == io
            g_off, g_lg = g_packed[..., :M * L * P * 2].reshape(B, Lq, M, L, P, 2), g_packed[..., M * L * P * 2:].reshape(B, Lq, M, L * P)
        else:
            if form == "odd":
                o, l_ = _odd(off, device), _odd(lg, device)
            else:
                o, l_ = off.to(device).requires_grad_(True), lg.to(device).requires_grad_(True)
            loc, attn = ext.msda_prologue(o, l_, ref, shapes)
            g_off, g_lg, g_ref = torch.autograd.grad([loc, attn], [o, l_, ref], [g_loc, g_attn])
            assert g_off.dtype == io and g_lg.dtype == io
    assert loc.dtype == F32 and attn.dtype == F32 and g_ref.dtype == c.base.dtype and g_ref.shape == (B, Lq, L, c.R)
    return {k: v.detach().cpu().contiguous() for k, v in dict(loc=loc, attn=attn, g_off=g_off, g_lg=g_lg, g_ref=g_ref).items()}


def framework32(c, device):
    """The project's own fp32 framework path (`torch_prologue` and autograd) on `device`, on the widened inputs."""
    B, Lq, M, L, P = c.shape
    off, lg = c.off.float().to(device).requires_grad_(True), c.lg.float().to(device).requires_grad_(True)
    base = c.base.to(device).requires_grad_(True)
    ref = _full_ref(base, c.expanded, L)
    loc, attn = torch_prologue(off, lg, ref, c.shapes.to(device), P)
    g_off, g_lg, g_ref = torch.autograd.grad([loc, attn], [off, lg, ref], [c.g_loc.to(device), c.g_attn.to(device)])
    return {k: v.detach().cpu().contiguous() for k, v in dict(loc=loc, attn=attn, g_off=g_off, g_lg=g_lg, g_ref=g_ref).items()}


def cpu_locations(c):
    """The module's fp32 formula on the CPU: one correctly rounded operation after the other."""
    B, Lq, M, L, P = c.shape
    return torch_prologue(c.off.float(), c.lg.float(), _full_ref(c.base, c.expanded, L), c.shapes, P)[0].contiguous()


# ---- figures ---------------------------------------------------------------------------------------------------------------------------
def _rowmax(t, dims):
    return t.amax(dims, keepdim=True).expand_as(t) if dims else t


ROW = dict(attn=(3, 4), g_lg=(3,), g_off=(3, 4, 5), g_ref=(3,))


def bound(name, fw, ref64, scale):
    err32 = (fw.double() - ref64).abs()
    return torch.maximum(MARGIN * _rowmax(err32, ROW[name]), FLOOR * scale), err32


def _ratio(err, B):
    r = torch.where(B > 0, err / B, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
    r = torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)
    return float(r.max()) if r.numel() else 0.0


def _half_step(v):
    return torch.ldexp(torch.ones_like(v), torch.frexp(v)[1] - 9)              # half the bf16 spacing in v's binade (v > 0)


def within(tag, name, got, c, fw, figs, failures):
    """got within B of the fp64 value, element by element; records err/B and the framework's err over the floor."""
    ref64, scale = c.ref[name], c.ref["scale"][name]
    B, err32 = bound(name, fw[name], ref64, scale)
    if got.dtype == BF16:                                                      # (g_ref of bf16 reference points: rounded once more)
        B = B + _half_step(ref64.abs() + B)
    err = (got.double() - ref64).abs()
    figs[name] = (_ratio(err, B), _ratio(err32, FLOOR * scale))
    bad = ~(err <= B)
    if bool(bad.any()):
        idx = tuple(int(i) for i in torch.nonzero(bad)[0])
        failures.append("%s %s: %d elements beyond the bound, worst err/B %.3g, first at %s: got %r, fp64 %r, B %.3g" % (
            tag, name, int(bad.sum()), figs[name][0], idx, float(got[idx]), float(ref64[idx]), float(B[idx])))


# ---- cases ----------------------------------------------------------------------------------------------------------------------------
class Case:
    pass


def _finish(c, off, lg, base, g):
    B, Lq, M, L, P = c.shape
    c.off, c.lg, c.base = off.to(c.io), lg.to(c.io), base.to(c.rdt)
    c.ref = reference(c.off.double(), c.lg.double(), _full_ref(c.base.double(), c.expanded, L).contiguous(), c.shapes,
                      c.g_loc.double(), c.g_attn.double())
    return c


@functools.lru_cache(maxsize=8)
def bounded_case(name, kind, R, expanded, rdt, io):
    B, Lq, M, L, P = shape = SHAPES[name]
    LP = L * P
    g = gen("prologue", name, kind, R, expanded)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)                    # noqa: E731
    c = Case()
    c.shape, c.kind, c.R, c.expanded, c.rdt, c.io = shape, kind, R, expanded, rdt, io
    c.shapes = torch.tensor(LEVELS[:L], dtype=torch.int64)
    off, lg = 3 * rn(B, Lq, M, L, P, 2), rn(B, Lq, M, LP)
    base = torch.rand(*((B, Lq, R) if expanded else (B, Lq, L, R)), generator=g, dtype=F64)
    c.g_loc, c.g_attn = rn(B, Lq, M, L, P, 2).float(), rn(B, Lq, M, L, P).float()
    j = torch.randint(0, LP, (B, Lq, M, 1), generator=g)
    if kind.startswith("peak"):
        lg.scatter_add_(-1, j, torch.full((B, Lq, M, 1), float(kind[4:]), dtype=F64))
    elif kind == "shift80":
        lg += 80.0
    elif kind == "offsets1e3":
        off *= 1e3 / 3
    elif kind == "extents":                                                    # t + b, l + r near 0 and near 2
        near0 = torch.rand(base[..., 2:].shape, generator=g) < 0.5
        u = torch.rand(base[..., 2:].shape, generator=g, dtype=F64)
        base[..., 2:] = torch.where(near0, 1e-6 * u, 1 - 1e-3 * u)
    elif kind == "edges":
        rows = torch.arange(B * Lq * M).view(B, Lq, M, 1) % 4
        j2 = (j + 1 + torch.randint(0, max(LP - 1, 1), (B, Lq, M, 1), generator=g)) % LP       # another sample (LP >= 2)
        at = lambda k: torch.zeros(B, Lq, M, LP, dtype=torch.bool).scatter_(-1, k, True)       # noqa: E731
        if LP >= 2:
            lg = torch.where((rows == 0) & at(j), lg - 1e4, lg)                # one logit 10^4 below the row's maximum
            lg = torch.where(rows == 1, torch.where(at(j) | at(j2), torch.full_like(lg, 5.0), lg - 60.0), lg)    # two tied maxima, the rest far below
            lg = torch.where((rows == 2) & ~at(j), lg - 1e4, lg)               # every logit but one 10^4 below
        if R == 6:
            base[:, ::2, ..., 2:] = 0.0                                        # zero extent: every other query
    _finish(c, off, lg, base, g)
    # the rows the facts of the module docstring are asserted on, from the operands and the fp64 reference alone
    lg64 = c.lg.double()
    c.dead = c.ref["attn"].view(B, Lq, M, LP) == 0
    c.tied = (lg64 == lg64.amax(-1, keepdim=True))
    full = _full_ref(c.base.double(), expanded, L)
    c.flat = (full[..., 2::2] + full[..., 3::2]) == 0 if R == 6 else None      # [B,Lq,L,2]: the extent of x, of y
    if kind == "edges" and LP >= 2:
        if not (bool(c.dead.any()) and (B * Lq * M < 2 or bool((c.tied.sum(-1) == 2).any()))):
            raise PremiseError("edges: no dead weight or no tied pair of maxima")
        if not bool(((lg64.amax(-1, keepdim=True) - lg64) >= 9e3).any()):
            raise PremiseError("edges: no logit 10^4 below its row's maximum")
        if R == 6 and not bool(c.flat.any()):
            raise PremiseError("edges: no zero extent")
    if kind == "extents" and not (float(c.base[..., 2:].min()) < 1e-5 and float(c.base[..., 2:].max()) > 0.99):
        raise PremiseError("extents: not near 0 and near 2")
    return c


def _line(tag, figs):
    return "prologue_case %s  err/B (fp32 framework err/floor):  " % tag + "  ".join("%s %.3f (%.3f)" % ((k,) + figs[k]) for k in figs)


def check_facts(tag, c, got, failures):
    B, Lq, M, L, P = c.shape
    LP = L * P
    attn, g_lg = got["attn"].view(B, Lq, M, LP), got["g_lg"].float()
    if LP == 1 and not (bool((attn == 1).all()) and bool((g_lg == 0).all())):
        failures.append(tag + ": LP = 1 but attn != 1 or g_logits != 0")
    if bool(c.dead.any()) and not (bool((attn[c.dead] == 0).all()) and bool((g_lg[c.dead] == 0).all())):
        failures.append(tag + ": a weight that is 0 in fp64 is not 0, or its gradient is not")
    hi = torch.where(c.tied, attn, torch.full_like(attn, -1.0)).amax(-1)
    lo = torch.where(c.tied, attn, torch.full_like(attn, 2.0)).amin(-1)
    if not bool((hi == lo).all()):
        failures.append(tag + ": logits tied for the row's maximum got different weights")
    if c.flat is not None and bool(c.flat.any()):
        full = _full_ref(c.base.float(), c.expanded, L)
        flat = c.flat[:, :, None, :, None, :].expand(B, Lq, M, L, P, 2)
        want = full[:, :, None, :, None, :2].expand(B, Lq, M, L, P, 2)
        if not (bool((got["loc"][flat] == want[flat]).all()) and bool((got["g_off"].float()[flat] == 0).all())):
            failures.append(tag + ": zero extent but loc != ref or g_offsets != 0")


def check_bounded(name, kind, R, expanded, rdt, io, form, device, backend=None):
    c = bounded_case(name, kind, R, expanded, rdt, io)
    tag = "%s/%s/R%d/%s/ref_%s/io_%s/%s" % (name, kind, R, "expanded" if expanded else "full", str(rdt)[6:], str(io)[6:], form)
    fw = framework32(c, device)
    k32 = run(c, F32, form, device, backend)
    figs, failures = {}, []
    for t in ("attn", "g_lg", "g_off", "g_ref"):
        if not bool(torch.isfinite(k32[t].float()).all()):
            failures.append("%s %s is not finite" % (tag, t))
        within(tag, t, k32[t], c, fw, figs, failures)
    loc_bits = int((k32["loc"] != cpu_locations(c)).sum())
    checks = ["loc differs from the CPU formula in %d elements" % loc_bits]
    if loc_bits:
        failures.append("%s: loc differs from the module's fp32 formula in %d elements" % (tag, loc_bits))
    check_facts(tag, c, k32, failures)
    others = []
    if io == BF16:
        kb = run(c, BF16, form, device, backend)
        others.append(("bf16 I/O", kb, True))
        check_facts(tag + " bf16 I/O", c, kb, failures)
    if form == "packed":
        others.append(("two-tensor form", run(c, io, "two", device, backend), False))
    last = kb if io == BF16 else k32
    for what, o, narrow in others:
        a = k32 if narrow else last
        diff = {t: int((o[t] != (a[t].to(BF16) if narrow and t in ("g_off", "g_lg") else a[t])).sum()) for t in ("loc", "attn", "g_off", "g_lg")}
        checks.append("%s differs in %s" % (what, diff))
        if any(diff.values()):
            failures.append("%s: %s is not bit-identical: %s" % (tag, what, diff))
        f2 = {}
        within(tag + " " + what, "g_ref", o["g_ref"], c, fw, f2, failures)
        checks.append("its g_ref err/B %.3f" % f2["g_ref"][0])
    print(_line(tag, figs) + "  " + "; ".join(checks))
    assert not failures, "\n".join(failures)
    return figs


# ---- exact -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def exact_case(name, R, expanded, rdt, io):
    B, Lq, M, L, P = shape = SHAPES[name]
    LP = L * P
    g = gen("prologue_exact", name, R, expanded)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).double()                 # noqa: E731
    c = Case()
    c.shape, c.kind, c.R, c.expanded, c.rdt, c.io = shape, "exact", R, expanded, rdt, io
    c.shapes = torch.tensor(EXACT_LEVELS[:L], dtype=torch.int64)
    lg = ri(-3, 3, B, Lq, M, 1).expand(B, Lq, M, LP).contiguous()
    off = ri(-8, 8, B, Lq, M, L, P, 2)
    base = ri(0, 64, *((B, Lq, R) if expanded else (B, Lq, L, R))) / 64
    c.g_loc, c.g_attn = ri(-64, 64, B, Lq, M, L, P, 2).float(), ri(-64, 64, B, Lq, M, L, P).float()
    _finish(c, off, lg, base, g)
    if not (torch.equal(c.off.double(), off) and torch.equal(c.lg.double(), lg) and torch.equal(c.base.double(), base)):
        raise PremiseError("exact: an operand is not exact in its type")
    c.pow2 = LP & (LP - 1) == 0
    ga = c.g_attn.double().view(B, Lq, M, LP)
    c.want_glg = (ga - ga.sum(-1, keepdim=True) / LP) / LP
    if c.pow2 and not (torch.equal(c.ref["g_lg"], c.want_glg) and bool((c.ref["attn"] == 1.0 / LP).all())):
        raise PremiseError("exact: the fp64 reference is not the analytic value")
    for t in ("g_off", "g_ref", "loc") + (("g_lg",) if c.pow2 else ()):
        if not torch.equal(c.ref[t].float().double(), c.ref[t]):
            raise PremiseError("exact: %s is not exact in fp32" % t)
    c.shares = bf16_rounding_shares(c.want_glg)
    n = c.want_glg.numel()
    if c.pow2 and LP >= 16 and io == BF16 and (c.shares[0] * n < _need(0.10, n) or c.shares[1] * n < _need(0.01, n)):
        raise PremiseError("exact: g_logits that are no bf16 numbers %.3f, ties %.3f" % c.shares)
    return c


def check_exact(name, R, expanded, rdt, io, form, device, backend=None):
    c = exact_case(name, R, expanded, rdt, io)
    B, Lq, M, L, P = c.shape
    LP = L * P
    tag = "%s/exact/R%d/%s/ref_%s/io_%s/%s" % (name, R, "expanded" if expanded else "full", str(rdt)[6:], str(io)[6:], form)
    got = run(c, io, form, device, backend)
    want = dict(attn=torch.full((B, Lq, M, L, P), 1.0 / LP, dtype=F64).float(), loc=c.ref["loc"].float().expand(B, Lq, M, L, P, 2),
                g_off=c.ref["g_off"].float().to(io).expand(B, Lq, M, L, P, 2), g_ref=c.ref["g_ref"].float().to(rdt))
    if c.pow2:
        want["g_lg"] = c.want_glg.float().to(io)
    if LP == 1:
        want["g_lg"] = torch.zeros(B, Lq, M, 1, dtype=io)
    wrong = {k: int((got[k] != want[k]).sum()) for k in want}
    print("prologue_case %s premises: g_logits that are no bf16 numbers %.3f, exact ties %.3f; elements that differ: %s" % ((tag,) + c.shares + (wrong,)))
    assert_bits_equal(got["loc"], cpu_locations(c), tag + " loc against the CPU formula")
    for k in want:
        assert_bits_equal(got[k], want[k].contiguous(), "%s %s" % (tag, k))
