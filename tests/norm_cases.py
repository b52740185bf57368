"""Cases, references and checks for the two normalisation kernels: csrc/add_ln.hip (y = LayerNorm(a + dropout(b)) and its four
gradients) and csrc/group_norm.hip (GroupNorm (+ ReLU) of channels-last data, 8 channels per group, and its three gradients).  Test
infrastructure: plain torch in fp64, no kernel code; tests/test_norm_cases_gpu.py runs the cases on the device,
tests/test_norm_cases_emulated_cpu.py through tests/native_emul.py.

REFERENCES.  `ln_reference` / `gn_reference` are the operators written out in fp64 -- mean, centred second moment, 1 / sqrt(var + eps),
and the backward formulas of the kernels' header comments -- together with the NATURAL MAGNITUDE of every result: the same expression
with every term replaced by its absolute value (x - mean counts |x| + |mean|).  They model the kernels' documented rounding points and
nothing else: with bf16 I/O the saved sum s = a + keep b / (1 - p) is rounded to bf16 before the statistics; every output is the fp64
value rounded once; db = da keep / (1 - p) from the unrounded da.  `anchor_ln` / `anchor_gn` show once, on random inputs, that they
are F.layer_norm / F.group_norm (+ relu) with autograd in float64 to 1e-12.  The framework's float64 operators are NOT the expected
value of an exact case: on the zero-mean rows below F.layer_norm returns ~1e-17 where the value is exactly 0.

EXACT CASES (equality, no tolerance; premises raise `PremiseError` from the operands and the reference alone).
LayerNorm: eps = 0, p = 0, a row holds C/2 entries +v and C/2 entries -v (v = 2^k, k cycling over -2 .. 2 by row), a = x / 4,
b = 3 x / 4, integer gamma / beta / dy: mean 0, variance v^2, rstd 1 / v, and every intermediate of both directions is a dyadic
rational that fp32 holds in any order.  y == sign(x) gamma + beta, da == db, dgamma / dbeta / da == the fp64 value rounded once,
through the immediate column sum and through the deferred chunk sums alike.  Premises: every y is an integer; with bf16 I/O at least
10 % of the da values are no bf16 numbers (at every row count: a case takes the first draw that holds it).
GroupNorm: eps = 0, every pixel's 8 channels of a group hold four +v and four -v: every per-pixel mean is 0, the Chan combination
keeps mean = 0 and m2 = 8 HW v^2, and the forward is exact for any HW.  The backward multiplies by 1 / (8 HW), a power of two only
for HW = 2^k: backward equality is asserted there only (the other pixel counts get their backward from the bounded cases).  Premise:
at least 5 % of the pre-activations are exactly 0; the output there is +0 and, under ReLU, the gradient is 0 (`> 0`, not `>= 0`).

BOUNDED CASES.  The yardstick is the project's rule (criterion_cases.py): the framework's own fp32 operator, on the device under
test, against the same fp64 reference.  Per ELEMENT
    B = max(8 x the framework's worst error in that element's row (LayerNorm) or (image, group) (GroupNorm), 64 x 2^-24 x scale),
scale = the element's natural magnitude; for a parameter gradient the unit is the column.  Nothing global enters, so an error
confined to the smallest rows of a batch, or leaking from a neighbouring row, is measured against that row alone.  eps and the
dropout probability are the fp32 numbers the C ABI carries (`abi_float`: p = 0.999 means 1 / (1 - p) = 1000.013).  An fp32 output
must lie within B of the fp64 value.  A bf16 output has no tolerance of its own: it must lie between the bf16 number at or below
v - B and the one at or above v + B -- for B below the distance to the neighbours that is "one of the two bf16 neighbours of v";
where v sits nearer to 0 than B (y = xhat gamma + beta cancelling) no fp32 computation can promise more than that interval -- and
it must EQUAL the round-to-nearest-even of v wherever v - B and v + B round to the same bf16 number.  The elements where they do
not form the guard band.
THE CAP on the guard band is a premise on the inputs, taken from the reference alone (the band of 64 x 2^-24 x scale; the
framework's error belongs to a device): at most 1 % of a bf16 output may lie in it -- y, da, db, dx without ReLU, and dgamma / dbeta
where the parameters are bf16 -- and a case draws its inputs again until that holds for all of them (`first_draw_within_the_cap`,
`GuardCapError`).  The inputs are chosen for it:
  * the upstream gradient is not Gaussian (`structured_dy`): |dy| in [0.5, 1.5], its sign a column's sign x sign(xhat + 1).  A gradient
    that crosses 0 while its natural magnitude does not spends ~ 6.5e-3 x scale / sigma of its elements in the band (1.4 - 1.7 % for
    da / dx under a Gaussian dy, 5 - 20 % for column sums that cancel to sqrt(rows) of their terms); with this dy, da ~ rstd dy gamma
    stays clear of 0 (measured 0.2 - 0.8 %, dx 0.5 - 0.95 %) and a column's sums keep most of their terms' sign (dgamma 0 - 0.8 %);
  * a dropped element of db is an exact 0 and a dbeta column of bf16 dy is an exact sum in fp32 (`exact_column_sums`): B = 0 there,
    the result must be the fp64 value rounded once, ties included, and the element is not in any band;
  * a common offset of 1000 sigma puts a whole row into the band (64 x 2^-24 x 2000 exceeds half a bf16 step), as does a constant
    group under GroupNorm's x (gamma rstd) + (beta - mean gamma rstd) form, so the bf16 batches carry one such row among 512 / one
    such group among 768 (held by the interval only) and the fp32 batches carry them throughout; a batch with bf16 parameters
    carries no offset row (its 2000 |dy| enters every column's natural magnitude: dgamma would lie in the band whole).
One tensor does not reach 1 %: dx under ReLU.  A switched-off element's dx = -rstd (a + xhat b) and a live one's rstd (dy gamma - a -
xhat b) both cross 0 inside the data's range of xhat whatever the sign pattern of dy; with the best inputs tried (every dy gamma
positive, so that a does not cancel) the reference alone has 2.0 - 2.4 % of dx in the band (3.1 - 3.7 % at HW = 1, 192 elements;
5 - 29 % under a Gaussian or sign-symmetric dy).  That share is printed and not capped; the other 97.6 % are held to the nearest bf16
number.
ReLU: with dy = 1 the kernel's dbeta must equal the count of y > 0 per channel exactly (the backward recomputes the forward's
pre-activation: the two must agree to the bit); the kernel's mask must equal the fp64 sign wherever |pre| > B; dx / dgamma / dbeta
are compared against the fp64 backward GIVEN the kernel's mask, so the discontinuity needs no excluded band and no allowance.

Every check prints its figures before it asserts ("norm_case ..." lines: worst error / bound per tensor, premise shares); the
measured ones are in profiles/norm_cases_measured.txt.  No bound was widened.  The closest fp32 figure, on the emulation (0.179) and
the device (0.177) alike, is GroupNorm's dx under ReLU at C = 2048, HW = 65 in fp32: element (0, 58, 26, 2), switched off, dx = -rstd
(a + xhat b) = -0.319 at natural magnitude 0.406, 11.4 x 2^-24 of that off.  With every dy gamma positive the group sums a and b are
as large as their natural magnitude, and their fp32 error -- 520 terms added per thread, across the row lanes and chunks, then
multiplied by 1 / (8 x 65), no power of two -- reaches every element of the group undiminished; the framework's operator
(0.006 of the floor there) accumulates wider.  The forward's closest is GroupNorm's y in the same shape (0.09: the statistics' fp32
error plus the roundings of gamma rstd and beta - mean gamma rstd); LayerNorm's is y at 0.07.  A bf16 line's "widest interval" is
counted in bf16 steps of v's own binade: it is 1 - 2 wherever |v| exceeds B and large only where v cancels to far below B."""
import contextlib
import functools
import math
import zlib

import torch
import torch.nn.functional as F

from chunk_sums_tall_cases import chunk_sums_on
from exact_cases import PremiseError, _need, assert_bits_equal, bf16_rounding_shares
from test_add_ln_emulated_cpu import keep_mask

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
FLOOR = 64.0 * 2.0 ** -24
MARGIN = 8.0
GUARD_CAP = 0.01
SEED = 0x1234567887654321 & 0x7FFFFFFFFFFFFFFF


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


@contextlib.contextmanager
def kernels_on(backend=None):
    """Route both extensions to `backend` (the emulated library) for the duration; None: the device library."""
    from monodetr_amd import add_ln_ext, group_norm_ext
    saved = (add_ln_ext._backend, group_norm_ext._backend)
    if backend is not None:
        add_ln_ext._backend = group_norm_ext._backend = backend
    try:
        yield
    finally:
        add_ln_ext._backend, group_norm_ext._backend = saved


# ---- bf16 numbers in fp64 -------------------------------------------------------------------------------------------------------------
def _quantum(v):
    """the spacing of bf16 numbers in v's binade (normal range; 0 -> any spacing: floor / ceil / round give 0)."""
    return torch.ldexp(torch.ones_like(v), torch.frexp(v.abs())[1] - 8)


def bf16_floor(v):
    q = _quantum(v)
    return torch.floor(v / q) * q


def bf16_ceil(v):
    q = _quantum(v)
    return torch.ceil(v / q) * q


def bf16_rne(v):
    q = _quantum(v)
    return torch.round(v / q) * q                                              # (torch.round: halves to even)


def guard_band(v, B):
    """elements whose fp64 value is within B of a bf16 rounding boundary: v - B and v + B round to different bf16 numbers."""
    return bf16_rne(v - B) != bf16_rne(v + B)


# ---- figures --------------------------------------------------------------------------------------------------------------------------
def elementwise_bound(err32, scale, unit_dims):
    """B: max(8 x the framework's worst error within the element's unit (the dims reduced by amax), 64 x 2^-24 x scale)."""
    worst32 = err32.amax(unit_dims, keepdim=True) if unit_dims else err32
    return torch.maximum(MARGIN * worst32, FLOOR * scale)


def _ratio(err, B):
    r = torch.where(B > 0, err / B, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
    r = torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)
    return float(r.max()) if r.numel() else 0.0


def check_output(tag, name, got, ref, fw32, scale, unit_dims, zero_where=None):
    """One output tensor against its fp64 reference under the rule of the module docstring.  Returns the printed figures."""
    got64, err32 = got.detach().cpu().double(), (fw32.detach().cpu().double() - ref).abs()
    assert got64.shape == ref.shape, (name, got64.shape, ref.shape)
    B = elementwise_bound(err32, scale, unit_dims)
    if zero_where is not None:                                                 # elements whose fp32 value is exact by construction
        B = torch.where(zero_where, torch.zeros_like(B), B)
    err = (got64 - ref).abs()
    fig = {"torch32": _ratio(err32, FLOOR * scale)}                            # (inf where the scale is 0 and the framework is not exact)
    if got.dtype == BF16:
        lo, hi = bf16_floor(ref - B), bf16_ceil(ref + B)
        band = guard_band(ref, B)
        fig["guard"] = float(band.double().mean())
        outside = (got64 < lo) | (got64 > hi) | torch.isnan(got64)
        wrong = ~band & (got64 != bf16_rne(ref))
        half = 0.5 * _quantum(ref)
        fig["kernel"] = _ratio(err, B + half)
        fig["width"] = float(((hi - lo) / _quantum(ref)).max()) if ref.numel() else 0.0       # 1: the two neighbours of v (0: v is a bf16 number)
        print("norm_case %s %s bf16: err/(B + half step) %.3f  outside [floor(v-B), ceil(v+B)] %d  misrounded outside the guard band %d  "
              "guard share %.4f  widest interval %.0f steps  (fp32 framework err/floor %.3f)" % (
                  tag, name, fig["kernel"], int(outside.sum()), int(wrong.sum()), fig["guard"], fig["width"], fig["torch32"]))
        assert not bool(outside.any()), "%s %s: %d elements outside the interval, first %s" % (tag, name, int(outside.sum()), _first(outside, got64, ref))
        assert not bool(wrong.any()), "%s %s: %d elements are not the nearest bf16, first %s" % (tag, name, int(wrong.sum()), _first(wrong, got64, ref))
    else:
        fig["kernel"] = _ratio(err, B)
        print("norm_case %s %s fp32: err/B %.3f  (fp32 framework err/floor %.3f)" % (tag, name, fig["kernel"], fig["torch32"]))
        bad = ~(err <= B)
        assert not bool(bad.any()), "%s %s: %d elements beyond the bound, worst ratio %.3g, first %s" % (tag, name, int(bad.sum()), fig["kernel"], _first(bad, got64, ref))
    return fig


def _first(mask, got, ref):
    idx = tuple(int(i) for i in torch.nonzero(mask)[0])
    return "at %s: got %r, fp64 %r" % (idx, float(got[idx]), float(ref[idx]))


# ======================================================================================================================================
#  LayerNorm(a + dropout(b))
# ======================================================================================================================================
def ln_reference(s, gamma, beta, dy, keep, p, eps, const_rows=None, s_mag=None):
    """fp64.  s [R, C] is the (already rounded, where the kernel rounds it) sum a + keep b / (1 - p); s_mag its natural magnitude
    |a| + |keep b / (1 - p)| where the kernel forms it in fp32 without a rounding point of its own (fp32 I/O), |s| otherwise."""
    C = s.shape[-1]
    mean = s.sum(-1, keepdim=True) / C
    d = s - mean
    var = (d * d).sum(-1, keepdim=True) / C
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = d * rstd
    g = dy * gamma
    s1, s2 = g.sum(-1, keepdim=True) / C, (g * xh).sum(-1, keepdim=True) / C
    da = rstd * (g - s1 - xh * s2)
    sc = keep / (1.0 - p)
    out = dict(y=xh * gamma + beta, da=da, db=da * sc, dgamma=(dy * xh).sum(0), dbeta=dy.sum(0), mean=mean, rstd=rstd, var=var)
    xn, gn = ((s.abs() if s_mag is None else s_mag) + mean.abs()) * rstd, g.abs()
    if const_rows is not None:                                                 # C equal numbers: their sum, its division by C = 2^k and
        xn = torch.where(const_rows[:, None], torch.zeros_like(xn), xn)        # x - mean = 0 are exact in fp32; no magnitude is at stake
    dan = rstd * (gn + gn.sum(-1, keepdim=True) / C + xn * (gn * xn).sum(-1, keepdim=True) / C)
    out["scale"] = dict(y=xn * gamma.abs() + beta.abs(), da=dan, db=dan * sc, dgamma=(dy.abs() * xn).sum(0), dbeta=dy.abs().sum(0))
    return out


def anchor_ln():
    """`ln_reference` is F.layer_norm with autograd in float64 (1e-12 of each tensor's largest entry), dropout mask as data."""
    g = gen("anchor_ln")
    R, C, p, eps = 37, 256, 0.3, 1e-5
    a, b, dy = (torch.randn(R, C, generator=g, dtype=F64) for _ in range(3))
    gamma, beta = 1 + 0.3 * torch.randn(C, generator=g, dtype=F64), torch.randn(C, generator=g, dtype=F64)
    keep = keep_mask(SEED, R * C, p).view(R, C).double()
    a, b, gamma, beta = (t.requires_grad_(True) for t in (a, b, gamma, beta))
    y = F.layer_norm(a + b * keep / (1 - p), (C,), gamma, beta, eps)
    y.backward(dy)
    ref = ln_reference((a + b * keep / (1 - p)).detach(), gamma.detach(), beta.detach(), dy, keep, p, eps)
    for name, t in (("y", y.detach()), ("da", a.grad), ("db", b.grad), ("dgamma", gamma.grad), ("dbeta", beta.grad)):
        assert float((t - ref[name]).abs().max()) <= 1e-12 * float(ref[name].abs().max()), name


class LnCase:
    pass


def exact_column_sums(dy, dims):
    """Columns of dbeta = sum dy (or sum dy mask: a subset of the terms) that fp32 adds exactly in ANY order: every |dy| is a multiple
    of q = 2^-9 (bf16 numbers >= 0.5 are) and sum |dy| < 2^24 q, so every partial sum is a multiple of q below 2^24 q.  Such a sum
    is the fp64 value itself: B = 0, an fp32 result equals it and a bf16 result is its one rounding, ties included."""
    d = dy.double().abs()
    q = 2.0 ** -9
    on_grid = ((d / q) == (d / q).round()).all(dims[0]) if len(dims) == 1 else ((d / q) == (d / q).round()).flatten(0, 1).all(0)
    total = d.sum(dims)
    return on_grid & (total < 2.0 ** 24 * q)


def structured_dy(centred, unit_dims, col_sign, g):
    """The upstream gradient of the bounded cases: |dy| uniform in [0.5, 1.5], sign = col_sign (per column / channel) x sign(xhat + 1).
    Chosen from the inputs alone so that the gradients stay clear of 0 relative to their natural magnitude (the guard-band cap):
    |dy gamma| >= 0.5 |gamma| while s1, s2 (sums over the columns, whose signs alternate) stay small, so da ~ rstd dy gamma does not
    cross 0; a column's sums of dy and of dy xhat (dbeta, dgamma) keep one sign for 84 % / all but the -1 < xhat < 0 terms
    instead of cancelling to sqrt(rows) of their natural magnitude, as they do for a symmetric dy."""
    sd = (centred * centred).mean(unit_dims, keepdim=True).sqrt()
    mag = 0.5 + torch.rand(centred.shape, generator=g, dtype=F64)
    return mag * col_sign * torch.where(centred + sd >= 0, 1.0, -1.0)


class GuardCapError(PremiseError):
    """More than GUARD_CAP of a bf16 forward output lies in the guard band: another draw is taken."""


def abi_float(v):
    """The C ABI carries eps and dropout_p as float: the operator's parameter is that fp32 number (p = 0.999 -> 1 / (1 - p) = 1000.013)."""
    return float(torch.tensor(v, dtype=F32))


def cap_premise(what, v, scale, zero_where=None):
    """From the reference alone: at most GUARD_CAP of a bf16 forward output within 64 x 2^-24 x scale of a bf16 rounding boundary."""
    B = FLOOR * scale
    if zero_where is not None:
        B = torch.where(zero_where, torch.zeros_like(B), B)
    share = float(guard_band(v, B).double().mean())
    if share > GUARD_CAP:
        raise GuardCapError("%s: %.4f of the elements lie in the guard band" % (what, share))
    return share


def first_draw_within_the_cap(build, *key):
    """`build(*key, attempt)` for attempt = 0, 1, ..: the first draw whose forward output keeps the guard-band cap (the inputs are
    chosen from the reference alone, before any kernel runs)."""
    for attempt in range(48):
        try:
            return build(*key, attempt)
        except GuardCapError as e:
            last = e
    raise last


def _to_io(t64, io):
    return t64.to(F32).to(io)


def ln_run(c, device, backend=None, seed_form="host", odd_view=False, finish="immediate"):
    """The kernel through the product's autograd function -> dict of CPU tensors y, da, db, dgamma, dbeta (+ s, the saved sum)."""
    from monodetr_amd import add_ln_ext

    def leaf(t, odd):
        if not odd:
            return t.clone().to(device).requires_grad_(True), None
        base = torch.zeros(t.numel() + 1, dtype=t.dtype)
        base[1:] = t.reshape(-1)
        base = base.to(device).requires_grad_(True)
        return base[1:].view(t.shape), base

    (a, a_base), (b, b_base) = leaf(c.a, odd_view), leaf(c.b, odd_view)
    gamma, beta = c.gamma.detach().clone().to(device).requires_grad_(True), c.beta.detach().clone().to(device).requires_grad_(True)
    dy = c.dy.to(device)
    if odd_view:
        if a.data_ptr() % 16 == 0 or b.data_ptr() % 16 == 0:
            raise PremiseError("the view is 16-byte aligned: the copy path of _rows is not taken")
        pad = torch.zeros(dy.numel() + 1, dtype=dy.dtype, device=device)
        pad[1:] = dy.reshape(-1)
        dy = pad[1:].view(dy.shape)
    with kernels_on(backend):
        if seed_form == "dev":                                                 # the same total, split between the host word and a device word
            part = 0x0123456789ABCDEF
            seed_dev = torch.tensor([part], dtype=torch.int64, device=device)
            y = add_ln_ext._AddLayerNorm.apply(a, b, gamma, beta, c.eps, c.p, (c.seed - part) % 2 ** 63, seed_dev)
        else:
            y = add_ln_ext._AddLayerNorm.apply(a, b, gamma, beta, c.eps, c.p, c.seed, None)
        s = y.grad_fn.saved_tensors[0].detach().cpu().view(c.a.shape)
        if finish == "deferred":
            with chunk_sums_on(backend, poison=True) as cs:
                with cs.deferred():
                    y.backward(dy)
                    assert len(cs._pending) == 2, "the gamma / beta sums did not take the deferred route"
        else:
            y.backward(dy)
    ga, gb = (a_base.grad[1:].view(c.a.shape), b_base.grad[1:].view(c.a.shape)) if odd_view else (a.grad, b.grad)
    out = dict(y=y.detach(), da=ga, db=gb, dgamma=gamma.grad, dbeta=beta.grad)
    out = {k: v.cpu() for k, v in out.items()}
    out["s"] = s
    return out


def ln_torch32(c, device):
    """The framework's fp32 LayerNorm and its autograd on the device, fed the reference's s: y, da, db, dgamma, dbeta (unrounded fp32)."""
    s = c.s.to(F32).to(device).requires_grad_(True)
    gamma, beta = c.gamma.float().clone().to(device).requires_grad_(True), c.beta.float().clone().to(device).requires_grad_(True)
    y = F.layer_norm(s, (s.shape[-1],), gamma, beta, c.eps)
    y.backward(c.dy.float().to(device))
    sc = (c.keep / (1.0 - abi_float(c.p))).float().to(device)
    return {k: v.detach().cpu() for k, v in dict(y=y, da=s.grad, db=s.grad * sc, dgamma=gamma.grad, dbeta=beta.grad).items()}


# ---- exact -----------------------------------------------------------------------------------------------------------------------------
LN_WIDTHS = (128, 256, 512)
LN_EXACT_ROWS = (1, 3, 4, 5, 4101)          # a partial workgroup, the early-returning waves; > 4 kMaxBwdBlocks: two rows per wave, ragged end


@functools.lru_cache(maxsize=8)
def ln_exact_case(R, C, io, pdt):
    """The first draw that holds the premises (a single row's share of da values that need rounding varies with the draw)."""
    for attempt in range(64):
        try:
            return _ln_exact_case(R, C, io, pdt, attempt)
        except RoundingShareError as e:
            last = e
    raise last


class RoundingShareError(PremiseError):
    pass


def _ln_exact_case(R, C, io, pdt, attempt):
    g = gen("ln_exact", R, C, attempt)
    k = torch.arange(R) % 5 - 2
    v = torch.ldexp(torch.ones(R, dtype=F64), k)[:, None]
    sign = torch.where(torch.rand(R, C, generator=g).argsort(-1) < C // 2, 1.0, -1.0).double()
    x = sign * v
    c = LnCase()
    c.R, c.C, c.io, c.pdt, c.eps, c.p, c.seed = R, C, io, pdt, 0.0, 0.0, 0
    c.a, c.b = (x / 4).to(io), (3 * x / 4).to(io)
    c.gamma = torch.randint(-4, 5, (C,), generator=g).to(pdt)
    c.beta = torch.randint(-8, 9, (C,), generator=g).to(pdt)
    c.dy = torch.randint(-3, 4, (R, C), generator=g).to(io)
    c.keep = torch.ones(R, C, dtype=F64)
    if not (torch.equal(c.a.double() * 4, x) and torch.equal(c.b.double() * 4, 3 * x) and bool((x.sum(-1) == 0).all())):
        raise PremiseError("ln_exact: a, b do not hold x / 4, 3 x / 4 exactly, or a row's mean is not 0")
    c.s = x
    c.ref = ln_reference(x, c.gamma.double(), c.beta.double(), c.dy.double(), c.keep, 0.0, 0.0)
    ref = c.ref
    # the analytic values, not the framework's: mean 0, rstd 1 / v
    if not (bool((ref["mean"] == 0).all()) and torch.equal(ref["rstd"], 1 / v) and torch.equal(ref["y"], sign * c.gamma.double() + c.beta.double())):
        raise PremiseError("ln_exact: the fp64 reference is not the analytic value")
    if not bool((ref["y"] == ref["y"].round()).all()):
        raise PremiseError("ln_exact: y is not an integer everywhere")
    for name in ("da", "dgamma", "dbeta"):                                     # every value a dyadic rational that fp32 holds
        if not torch.equal(ref[name].float().double(), ref[name]):
            raise PremiseError("ln_exact: %s is not exact in fp32" % name)
    c.inexact = bf16_rounding_shares(ref["da"])[0]
    if c.inexact * ref["da"].numel() < _need(0.10, ref["da"].numel()):         # (asked of the fp32 cases' draw too: one draw per shape)
        raise RoundingShareError("ln_exact: only %.3f of the da values need rounding" % c.inexact)
    c.want = dict(y=_to_io(ref["y"], io), da=_to_io(ref["da"], io), db=_to_io(ref["db"], io),
                  dgamma=_to_io(ref["dgamma"], pdt), dbeta=_to_io(ref["dbeta"], pdt), s=_to_io(x, io))
    return c


def check_ln_exact(R, C, io, pdt, device, backend=None):
    c = ln_exact_case(R, C, io, pdt)
    tag = "ln_exact/R%d/C%d/%s/%s" % (R, C, str(io)[6:], str(pdt)[6:])
    print("norm_case %s premises: da values that are no bf16 numbers %.3f, y integer, mean 0, rstd 1 / v" % (tag, c.inexact))
    first = None
    for finish in ("immediate", "deferred"):
        got = ln_run(c, device, backend, finish=finish)
        wrong = {k: int((got[k] != c.want[k]).sum()) for k in c.want}
        print("norm_case %s %s elements that differ: %s" % (tag, finish, wrong))
        for k in ("s", "y", "da", "db", "dgamma", "dbeta"):
            assert_bits_equal(got[k], c.want[k], "%s %s (%s)" % (tag, k, finish))
        assert_bits_equal(got["da"], got["db"], tag + " da == db")
        if first is not None:
            for k in ("dgamma", "dbeta"):
                assert_bits_equal(got[k], first[k], "%s %s: deferred against immediate" % (tag, k))
        first = got


# ---- bounded ---------------------------------------------------------------------------------------------------------------------------
LN_KINDS = ("normal", "offset", "constant", "tiny", "big")
#                  name          kind     p      rows(fp32 io)  rows(bf16 io)
LN_BOUNDED = {
    "p0":          ("normal",    0.0,   37,  37),
    "p01":         ("normal",    0.1,   64,  64),
    "p05":         ("normal",    0.5,   5,   5),
    "p0999":       ("normal",    0.999, 64,  64),
    "offset":      ("offset",    0.0,   23,  512),      # bf16: one offset row among 512 (the guard-band cap, module docstring)
    "constant":    ("constant",  0.0,   9,   9),
    "tiny":        ("tiny",      0.1,   33,  33),       # |x| ~ 1e-4: eps = 1e-5 decides rstd
    "big":         ("big",       0.1,   33,  33),       # |x| ~ 1e4
    "mixed":       ("mixed",     0.1,   64,  512),
}


def _row_kinds(kind, R, io, pdt):
    """bf16 parameter gradients are column sums over the rows: one 1000 sigma row puts every column's sum into the guard band (its
    natural magnitude is 2000 |dy| against a sum of ~ sqrt(R)), so the batches with bf16 parameters carry no offset row."""
    if kind == "mixed":
        cyc = LN_KINDS if io == F32 and pdt == F32 else ("normal", "constant", "tiny", "big")
        kinds = [cyc[r % len(cyc)] for r in range(R)]
    elif kind == "offset" and io == BF16:
        kinds = ["normal"] * R
    else:
        return [kind] * R
    if io == BF16 and pdt == F32:
        kinds[R - 3] = "offset"
    return kinds


@functools.lru_cache(maxsize=8)
def ln_bounded_case(name, C, io, pdt):
    return first_draw_within_the_cap(_ln_bounded_case, name, C, io, pdt)


def _ln_bounded_case(name, C, io, pdt, attempt):
    kind, p, r32, r16 = LN_BOUNDED[name]
    R = r32 if io == F32 else r16
    g = gen("ln_bounded", name, C, str(io), str(pdt), attempt)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)                    # noqa: E731
    kinds = _row_kinds(kind, R, io, pdt)
    a, b = rn(R, C), 0.7 * rn(R, C) + 0.2
    for r, kd in enumerate(kinds):
        sigma = float(torch.rand((), generator=g)) + 0.5
        if kd == "offset":                                                     # 1000 sigma: E[x^2] - E[x]^2 would lose every bit of the variance
            a[r], b[r] = sigma * (1000.0 * (1 if r % 2 else -1) + a[r]), sigma * 0.1 * b[r]
        elif kd == "constant":
            a[r], b[r] = (3.0 + r) * (1 if r % 2 else -1), 0.0
        elif kd == "tiny":
            a[r], b[r] = 1e-4 * a[r], 1e-4 * b[r]
        elif kd == "big":
            a[r], b[r] = 1e4 * a[r], 1e4 * b[r]
    c = LnCase()
    c.name, c.R, c.C, c.io, c.pdt, c.eps, c.p, c.seed, c.kinds = name, R, C, io, pdt, 1e-5, p, SEED, kinds
    eps, p = abi_float(c.eps), abi_float(p)                                    # what the kernel is given
    c.a, c.b = a.to(io), b.to(io)
    c.gamma, c.beta = (1 + 0.3 * rn(C)).to(pdt), (0.5 * rn(C)).to(pdt)
    c.keep = keep_mask(SEED, R * C, p).view(R, C).double() if p > 0 else torch.ones(R, C, dtype=F64)
    if p > 0:
        share = float(c.keep.mean())
        if abs(share - (1 - p)) >= 4 * (p * (1 - p) / (R * C)) ** 0.5 + 1e-3:
            raise PremiseError("%s: keep share %.4f for p = %g" % (name, share, p))
    sc = 1.0 / (1.0 - p)
    if io == BF16:
        # the saved sum is rounded to bf16 by an fp32 computation: keep every fp64 sum further from a bf16 rounding boundary than
        # that computation's error (8 x 2^-24 of its terms), unless fp32 holds product and sum exactly (p = 0, p = 0.5: ties round alike)
        for _ in range(32):
            a64, b64 = c.a.double(), c.b.double()
            s64 = a64 + c.keep * b64 * sc
            thr = 8 * 2.0 ** -24 * (a64.abs() + (c.keep * b64 * sc).abs())
            prod32 = c.b.float() * torch.tensor(sc, dtype=F32) * c.keep.float()
            exact32 = (prod32.double() == c.keep * b64 * sc) & ((c.a.float() + prod32).double() == s64)
            bad = guard_band(s64, thr) & ~exact32
            if not bool(bad.any()):
                break
            # move b by one bf16 step where it enters (b / (1 - p) is exact now and then, 207 / 0.9 = 230: a step of a keeps a tie), a elsewhere
            in_b = bad & (c.keep > 0) & (c.b != 0)
            c.b = torch.where(in_b, (c.b.view(torch.int16) + 1).view(BF16), c.b)
            c.a = torch.where(bad & ~in_b & (c.a != 0), (c.a.view(torch.int16) + 1).view(BF16), c.a)
        else:
            raise PremiseError("%s: sums stay on a bf16 rounding boundary" % name)
        c.s = bf16_rne(s64)
        if not torch.equal(c.s.to(F32).to(BF16).double(), c.s):
            raise PremiseError("%s: the rounded sum is no bf16 number" % name)
        s_mag = None
    else:
        c.s = c.a.double() + c.keep * c.b.double() * sc
        s_mag = c.a.double().abs() + (c.keep * c.b.double() * sc).abs()
    const = torch.tensor([kd == "constant" for kd in kinds])
    c.const = const
    c.dy = structured_dy(c.s - c.s.mean(-1, keepdim=True), (-1,), torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0).double(), g).to(io)
    c.ref = ln_reference(c.s, c.gamma.double(), c.beta.double(), c.dy.double(), c.keep, p, eps, const_rows=const, s_mag=s_mag)
    ref = c.ref
    c.cap = {}
    if io == BF16:
        c.cap["y"] = cap_premise("ln %s y" % name, ref["y"], ref["scale"]["y"])
        c.cap["da"] = cap_premise("ln %s da" % name, ref["da"], ref["scale"]["da"])
        c.cap["db"] = cap_premise("ln %s db" % name, ref["db"], ref["scale"]["db"], c.keep == 0)      # (a dropped element is an exact 0)
    if pdt == BF16:
        c.cap["dgamma"] = cap_premise("ln %s dgamma" % name, ref["dgamma"], ref["scale"]["dgamma"])
        c.cap["dbeta"] = cap_premise("ln %s dbeta" % name, ref["dbeta"], ref["scale"]["dbeta"], exact_column_sums(c.dy, (0,)))
    if bool(const.any()) and not (bool((ref["var"][const] == 0).all()) and bool((ref["y"][const] == c.beta.double()).all())):
        raise PremiseError("%s: a constant row has variance" % name)
    tiny = torch.tensor([kd == "tiny" for kd in kinds])
    if bool(tiny.any()) and not bool((ref["var"][tiny] < 0.1 * eps).all()):
        raise PremiseError("%s: eps does not decide rstd of the tiny rows" % name)
    off = torch.tensor([kd == "offset" for kd in kinds])
    if bool(off.any()) and io == F32 and not bool((ref["mean"][off].abs() > 500 * ref["var"][off].sqrt()).all()):
        raise PremiseError("%s: the offset rows' mean is not 500 sigma" % name)
    return c


def check_ln_bounded(name, C, io, pdt, device, backend=None, seed_form="host", odd_view=False):
    c = ln_bounded_case(name, C, io, pdt)
    ref, sc = c.ref, c.ref["scale"]
    tag = "ln/%s/C%d/%s/%s%s%s" % (name, C, str(io)[6:], str(pdt)[6:], "/seed_dev" if seed_form == "dev" else "", "/odd_view" if odd_view else "")
    fw = ln_torch32(c, device)
    print("norm_case %s premises: rows %d keep share %.4f (p %g) kinds %s; within the floor of a bf16 boundary %s" % (
        tag, c.R, float(c.keep.mean()), c.p, sorted(set(c.kinds)), " ".join("%s %.4f" % kv for kv in c.cap.items()) or "-"))
    got = ln_run(c, device, backend, seed_form=seed_form, odd_view=odd_view)
    for k in ("y", "da", "db", "dgamma", "dbeta"):
        assert bool(torch.isfinite(got[k]).all()), "%s %s is not finite" % (tag, k)
    if io == BF16:
        assert_bits_equal(got["s"], c.s.to(F32).to(BF16), tag + " saved sum")
    figs = {}
    for k in ("y", "da", "db"):
        figs[k] = check_output(tag, k, got[k], ref[k], fw[k], sc[k], (-1,), zero_where=(c.keep == 0) if k == "db" else None)
    figs["dgamma"] = check_output(tag, "dgamma", got["dgamma"], ref["dgamma"], fw["dgamma"], sc["dgamma"], ())
    figs["dbeta"] = check_output(tag, "dbeta", got["dbeta"], ref["dbeta"], fw["dbeta"], sc["dbeta"], (), zero_where=exact_column_sums(c.dy, (0,)))
    dropped = c.keep == 0
    assert bool((got["db"][dropped] == 0).all()), tag + ": a dropped element's db is not exactly 0"
    if bool(c.const.any()):                                                    # variance 0: y is beta, rounded once
        want = c.beta.double().expand(c.R, c.C).to(F32).to(io)
        assert_bits_equal(got["y"][c.const], want[c.const], tag + " constant rows: y == beta")
    return got, figs


def check_ln_seed_forms(C, io, device, backend=None):
    """The mask is the same with the seed as a host integer and as a device word holding part of the same total."""
    host, _ = check_ln_bounded("p05", C, io, F32, device, backend, seed_form="host")
    dev, _ = check_ln_bounded("p05", C, io, F32, device, backend, seed_form="dev")
    for k in host:
        assert_bits_equal(dev[k], host[k], "seed forms: " + k)


# ======================================================================================================================================
#  GroupNorm (+ ReLU), 8 channels per group, channels-last
# ======================================================================================================================================
def gn_reference(x, gamma, beta, dy, eps, relu, mask=None, const_groups=None):
    """fp64.  x, dy [N, HW, G, 8]; gamma, beta [G, 8]; mask (the ReLU's, 0 / 1) defaults to pre > 0."""
    m = 8 * x.shape[1]
    mean = x.sum((1, 3), keepdim=True) / m
    d = x - mean
    var = (d * d).sum((1, 3), keepdim=True) / m
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = d * rstd
    pre = xh * gamma + beta
    if mask is None:
        mask = (pre > 0).double() if relu else torch.ones_like(pre)
    dd = dy * mask
    g = dd * gamma
    a, b = g.sum((1, 3), keepdim=True) / m, (g * xh).sum((1, 3), keepdim=True) / m
    out = dict(pre=pre, y=torch.where(pre > 0, pre, torch.zeros_like(pre)) if relu else pre, dx=rstd * (g - a - xh * b),
               dgamma=(dd * xh).sum((0, 1)), dbeta=dd.sum((0, 1)), mean=mean, var=var, rstd=rstd)
    xn, gn = (x.abs() + mean.abs()) * rstd, g.abs()
    # a constant group: the per-pixel means, their Chan combination (d = 0) and x - mean = 0 are exact in fp32, so the backward's
    # xhat carries no magnitude; the forward's x (gamma rstd) + (beta - mean gamma rstd) form does cancel, and keeps it
    xb = xn if const_groups is None else torch.where(const_groups, torch.zeros_like(xn), xn)
    out["scale"] = dict(y=xn * gamma.abs() + beta.abs(),
                        dx=rstd * (gn + gn.sum((1, 3), keepdim=True) / m + xb * (gn * xb).sum((1, 3), keepdim=True) / m),
                        dgamma=(dd.abs() * xb).sum((0, 1)), dbeta=dd.abs().sum((0, 1)))
    return out


def _nchw(t):
    """[N, HW, G, 8] -> [N, C, HW, 1] in channels-last memory (a view)."""
    N, HW, G, _ = t.shape
    return t.reshape(N, HW, 1, G * 8).permute(0, 3, 1, 2)


def _nhwc(t, G):
    N, C, H, W = t.shape
    return t.permute(0, 2, 3, 1).reshape(N, H * W, G, 8)


def anchor_gn():
    """`gn_reference` is F.group_norm (+ relu) with autograd in float64 (1e-12 of each tensor's largest entry)."""
    g = gen("anchor_gn")
    N, HW, G, eps = 2, 77, 4, 1e-5
    x, dy = torch.randn(N, HW, G, 8, generator=g, dtype=F64) + 0.5, torch.randn(N, HW, G, 8, generator=g, dtype=F64)
    gamma, beta = 1 + 0.3 * torch.randn(G, 8, generator=g, dtype=F64), torch.randn(G, 8, generator=g, dtype=F64)
    for relu in (False, True):
        xr, wr, br = _nchw(x).clone().requires_grad_(True), gamma.reshape(-1).clone().requires_grad_(True), beta.reshape(-1).clone().requires_grad_(True)
        y = F.group_norm(xr, G, wr, br, eps)
        y = F.relu(y) if relu else y
        y.backward(_nchw(dy))
        ref = gn_reference(x, gamma, beta, dy, eps, relu)
        for name, t in (("y", _nhwc(y.detach(), G)), ("dx", _nhwc(xr.grad, G)), ("dgamma", wr.grad.view(G, 8)), ("dbeta", br.grad.view(G, 8))):
            assert float((t - ref[name]).abs().max()) <= 1e-12 * float(ref[name].abs().max()), (name, relu)


class GnCase:
    pass


def gn_run(c, relu, device, dy, backend=None, backward=True):
    """The kernel through the product's autograd function -> y, dx [N, HW, G, 8], dgamma, dbeta [G, 8] on the CPU."""
    from monodetr_amd import group_norm_ext
    G = c.C // 8
    x = _nchw(c.x).to(device).contiguous(memory_format=torch.channels_last).clone(memory_format=torch.preserve_format).requires_grad_(True)
    w, b = c.gamma.reshape(-1).clone().to(device).requires_grad_(True), c.beta.reshape(-1).clone().to(device).requires_grad_(True)
    with kernels_on(backend):
        y = group_norm_ext.group_norm(x, w, b, G, c.eps, relu)
        out = dict(y=_nhwc(y.detach(), G).cpu())
        if backward:
            y.backward(_nchw(dy).to(device).contiguous(memory_format=torch.channels_last))
            out.update(dx=_nhwc(x.grad, G).cpu(), dgamma=w.grad.view(G, 8).cpu(), dbeta=b.grad.view(G, 8).cpu())
    return out


def gn_torch32(c, relu, device, dy, mask):
    """The framework's fp32 GroupNorm and its autograd on the device; the ReLU's backward is the upstream gradient times `mask`."""
    G = c.C // 8
    x = _nchw(c.x.float()).to(device).contiguous().clone().requires_grad_(True)
    w, b = c.gamma.float().reshape(-1).clone().to(device).requires_grad_(True), c.beta.float().reshape(-1).clone().to(device).requires_grad_(True)
    pre = F.group_norm(x, G, w, b, c.eps)
    pre.backward(_nchw((dy.double() * mask).float()).to(device).contiguous())
    pre = _nhwc(pre.detach(), G).cpu()
    return dict(pre=pre, y=torch.where(pre > 0, pre, torch.zeros_like(pre)) if relu else pre, dx=_nhwc(x.grad, G).cpu(),
                dgamma=w.grad.view(G, 8).cpu(), dbeta=b.grad.view(G, 8).cpu())


# ---- exact -----------------------------------------------------------------------------------------------------------------------------
GN_CHANNELS = (8, 64, 256, 2048)            # one group lane with 256 row lanes .. 256 group lanes with one row lane
GN_HW = (1, 63, 64, 65, 257, 2048, 2049)    # below / at / above the 64-row chunk, chunks shorter than the row lanes, 32 chunks, a last chunk of one row
GN_HW_POW2 = (1, 64, 128, 2048, 4096)       # 1 / (8 HW) is a power of two: the backward is exact too


def gn_exact_shapes(hws, max_elems):
    """(C, HW, N) over every C, HW and N in {1, 3} whose tensor stays within `max_elems` (N = 1 always runs for the small C)."""
    return [(C, HW, N) for C in GN_CHANNELS for HW in hws for N in (1, 3) if N * HW * C <= max_elems]


_BALANCED = torch.tensor([[1.0 if (m >> i) & 1 else -1.0 for i in range(8)] for m in range(256) if bin(m).count("1") == 4], dtype=F64)


@functools.lru_cache(maxsize=4)
def gn_exact_case(C, HW, N, io, pdt):
    g = gen("gn_exact", C, HW, N)
    G = C // 8
    sign = _BALANCED[torch.randint(0, 70, (N, HW, G), generator=g)]            # four +1 and four -1 per pixel and group
    v = torch.ldexp(torch.ones(N, 1, G, 1, dtype=F64), torch.randint(-2, 3, (N, 1, G, 1), generator=g))
    c = GnCase()
    c.C, c.HW, c.N, c.io, c.pdt, c.eps = C, HW, N, io, pdt, 0.0
    c.x = (sign * v).to(io)
    gamma, beta = torch.randint(-4, 5, (G, 8), generator=g).double(), torch.randint(-4, 5, (G, 8), generator=g).double()
    gamma[0, 1], beta[0, 1], gamma[0, 6], beta[0, 6] = 2.0, -2.0, -3.0, -3.0   # pre == 0 where the sign is +1 / -1, whatever the draw
    c.gamma, c.beta = gamma.to(pdt), beta.to(pdt)
    c.dy = torch.randint(-3, 4, (N, HW, G, 8), generator=g).to(io)
    if not torch.equal(c.x.double(), sign * v):
        raise PremiseError("gn_exact: x is not exact in its dtype")
    c.pre = sign * gamma + beta                                                # the analytic value: mean 0, rstd 1 / v
    c.zeros = float((c.pre == 0).double().mean())
    if c.zeros * c.pre.numel() < _need(0.05, c.pre.numel()):
        raise PremiseError("gn_exact: %.4f of the pre-activations are 0" % c.zeros)
    c.sign, c.v = sign, v
    return c


def check_gn_exact(C, HW, N, io, pdt, device, backend=None):
    """Forward equality for any HW, with and without ReLU; backward equality where 1 / (8 HW) is a power of two."""
    c = gn_exact_case(C, HW, N, io, pdt)
    backward = HW & (HW - 1) == 0
    tag = "gn_exact/C%d/HW%d/N%d/%s/%s" % (C, HW, N, str(io)[6:], str(pdt)[6:])
    print("norm_case %s premises: pre-activations exactly 0: %.4f; backward asserted: %s" % (tag, c.zeros, backward))
    for relu in (False, True):
        ref = gn_reference(c.x.double(), c.gamma.double(), c.beta.double(), c.dy.double(), 0.0, relu)
        if not (torch.equal(ref["pre"], c.pre) and bool((ref["mean"] == 0).all()) and torch.equal(ref["rstd"], 1 / c.v)):
            raise PremiseError("gn_exact: the fp64 reference is not the analytic value")
        got = gn_run(c, relu, device, c.dy, backend, backward=backward)
        want_y = _to_io(ref["y"], io)
        assert torch.equal(want_y.double(), ref["y"])
        print("norm_case %s relu %d y elements that differ: %d" % (tag, relu, int((got["y"] != want_y).sum())))
        assert_bits_equal(got["y"], want_y, "%s y (relu %d)" % (tag, relu))
        zero = c.pre == 0
        assert not bool(torch.signbit(got["y"].float())[zero].any()), "%s: -0 where the pre-activation is 0" % tag
        if backward:
            for k, dt in (("dx", io), ("dgamma", pdt), ("dbeta", pdt)):
                if not torch.equal(ref[k].float().double(), ref[k]):
                    raise PremiseError("gn_exact: %s is not exact in fp32" % k)
                want = _to_io(ref[k], dt)
                print("norm_case %s relu %d %s elements that differ: %d" % (tag, relu, k, int((got[k] != want).sum())))
                assert_bits_equal(got[k], want, "%s %s (relu %d)" % (tag, k, relu))


# ---- bounded ---------------------------------------------------------------------------------------------------------------------------
#            name        C     HW    N   offset groups
GN_BOUNDED = {
    "one_lane":   (8,    257,  3),
    "ragged":     (64,   65,   3),
    "depth_head": (256,  2049, 1),
    "short":      (256,  63,   3),
    "wide":       (2048, 65,   1),
    "pixel":      (64,   1,    3),
    "groups768":  (2048, 21,   3),                       # one special (image, group) among 768: the bf16 offset / constant variants
}
GN_DTYPES = ((F32, F32), (BF16, F32), (BF16, BF16))       # (io, parameters): fp32 io with bf16 parameters is not a combination the kernel takes


@functools.lru_cache(maxsize=4)
def gn_bounded_case(name, io, pdt, variant):
    return first_draw_within_the_cap(_gn_bounded_case, name, io, pdt, variant)


def _gn_bounded_case(name, io, pdt, variant, attempt):
    """variant: "plain", "offset" (fp32 io: every group 300 sigma off; bf16 io: one (image, group), see the module docstring),
    "constant" (one group constant)."""
    C, HW, N = GN_BOUNDED[name]
    G = C // 8
    g = gen("gn_bounded", name, variant, attempt)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)                    # noqa: E731
    x = 1.7 * rn(N, HW, G, 8) + 0.3
    c = GnCase()
    c.special = torch.zeros(N, 1, G, 1, dtype=torch.bool)
    if variant == "offset":
        if io == F32:
            c.special[:] = True
        else:
            c.special[N - 1, 0, G // 2, 0] = True
        x = torch.where(c.special, x + 300.0 * 1.7 * torch.where(torch.rand(N, 1, G, 1, generator=g) < 0.5, -1.0, 1.0), x)
    elif variant == "constant":
        c.special[0, 0, G - 1, 0] = True
        x = torch.where(c.special, torch.full_like(x, -2.5), x)
    c.name, c.C, c.HW, c.N, c.io, c.pdt, c.eps, c.variant = name, C, HW, N, io, pdt, 1e-5, variant
    c.x = x.to(io)
    c.gamma, c.beta = (1 + 0.5 * rn(G, 8)).to(pdt), (0.5 * rn(G, 8)).to(pdt)
    # the upstream gradient (structured_dy): without ReLU the channels' signs alternate within a group (a, b stay small: dx ~ rstd dy
    # gamma stays clear of 0); under ReLU every dy gamma is positive, so that a = mean(dy gamma mask) is large and the switched-off
    # elements' dx = -rstd (a + xhat b) is not a small difference of large terms
    centred = c.x.double() - c.x.double().mean((1, 3), keepdim=True)
    alt = torch.tensor([1.0, -1.0] * 4, dtype=F64) * torch.where(torch.rand(G, 1, generator=g) < 0.5, -1.0, 1.0)
    c.dy = {False: structured_dy(centred, (1, 3), alt, g).to(io),
            True: (0.5 + torch.rand(N, HW, G, 8, generator=g, dtype=F64)).mul(torch.where(c.gamma.double() < 0, -1.0, 1.0)).to(io)}
    c.ref = {relu: gn_reference(c.x.double(), c.gamma.double(), c.beta.double(), c.dy[relu].double(), abi_float(c.eps), relu) for relu in (False, True)}
    c.cap = {False: {}, True: {}}
    for relu, r in c.ref.items():
        if io == BF16:
            c.cap[relu]["y"] = cap_premise("gn %s y" % name, r["y"], r["scale"]["y"], r["pre"] < 0 if relu else None)
            if relu:                                                           # (not capped: the module docstring states its floor)
                c.cap[relu]["dx (no cap)"] = float(guard_band(r["dx"], FLOOR * r["scale"]["dx"]).double().mean())
            else:
                c.cap[relu]["dx"] = cap_premise("gn %s dx" % name, r["dx"], r["scale"]["dx"])
        if pdt == BF16:
            c.cap[relu]["dgamma"] = cap_premise("gn %s dgamma" % name, r["dgamma"], r["scale"]["dgamma"])
            c.cap[relu]["dbeta"] = cap_premise("gn %s dbeta" % name, r["dbeta"], r["scale"]["dbeta"], exact_column_sums(c.dy[relu], (0, 1)))
    if variant == "constant" and not bool((c.ref[False]["var"][c.special] == 0).all()):
        raise PremiseError("gn constant: the group has variance")
    if variant == "offset" and io == F32 and not bool((c.ref[False]["mean"].abs() > 150 * c.ref[False]["var"].sqrt()).all()):
        raise PremiseError("gn offset: the mean is not 150 sigma")
    return c


def check_gn_bounded(name, io, pdt, variant, relu, device, backend=None):
    c = gn_bounded_case(name, io, pdt, variant)
    tag = "gn/%s/%s/%s/%s/relu%d" % (name, variant, str(io)[6:], str(pdt)[6:], relu)
    ref0 = c.ref[relu]
    unit = (1, 3)                                                              # an (image, group)
    got = gn_run(c, relu, device, c.dy[relu], backend)
    for k, t in got.items():
        assert bool(torch.isfinite(t).all()), "%s %s is not finite" % (tag, k)
    const = c.special if variant == "constant" else None
    if relu:
        mask = (got["y"] > 0).double()
        # the backward's mask is the forward's: with dy = 1, dbeta is the count of y > 0 per channel, exactly
        ones = gn_run(c, relu, device, torch.ones_like(c.dy[relu]), backend)
        count = mask.sum((0, 1))
        assert float(count.max()) < 2 ** 24
        assert_bits_equal(ones["dbeta"], _to_io(count, c.pdt), tag + " dbeta at dy = 1 against the count of y > 0")
    else:
        mask = torch.ones_like(ref0["pre"])
    fw = gn_torch32(c, relu, device, c.dy[relu], mask)
    ref = gn_reference(c.x.double(), c.gamma.double(), c.beta.double(), c.dy[relu].double(), abi_float(c.eps), relu, mask=mask, const_groups=const)
    print("norm_case %s premises: within the floor of a bf16 boundary %s" % (tag, " ".join("%s %.4f" % kv for kv in c.cap[relu].items()) or "-"))
    sc = ref["scale"]
    figs = {}
    if relu:                                                                   # the mask is the fp64 sign wherever |pre| exceeds the fp32 bound
        Bpre = elementwise_bound((fw["pre"].double() - ref["pre"]).abs(), sc["y"], unit)
        decided = ref["pre"].abs() > Bpre
        flips = decided & (mask != (ref["pre"] > 0).double())
        print("norm_case %s mask: undecided (|pre| <= B) %.5f, differing from the fp64 sign where decided: %d, elsewhere: %d" % (
            tag, 1 - float(decided.double().mean()), int(flips.sum()), int((~decided & (mask != (ref["pre"] > 0).double())).sum())))
        assert not bool(flips.any()), "%s: %d mask elements contradict the fp64 sign, first %s" % (tag, int(flips.sum()), _first(flips, mask, ref["pre"]))
        # y under the kernel's mask: an undecided element may be 0 or its pre-activation; both lie within B of the reference's
        y_ref = torch.where(decided, ref["y"], torch.where(mask > 0, ref["pre"], torch.zeros_like(ref["pre"])))
        y_fw = torch.where(decided, fw["y"].double(), torch.where(mask > 0, fw["pre"].double(), torch.zeros_like(ref["pre"])))
        off = decided & (ref["pre"] < 0)                                       # switched off beyond doubt: an exact 0
    else:
        y_ref, y_fw, off = ref["y"], fw["y"], None
    figs["y"] = check_output(tag, "y", got["y"], y_ref, y_fw, sc["y"], unit, zero_where=off)
    figs["dx"] = check_output(tag, "dx", got["dx"], ref["dx"], fw["dx"], sc["dx"], unit)
    figs["dgamma"] = check_output(tag, "dgamma", got["dgamma"], ref["dgamma"], fw["dgamma"], sc["dgamma"], ())
    figs["dbeta"] = check_output(tag, "dbeta", got["dbeta"], ref["dbeta"], fw["dbeta"], sc["dbeta"], (), zero_where=exact_column_sums(c.dy[relu], (0, 1)))
    return figs
