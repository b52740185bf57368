"""Exact-arithmetic cases for the product and convolution kernels (test infrastructure; tests/test_exact_products_gpu.py runs them on
the GPU, tests/test_exact_products_emulated_cpu.py through tests/native_emul.py).

Every kernel here is linear with fp32 accumulation.  On small-integer operands every partial sum is an integer below 2^24 -- exact
in fp32 in ANY summation order and any split of the contraction -- so the right answer is known to the bit: the fp64 value, rounded
ONCE to the output dtype.  The assertion is equality, not a tolerance.  Three things random floats never reach are put there on
purpose, and each generator checks from the operands and the fp64 reference alone (before any kernel runs) that they are there:

  * "wide" operands: bf16 results of which >= 10 % are not bf16 numbers (the store must round) and >= 1 % are exact ties (an odd
    integer in 256 .. 512: 257 -> 256, 259 -> 260; truncation or round-half-up gives another bit);
  * "narrow" operands (|v| <= 2, integer bias): >= 0.5 % of the pre-activations / mask elements are exactly 0, where `<= 0` and `< 0`
    part ways (the project's convention is threshold_backward's: mask <= 0 -> 0);
  * fp32 operands for the three-way bf16 split of csrc/tgemm.hip: a full-mantissa matrix against a +-2^e one-hot matrix (the result is
    a scaled copy of one operand column, bit for bit, which needs every x.hi / x.mid / x.lo term against the other side's hi), and
    11-bit integers against 10-bit ones (mid x mid and the cross terms).

A share is a condition on the reference, not a measurement: a result of n elements must hold at least ceil(share n) such elements
(nothing is asked of a result so small that share n < 1 -- the one-token shape is there for its geometry), and `PremiseError` is
raised otherwise."""
import functools
import math

import torch

from gemm_bounds import conv2d_f64

CAP = float(2 ** 24)
BF16, F32 = torch.bfloat16, torch.float32


class PremiseError(AssertionError):
    """The operands do not have the property the case was built for (a fault of the test, not of a kernel)."""


# ---- operands -------------------------------------------------------------------------------------------------------------------------
def wide_amp(K):
    """Integer amplitude A for a contraction of K: sums of K products of two uniform [-A, A] integers have sigma ~ (A^2 / 3) sqrt(K);
    A^2 sqrt(K) ~ 1800 puts sigma near 600: two thirds of the results beyond 256, a fifth of them ties."""
    return max(2, min(32, int(round(math.sqrt(1800.0 / math.sqrt(K))))))


def narrow_amp(K):
    """[-2, 2] (sigma of a K-sum ~ 2 sqrt(K): P(sum == 0) ~ 0.2 / sqrt(K)); [-1, 1] beyond K = 256 keeps that share above 1 %."""
    return 2 if K <= 256 else 1


def ints(g, shape, amp, dtype=BF16):
    return torch.randint(-amp, amp + 1, tuple(shape), generator=g).to(dtype)


def gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def cl(t):
    return t.contiguous(memory_format=torch.channels_last)


# ---- premises and the expected value --------------------------------------------------------------------------------------------------
def _need(share, n):
    return int(math.ceil(share * n)) if share * n >= 1.0 else 0


def bf16_rounding_shares(ref64):
    """(share that is no bf16 number, share of exact ties) of an fp64 tensor."""
    r = ref64.to(F32)
    down = (r.view(torch.int32) & -65536).view(F32).double()          # truncation: the bf16 neighbour towards zero
    inexact = down != ref64
    up = ((r.view(torch.int32) & -65536) + 65536).view(F32).double()
    tie = inexact & ((ref64 - down).abs() == (up - ref64).abs())
    return inexact.double().mean().item(), tie.double().mean().item()


def expected(ref64, mag64, dtype, wide=False, zeros_of=None, what=""):
    """The fp64 value rounded once to `dtype`, after the premises: integers, sum |a||w| + |bias| + |res| < 2^24 per element, and the
    shares of the set the case belongs to (wide: of a bf16 result; zeros_of: a pre-activation / mask tensor with >= 0.5 % zeros)."""
    if not bool((ref64 == ref64.round()).all()) or not float(mag64.max()) < CAP:
        raise PremiseError("%s: not integers below 2^24 (max magnitude %g)" % (what, float(mag64.max())))
    if not bool((ref64.abs() <= mag64).all()):
        raise PremiseError("%s: magnitude does not bound the value" % what)
    if wide and dtype == BF16:
        inexact, tie = bf16_rounding_shares(ref64)
        n = ref64.numel()
        if inexact * n < _need(0.10, n) or tie * n < _need(0.01, n):
            raise PremiseError("%s: %.3f of the results need rounding, %.4f are ties (wanted 0.10 / 0.01 of %d)" % (what, inexact, tie, n))
    if zeros_of is not None:
        z = int((zeros_of == 0).sum())
        if z < _need(0.005, zeros_of.numel()):
            raise PremiseError("%s: %d exact zeros among %d (wanted 0.005)" % (what, z, zeros_of.numel()))
    out = ref64.to(F32)
    assert bool((out.double() == ref64).all())                         # (double -> float is exact under the cap)
    return out.to(dtype)


def _ordered(t):
    """Bit patterns as integers that order like the values (for distances in ulps)."""
    if t.dtype == BF16:
        i = t.contiguous().view(torch.int16).to(torch.int64)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    if t.dtype == torch.float64:
        i = t.contiguous().view(torch.int64)
        return torch.where(i < 0, -(i & 0x7FFFFFFFFFFFFFFF), i)
    i = t.contiguous().view(torch.int32).to(torch.int64)
    return torch.where(i < 0, -(i & 0x7FFFFFFF), i)


def assert_bits_equal(got, want, what=""):
    """got == want element by element (+0 == -0; a NaN only where the other has one)."""
    assert got.shape == want.shape and got.dtype == want.dtype, "%s: %s %s against %s %s" % (what, tuple(got.shape), got.dtype, tuple(want.shape), want.dtype)
    got, want = got.detach().cpu().contiguous(), want.detach().cpu().contiguous()
    bad = (got != want) & ~(got.isnan() & want.isnan())
    if bool(bad.any()):
        idx = tuple(int(i) for i in torch.nonzero(bad)[0])
        ulps = (_ordered(got) - _ordered(want)).abs()[bad].max().item()
        raise AssertionError("%s: %d of %d elements differ; first at %s: got %r, want %r; largest difference %d ulp of %s" % (
            what, int(bad.sum()), bad.numel(), idx, float(got[idx]), float(want[idx]), ulps, str(got.dtype).replace("torch.", "")))


# ---- csrc/tgemm.hip, bf16 form --------------------------------------------------------------------------------------------------------
TGEMM_SHAPES = [(1, 8, 8), (67, 72, 72), (130, 136, 264), (300, 1032, 72)]     # below a tile; tile + ragged rest; two N tiles; 17 slabs, the last ragged
TGEMM_VARIANTS = [("plain", "wide"), ("bias_bf16", "wide"), ("bias_f32", "wide"), ("res", "wide"), ("accum", "wide"), ("relu", "wide"),
                  ("relu", "narrow"), ("out_f32", "wide"), ("dropout", "narrow")]


@functools.lru_cache(maxsize=None)
def tgemm_operands(T, K, N, nn, kind, dtype=BF16):
    """a [T, K], w [N, K] ([K, N] with nn), bias [N], res [T, N]: integers, |a|, |w| <= the set's amplitude, |bias|, |res| <= 64 (wide)
    or the amplitude (narrow).  Shared by every test that asks for the same key: never written to."""
    g = gen(T, K, N, int(nn), len(kind))
    amp = wide_amp(K) if kind == "wide" else narrow_amp(K)
    a = ints(g, (T, K), amp, dtype)
    w = ints(g, (K, N) if nn else (N, K), amp, dtype)
    side = 64 if kind == "wide" else amp
    return a, w, ints(g, (N,), side, dtype), ints(g, (T, N), side, dtype)


def product_f64(a, w, nn, bias=None, res=None):
    wd = w.double() if nn else w.double().t()
    ref, mag = a.double() @ wd, a.double().abs() @ wd.abs()
    for extra in (bias, res):
        if extra is not None:
            ref, mag = ref + extra.double(), mag + extra.double().abs()
    return ref, mag


def dropout_want(pre32, dev, seed, dtype):
    """bias_act's relu + dropout(p = 0.5) on the exact fp32 pre-activation: the keep scale 2 is exact, so is the result."""
    from monodetr_amd import bias_act_ext
    want = bias_act_ext.bias_act(pre32.to(dev), None, None, relu=True, dropout_p=0.5, seed=seed).cpu()
    twice = 2.0 * pre32.clamp(min=0)
    assert bool(((want == 0) | (want == twice)).all())
    kept = float((want != 0).sum()) / max(1.0, float((twice != 0).sum()))
    if pre32.numel() >= 512 and not 0.35 < kept < 0.65:
        raise PremiseError("dropout keeps %.2f of the positive elements at p = 0.5" % kept)
    return want.to(dtype)


def check_tgemm(dev, T, K, N, nn, variant, kind, dtype=BF16):
    """One epilogue variant of mdetr_tgemm (dtype bf16) / mdetr_tgemm_f32 (dtype fp32, integer operands) against the exact value."""
    from monodetr_amd import tgemm_ext
    what = "tgemm %s T=%d K=%d N=%d nn=%s %s/%s" % (str(dtype)[6:], T, K, N, nn, variant, kind)
    a, w, b, r = tgemm_operands(T, K, N, nn, kind, dtype)
    bias = {"bias_bf16": b, "bias_f32": b.float(), "relu": b, "dropout": b}.get(variant)
    res = r if variant in ("res", "accum") else None
    out_dtype = F32 if variant == "out_f32" or dtype == F32 else BF16
    ref, mag = product_f64(a, w, nn, bias, res)
    relu = variant in ("relu", "dropout")
    want = expected(ref.clamp(min=0) if relu else ref, mag, out_dtype, wide=kind == "wide", zeros_of=ref if kind == "narrow" else None, what=what)
    ad, wd = a.to(dev), w.to(dev)
    bd = bias.to(dev) if bias is not None else None
    rd = res.to(dev).clone() if res is not None else None
    assert tgemm_ext.supported(ad, wd, nn=nn, res=rd, bias=bd, out=rd if variant == "accum" else None), what
    if variant == "dropout":
        want = dropout_want(expected(ref, mag, F32), dev, 4321, out_dtype)
        y = tgemm_ext.tgemm(ad, wd, bd, None, relu=True, nn=nn, dropout_p=0.5, seed=4321)
    else:
        y = tgemm_ext.tgemm(ad, wd, bd, rd, relu=relu, nn=nn, out=rd if variant == "accum" else None,
                            out_dtype=F32 if variant == "out_f32" else None)
        assert variant != "accum" or y.data_ptr() == rd.data_ptr()
    assert_bits_equal(y, want, what)


def check_tgemm_masked(dev, T, K, N, with_res, dtype=BF16):
    """mdetr_tgemm[_f32]_masked on the narrow set: y = mask <= 0 ? 0 : dy w + res, a fifth of the mask exactly 0."""
    from monodetr_amd import tgemm_ext
    what = "tgemm_masked %s T=%d K=%d N=%d res=%s" % (str(dtype)[6:], T, K, N, with_res)
    dy, w, _, r = tgemm_operands(T, K, N, True, "narrow", dtype)
    mask = ints(gen(T, K, N, 5), (T, N), 2, dtype)
    res = r if with_res else None
    ref, mag = product_f64(dy, w, True, None, res)
    if not bool(((mask == 0) & (ref != 0)).any()) or not bool(((mask < 0) & (ref != 0)).any()):
        raise PremiseError(what + ": no nonzero result under a zero / a negative mask element")
    want = expected(torch.where(mask.double() <= 0, torch.zeros_like(ref), ref), mag, dtype, zeros_of=mask, what=what)
    args = [t.to(dev) if t is not None else None for t in (dy, w, mask, res)]
    assert tgemm_ext.masked_supported(*args), what
    assert_bits_equal(tgemm_ext.tgemm_masked(*args), want, what)


# ---- csrc/tgemm.hip, fp32 form: the three-way split --------------------------------------------------------------------------------------
def full_mantissa(g, shape):
    """randn x 2^[-20, 20]: 24 significant bits, 40 binades."""
    return (torch.randn(shape, generator=g) * torch.exp2(torch.randint(-20, 21, shape, generator=g).float())).float()


def one_hot_rows(g, rows, cols):
    """[rows, cols] with one nonzero +-2^e (e in -8 .. 8) per row -> (matrix, its column per row, its value per row)."""
    k = torch.randint(0, cols, (rows,), generator=g)
    s = torch.exp2(torch.randint(-8, 9, (rows,), generator=g).float()) * (torch.randint(0, 2, (rows,), generator=g).float() * 2 - 1)
    m = torch.zeros(rows, cols)
    m[torch.arange(rows), k] = s
    return m, k, s


@functools.lru_cache(maxsize=None)
def split_case(T, K, N, nn, kind):
    """-> (a [T, K], w in the layout `nn` asks for, the expected fp32 product).
    "a": full-mantissa a, one-hot [N, K] weight: y[t, n] = a[t, k(n)] s(n).   "w": one-hot a, full-mantissa weight: y[t, n] = s(t) w[n, k(t)].
    "int": |a| < 2^11, |w| < 2^10 with at most 4 nonzeros per row of the [N, K] form: sum |a||w| < 2^23."""
    g = gen(T, K, N, int(nn), ord(kind[0]))
    if kind == "a":
        a = full_mantissa(g, (T, K))
        w_nk, k, s = one_hot_rows(g, N, K)
        want = a[:, k] * s
    elif kind == "w":
        a, k, s = one_hot_rows(g, T, K)
        w_nk = full_mantissa(g, (N, K))
        want = w_nk[:, k].t() * s[:, None]
    else:
        a = torch.randint(-2047, 2048, (T, K), generator=g).float()
        w_nk = torch.zeros(N, K)
        for _ in range(min(4, K)):
            w_nk[torch.arange(N), torch.randint(0, K, (N,), generator=g)] = torch.randint(-1023, 1024, (N,), generator=g).float()
        ref, mag = product_f64(a, w_nk, False)
        want = expected(ref, mag, F32, what="split integers")
        if not bool((a.abs() >= 256).any()) or not bool((w_nk.abs() >= 256).any()):
            raise PremiseError("split integers: no operand beyond 8 bits")
    ref = a.double() @ w_nk.double().t()                                # premises: the product is exact in fp32 and is what `want` holds
    if not bool((want.double() == ref).all()) or not bool(torch.isfinite(want).all()):
        raise PremiseError("split case %s: the expected product is not exact in fp32" % kind)
    if kind in ("a", "w"):
        full = a if kind == "a" else w_nk
        low = (full.view(torch.int32) & 0xFF) != 0                      # (bits that only the .lo part of the split carries)
        if float(low.float().mean()) < 0.9:
            raise PremiseError("split case %s: operand without low mantissa bits" % kind)
    return a, (w_nk.t().contiguous() if nn else w_nk), want


def check_tgemm_split(dev, T, K, N, nn, kind):
    from monodetr_amd import tgemm_ext
    a, w, want = split_case(T, K, N, nn, kind)
    ad, wd = a.to(dev), w.to(dev)
    assert tgemm_ext.supported(ad, wd, nn=nn)
    assert_bits_equal(tgemm_ext.tgemm(ad, wd, nn=nn), want, "tgemm f32 split case (%s) T=%d K=%d N=%d nn=%s" % (kind, T, K, N, nn))


# ---- weight gradients over token rows (csrc/twgrad.hip, csrc/conv_wgrad.hip's 1x1 case, csrc/small_wgrad.hip) -------------------------------
@functools.lru_cache(maxsize=None)
def wgrad_operands(T, K, N, dtype=BF16):
    g = gen(T, K, N, 3)
    amp = wide_amp(T)
    x, dy = ints(g, (T, K), amp, dtype), ints(g, (T, N), amp, dtype)
    rw, mw = dy.double().t() @ x.double(), dy.double().abs().t() @ x.double().abs()
    return x, dy, rw, mw, dy.double().sum(0), dy.double().abs().sum(0)


def check_token_wgrad(dev, T, K, N):
    """mdetr_token_wgrad through conv_wgrad_ext.token_weight_gradient (whichever form MDETR_TUNE's twgrad selects), with the bias gradient."""
    from monodetr_amd import conv_wgrad_ext
    x, dy, rw, mw, rb, mb = wgrad_operands(T, K, N)
    xd, dyd = x.to(dev), dy.to(dev)
    if not conv_wgrad_ext.token_supported(xd, dyd):
        return False
    for dtype in (F32, BF16):
        what = "token_wgrad T=%d K=%d N=%d -> %s" % (T, K, N, dtype)
        dw, db = conv_wgrad_ext.token_weight_gradient(xd, dyd, dtype, bias=True)
        assert_bits_equal(dw, expected(rw, mw, dtype, wide=True, what=what), what + " dW")
        assert_bits_equal(db, expected(rb, mb, dtype, what=what), what + " db")
        dw, none = conv_wgrad_ext.token_weight_gradient(xd, dyd, dtype, bias=False)
        assert none is None
        assert_bits_equal(dw, expected(rw, mw, dtype), what + " dW alone")
    return True


def check_small_wgrad(dev, T, N, K, dtype):
    from monodetr_amd import small_wgrad_ext
    x, dy, rw, mw, rb, mb = wgrad_operands(T, K, N, dtype)
    what = "small_wgrad T=%d N=%d K=%d %s" % (T, N, K, dtype)
    dw, db = small_wgrad_ext.small_wgrad(dy.to(dev), x.to(dev), dtype)
    assert_bits_equal(dw, expected(rw, mw, dtype, wide=True, what=what), what + " dW")
    assert_bits_equal(db, expected(rb, mb, dtype, what=what), what + " db")


# ---- csrc/sgemm.hip -------------------------------------------------------------------------------------------------------------------
def check_sgemm_nt(dev):
    """An NT group: a ragged wide product with bias and a partial ReLU into a column slice, the 3-wide and the 6-wide heads, and a
    bf16 result with res and mask (narrow: zeros in the pre-activation and in the mask)."""
    from monodetr_amd import sgemm_ext as S
    g = gen(11)
    T = 150
    x = ints(g, (T, 256), 8)                                                 # bf16 operand
    wide = ints(g, (T, 300), 8, F32)
    w1, b1 = ints(g, (70, 256), 8, F32), ints(g, (70,), 64, F32)
    w3, b3 = ints(g, (3, 40), 8, F32), ints(g, (3,), 8, F32)
    w6, b6 = ints(g, (6, 37), 8, F32), ints(g, (6,), 8, F32)
    xn, wn = ints(g, (T, 37), 2, F32), ints(g, (33, 37), 2, F32)
    res, mask = ints(g, (T, 33), 2), ints(g, (T, 33), 2, F32)
    o1 = torch.full((T, 80), 7.0)
    o3, o6, on = torch.empty(T, 3), torch.empty(T, 6), torch.empty(T, 33, dtype=BF16)
    o1w = torch.empty(T, 70, dtype=BF16)
    dv = lambda t: t.to(dev)                                                  # noqa: E731
    d = {k: dv(v) for k, v in dict(x=x, wide=wide, w1=w1, b1=b1, w3=w3, b3=b3, w6=w6, b6=b6, xn=xn, wn=wn, res=res, mask=mask,
                                   o1=o1, o3=o3, o6=o6, on=on, o1w=o1w).items()}
    S.grouped(S.NT, [S.Problem([(d["x"], d["w1"])], d["o1"][:, 5:75], bias=d["b1"], relu_cols=64),
                     S.Problem([(d["wide"][:, 100:140], d["w3"])], d["o3"], bias=d["b3"]),
                     S.Problem([(d["wide"][:, 3:40], d["w6"])], d["o6"], bias=d["b6"]),
                     S.Problem([(d["xn"], d["wn"])], d["on"], res=d["res"], mask=d["mask"], relu_cols=True),
                     S.Problem([(d["x"], d["w1"])], d["o1w"], bias=d["b1"])])
    r1, m1 = product_f64(x, w1, False, b1)
    relu1 = r1.clone()
    relu1[:, :64] = relu1[:, :64].clamp(min=0)
    assert_bits_equal(d["o1"][:, 5:75], expected(relu1, m1, F32, what="sgemm NT wide"), "sgemm NT bias + partial relu")
    assert bool((d["o1"][:, :5] == 7.0).all()) and bool((d["o1"][:, 75:] == 7.0).all())
    assert_bits_equal(d["o1w"], expected(r1, m1, BF16, wide=True, what="sgemm NT bf16"), "sgemm NT bf16 result")
    assert_bits_equal(d["o3"], expected(*product_f64(wide[:, 100:140], w3, False, b3), F32), "sgemm NT 3-wide")
    assert_bits_equal(d["o6"], expected(*product_f64(wide[:, 3:40], w6, False, b6), F32), "sgemm NT 6-wide")
    rn, mn = product_f64(xn, wn, False, None, res)
    want = torch.where(mask.double() <= 0, torch.zeros_like(rn), rn.clamp(min=0))
    if not bool(((mask == 0) & (rn > 0)).any()):
        raise PremiseError("sgemm NT: no positive result under a zero mask element")
    expected(rn, mn, BF16, zeros_of=rn, what="sgemm NT narrow pre-activation")
    assert_bits_equal(d["on"], expected(want, mn, BF16, zeros_of=mask, what="sgemm NT narrow"), "sgemm NT res + relu + mask")


def check_sgemm_nn(dev):
    """NN: a contraction split over three tensors (256 + 96 + 3) with a bf16 res into a bf16 result, and a masked 3-deep product."""
    from monodetr_amd import sgemm_ext as S
    g = gen(12)
    T = 131
    dh, dcls = ints(g, (T, 352), 8, F32), ints(g, (T, 3), 2, F32)
    wa, wb, wc = ints(g, (256, 256), 8, F32), ints(g, (96, 256), 8, F32), ints(g, (3, 256), 2, F32)
    skip, saved = ints(g, (T, 256), 64), ints(g, (T, 256), 2, F32)
    out, plain = torch.empty(T, 256, dtype=BF16), torch.empty(T, 256)
    d = [t.to(dev) for t in (dh, dcls, wa, wb, wc, skip, saved, out, plain)]
    S.grouped(S.NN, [S.Problem([(d[0][:, :256], d[2]), (d[0][:, 256:], d[3]), (d[1], d[4])], d[7], res=d[5]),
                     S.Problem([(d[1], d[4])], d[8], mask=d[6])])
    parts = [product_f64(a, w, True) for a, w in ((dh[:, :256], wa), (dh[:, 256:], wb), (dcls, wc))]
    ref = sum(p[0] for p in parts) + skip.double()
    mag = sum(p[1] for p in parts) + skip.double().abs()
    assert_bits_equal(d[7], expected(ref, mag, BF16, wide=True, what="sgemm NN"), "sgemm NN three terms + res")
    rc, mc = parts[2]
    if not bool(((saved == 0) & (rc != 0)).any()):
        raise PremiseError("sgemm NN: no nonzero result under a zero mask element")
    assert_bits_equal(d[8], expected(torch.where(saved.double() <= 0, torch.zeros_like(rc), rc), mc, F32, zeros_of=saved, what="sgemm NN mask"),
                      "sgemm NN mask")


def check_sgemm_tn(dev, T):
    """TN: weight gradients (45 x 256 from a bf16 activation, the 6-wide and the 3-wide heads) with their column sums."""
    from monodetr_amd import sgemm_ext as S
    g = gen(13, T)
    amp = wide_amp(T)
    dy, x, h = ints(g, (T, 300), amp, F32), ints(g, (T, 256), amp), ints(g, (T, 70), amp, F32)
    outs = [torch.empty(45, 256), torch.empty(45), torch.empty(6, 70), torch.empty(6), torch.empty(3, 70), torch.empty(3)]
    d = [t.to(dev) for t in [dy, x, h] + outs]
    S.grouped(S.TN, [S.Problem([(d[0][:, 10:55], d[1])], d[3], colsum=d[4]),
                     S.Problem([(d[0][:, 100:106], d[2])], d[5], colsum=d[6]),
                     S.Problem([(d[0][:, 200:203], d[2])], d[7], colsum=d[8])])
    for (a, b), dw, db, name in (((dy[:, 10:55], x), d[3], d[4], "45 x 256"), ((dy[:, 100:106], h), d[5], d[6], "6-wide"),
                                 ((dy[:, 200:203], h), d[7], d[8], "3-wide")):
        assert_bits_equal(dw, expected(a.double().t() @ b.double(), a.double().abs().t() @ b.double().abs(), F32), "sgemm TN " + name)
        assert_bits_equal(db, expected(a.double().sum(0), a.double().abs().sum(0), F32), "sgemm TN column sums " + name)


# ---- convolutions ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def conv_case(B, H, W, C, N, k, stride, kind):
    """Integer x [B, C, H, W], w [N, C, k, k] (channels_last bf16), shift [N] fp32, dy like the output -- and, from fp64 autograd on
    the same operands: pre = conv + shift, the gradients of x and w for dy (no ReLU) and their magnitudes."""
    g = gen(B, H, W, C, N, k, stride, len(kind))
    K = k * k * C
    amp = wide_amp(K) if kind == "wide" else narrow_amp(K)
    pad = 3 if k == 7 else k // 2
    x = cl(ints(g, (B, C, H, W), amp))
    w = cl(ints(g, (N, C, k, k), amp))
    shift = ints(g, (N,), 64 if kind == "wide" else amp, F32)
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    pre = conv2d_f64(x64, w64, shift.double(), stride=stride, padding=pad)
    # (dy: an input pixel sees k k N / stride^2 products of dy and w; amplitude for a sigma of ~600 there as well)
    dy_amp = max(2, min(32, int(round(1800.0 / (amp * math.sqrt(k * k * N / float(stride * stride)))))))
    dy = cl(ints(g, pre.shape, dy_amp if kind == "wide" else 2))
    gx, gw = torch.autograd.grad(pre, (x64, w64), dy.double())
    xa, wa = x.double().abs().requires_grad_(True), w.double().abs().requires_grad_(True)
    mpre = conv2d_f64(xa, wa, shift.double().abs(), stride=stride, padding=pad)
    mx, mw = torch.autograd.grad(mpre, (xa, wa), dy.double().abs())
    return dict(x=x, w=w, shift=shift, dy=dy, pre=pre.detach(), mpre=mpre.detach(), gx=gx, mx=mx, gw=gw, mw=mw, pad=pad)


def check_conv3x3(dev, B, H, W, C, N, monkeypatch):
    """conv3x3_ext.conv3x3: forward (wide without ReLU and shift, wide with shift, narrow with shift + ReLU), the mirrored input gradient,
    the input gradient masked through an in_token, the weight gradient of csrc/conv_wgrad.hip."""
    from monodetr_amd import conv3x3_ext, conv_wgrad_ext
    from monodetr_amd.monodetr.linear import ReluToken
    monkeypatch.setattr(conv_wgrad_ext, "ENABLED", True)
    tag = "conv3x3 B=%d H=%d W=%d C=%d N=%d " % (B, H, W, C, N)
    c = conv_case(B, H, W, C, N, 3, 1, "wide")
    x, w, dy = c["x"].to(dev), c["w"].to(dev), c["dy"].to(dev)
    noshift = c["pre"] - c["shift"].double().view(1, -1, 1, 1)
    assert_bits_equal(conv3x3_ext.conv3x3(x, w, None, relu=False), expected(noshift, c["mpre"], BF16, wide=True, what=tag), tag + "plain")
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = conv3x3_ext.conv3x3(xr, wr, c["shift"].to(dev), relu=False)
    assert_bits_equal(y, expected(c["pre"], c["mpre"], BF16, wide=True, what=tag), tag + "shift")
    y.backward(dy)
    dx_by_kernel = N % 64 == 0 and C % 32 == 0                                 # (conv3x3_ext._Conv3x3.backward: otherwise the library's)
    if dx_by_kernel:
        assert_bits_equal(xr.grad, expected(c["gx"], c["mx"], BF16, wide=True, what=tag + "dx"), tag + "dx (mirrored taps)")
    assert conv_wgrad_ext.supported(x, dy, 3, 1)
    assert_bits_equal(wr.grad, expected(c["gw"], c["mw"], BF16, wide=B * H * W >= 64, what=tag + "dw"), tag + "dw")
    n = conv_case(B, H, W, C, N, 3, 1, "narrow")
    x, w, dy = n["x"].to(dev), n["w"].to(dev), n["dy"].to(dev)
    want = expected(n["pre"].clamp(min=0), n["mpre"], BF16, zeros_of=n["pre"], what=tag + "narrow")
    assert_bits_equal(conv3x3_ext.conv3x3(x, w, n["shift"].to(dev), relu=True), want, tag + "shift + relu")
    if dx_by_kernel:
        token = ReluToken()
        xr = x.clone().requires_grad_(True)
        conv3x3_ext.conv3x3(xr, w, None, relu=False, in_token=token).backward(dy)
        assert token.premasked
        xm = n["x"].double()
        if not bool(((xm == 0) & (n["gx"] != 0)).any()):
            raise PremiseError(tag + "no nonzero gradient under a zero input")
        want = expected(torch.where(xm <= 0, torch.zeros_like(xm), n["gx"]), n["mx"], BF16, zeros_of=xm, what=tag + "masked dx")
        assert_bits_equal(xr.grad, want, tag + "dx masked by the input")


def check_conv_strided(dev, B, H, W, C, N, k, monkeypatch, expect_split=False):
    """conv_taps_ext.conv_strided (3x3 / 1x1, stride 2): forward without ReLU (the split-K route where it applies), forward with shift +
    ReLU on the narrow set, input gradient (four parity classes) and weight gradient."""
    from monodetr_amd import conv_taps_ext, conv_wgrad_ext
    monkeypatch.setattr(conv_wgrad_ext, "ENABLED", True)
    tag = "conv_strided B=%d H=%d W=%d C=%d N=%d k=%d " % (B, H, W, C, N, k)
    c = conv_case(B, H, W, C, N, k, 2, "wide")
    OH, OW = c["pre"].shape[2:]
    assert bool(conv_taps_ext._split_count(B, OH, OW, N, C, k, False)) == expect_split, tag
    xr, wr = c["x"].to(dev).requires_grad_(True), c["w"].to(dev).requires_grad_(True)
    y = conv_taps_ext.conv_strided(xr, wr, c["shift"].to(dev), relu=False)
    assert_bits_equal(y, expected(c["pre"], c["mpre"], BF16, wide=True, what=tag), tag + "forward")
    y.backward(c["dy"].to(dev))
    assert_bits_equal(xr.grad, expected(c["gx"], c["mx"], BF16, wide=True, what=tag + "dx"), tag + "dx")
    assert conv_wgrad_ext.supported(xr.detach(), c["dy"].to(dev), k, 2)
    assert_bits_equal(wr.grad, expected(c["gw"], c["mw"], BF16, wide=B * OH * OW >= 64, what=tag + "dw"), tag + "dw")
    n = conv_case(B, H, W, C, N, k, 2, "narrow")
    want = expected(n["pre"].clamp(min=0), n["mpre"], BF16, zeros_of=n["pre"], what=tag + "narrow")
    assert_bits_equal(conv_taps_ext.conv_strided(n["x"].to(dev), n["w"].to(dev), n["shift"].to(dev), relu=True), want, tag + "shift + relu")


def check_conv_wgrad(dev, B, H, W, C, N, k, stride, monkeypatch):
    """conv_wgrad_ext.weight_gradient directly, fp32 and bf16 results."""
    from monodetr_amd import conv_wgrad_ext
    monkeypatch.setattr(conv_wgrad_ext, "ENABLED", True)
    c = conv_case(B, H, W, C, N, k, stride, "wide")
    x, dy = c["x"].to(dev), c["dy"].to(dev)
    assert conv_wgrad_ext.supported(x, dy, k, stride)
    for dtype in (F32, BF16):
        what = "conv_wgrad B=%d H=%d W=%d C=%d N=%d k=%d stride %d -> %s" % (B, H, W, C, N, k, stride, dtype)
        dw = conv_wgrad_ext.weight_gradient(x, dy, k, stride, dtype)
        assert_bits_equal(dw, expected(c["gw"], c["mw"], dtype, wide=True, what=what), what)


def check_conv_stem(dev, B, H, W):
    """conv_stem_ext.conv_stem: relu(conv7x7 / 2 + shift), wide (rounding of the positive half) and narrow (zeros)."""
    from monodetr_amd import conv_stem_ext
    for kind in ("wide", "narrow"):
        c = conv_case(B, H, W, 3, 64, 7, 2, kind)
        what = "conv_stem B=%d H=%d W=%d %s" % (B, H, W, kind)
        want = expected(c["pre"].clamp(min=0), c["mpre"], BF16, wide=kind == "wide", zeros_of=c["pre"] if kind == "narrow" else None, what=what)
        w = c["w"].to(dev).contiguous()
        assert conv_stem_ext.supported(c["x"].to(dev), w)
        assert_bits_equal(conv_stem_ext.conv_stem(c["x"].to(dev), w, c["shift"].to(dev)), want, what)


def check_decimate_pointwise(dev, monkeypatch, B=2, C=64, H=96, W=95, N=128):
    """The 1x1 / stride-2 projection shortcut as decimate2 + pointwise_conv with the token products on csrc/tgemm.hip and the weight
    gradient on csrc/twgrad.hip (4 608 tokens: above linear._MIN_TOKENS): output, input gradient, weight and bias gradient."""
    from monodetr_amd import conv_wgrad_ext, decimate_ext
    from monodetr_amd.monodetr import linear
    monkeypatch.setattr(linear, "_TGEMM", True)
    monkeypatch.setattr(conv_wgrad_ext, "ENABLED", True)
    c = conv_case(B, H, W, C, N, 1, 2, "wide")
    T = B * c["pre"].shape[2] * c["pre"].shape[3]
    assert T >= linear._MIN_TOKENS
    xr, wr = c["x"].to(dev).requires_grad_(True), c["w"].to(dev).contiguous().requires_grad_(True)
    br = c["shift"].to(BF16).to(dev).requires_grad_(True)
    calls = []
    from monodetr_amd import tgemm_ext
    real_t, real_w = tgemm_ext.tgemm, conv_wgrad_ext.token_weight_gradient
    monkeypatch.setattr(tgemm_ext, "tgemm", lambda *a, **k: (calls.append("tgemm"), real_t(*a, **k))[1])
    monkeypatch.setattr(conv_wgrad_ext, "token_weight_gradient", lambda *a, **k: (calls.append("twgrad"), real_w(*a, **k))[1])
    y = linear.pointwise_conv(decimate_ext.decimate2(xr), wr, br)
    tag = "decimate2 + pointwise_conv "
    assert_bits_equal(y, expected(c["pre"], c["mpre"], BF16, wide=True, what=tag), tag + "forward")
    y.backward(c["dy"].to(dev))
    assert calls == ["tgemm", "tgemm", "twgrad"], calls                       # this repository's kernels produced all of it
    assert_bits_equal(xr.grad, expected(c["gx"], c["mx"], BF16, what=tag + "dx"), tag + "dx")
    assert_bits_equal(wr.grad, expected(c["gw"], c["mw"], BF16, wide=True, what=tag + "dw"), tag + "dw")
    db, mb = c["dy"].double().sum((0, 2, 3)), c["dy"].double().abs().sum((0, 2, 3))
    assert_bits_equal(br.grad, expected(db, mb, BF16, what=tag + "db"), tag + "db")
