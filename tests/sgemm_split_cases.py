"""Cases for the three-way bf16 split form of csrc/sgemm.hip (MDETR_SGEMM_SPLIT; test infrastructure: tests/test_sgemm_split_gpu.py runs
them on the GPU, tests/test_sgemm_split_emulated_cpu.py through tests/native_emul.py).

  1. equality on exact operands: the three groups of tests/exact_cases.py launched with split=True, and `split_case`'s "a" / "w" /
     "int" kinds in the three modes (for TN, A = a.t(), contracted over rows), also with the one-hot operand as bf16 (three terms);
  2. random operands against float64 with the exact form's bound, |got - ref| <= 2 K 2^-24 sum|a||b| + one output rounding: the split
     drops mid.lo + lo.mid + lo.lo <= 2^-25 |a||b| per product, next to an fp32 accumulation whose own worst case is K 2^-24 sum|a||b|;
  3. the same TN group twice: identical bits;
  4. the unflagged call is still the f32-input instruction's k-ordered fmaf chain, to the bit;
  5. a decoder level's heads with a bf16 input (the split form) against the float64 modules."""
import copy
import functools

import torch

import exact_cases as X

BF16, F32 = torch.bfloat16, torch.float32
SHAPES = [(1, 8, 3), (67, 40, 6), (150, 256, 70), (131, 355, 64), (130, 96, 256)]        # (T, K, N)
TN_SHAPES = SHAPES + [(45, 4400, 256), (6, 611, 256)]                                    # ... across the contraction split, ragged last part
KINDS = ("a", "w", "int")
MODES = ("nt", "nn", "tn")
# the launcher's rules (MDETR_TUNE keys of csrc/sgemm.hip): rows of the NT / NN tile, workgroups a TN group aims at
TUNES = ("", "sgemm_split_tm=32,sgemm_split_tn_wgs=100", "sgemm_split_tm=64,sgemm_split_tn_wgs=4096")


def _S():
    from monodetr_amd import sgemm_ext
    return sgemm_ext


def tr(t):
    """t^T with fresh row-major strides (contiguous() keeps the strides of a [K, 1] view as they are)."""
    return torch.empty(t.shape[1], t.shape[0], dtype=t.dtype).copy_(t.t())


def product(dev, mode, a, w_nk, split, a_dtype=F32, w_dtype=F32):
    """a [T, K] @ w_nk [N, K]^T -> [T, N] fp32 through the given mode's layout of the operands."""
    S = _S()
    T, N = a.shape[0], w_nk.shape[0]
    out = torch.empty(T, N, device=dev)
    ad, wd = a.to(a_dtype), w_nk.to(w_dtype)
    if mode == "nt":
        S.grouped(S.NT, [S.Problem([(ad.to(dev), wd.to(dev))], out)], split=split)
    elif mode == "nn":
        S.grouped(S.NN, [S.Problem([(ad.to(dev), tr(wd).to(dev))], out)], split=split)
    else:
        S.grouped(S.TN, [S.Problem([(tr(ad).to(dev), tr(wd).to(dev))], out)], split=split)
    return out


# ---- 1. equality ------------------------------------------------------------------------------------------------------------------------
def check_exact_groups(dev, monkeypatch):
    """exact_cases' three sgemm groups (bias, partial ReLU into a column slice, the 3- and 6-wide heads, bf16 result with res and mask,
    five-term NN with a 3-deep term, TN with column sums) with every launch in the split form."""
    S = _S()
    plain = S.grouped
    calls = []

    def split_grouped(mode, problems, split=False):
        calls.append(mode)
        return plain(mode, problems, split=True)
    monkeypatch.setattr(S, "grouped", split_grouped)
    X.check_sgemm_nt(dev)
    X.check_sgemm_nn(dev)
    X.check_sgemm_tn(dev, 37)
    X.check_sgemm_tn(dev, 611)
    assert calls == [S.NT, S.NN, S.TN, S.TN]


def check_split_case(dev, mode, kind, shape):
    T, K, N = shape
    a, w_nk, want = X.split_case(T, K, N, False, kind)
    X.assert_bits_equal(product(dev, mode, a, w_nk, True), want, "sgemm split %s (%s) T=%d K=%d N=%d" % (mode, kind, T, K, N))


def check_three_term_case(dev, mode, shape):
    """The "w" kind (one-hot a against a full-mantissa weight) with the one-hot operand as bf16 (+-2^e is exact): the bf16 A of NT, the
    bf16 B of TN -- the operand the heads pass as bf16, their input x.  Three terms, still bit-exact."""
    T, K, N = shape
    a, w_nk, want = X.split_case(T, K, N, False, "w")
    assert bool((a.to(BF16).float() == a).all())
    if mode == "nt":
        got = product(dev, "nt", a, w_nk, True, a_dtype=BF16)
    else:                                                            # C^T [N, T] = w_nk a^T: A = w_nk^T [K, N] fp32, B = a^T [K, T] bf16
        got = product(dev, "tn", w_nk, a, True, w_dtype=BF16).t()
    X.assert_bits_equal(got.contiguous(), want, "sgemm split %s, bf16 one-hot operand, T=%d K=%d N=%d" % (mode, T, K, N))


# ---- 2. bounded -------------------------------------------------------------------------------------------------------------------------
def close(got, ref, absref, K, what=""):
    """tests/test_sgemm_gpu.py::_close: |got - ref| <= 2 K 2^-24 sum|a||b| + one output rounding."""
    got = got.detach().cpu()
    bound = 2.0 * K * 2.0 ** -24 * absref + (2.0 ** -8 * ref.abs() if got.dtype == BF16 else 2.0 ** -23 * ref.abs()) + 1e-30
    err = (got.double() - ref).abs()
    print("%s: worst |got - ref| / bound = %.4f" % (what, float((err / bound).max())))
    bad = err > bound
    assert not bad.any(), (what, int(bad.sum()), float((err / bound).max()))


@functools.lru_cache(maxsize=None)
def heads_operands(T, x_dtype):
    g = torch.Generator().manual_seed(1000 + T + (1 if x_dtype == BF16 else 0))
    r = lambda *s: torch.randn(*s, generator=g)                                    # noqa: E731
    d = dict(x=r(T, 256).to(x_dtype), w1=[r(256, 256) * 0.06 for _ in range(4)], b1=[r(256) for _ in range(4)], wc=r(3, 256), bc=r(3),
             w2b=r(256, 256) * 0.06, b2b=r(256), wd=r(3, 256), bd=r(3), wp=r(2, 256), bp=r(2), wa=r(24, 256), ba=r(24), w3b=r(6, 256), b3b=r(6),
             g_delta=r(T, 6), g_size=r(T, 3), g_depth=r(T, 2), g_angle=r(T, 24), g_logits=r(T, 3), dh1=r(T, 1024), dh2=r(T, 256),
             h1=r(T, 1024).clamp(min=0), h2=r(T, 256).clamp(min=0), skip=r(T, 256).to(x_dtype))
    return d


def check_heads_groups_bounded(dev, T, x_dtype):
    """The seven launches of a decoder level (monodetr/heads.py) in the split form on random operands; x_dtype = bf16 gives the
    bf16 x fp32 mix (first layers, half of the weight gradients), fp32 the fp32 x fp32 one."""
    S = _S()
    o = heads_operands(T, x_dtype)
    dv = lambda t: t.to(dev)                                                       # noqa: E731
    P, G = S.Problem, functools.partial(S.grouped, split=True)
    dbl = lambda t: t.double()                                                     # noqa: E731
    new = lambda *s, **k: torch.empty(*s, device=dev, **k)                         # noqa: E731
    sl = [slice(256 * i, 256 * (i + 1)) for i in range(4)]
    x, xd = dv(o["x"]), dbl(o["x"])
    # NT group 1: four first layers + the class head on x
    h1, logits = new(T, 1024), new(T, 3)
    G(S.NT, [P([(x, dv(w))], h1[:, s], bias=dv(b), relu_cols=True) for w, b, s in zip(o["w1"], o["b1"], sl)] + [P([(x, dv(o["wc"]))], logits, bias=dv(o["bc"]))])
    for i in range(4):
        close(h1[:, sl[i]], (xd @ dbl(o["w1"][i]).t() + dbl(o["b1"][i])).clamp(min=0), xd.abs() @ dbl(o["w1"][i]).abs().t() + dbl(o["b1"][i]).abs(), 256, "NT1 first layer %d" % i)
    close(logits, xd @ dbl(o["wc"]).t() + dbl(o["bc"]), xd.abs() @ dbl(o["wc"]).abs().t() + dbl(o["bc"]).abs(), 256, "NT1 class head")
    # NT group 2: 256 -> 256 + three narrow heads on slices of h1;  NT group 3: 256 -> 6
    H1, H2 = dv(o["h1"]), dv(o["h2"])
    outs = [new(T, 256), new(T, 3), new(T, 2), new(T, 24)]
    ws, bs = (o["w2b"], o["wd"], o["wp"], o["wa"]), (o["b2b"], o["bd"], o["bp"], o["ba"])
    G(S.NT, [P([(H1[:, s], dv(w))], out, bias=dv(b), relu_cols=(True if i == 0 else 0)) for i, (s, w, b, out) in enumerate(zip(sl, ws, bs, outs))])
    for i, (s, w, b, out) in enumerate(zip(sl, ws, bs, outs)):
        ref = dbl(o["h1"][:, s]) @ dbl(w).t() + dbl(b)
        close(out, ref.clamp(min=0) if i == 0 else ref, dbl(o["h1"][:, s]).abs() @ dbl(w).abs().t() + dbl(b).abs(), 256, "NT2 problem %d" % i)
    delta = new(T, 6)
    G(S.NT, [P([(H2, dv(o["w3b"]))], delta, bias=dv(o["b3b"]))])
    close(delta, dbl(o["h2"]) @ dbl(o["w3b"]).t() + dbl(o["b3b"]), dbl(o["h2"]).abs() @ dbl(o["w3b"]).abs().t() + dbl(o["b3b"]).abs(), 256, "NT3")
    # NN 1: g_delta w3b under the mask h2;  NN 2: four products under the mask h1
    dh2 = new(T, 256)
    G(S.NN, [P([(dv(o["g_delta"]), dv(o["w3b"]))], dh2, mask=H2)])
    close(dh2, (dbl(o["g_delta"]) @ dbl(o["w3b"])) * (o["h2"] > 0), dbl(o["g_delta"]).abs() @ dbl(o["w3b"]).abs(), 6, "NN1")
    dh1 = new(T, 1024)
    gs2 = (o["dh2"], o["g_size"], o["g_depth"], o["g_angle"])
    G(S.NN, [P([(dv(g), dv(w))], dh1[:, s], mask=H1[:, s]) for g, w, s in zip(gs2, ws, sl)])
    for i, (g, w, s) in enumerate(zip(gs2, ws, sl)):
        close(dh1[:, s], (dbl(g) @ dbl(w)) * (o["h1"][:, s] > 0), dbl(g).abs() @ dbl(w).abs(), g.shape[1], "NN2 problem %d" % i)
    # NN 3: dx, five terms, K = 1027, res and result in x's dtype
    DH1 = dv(o["dh1"])
    dx = new(T, 256, dtype=x_dtype)
    G(S.NN, [P([(DH1[:, s], dv(w)) for s, w in zip(sl, o["w1"])] + [(dv(o["g_logits"]), dv(o["wc"]))], dx, res=dv(o["skip"]))])
    ref = sum(dbl(o["dh1"][:, s]) @ dbl(w) for s, w in zip(sl, o["w1"])) + dbl(o["g_logits"]) @ dbl(o["wc"]) + dbl(o["skip"])
    absref = sum(dbl(o["dh1"][:, s]).abs() @ dbl(w).abs() for s, w in zip(sl, o["w1"])) + dbl(o["g_logits"]).abs() @ dbl(o["wc"]).abs() + dbl(o["skip"]).abs()
    close(dx, ref, absref, 1027, "NN3 dx")
    check_tn_bounded(dev, T, x_dtype, full=True)


def tn_jobs(T, x_dtype, full):
    """(dy, act) pairs of a level's weight-gradient group; full: all ten, else a light group that still takes the largest split."""
    o = heads_operands(T, x_dtype)
    sl = [slice(256 * i, 256 * (i + 1)) for i in range(4)]
    if not full:
        return [(o["dh1"][:, 0:45], o["x"][:, :64]), (o["g_delta"], o["h1"][:, 5:75])]
    return [(o["g_delta"], o["h2"]), (o["dh2"], o["h1"][:, sl[0]]), (o["g_size"], o["h1"][:, sl[1]]), (o["g_depth"], o["h1"][:, sl[2]]),
            (o["g_angle"], o["h1"][:, sl[3]])] + [(o["dh1"][:, s], o["x"]) for s in sl] + [(o["g_logits"], o["x"])]


def check_tn_bounded(dev, T, x_dtype, full):
    """Weight gradients with their column sums, then the same group again: identical bits (fixed summation order, no atomics)."""
    S = _S()
    jobs = tn_jobs(T, x_dtype, full)
    cache = {}

    def dv(t):                                                       # (slices of one tensor stay slices of one device tensor)
        base = t._base if t._base is not None else t
        if id(base) not in cache:
            cache[id(base)] = base.to(dev)
        return cache[id(base)].as_strided(t.shape, t.stride(), t.storage_offset())
    res = []
    for _ in range(2):
        dws = [torch.empty(dy.shape[1], act.shape[1], device=dev) for dy, act in jobs]
        dbs = [torch.empty(dy.shape[1], device=dev) for dy, act in jobs]
        S.grouped(S.TN, [S.Problem([(dv(dy), dv(act))], dw, colsum=db) for (dy, act), dw, db in zip(jobs, dws, dbs)], split=True)
        res.append((dws, dbs))
    for i, ((dy, act), dw, db) in enumerate(zip(jobs, *res[0])):
        close(dw, dy.double().t() @ act.double(), dy.double().abs().t() @ act.double().abs(), T, "TN T=%d problem %d dW" % (T, i))
        close(db, dy.double().sum(0), dy.double().abs().sum(0), T, "TN T=%d problem %d db" % (T, i))
    for a, b in zip(res[0][0] + res[0][1], res[1][0] + res[1][1]):
        assert torch.equal(a, b)


# ---- 4. the unflagged call ----------------------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fp32 fmaf(a, b, c) on fp32 values held in float64 tensors: the product is exact in float64; the sum is rounded to odd at 53 bits
    (TwoSum gives the error), so that the final rounding to 24 bits is the correct one."""
    p = a * b
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    bits = s.view(torch.int64)
    fix = (e != 0) & ((bits & 1) == 0)
    away = (e > 0) == (s > 0)
    bits = torch.where(fix, torch.where(away, bits + 1, bits - 1), bits)
    return bits.view(torch.float64).float().double()


def chain_nt_nn(a, w_nk):
    """sgemm_kernel's order: slabs of 32; instruction (q, j) of a slab contracts k = 8 q + j, then k = 8 q + 4 + j."""
    T, K = a.shape
    a64, w64 = a.double(), w_nk.double()
    acc = torch.zeros(T, w_nk.shape[0], dtype=torch.float64)
    for k0 in range(0, K, 32):
        for q in range(4):
            for j in range(4):
                for k in (k0 + 8 * q + j, k0 + 8 * q + 4 + j):
                    if k < K:
                        acc = fma32(a64[:, k:k + 1], w64[:, k].unsqueeze(0), acc)
                    # (a missing element is a zero operand: fmaf(0, 0, acc) == acc)
    return acc.float()


def chain_tn(a, w_nk, waves=4):
    """sgemm_tn_kernel without a contraction split: the rows in `waves` chunks (an even count each), a chain per wave in row order,
    then (w0 + w2) + (w1 + w3)."""
    T, K = a.shape
    a64, w64 = a.double(), w_nk.double()
    chunk = ((K + 2 * waves - 1) // (2 * waves)) * 2
    parts = []
    for wv in range(waves):
        acc = torch.zeros(T, w_nk.shape[0], dtype=torch.float64)
        for k in range(min(K, wv * chunk), min(K, (wv + 1) * chunk)):
            acc = fma32(a64[:, k:k + 1], w64[:, k].unsqueeze(0), acc)
        parts.append(acc.float())
    return (parts[0] + parts[2]) + (parts[1] + parts[3])


def check_unflagged_is_the_fmaf_chain(dev):
    T, K, N = 150, 256, 70
    g = X.gen(T, K, N, 99)
    a, w_nk = X.full_mantissa(g, (T, K)), X.full_mantissa(g, (N, K))
    X.assert_bits_equal(product(dev, "nt", a, w_nk, False), chain_nt_nn(a, w_nk), "exact form NT")
    X.assert_bits_equal(product(dev, "nn", a, w_nk, False), chain_nt_nn(a, w_nk), "exact form NN")
    X.assert_bits_equal(product(dev, "tn", a, w_nk, False), chain_tn(a, w_nk), "exact form TN")
    # ... and the flag does change the arithmetic (the test above would pass vacuously if it were ignored)
    assert not torch.equal(product(dev, "nt", a, w_nk, True).cpu(), chain_nt_nn(a, w_nk))


# ---- 5. a heads level -------------------------------------------------------------------------------------------------------------------
def check_heads_level_split(dev):
    """tests/test_sgemm_gpu.py::test_heads_level_matches_the_modules_on_the_gpu at B = 2, Q = 50 with a bf16 x (the split form): its
    tolerances, its exclusion of rows with a hidden pre-activation within 2e-5 of zero, its premise on the excluded share."""
    from torch import nn
    from monodetr_amd.monodetr import heads as H
    from monodetr_amd.monodetr.depthaware_transformer import MLP
    S = _S()
    torch.manual_seed(5)
    mods = [MLP(256, 256, 6, 3), MLP(256, 256, 3, 2), MLP(256, 256, 2, 2), MLP(256, 256, 24, 2), nn.Linear(256, 3)]
    ref = [copy.deepcopy(m).double() for m in mods]
    mods = [m.to(dev) for m in mods]
    B, Q = 2, 50
    x = torch.randn(B, Q, 256).to(BF16).to(dev).requires_grad_(True)
    with torch.no_grad():
        xd0 = x.detach().cpu().double()
        pre = [m.layers[0](xd0) for m in ref[:4]]
        near = torch.stack([p.abs().amin(-1) for p in pre] + [ref[0].layers[1](pre[0].clamp(min=0)).abs().amin(-1)]).amin(0) < 2e-5
        keep = (~near).float().unsqueeze(-1)
    assert 0.0 < float(near.float().mean()) < 0.2
    modes = []
    plain = S.grouped

    def spy(mode, problems, split=False):
        modes.append(bool(split))
        return plain(mode, problems, split=split)
    was, H.ENABLED, S.grouped = H.ENABLED, True, spy
    try:
        out = H.heads_level(x, *mods)
        assert out is not None
        delta, size, depth, angle, logits, xs = out
        gs = [torch.randn(t.shape) * keep for t in (delta, size, depth, angle, logits)]
        skip_w = torch.randn(B, Q, 256)
        (sum((t * g.to(dev)).sum() for t, g in zip((delta, size, depth, angle, logits), gs)) + (xs.float() * skip_w.to(dev)).sum()).backward()
    finally:
        H.ENABLED, S.grouped = was, plain
    assert modes == [True] * 7                                         # a bf16 x: every launch of the level in the split form
    xd = x.detach().cpu().double().requires_grad_(True)
    outs = [m(xd) for m in ref]
    (sum((t * g.double()).sum() for t, g in zip(outs, gs)) + (xd * skip_w.double()).sum()).backward()
    for got, want in zip((delta, size, depth, angle, logits), outs):
        assert (got.detach().cpu().double() - want.detach()).abs().max() <= 1e-5 * max(1.0, float(want.detach().abs().max()))
    assert (x.grad.cpu().double() - xd.grad).abs().max() <= 2.0 ** -7 * float(xd.grad.abs().max())
    for m, r in zip(mods, ref):
        for (n, p), (_, q) in zip(m.named_parameters(), r.named_parameters()):
            assert (p.grad.cpu().double() - q.grad).abs().max() <= 1e-5 * max(1.0, float(q.grad.abs().max())), n
