"""Exact cases for the MSDA sampling kernels (csrc/msda.hip, csrc/msda_tiled.hip, csrc/msda_fused.hip): forward, gather indices and the
three backward routes, held to BIT EQUALITY with an fp64 reference on operands where every route is exact.  Test infrastructure: plain
torch, no kernel code; tests/test_msda_lattice_cases_gpu.py runs the cases on the device, tests/test_msda_lattice_cases_emulated_cpu.py
through tests/native_emul.py.  The backend (how a kernel is called) is passed in.

OPERANDS: a dyadic lattice.  The PIXEL coordinate of a sample is chosen first, on the quarter-pixel lattice pix + 0.5 = k / 4; the location
the kernels get is loc = fl32((pix + 0.5) / size), and the module checks in fp32 that fl32(loc * size) - 0.5 (pix_coord_f, contraction off;
reference .cuh:285-286) gives pix back for EVERY sample, redrawing the lattice point where it does not (`round_trip`).  Bilinear weights are
then multiples of 2^-4, derivative weights of 2^-2; `attn` holds multiples of 2^-6 in [0, A / 64] with exact zeros; `value` and `grad_out`
hold integers |v| <= V, |g| <= G (bf16 numbers: the bf16 operators see the same values).  `budget` computes, from these amplitude maxima
and the largest number of contributions the drawn POSITIONS give one cell, the sum of the magnitudes of all terms of every output in
units of its quantum:
    out         2^-10 (w attn v)        L P  x 16 A V
    grad_attn   2^-4  (w g v)           16 D G V
    grad_loc    2^-8  (dw attn g v)     size x A x 8 D G V        (the tight one: size = 80, D = 32 leaves V <= 3)
    grad_value  2^-10 (w attn g)        n x 16 A G,   n = the largest number of corners on one cell
each below 2^24, so every partial sum in every order is an fp32 number: the fp32 atomics, the partial-window scratch, the finalize pass and
the lane reductions are exact.  The one-pass kernel's 32-bit fixed point has the quantum 2^(e - 22 + shift), 2^e > max|g| max|attn|; with
the largest shift the sample count allows (the least s with Lq P < 512 << s) it must be no coarser than 2^-10, which `budget` asserts; the
tiled kernel's 64-bit fixed point (2^(e - 44)) is finer still.  Premises raise `PremiseError` (exact_cases.py).

REFERENCE.  `reference` is the operator in fp64 torch on the lattice pixel coordinates themselves (not loc): a sample counts iff
-1 < y < H and -1 < x < W (strict), a corner iff it lies in the map, grad_loc = size attn sum_c g_c d/dpix INCLUDING the corners whose own
bilinear weight is 0, grad_loc = grad_attn = 0 outside the window; gather indices (in_window, h_low, w_low, corner mask).  `anchor` shows
that on random floats it is the fp64 C oracle to 1e-12, and every case checks that on its lattice operands it equals the oracle evaluated
in fp32 on the same tensors bit for bit (the oracle's arithmetic is exact there too).  The expected value of an output is the reference
rounded once to the output's type.

PLACED ON PURPOSE (premises: counts from the operands and the plan alone, before any kernel runs)
  * integer pixel coordinates in x, in y, in both (the high corners have weight 0: skipped for grad_value, needed for grad_loc);
  * per level and axis: pix == -1, in (-1, 0), == 0, == size - 1, in (size - 1, size), == size, beyond (the "far" and "any" sets);
  * levels of extent 1 (the ODD pyramid);
  * footprints that straddle two core tiles in x, in y, four at a core corner (levels the plan splits into tiles);
  * queries whose own position is exactly R cells from the neighbouring core that owns a corner (the "near" set: that block still sees
    the query) and R + 1 cells (the "far" set: the corner goes to the `far` buffer) -- the rule of msda_fused.hip's stray-corner test;
  * "near": every footprint within R cells of the query's own cell: nothing touches the `far` buffer (the emulated run reads Header.far);
  * "contention": every sample of a head on two footprints that share one cell; `block_counts` models which workgroup of the plan
    accumulates which corner (query chunks of a whole level, every query in cross-attention, the queries within reach of a core tile) and
    derives the number of repeated passes: under the plan whose small levels are one chunk, 255 x 4 = 1020 contributions (shift 1) and
    640 x 4 = 2560 (shift 3).  Channels 0 and 1 of grad_out hold +G throughout and attn its maximum there, so a pass that is NOT
    repeated overflows its 32-bit field.

ONE OUTPUT IS NOT EXACT, for a documented operation: with a bf16 grad_value and the `far` buffer in use, the finalize pass adds the fp32
side buffer to the core tile's ALREADY ROUNDED value and rounds again (msda_fused.hip finalize_row).  got = rn(rn(c) + f) for the exact
r = c + f and bf16's unit roundoff 2^-8 (8 significant bits):  |got - r| <= 2^-8 |c| + 2^-8 (|r| + 2^-8 |c|) <= 2^-8 ((1 + 2^-8) T + |r|),
T = the sum of the magnitudes of the cell's terms (from the reference).  Those cases (`far_expected` from the plan model, bf16 grad_value) hold grad_value to that bound; everything else,
and grad_loc / grad_attn always, is equality."""
import functools
import math
import zlib

import torch

from exact_cases import PremiseError, _need, assert_bits_equal, bf16_rounding_shares

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
CAP = float(2 ** 24)
G_AMP, A_NUM, V_MAX = 15, 16, 4            # |grad_out| <= 15, attn in {0 .. 16} / 64, |value| <= V <= 4 (V from the grad_loc budget)
MIN_COUNT = 2                              # samples wanted in every placed class

TINY = ((8, 24), (4, 12), (2, 6), (1, 3))              # S = 255
SMALL = ((12, 40), (6, 20), (3, 10), (2, 5))           # S = 640
ODD = ((1, 1), (2, 3), (1, 7), (5, 1))                 # S = 19
BIG = ((24, 80), (12, 40), (6, 20), (3, 10))           # S = 2550: level 0 in core tiles next to whole-level chunks under the default plan
TWO = ((6, 4), (3, 2))                                 # the generic kernels
GEOMS = dict(tiny=TINY, small=SMALL, odd=ODD, big=BIG, two=TWO)

#             msda_tile_h, msda_tile_w, msda_reach, msda_whole_level_cells, msda_chunks
PLANS = {"tiles_chunks": (4, 8, 2, 30, 3), "tiles_only": (3, 5, 1, 0, 1), "whole": (16, 32, 4, 512, 8), "default": None,
         "one_chunk": (4, 8, 2, 30, 1)}                # one_chunk: the small levels held by ONE workgroup -- the repeated pass
DEFAULT_PLAN = (24, None, 5, 512, 12)                  # tile_w: 32 with bf16 operands, 40 with fp32
#             msda_threads, msda_lps, msda_groups: the six bf16 instantiations of msda_backward_fused_launch; the fp32 form is the seventh
VARIANTS = ((512, 8, 2), (1024, 8, 2), (1024, 4, 2), (1024, 2, 2), (768, 4, 2), (768, 4, 4), "fp32")
ROUTES = ("fused", "tiled", "atomic")


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def set_plan(monkeypatch, plan, variant=None, route=None):
    """MDETR_TUNE for one call: the tile plan, the launch variant and the grad_value route (None: the untuned default)."""
    from conftest import tune
    keys = ("msda_tile_h", "msda_tile_w", "msda_reach", "msda_whole_level_cells", "msda_chunks")
    vals = PLANS[plan] or (None,) * 5
    tune(monkeypatch, **dict(zip(keys, vals)))
    t, l, g = variant if variant not in (None, "fp32") else (None, None, None)
    tune(monkeypatch, msda_threads=t, msda_lps=l, msda_groups=g, msda_bwd=route)


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
def reference(value, shapes, pix, attn, grad_out):
    """fp64.  value [B,S,M,D], shapes ((H, W), ...), pix [B,Lq,M,L,P,2] = (x, y) PIXEL coordinates, attn [B,Lq,M,L,P], grad_out [B,Lq,M*D]
    -> out [B,Lq,M*D], grad_value, grad_loc (w.r.t. the normalised location: x size), grad_attn, idx int32 [B,Lq,M,L,P,4] and
    gv_mag (grad_value with every term replaced by its magnitude)."""
    B, S, M, D = value.shape
    Lq, P = pix.shape[1], pix.shape[4]
    g = grad_out.reshape(B, Lq, M, 1, D)
    out = torch.zeros(B, Lq, M, D, dtype=F64)
    gv, mag = torch.zeros(B, M, S, D, dtype=F64), torch.zeros(B, M, S, D, dtype=F64)
    gl, ga = torch.zeros_like(pix), torch.zeros_like(attn)
    idx = torch.zeros(pix.shape[:-1] + (4,), dtype=torch.int32)
    vt = value.permute(0, 2, 1, 3)                                            # [B,M,S,D]
    start = 0
    for l, (H, W) in enumerate(shapes):
        x, y = pix[:, :, :, l, :, 0], pix[:, :, :, l, :, 1]                  # [B,Lq,M,P]
        inwin = (y > -1) & (y < H) & (x > -1) & (x < W)
        y0, x0 = torch.floor(y), torch.floor(x)
        ly, lx = y - y0, x - x0
        a = torch.where(inwin, attn[:, :, :, l], torch.zeros_like(x))
        samp, dxs, dys = (torch.zeros(B, Lq, M, P, D, dtype=F64) for _ in range(3))
        mask = torch.zeros(B, Lq, M, P, dtype=torch.int32)
        for c, (cy, cx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
            yy, xx = y0 + cy, x0 + cx
            ok = inwin & (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            wy, wx = (ly if cy else 1 - ly), (lx if cx else 1 - lx)
            cell = (start + yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).long()
            flat = cell.permute(0, 2, 1, 3).reshape(B, M, Lq * P, 1).expand(-1, -1, -1, D)
            v = vt.gather(2, flat).view(B, M, Lq, P, D).permute(0, 2, 1, 3, 4) * ok[..., None]
            samp += (wy * wx)[..., None] * v
            dxs += ((1 if cx else -1) * wy)[..., None] * v
            dys += ((1 if cy else -1) * wx)[..., None] * v
            term = ((wy * wx * a * ok)[..., None] * g).permute(0, 2, 1, 3, 4).reshape(B, M, Lq * P, D)
            gv.scatter_add_(2, flat, term)
            mag.scatter_add_(2, flat, term.abs())
            mask |= ok.int() << c
        out += (a[..., None] * samp).sum(3)
        ga[:, :, :, l] = (samp * g).sum(-1) * inwin
        gl[:, :, :, l, :, 0] = W * a * (dxs * g).sum(-1)
        gl[:, :, :, l, :, 1] = H * a * (dys * g).sum(-1)
        iw = inwin.int()
        idx[:, :, :, l] = torch.stack((iw, y0.int() * iw, x0.int() * iw, mask * iw), -1)
        start += H * W
    return dict(out=out.reshape(B, Lq, M * D), gv=gv.permute(0, 2, 1, 3).contiguous(), gl=gl, ga=ga, idx=idx,
                gv_mag=mag.permute(0, 2, 1, 3).contiguous())


def _sizes(shapes):
    return torch.tensor([[w, h] for h, w in shapes], dtype=F64).view(1, 1, 1, len(shapes), 1, 2)


def anchor():
    """`reference` on make_problem's random floats is the fp64 C oracle to 1e-12 of each tensor's largest entry (self- and cross-attention,
    samples outside the maps)."""
    from conftest import make_problem
    from oracle import msda_oracle as oracle
    for shapes, Lq, lo, hi in ((SMALL, 50, -0.3, 1.3), (ODD, 19, -0.2, 1.2), (TWO, 7, 0.0, 1.0)):
        p = make_problem(2, 3, 32, Lq, shapes, 4, F64, seed=7, lo=lo, hi=hi)
        pix = p["loc"] * _sizes(shapes) - 0.5
        r = reference(p["value"], shapes, pix, p["attn"], p["grad_out"])
        want = (oracle.forward(p["value"], p["shapes"], p["level_start"], p["loc"], p["attn"]),) + tuple(
            oracle.backward(p["value"], p["shapes"], p["level_start"], p["loc"], p["attn"], p["grad_out"]))
        for name, w in zip(("out", "gv", "gl", "ga"), want):
            err, top = float((r[name] - w).abs().max()), float(w.abs().max())
            assert err <= 1e-12 * max(top, 1e-300), (shapes, name, err, top)
        assert torch.equal(r["idx"], oracle.indices(p["shapes"], p["loc"]))


# ---- the plan, as far as the cases need it ---------------------------------------------------------------------------------------------
class Level:
    pass


def plan_model(shapes, Lq, plan, tile_w_default):
    """What build_plan (msda_fused.hip) decides per level: mode 0 core tiles with candidate queries, 1 whole level in query chunks,
    2 core tiles scanning every query."""
    th, tw, reach, whole, chunks = PLANS[plan] or DEFAULT_PLAN
    tw = tile_w_default if tw is None else tw
    S = sum(h * w for h, w in shapes)
    out = []
    for H, W in shapes:
        lv = Level()
        lv.H, lv.W, lv.R = H, W, reach
        if Lq == S and H * W <= whole:
            lv.mode, lv.nch, lv.TH, lv.TW = 1, min(chunks, Lq), H, W
        else:
            lv.mode, lv.nch = (0 if Lq == S else 2), 1
            lv.TH, lv.TW = min(th, H), min(tw, W)
            if Lq != S and H * W <= 1024:
                lv.TH, lv.TW = H, W
        out.append(lv)
    return out


def query_cells(shapes):
    """Self-attention: (level, y, x) of every query, in pyramid order."""
    lq, qy, qx = [], [], []
    for l, (H, W) in enumerate(shapes):
        ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        lq.append(torch.full((H * W,), l)), qy.append(ys.reshape(-1)), qx.append(xs.reshape(-1))
    return torch.cat(lq), torch.cat(qy), torch.cat(qx)


def centre_cells(shapes, l):
    """centre_cell (msda_fused.hip) of every query on level l: (qcy, qcx), each [S]."""
    lq, qy, qx = query_cells(shapes)
    hs, ws = torch.tensor([h for h, _ in shapes])[lq], torch.tensor([w for _, w in shapes])[lq]
    H, W = shapes[l]
    return (2 * qy + 1) * H // (2 * hs), (2 * qx + 1) * W // (2 * ws)


def _corners(c, l):
    """Per corner of level l: cell y, x [B,Lq,M,P] (int64) and `live`: in the window, in the map, bilinear weight != 0 -- what the
    one-pass kernel accumulates and counts."""
    H, W = c.shapes[l]
    x, y = c.pix[:, :, :, l, :, 0], c.pix[:, :, :, l, :, 1]
    inwin = (y > -1) & (y < H) & (x > -1) & (x < W)
    y0, x0 = torch.floor(y), torch.floor(x)
    out = []
    for cy, cx in ((0, 0), (0, 1), (1, 0), (1, 1)):
        yy, xx = y0 + cy, x0 + cx
        w = ((y - y0) if cy else 1 - (y - y0)) * ((x - x0) if cx else 1 - (x - x0))
        out.append((yy.long(), xx.long(), inwin & (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W) & (w != 0)))
    return out


def _distance(cell, qc, T):
    """Cells from the query's own position qc to the core tile that holds `cell` (0: inside)."""
    o = cell // T * T
    return torch.clamp(torch.maximum(o - qc, qc - (o + T - 1)), min=0)


def block_counts(c, model):
    """-> (largest number of contributions one workgroup counts on one cell, per level; whether any corner goes to the `far` buffer;
    the largest number of corners on one cell whoever accumulates them)."""
    B, Lq, M, P = c.B, c.Lq, c.M, c.P
    per_level, far, total = [], False, 0
    b_ = torch.arange(B).view(B, 1, 1, 1).expand(B, Lq, M, P)
    m_ = torch.arange(M).view(1, 1, M, 1).expand(B, Lq, M, P)
    q_ = torch.arange(Lq).view(1, Lq, 1, 1).expand(B, Lq, M, P)
    for l, lv in enumerate(model):
        H, W = c.shapes[l]
        n = B * M * lv.nch * H * W
        cnt, tot = torch.zeros(n, dtype=torch.int64), torch.zeros(B * M * H * W, dtype=torch.int64)
        if lv.mode == 0:
            qcy, qcx = (t.view(1, Lq, 1, 1) for t in centre_cells(c.shapes, l))
        for yy, xx, live in _corners(c, l):
            cell = yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)
            tot.index_add_(0, ((b_ * M + m_) * H * W + cell)[live], torch.ones(int(live.sum()), dtype=torch.int64))
            seen = live
            if lv.mode == 0:
                near = (_distance(yy, qcy, lv.TH) <= lv.R) & (_distance(xx, qcx, lv.TW) <= lv.R)
                far = far or bool((live & ~near).any())
                seen = live & near
            chunk = torch.zeros_like(q_)
            if lv.mode == 1:                                                   # chunk t holds queries [Lq t / n, Lq (t + 1) / n)
                edges = torch.tensor([Lq * t // lv.nch for t in range(1, lv.nch)], dtype=torch.int64)
                chunk = torch.bucketize(q_.contiguous(), edges, right=True)
            key = (((b_ * M + m_) * lv.nch + chunk) * H * W + cell)[seen]
            cnt.index_add_(0, key, torch.ones(key.numel(), dtype=torch.int64))
        per_level.append(int(cnt.max()))
        total = max(total, int(tot.max()))
    return per_level, far, total


def shift_of(count):
    """Passes the one-pass kernel repeats: the least s with count < 512 << s."""
    s = 0
    while count >= (512 << s):
        s += 1
    return s


# ---- generators ------------------------------------------------------------------------------------------------------------------------
def round_trip(pix, shapes, dtype=F32):
    """-> (loc, ok): loc = fl((pix + 0.5) / size) and whether fl(loc * size) - 0.5 is pix again, in the operator's location type (fp32;
    fp64 for the fp64 operator), one operation after the other (pix_coord_f with contraction off)."""
    size = _sizes(shapes).to(dtype)
    k4 = (pix + 0.5).to(dtype)
    if not torch.equal(k4.double(), pix + 0.5):
        raise PremiseError("a lattice point is not a number of the location type")
    loc = k4 / size
    prod = loc * size
    back = prod - 0.5
    return loc, back.double() == pix


def _uniform_lattice(g, lo, hi, shape):
    """Quarter-lattice points in [lo, hi] (multiples of 1/4)."""
    return torch.randint(int(round(4 * lo)), int(round(4 * hi)) + 1, shape, generator=g).double() / 4


def _draw(c, kind, g, models, place=True):
    """One full draw of the pixel coordinates [B,Lq,M,L,P,2] of the set `kind`; place: with the samples put on purpose (a redraw of a
    point that failed the round trip is a random one)."""
    B, Lq, M, L, P = c.B, c.Lq, c.M, len(c.shapes), c.P
    pix = torch.zeros(B, Lq, M, L, P, 2, dtype=F64)
    self_ = Lq == c.S
    b_, q_, m_, p_ = torch.meshgrid(torch.arange(B), torch.arange(Lq), torch.arange(M), torch.arange(P), indexing="ij")
    flat = ((b_ * Lq + q_) * M + m_) * P + p_
    if self_:
        lq, qy, qx = query_cells(c.shapes)
    for l, (H, W) in enumerate(c.shapes):
        R = models[0][l].R
        for ax, n in ((0, W), (1, H)):
            if kind == "near":
                qc = centre_cells(c.shapes, l)[1 - ax].view(1, Lq, 1, 1).double()
                v = qc + _uniform_lattice(g, -R, R - 0.25, (B, Lq, M, P))
            elif kind == "contention":                                         # footprint A on an integer cell, B half a cell before it
                cell = torch.randint(0, n, (B, 1, M, 1), generator=g).double()
                on_b = (torch.arange(Lq * P).view(1, Lq, 1, P) % 16) == 15
                v = torch.where(on_b, cell - 0.5, cell).expand(B, Lq, M, P)
            else:                                                              # "far" / "any": anywhere, and beyond the window
                v = _uniform_lattice(g, -1.5, n + 1.5, (B, Lq, M, P))
                edge = torch.tensor([-1.25, -1, -0.75, -0.25, 0, n - 1, n - 0.75, n - 0.25, n, n + 0.25], dtype=F64)
                if place:                                                      # every third sample on a window / map edge, in turn
                    v = torch.where(flat % 3 == 1, edge[(flat // 3 + 3 * ax + l) % len(edge)], v)
            pix[:, :, :, l, :, ax] = v
        if kind == "contention" or not place:
            continue
        # integer pixel coordinates inside the map, in x only, in y only, in both (the last point of every other (b, q, m))
        cls = (b_ + q_ + m_)[..., -1] // 2 % 3
        on = ((b_ + q_ + m_)[..., -1] % 2 == 0)
        x, y = pix[:, :, :, l, -1, 0], pix[:, :, :, l, -1, 1]
        xi, yi = torch.floor(x).clamp(0, W - 1), torch.floor(y).clamp(0, H - 1)
        pix[:, :, :, l, -1, 0] = torch.where(on, torch.where(cls == 1, xi + 0.5, xi), x)
        pix[:, :, :, l, -1, 1] = torch.where(on, torch.where(cls == 0, yi + 0.5, yi), y)
        if not self_:
            continue
        # seams and the reach boundary, with the queries of level l itself (their centre cell is their own cell)
        own = (lq == l)
        for model in models:
            lv = model[l]
            if lv.mode != 0:
                continue
            for ax, n, T, qc, qo in ((0, W, lv.TW, qx, qy), (1, H, lv.TH, qy, qx)):
                for s in range(T, n, T):                                       # a seam: cells s - 1 | s
                    if kind == "near":
                        lo_q, hi_q = s - R, s + R - 1                          # exactly R cells from the core across the seam: still seen
                    else:
                        lo_q, hi_q = s - R - 1, s + R                          # R + 1 cells: the corner across the seam goes to `far`
                    for p, at in ((0, lo_q), (1, hi_q)):
                        sel = own & (qc == at)
                        if 0 <= at < n and bool(sel.any()):
                            pix[:, sel, :, l, p, ax] = s - 0.5
                            pix[:, sel, :, l, p, 1 - ax] = qo[sel].double().view(1, -1, 1) + 0.25
            for sy in range(lv.TH, H, lv.TH):                                  # four cores at a corner
                for sx in range(lv.TW, W, lv.TW):
                    sel = own & (qy == sy - 1) & (qx == sx - 1)
                    pix[:, sel, :, l, 2, 0], pix[:, sel, :, l, 2, 1] = sx - 0.5, sy - 0.25
    return pix


class Case:
    pass


def _class_counts(c):
    """Samples per placed class, per level and axis: {name: [L][2]}."""
    out = {}
    for l, (H, W) in enumerate(c.shapes):
        for ax, n in ((0, W), (1, H)):
            v = c.pix[:, :, :, l, :, ax]
            cls = {"== -1": v == -1, "in (-1, 0)": (v > -1) & (v < 0), "== 0": v == 0, "== size - 1": v == n - 1,
                   "in (size - 1, size)": (v > n - 1) & (v < n), "== size": v == n, "beyond": (v < -1) | (v > n)}
            for k, m in cls.items():
                out.setdefault(k, {})[(l, ax)] = int(m.sum())
    return out


def _integer_counts(c):
    """In-window samples with an integer pixel coordinate in x only, in y only, in both, per level."""
    out = []
    for l, (H, W) in enumerate(c.shapes):
        x, y = c.pix[:, :, :, l, :, 0], c.pix[:, :, :, l, :, 1]
        inwin = (y > -1) & (y < H) & (x > -1) & (x < W)
        xi, yi = x == x.round(), y == y.round()
        out.append((int((inwin & xi & ~yi).sum()), int((inwin & yi & ~xi).sum()), int((inwin & xi & yi).sum())))
    return out


def _seam_counts(c, model):
    """Per tiled level of self-attention: live footprints straddling a seam in x, in y, in both; corners whose owner block is exactly
    R / R + 1 cells from the query's own position, per axis.  {l: dict}."""
    out = {}
    for l, lv in enumerate(model):
        if lv.mode != 0:
            continue
        H, W = c.shapes[l]
        qcy, qcx = (t.view(1, c.Lq, 1, 1) for t in centre_cells(c.shapes, l))
        cs = _corners(c, l)
        (y0, x0, live0), (_, _, live1), (_, _, live2), (_, _, live3) = cs
        sx = live0 & live1 & ((x0 + 1) % lv.TW == 0)
        sy = live0 & live2 & ((y0 + 1) % lv.TH == 0)
        d = dict(x=int((sx & ~sy).sum()), y=int((sy & ~sx).sum()), four=int((sx & sy & live3).sum()),
                 seams_x=W > lv.TW, seams_y=H > lv.TH)
        for name, k in (("R", lv.R), ("R+1", lv.R + 1)):
            nx = ny = 0
            for yy, xx, live in cs:
                dy, dx = _distance(yy, qcy, lv.TH), _distance(xx, qcx, lv.TW)
                nx += int((live & (dx == k) & (dy <= lv.R)).sum())
                ny += int((live & (dy == k) & (dx <= lv.R)).sum())
            d[name] = (nx, ny)
        out[l] = d
    return out


@functools.lru_cache(maxsize=6)
def case(geom, B, M, Lq, kind, plan, D=32, P=4, dtype=F32):
    """The operands, the reference and every premise of one case.  kind: "near" | "far" (self-attention), "any" (cross-attention or the
    generic kernels: anywhere), "contention".  Shared by every test that asks for the same key: never written to."""
    shapes = GEOMS[geom]
    c = Case()
    c.geom, c.shapes, c.kind, c.plan, c.B, c.M, c.D, c.P, c.dtype = geom, shapes, kind, plan, B, M, D, P, dtype
    c.S = sum(h * w for h, w in shapes)
    c.Lq = c.S if Lq is None else Lq
    c.L = L = len(shapes)
    c.tag = "%s/B%d/M%d/Lq%d/%s/%s/D%d" % (geom, B, M, c.Lq, kind, plan, D)
    self_ = c.Lq == c.S
    if kind in ("near", "far") and not self_:
        raise PremiseError(c.tag + ": near / far are sets of self-attention")
    # (the default plan's tile width depends on the operand type: both forms are modelled, the placements serve both)
    c.models = {tw: plan_model(shapes, c.Lq, plan, tw) for tw in ((32, 40) if PLANS[plan] is None else (0,))}
    models = list(c.models.values())
    g = gen("msda_lattice", geom, B, M, c.Lq, kind, plan, D, P)
    # -- pixel coordinates: draw, check the round trip of EVERY coordinate in fp32, redraw where it fails
    c.pix = _draw(c, kind, g, models)
    c.redrawn = 0
    for _ in range(16):
        c.loc, ok = round_trip(c.pix, shapes, F64 if dtype == F64 else F32)
        if bool(ok.all()):
            break
        c.redrawn += int((~ok).sum())
        c.pix = torch.where(ok, c.pix, _draw(c, kind, g, models, place=False))
    else:
        raise PremiseError(c.tag + ": the round trip fails for %d coordinates after 16 redraws" % int((~ok).sum()))
    c.loc = c.loc.contiguous()
    # -- amplitudes from the budget, then the operands
    size = max(max(h, w) for h, w in shapes)
    c.V = min(V_MAX, int((CAP - 1) // (size * A_NUM * 8 * D * G_AMP)))
    if c.V < 1:
        raise PremiseError(c.tag + ": no value amplitude fits the grad_loc budget")
    c.value = torch.randint(-c.V, c.V + 1, (B, c.S, M, D), generator=g).double()
    c.grad_out = torch.randint(-G_AMP, G_AMP + 1, (B, c.Lq, M * D), generator=g).double()
    num = torch.randint(0, A_NUM + 1, (B, c.Lq, M, L, P), generator=g)
    num = torch.where(torch.rand(num.shape, generator=g) < 0.125, torch.zeros_like(num), num)
    if kind == "contention":                                                   # one sign, full amplitude on channels 0 and 1
        c.grad_out.view(B, c.Lq, M, D)[..., :2] = G_AMP
        num = torch.full_like(num, A_NUM)
    c.attn = num.double() / 64
    c.shapes_t = torch.tensor(shapes, dtype=torch.int64)
    c.level_start = torch.cat((c.shapes_t.new_zeros(1), c.shapes_t.prod(1).cumsum(0)[:-1]))
    c.ref = reference(c.value, shapes, c.pix, c.attn, c.grad_out)
    _premises(c)
    return c


def budget(c, cell_count):
    """Sum of the magnitudes of all terms of every output, in units of its quantum, from the amplitude maxima (and the largest number
    of corners the positions put on one cell); the one-pass kernel's quantum at the largest shift the sample count allows."""
    size = max(max(h, w) for h, w in c.shapes)
    units = {"out": c.L * c.P * 16 * A_NUM * c.V, "grad_attn": 16 * c.D * G_AMP * c.V,
             "grad_loc": size * A_NUM * 8 * c.D * G_AMP * c.V, "grad_value": cell_count * 16 * A_NUM * G_AMP}
    for name, u in units.items():
        if not u < CAP:
            raise PremiseError("%s: the terms of %s sum to %d quanta (cap 2^24)" % (c.tag, name, u))
    e = math.frexp(G_AMP * A_NUM / 64.0)[1]                                    # max|g| max|attn| < 2^e
    c.shift_max = shift_of(c.Lq * c.P)                                         # (every sample of a head and level on one cell)
    if e - 22 + c.shift_max > -10:
        raise PremiseError("%s: the fixed-point quantum 2^%d is coarser than a contribution's 2^-10" % (c.tag, e - 22 + c.shift_max))
    return units


def _premises(c):
    r = c.ref
    c.counts, c.far_expected, c.cell_count = {}, False, 0
    for tw, model in c.models.items():
        per_level, far, total = block_counts(c, model)
        c.counts[tw] = per_level
        c.far_expected = c.far_expected or far
        c.cell_count = max(c.cell_count, total)
    c.units = budget(c, c.cell_count)
    for name in ("out", "gv", "gl", "ga"):                                     # (follows from the budget; cheap to see directly)
        if not torch.equal(r[name].float().double(), r[name]):
            raise PremiseError("%s: the reference's %s is not exact in fp32" % (c.tag, name))
    if not bool((r["gv"].abs() <= r["gv_mag"]).all()):
        raise PremiseError(c.tag + ": the magnitude does not bound grad_value")
    # the reference against the C oracle in fp32 on the same tensors, bit for bit
    from oracle import msda_oracle as oracle
    f = F64 if c.dtype == F64 else F32                                         # (the fp64 operator's case: its locations are fp64 numbers)
    v, a, go = c.value.to(f), c.attn.to(f), c.grad_out.to(f)
    o_out = oracle.forward(v, c.shapes_t, c.level_start, c.loc, a)
    o_gv, o_gl, o_ga = oracle.backward(v, c.shapes_t, c.level_start, c.loc, a, go)
    for name, got in (("out", o_out), ("gv", o_gv), ("gl", o_gl), ("ga", o_ga)):
        if not torch.equal(got.double(), r[name]):
            raise PremiseError("%s: the reference's %s is not the oracle's in the operator's type (%d elements)" % (c.tag, name, int((got.double() != r[name]).sum())))
    if not torch.equal(oracle.indices(c.shapes_t, c.loc), r["idx"]):
        raise PremiseError(c.tag + ": the reference's gather indices are not the oracle's")
    # placed classes
    self_ = c.Lq == c.S
    if c.kind != "contention":
        for l, trio in enumerate(_integer_counts(c)):
            if min(trio) < MIN_COUNT:
                raise PremiseError("%s: level %d has %s samples on integer x / y / both" % (c.tag, l, trio))
    if c.kind in ("far", "any"):
        for name, per in _class_counts(c).items():
            for (l, ax), n in per.items():
                if n < MIN_COUNT:
                    raise PremiseError("%s: %d samples with pix %s on level %d axis %d" % (c.tag, n, name, l, ax))
    c.seams = {tw: _seam_counts(c, model) for tw, model in c.models.items()} if self_ and c.kind in ("near", "far") else {}
    for tw, per in c.seams.items():
        for l, d in per.items():
            want = "R" if c.kind == "near" else "R+1"
            for ax, key, has in ((0, "x", d["seams_x"]), (1, "y", d["seams_y"])):
                if has and (d[key] < 1 or d[want][ax] < 1):
                    raise PremiseError("%s: level %d axis %s: %d footprints on a seam, %d corners at distance %s" % (c.tag, l, key, d[key], d[want][ax], want))
            if d["seams_x"] and d["seams_y"] and d["four"] < 1:
                raise PremiseError("%s: level %d: no footprint on four cores" % (c.tag, l))
    if c.kind == "near" and c.far_expected:
        raise PremiseError(c.tag + ": a corner of the near set leaves every block's reach")
    if c.kind == "far" and any(lv.mode == 0 for m in c.models.values() for lv in m) and not c.far_expected:
        raise PremiseError(c.tag + ": no corner of the far set reaches the `far` buffer")
    c.shifts = {tw: [shift_of(n) for n in per] for tw, per in c.counts.items()}
    if c.kind == "contention":
        if c.cell_count <= 511:
            raise PremiseError("%s: the busiest cell draws %d contributions" % (c.tag, c.cell_count))
        want = {(255, "one_chunk"): 1, (640, "one_chunk"): 3}.get((c.Lq, c.plan))
        if want is not None and max(max(s) for s in c.shifts.values()) != want:
            raise PremiseError("%s: shifts %s, wanted %d" % (c.tag, c.shifts, want))
    # bf16 results that need rounding, and exact ties (the spread sets; a contention set has a handful of non-zero cells)
    c.shares = {}
    if c.D == 32 and c.L == 4 and c.P == 4 and c.kind != "contention":
        for name in ("out", "gv"):                                             # (grad_value: of the elements any sample reaches)
            t = r[name] if name == "out" else r["gv"][r["gv_mag"] > 0]
            c.shares[name] = bf16_rounding_shares(t)
            n = t.numel()
            if c.shares[name][0] * n < _need(0.10, n) or c.shares[name][1] * n < _need(0.01, n):
                raise PremiseError("%s: %s: %.3f are no bf16 numbers, %.4f exact ties (wanted 0.10 / 0.01)" % ((c.tag, name) + c.shares[name]))


def describe(c):
    return "msda_lattice %s: redrawn %d, V %d, cell count %d, block counts %s, shifts %s, far %s, bf16 shares %s, seams %s" % (
        c.tag, c.redrawn, c.V, c.cell_count, c.counts, c.shifts, c.far_expected,
        {k: "%.3f/%.4f" % v for k, v in c.shares.items()}, c.seams)


# ---- backends --------------------------------------------------------------------------------------------------------------------------
def _problem(c, elem):
    """The tensors of one call in the operand type `elem` (fp32 / fp64 / bf16 value and grad_out; locations and weights fp32, fp64 for
    the fp64 operator)."""
    f = F64 if elem == F64 else F32
    if c.loc.dtype != f:
        raise PremiseError("%s: locations of %s for an operator that reads %s" % (c.tag, c.loc.dtype, f))
    return dict(value=c.value.to(elem), shapes=c.shapes_t, level_start=c.level_start, loc=c.loc, attn=c.attn.to(f),
                grad_out=c.grad_out.to(elem))


class EmulatedBackend:
    """The C ABI of the emulated library (tests/native_emul.py) on CPU tensors; a fresh workspace holding anything for every call.
    `far` is Header.far (msda_fused.hip) after the last backward call that had a workspace."""
    device = "cpu"

    def __init__(self, lib):
        self.L, self.far = lib, None

    def _ok(self, rc):
        import ctypes
        assert rc == 0, ctypes.string_at(self.L.mdetr_last_error())

    @staticmethod
    def _dims(p):
        B, S, M, D = p["value"].shape
        return B, S, M, D, p["loc"].shape[3], p["loc"].shape[1], p["loc"].shape[4]

    def forward(self, p):
        B, S, M, D, L, Lq, P = dims = self._dims(p)
        out = torch.empty(B, Lq, M * D, dtype=p["value"].dtype)
        ptrs = [p[k].data_ptr() for k in ("value", "shapes", "level_start", "loc", "attn")] + [out.data_ptr()]
        if p["value"].dtype == BF16:
            self._ok(self.L.mdetr_msda_forward_bf16(*ptrs, *dims, 0, None))
        else:
            self._ok(self.L.mdetr_msda_forward(int(p["value"].dtype == F64), *ptrs, *dims, 0, None))
        return out

    def indices(self, p):
        B, S, M, D, L, Lq, P = self._dims(p)
        idx = torch.empty(B, Lq, M, L, P, 4, dtype=torch.int32)
        self._ok(self.L.mdetr_msda_indices(int(p["loc"].dtype == F64), p["shapes"].data_ptr(), p["loc"].data_ptr(), idx.data_ptr(), B, M, L, Lq, P, 0, None))
        return idx

    def backward(self, p, gv_dtype=F32):
        B, S, M, D, L, Lq, P = dims = self._dims(p)
        elem = p["value"].dtype
        gv = torch.full((B, S, M, D), 9.0, dtype=F64 if elem == F64 else gv_dtype)
        gl, ga = torch.full_like(p["loc"], 7.0), torch.full_like(p["attn"], 5.0)
        sh, st = p["shapes"].data_ptr(), p["level_start"].data_ptr()
        n = self.L.mdetr_msda_backward_workspace_bytes(0, sh, st, *dims) if elem != F64 else 0
        ws = torch.randint(0, 255, (max(n, 16),), dtype=torch.uint8)
        self.far = None
        ins = [p[k].data_ptr() for k in ("value", "shapes", "level_start", "loc", "attn", "grad_out")]
        outs = [gv.data_ptr(), gl.data_ptr(), ga.data_ptr()]
        host = [sh if n else None, st if n else None, ws.data_ptr() if n else None, n]
        if gv_dtype == BF16:
            assert n > 0
            self._ok(self.L.mdetr_msda_backward_to(2 if elem == BF16 else 0, 2, ins[0], ins[3], ins[4], ins[5], *outs, *dims, *host, 0, None))
        elif elem == BF16:
            self._ok(self.L.mdetr_msda_backward_bf16(*ins, *outs, *dims, *host, 0, None))
        elif n:
            self._ok(self.L.mdetr_msda_backward_ex(0, *ins, *outs, *dims, *host, 0, None))
        else:
            self._ok(self.L.mdetr_msda_backward(int(elem == F64), *ins, *outs, *dims, 0, None))
        if n:
            self.far = int(ws[8:12].view(torch.int32).item())
        return gv, gl, ga


class DeviceBackend:
    """monodetr_amd.msda_ext on the GPU; results come back as CPU tensors."""
    device, far = "cuda", None

    def forward(self, p):
        from monodetr_amd import msda_ext
        d = {k: v.cuda() for k, v in p.items()}
        args = (d["value"], d["shapes"], d["level_start"], d["loc"], d["attn"])
        return (msda_ext.ms_deform_attn_forward_bf16(*args) if p["value"].dtype == BF16 else msda_ext.ms_deform_attn_forward(*args, 64)).cpu()

    def indices(self, p):
        from monodetr_amd import msda_ext
        return msda_ext.ms_deform_attn_indices(p["shapes"].cuda(), p["loc"].cuda()).cpu()

    def backward(self, p, gv_dtype=F32):
        from monodetr_amd import msda_ext
        d = {k: v.cuda() for k, v in p.items()}
        args = (d["value"], d["shapes"], d["level_start"], d["loc"], d["attn"], d["grad_out"])
        if p["value"].dtype == BF16:
            got = msda_ext.ms_deform_attn_backward_bf16(*args, grad_value_dtype=gv_dtype)
        else:
            got = msda_ext.ms_deform_attn_backward(*args, 64, grad_value_dtype=gv_dtype if gv_dtype == BF16 else None)
        return tuple(t.cpu() for t in got)


# ---- checks ----------------------------------------------------------------------------------------------------------------------------
def _exact(ref64, dtype):
    """The fp64 reference rounded once to `dtype`."""
    return ref64.to(dtype) if dtype == F64 else ref64.float().to(dtype)


def check_forward(c, be, elems=(F32, BF16)):
    """Forward (fp32 / fp64 operator, bf16 operator where it applies) and the gather indices: equality."""
    for elem in elems:
        if elem == BF16 and not (c.D == 32 and c.L == 4 and c.P == 4):
            continue
        p = _problem(c, elem)
        assert_bits_equal(be.forward(p), _exact(c.ref["out"], elem), "%s forward %s" % (c.tag, elem))
    got = be.indices(_problem(c, F64 if c.dtype == F64 else F32))
    assert torch.equal(got, c.ref["idx"]), "%s: %d gather indices differ" % (c.tag, int((got != c.ref["idx"]).any(-1).sum()))


def check_backward(c, be, elem=F32, gv_dtype=F32, what="", far_word=None):
    """One backward call: grad_loc and grad_attn equal the reference bit for bit; grad_value too, except a bf16 grad_value of a call
    that uses the `far` buffer, which is held to the double-rounding bound of the module docstring."""
    tag = "%s backward %s -> grad_value %s %s" % (c.tag, str(elem)[6:], str(gv_dtype)[6:], what)
    p = _problem(c, elem)
    gv, gl, ga = be.backward(p, gv_dtype)
    f = F64 if elem == F64 else F32
    assert_bits_equal(gl, _exact(c.ref["gl"], f), tag + " grad_loc")
    assert_bits_equal(ga, _exact(c.ref["ga"], f), tag + " grad_attn")
    if far_word is not None and be.far is not None:
        assert be.far == far_word, "%s: Header.far is %d" % (tag, be.far)
    if gv_dtype == BF16 and c.far_expected:
        r, T = c.ref["gv"], c.ref["gv_mag"]
        bound = 2.0 ** -8 * ((1 + 2.0 ** -8) * T + r.abs())
        err = (gv.double() - r).abs()
        print("%s: `far` buffer in use: %d elements are not the reference rounded once, worst err / bound %.3f" % (
            tag, int((gv != _exact(r, BF16)).sum()), float((err / bound.clamp(min=1e-300)).max())))
        bad = ~(err <= bound)
        assert not bool(bad.any()), "%s grad_value: %d elements beyond the double-rounding bound" % (tag, int(bad.sum()))
    else:
        assert_bits_equal(gv, _exact(c.ref["gv"], F64 if elem == F64 else gv_dtype), tag + " grad_value")


def check_variant(c, be, variant, monkeypatch):
    """The one-pass kernel in one launch variant under the case's plan: fp32 and bf16 grad_value."""
    set_plan(monkeypatch, c.plan, variant, "fused")
    elem = F32 if variant == "fp32" else BF16
    far_word = (0 if c.kind == "near" else None)
    for gv_dtype in (F32, BF16):
        check_backward(c, be, elem, gv_dtype, "variant %s" % (variant,), far_word)


def check_routes(c, be, monkeypatch, routes=ROUTES):
    """fp32 operator: forward, indices, and the backward through every grad_value route under the case's plan."""
    set_plan(monkeypatch, c.plan)
    check_forward(c, be)
    for route in routes:
        set_plan(monkeypatch, c.plan, None, route)
        check_backward(c, be, F32, F32, "route " + route, 0 if (c.kind == "near" and route == "fused") else None)


def sets_for(geom, plan, Lq):
    """The sets a geometry, plan and call shape are run on.  Cross-attention has no near / far (every block scans every query) and
    cannot reach 512 contributions with 50 x 4 samples; the ODD pyramid's maps are smaller than the reach of most plans: its near set is
    taken where the plan tiles it."""
    if Lq is not None:
        return ("any",)
    if geom == "odd":
        return ("near", "far") if plan == "tiles_only" else ("far",)
    if geom == "big":
        return ("near", "far")
    return ("near", "far", "contention")


def check_generic(be, D, dtype):
    """The generic kernels (any D, fp32 / fp64) on a two-level pyramid, P = 3."""
    c = case("two", 2, 2, 7, "any", "default", D=D, P=3, dtype=dtype)
    print(describe(c))
    check_forward(c, be, elems=(dtype,))
    check_backward(c, be, dtype, F32, "generic")
