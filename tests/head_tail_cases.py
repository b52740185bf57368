"""Cases, references and checks for csrc/head_tail.hip: `box_refine`, the head-tail forward and backward and
`head_tail_map_grad_kernel` (the depth map's gradient, per cell, from (level, query) pairs staged in LDS batches of 2048).  Test
infrastructure: plain torch in fp64, no kernel code; tests/test_head_tail_cases_gpu.py runs the cases on the device,
tests/test_head_tail_cases_emulated_cpu.py through tests/native_emul.py.

REFERENCE.  `reference()` of tests/test_head_tail_emulated_cpu.py (the product's framework path, monodetr.py:226-253) with autograd,
evaluated in float64; the same function in fp32 on the device under test is the yardstick's framework path.  `magnitudes` writes the
NATURAL MAGNITUDE of every result out -- the same expression with every term replaced by its absolute value (1 - c counts 1 + c) --
plus the amplification of an input's own fp32 rounding where it feeds a transcendental or a lookup.  With z = delta + inverse_sigmoid(ref),
|z| = |delta| + |inverse_sigmoid(ref)|, c = sigmoid(z), s = sigmoid(depth_reg_0), q = s + 1e-6, g0 = g_depth_0 / 3,
raw = (c_4 + c_5) img_h, h2d = max(raw, 1), pass = [raw >= 1]:
    n(c)            = c + |z| c (1 - c)
    a_h             = pass (n(c_4) + n(c_5)) img_h / h2d                                  (the relative error h2d inherits from c)
    scale(coord)    = n(c)
    scale(depth_0)  = ((1 / q) (1 + |depth_reg_0| s (1 - s) / q) + 1 + |size3d_0| focal / h2d (1 + a_h) + n(m)) / 3
    n(m)            = sum_cells |map| hx hy + (n(c_0) + 1) (W - 1) sum |map| dx hy + (n(c_1) + 1) (H - 1) sum |map| hx dy
                      hx = max(0, 1 - |x - X|) the bilinear weight of column X for the pixel coordinate x = c_0 (W - 1), dx = 1 on
                      |x - X| <= 1 + 2^-10 its Lipschitz bound (closed, with slack far above fp32's error in x: a cell next to the
                      footprint that receives a weight of rounding size is covered), likewise hy, dy
    scale(g_size3d_0)   = |g0| focal / h2d (1 + a_h)
    scale(g_depth_reg_0) = |g0| / q^2 s (1 + s) (1 + |depth_reg_0|)
    scale(g_delta_k)    = (|g_coord_k| + [k >= 4] pass |g0| |size3d_0| focal img_h / h2d^2 (1 + 2 a_h)) (c (1 + c) + |z| c (1 - c))
    scale(g_init_ref_k) = scale(g_delta_k at level 0) |d inverse_sigmoid / d ref|
    scale(g_map[cell])  = sum_pairs |g0| (hx hy + (n(c_0) + 1) (W - 1) dx hy + (n(c_1) + 1) (H - 1) hx dy)
`anchor` shows once that the dense hat-function form of the map gradient is F.grid_sample's autograd in float64 to 1e-12.

BOUND (the project's rule, criterion_cases.py; no new number).  Per element
    B = max(8 x the error of the framework path in fp32 within the element's row, 64 x 2^-24 x scale),
row = one (l, b, q) (one (b, q) for g_init_ref), one cell for g_map.  Checked: coord, depth_ave, and the gradients of delta, init_ref,
size3d, depth_reg and depth_map; box_refine's result against sigmoid(delta + inverse_sigmoid(ref)) under the same rule.  No share of
elements is left out.

PREMISES, from the inputs and fp64 alone: they keep the fp32 and the fp64 path on the same side of a discontinuity.  |raw - 1| >
64 x 2^-24 (except the built tie of the exact case); no reference within 64 x 2^-24 (relative) of eps or 1 - eps (fp32 1e-5f and the
double 1e-5 differ: the two paths clamp differently exactly there).  References at exactly 0 and 1 are asserted to the kernel's
convention, derivative 1, which is what autograd gives through the clamps.

ALWAYS ASSERTED: depth_ave[..., 1] is depth_reg[..., 1] and g_depth_reg[..., 1] is g_depth[..., 1], bit for bit; g_size3d[..., 1:] == 0;
with only `coord` used the gradients of size3d, depth_reg and depth_map are exact zeros, with only `depth_ave` used g_delta[..., :4]
and g_init_ref[..., :4] are; two runs give equal bits in every output (the map gradient is deterministic: no atomics).

EXACT CASE (equality).  delta = 0 and every reference 0.5, H and W odd, g_depth[..., 0] = 3 x integers, g_coord integers, size3d
integers, focal 512, the last image has img_h = 1: coord == 0.5 everywhere, every centre is the middle pixel with fractions 0, g_map
equals the integer sum at that one cell per image and exactly 0 elsewhere.  (c_4 + c_5) img_h == 1 in the last image is the clamp's
tie: the gradient passes, as clamp(min = 1) does, and g_delta of that image is the fp64 value exactly (premise: it is nonzero).

Every check prints its figures ("head_tail_case ..." lines: worst error / bound per tensor and the framework's own error over the
floor) before it asserts; the device's are in profiles/pointwise_cases_measured.txt.  No bound was widened and no defect showed.  The
closest figure is 0.125 = 1 / 8 (g_init_ref, coord and g_delta with delta = -100): sigmoid underflows to 0 in fp32, in the kernel as in
the framework path, where fp64 holds 1e-39 .. 1e-44; the natural magnitude is of that size and the framework's own error is the bound.
Everything else stays below 0.05 of B."""
import contextlib
import functools
import math
import zlib

import torch
import torch.nn.functional as F

from exact_cases import PremiseError, assert_bits_equal
from monodetr_amd.utils.misc import inverse_sigmoid
from test_head_tail_emulated_cpu import reference

F32, F64 = torch.float32, torch.float64
FLOOR = 64.0 * 2.0 ** -24
MARGIN = 8.0
EPS = 1e-5

#            (L, B, Q, H, W, nd0)
SHAPES = {
    "single":   (1, 1, 1, 1, 1, 2),         # single query, single cell
    "train2":   (3, 2, 37, 24, 80, 2),      # the training geometry, small Q
    "train6":   (3, 2, 37, 24, 80, 6),
    "batch2":   (3, 2, 700, 5, 7, 6),       # 2100 pairs: second LDS batch; 35 cells: partial last workgroup
    "pairs3300": (6, 1, 550, 24, 80, 6),    # 3300 pairs
    "narrow":   (2, 3, 300, 3, 50, 2),      # three images, narrow map
    "h1":       (3, 2, 9, 1, 17, 2),        # H = 1
    "w1":       (3, 2, 9, 13, 1, 6),        # W = 1
}
KINDS = ("benign", "saturated", "refs01", "tiny_boxes", "borders", "one_cell", "zero_rows")
EXACT_SHAPES = {"single": (1, 2, 1, 1, 1, 2), "batch2": (3, 2, 700, 5, 7, 6), "train": (3, 2, 37, 23, 79, 2), "h1": (3, 2, 9, 1, 17, 2), "w1": (3, 2, 9, 13, 1, 6)}
REFINE_ROWS = (1, 257, 1100)
NAMES = ("delta", "init_ref", "size3d", "depth_reg", "depth_map")


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


@contextlib.contextmanager
def kernels_on(backend=None):
    """The head-tail extension switched on and routed to `backend` (the emulated library) for the duration; None: the device library."""
    from monodetr_amd import head_tail_ext
    saved = (head_tail_ext._backend, head_tail_ext.ENABLED)
    if backend is not None:
        head_tail_ext._backend = backend
    head_tail_ext.ENABLED = True
    try:
        yield head_tail_ext
    finally:
        head_tail_ext._backend, head_tail_ext.ENABLED = saved


# ---- reference and magnitudes -----------------------------------------------------------------------------------------------------------
def _hats(c01, H, W):
    """c01 [P, 2] (x, y in [0, 1]) -> bilinear weights hx [P, W], hy [P, H] and their closed Lipschitz supports dx, dy."""
    x, y = ((c01[:, 0] - 0.5) * 2 + 1) * 0.5 * (W - 1), ((c01[:, 1] - 0.5) * 2 + 1) * 0.5 * (H - 1)
    ax, ay = (x[:, None] - torch.arange(W, dtype=F64)).abs(), (y[:, None] - torch.arange(H, dtype=F64)).abs()
    slack = 1 + 2.0 ** -10
    return (1 - ax).clamp(min=0), (1 - ay).clamp(min=0), (ax <= slack).double(), (ay <= slack).double()


def _framework(t, dtype, device, gc, gd):
    """`reference` with autograd at `dtype` on `device` -> coord, depth_ave and the five gradients (None where an output is unused)."""
    cast = lambda x: x.to(dtype).to(device)                                    # noqa: E731
    leaves = [cast(t[k]).clone().requires_grad_(True) for k in NAMES]
    coord, ave = reference(leaves[0], leaves[1], cast(t["inter"]), leaves[2], leaves[3], leaves[4], cast(t["img_h"]), cast(t["focal"]))
    outs, gs = [o for o, g in ((coord, gc), (ave, gd)) if g is not None], [cast(g) for g in (gc, gd) if g is not None]
    grads = torch.autograd.grad(outs, leaves, gs, allow_unused=True)
    out = dict(coord=coord.detach(), depth=ave.detach())
    out.update({"g_" + k: (g if g is not None else torch.zeros_like(leaf)) for k, g, leaf in zip(NAMES, grads, leaves)})
    return {k: v.detach().cpu() for k, v in out.items()}


def magnitudes(t, gc, gd, r64):
    """The scales of the module docstring, fp64, from the inputs and the fp64 reference alone."""
    d = {k: v.double() for k, v in t.items()}
    L, B, Q, _ = d["delta"].shape
    H, W = d["depth_map"].shape[-2:]
    nd0 = d["init_ref"].shape[-1]
    first = F.pad(inverse_sigmoid(d["init_ref"]), (0, 6 - nd0))
    inv = torch.cat((first[None], inverse_sigmoid(d["inter"])), 0)
    zabs = d["delta"].abs() + inv.abs()
    c = r64["coord"]
    amp = zabs * c * (1 - c)
    n = c + amp
    ih, fo = d["img_h"].view(1, -1, 1), d["focal"].view(1, -1, 1)
    raw = (c[..., 4] + c[..., 5]) * ih
    h2d, passes = raw.clamp(min=1.0), (raw >= 1.0).double()
    a_h = passes * (n[..., 4] + n[..., 5]) * ih / h2d
    dr, sz = d["depth_reg"][..., 0], d["size3d"][..., 0]
    s = torch.sigmoid(dr)
    q = s + 1e-6
    g0 = gd.double()[..., 0].abs() / 3
    gca = gc.double().abs()
    # the lookup and its transpose, image by image
    n_m, s_map = torch.zeros(L, B, Q, dtype=F64), torch.zeros(B, H, W, dtype=F64)
    for b in range(B):
        cb, nb = c[:, b].reshape(L * Q, 6), n[:, b].reshape(L * Q, 6)
        hx, hy, dx, dy = _hats(cb[:, :2], H, W)
        ex, ey = ((nb[:, 0] + 1) * (W - 1))[:, None], ((nb[:, 1] + 1) * (H - 1))[:, None]
        m = d["depth_map"][b].abs()
        n_m[:, b] = (((hy @ m) * hx).sum(-1) + ((hy @ m) * dx * ex).sum(-1) + (((dy * ey) @ m) * hx).sum(-1)).view(L, Q)
        gb = g0[:, b].reshape(L * Q, 1)
        s_map[b] = (hy * gb).t() @ hx + (hy * gb).t() @ (dx * ex) + (dy * ey * gb).t() @ hx
    geo = sz.abs() * fo / h2d * (1 + a_h)
    sc = dict(coord=n, depth=torch.stack((((1 / q) * (1 + dr.abs() * s * (1 - s) / q) + 1 + geo + n_m) / 3, torch.zeros_like(q)), -1))
    sc["g_size3d"] = F.pad((g0 * fo / h2d * (1 + a_h))[..., None], (0, 2))
    sc["g_depth_reg"] = torch.stack((g0 / (q * q) * s * (1 + s) * (1 + dr.abs()), torch.zeros_like(q)), -1)
    gh = passes * g0 * sz.abs() * fo * ih / (h2d * h2d) * (1 + 2 * a_h)
    gtot = gca + torch.cat((torch.zeros(L, B, Q, 4, dtype=F64), gh[..., None].expand(L, B, Q, 2)), -1)
    sc["g_delta"] = gtot * (c * (1 + c) + amp)
    x = d["init_ref"]
    inside = ((x >= 0) & (x <= 1)).double()
    slope = inside * (torch.where(x >= EPS, 1 / x.clamp(min=EPS), torch.zeros_like(x)) + torch.where(1 - x >= EPS, 1 / (1 - x).clamp(min=EPS), torch.zeros_like(x)))
    sc["g_init_ref"] = sc["g_delta"][0, ..., :nd0] * slope
    sc["g_depth_map"] = s_map
    return sc, dict(raw=raw, slope=slope, passes=passes)


def anchor():
    """The dense hat-function form of the lookup's transpose is F.grid_sample's autograd in float64."""
    g = gen("anchor_head_tail")
    for H, W in ((5, 7), (1, 9), (6, 1)):
        P = 50
        c01 = torch.rand(P, 2, generator=g, dtype=F64)
        c01[0], c01[1] = torch.tensor([0.0, 1.0]), torch.tensor([1.0, 0.0])
        gp = torch.randn(P, generator=g, dtype=F64)
        m = torch.randn(1, 1, H, W, generator=g, dtype=F64).requires_grad_(True)
        out = F.grid_sample(m, ((c01 - 0.5) * 2).view(1, P, 1, 2), mode="bilinear", align_corners=True).view(P)
        out.backward(gp)
        hx, hy, _, _ = _hats(c01, H, W)
        assert float((out.detach() - ((hy @ m.detach()[0, 0]) * hx).sum(-1)).abs().max()) <= 1e-12 * float(m.detach().abs().max())
        assert float((m.grad[0, 0] - (hy * gp[:, None]).t() @ hx).abs().max()) <= 1e-12 * float(gp.abs().sum())


# ---- running the kernel ---------------------------------------------------------------------------------------------------------------------
def run(t, gc, gd, device, backend=None):
    """The kernels through the product's autograd function -> CPU tensors coord, depth, g_delta .. g_depth_map (zeros for an absent one)."""
    with kernels_on(backend) as ext:
        leaves = [t[k].to(device).clone().requires_grad_(True) for k in NAMES]
        coord, ave = ext.head_tail(leaves[0], leaves[1], t["inter"].to(device), leaves[2], leaves[3], leaves[4], t["img_h"].to(device), t["focal"].to(device))
        outs, gs = [o for o, g in ((coord, gc), (ave, gd)) if g is not None], [g.to(device) for g in (gc, gd) if g is not None]
        grads = torch.autograd.grad(outs, leaves, gs, allow_unused=True)
    out = dict(coord=coord.detach(), depth=ave.detach())
    for k, g, leaf in zip(NAMES, grads, leaves):
        assert g is not None and g.shape == leaf.shape and g.dtype == F32, k
        out["g_" + k] = g
    return {k: v.detach().cpu() for k, v in out.items()}


# ---- figures ---------------------------------------------------------------------------------------------------------------------------------
def _ratio(err, B):
    r = torch.where(B > 0, err / B, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
    r = torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)
    return float(r.max()) if r.numel() else 0.0


def within(tag, name, got, ref64, fw, scale, figs, failures):
    err32 = (fw.double() - ref64).abs()
    row = err32 if name == "g_depth_map" else err32.amax(-1, keepdim=True).expand_as(err32)
    B = torch.maximum(MARGIN * row, FLOOR * scale)
    err = (got.double() - ref64).abs()
    figs[name] = (_ratio(err, B), _ratio(err32, FLOOR * scale))
    bad = ~(err <= B)
    if bool(bad.any()):
        idx = tuple(int(i) for i in torch.nonzero(bad)[0])
        failures.append("%s %s: %d elements beyond the bound, worst err/B %.3g, first at %s: got %r, fp64 %r, B %.3g" % (
            tag, name, int(bad.sum()), figs[name][0], idx, float(got[idx]), float(ref64[idx]), float(B[idx])))


def _line(tag, figs):
    return "head_tail_case %s  err/B (fp32 framework err/floor):  " % tag + "  ".join("%s %.3f (%.3f)" % ((k,) + figs[k]) for k in figs)


# ---- cases --------------------------------------------------------------------------------------------------------------------------------------
class Case:
    pass


def _logit(p):
    return math.log(p / (1 - p))


@functools.lru_cache(maxsize=4)
def bounded_case(name, kind):
    L, B, Q, H, W, nd0 = SHAPES[name]
    g = gen("head_tail", name, kind)
    rn = lambda *s: torch.randn(*s, generator=g)                               # noqa: E731
    ru = lambda *s: torch.rand(*s, generator=g)                                # noqa: E731
    t = dict(delta=rn(L, B, Q, 6), init_ref=ru(B, Q, nd0), inter=ru(L - 1, B, Q, 6), size3d=ru(L, B, Q, 3) + 0.5, depth_reg=rn(L, B, Q, 2),
             depth_map=ru(B, H, W) * 50, img_h=torch.tensor([375.0, 370.0, 384.0][:B]), focal=torch.tensor([721.5, 707.0, 718.25][:B]))
    if kind == "saturated":
        t["delta"] = t["delta"] * 8
        sat = ru(L, B, Q, 6)
        t["delta"] = torch.where(sat < 0.05, torch.full_like(sat, -100.0), torch.where(sat > 0.95, torch.full_like(sat, 100.0), t["delta"]))
        t["depth_reg"][..., 0] = ru(L, B, Q) * 60 - 30
        t["size3d"] = 10.0 ** (ru(L, B, Q, 3) * 3 - 1)
    elif kind == "refs01":
        for key in ("init_ref", "inter"):
            u = ru(*t[key].shape)
            t[key] = torch.where(u < 0.2, torch.zeros_like(u), torch.where(u > 0.8, torch.ones_like(u), t[key]))
        u = ru(B, Q, nd0)
        t["init_ref"] = torch.where(u < 0.05, -0.3 * ru(B, Q, nd0) - 0.01, torch.where(u > 0.95, 1.01 + 0.4 * ru(B, Q, nd0), t["init_ref"]))
    elif kind == "tiny_boxes":                                                 # (t + b) img_h ~ 0.1: the clamp's flat side
        t["delta"][:, :, ::2, 4:] = -9.0 - ru(L, B, (Q + 1) // 2, 2)
        t["inter"][:, :, ::2, 4:] = 0.5
        if nd0 == 6:
            t["init_ref"][:, ::2, 4:] = 0.5
    elif kind == "borders":                                                    # centres on the four borders and the four corners
        code = torch.randint(0, 9, (L, B, Q), generator=g)                     # 3 x 3: x in {0, free, 1} x y in {0, free, 1}
        for k, cc in ((0, code % 3), (1, code // 3)):
            t["delta"][..., k] = torch.where(cc == 0, torch.full((L, B, Q), -100.0), torch.where(cc == 2, torch.full((L, B, Q), 100.0), t["delta"][..., k]))
    elif kind == "one_cell":                                                   # every centre of image 0 inside one bilinear footprint
        for k, size in ((0, W), (1, H)):
            p = (math.floor((size - 1) / 2) + 0.5) / (size - 1) if size > 2 else 0.5
            t["delta"][:, 0, :, k] = _logit(p) + 1e-3 * rn(L, Q)
            t["inter"][:, 0, :, k] = 0.5
            t["init_ref"][0, :, k] = 0.5
    elif kind == "zero_rows":
        t["depth_map"][:, ::2] = 0.0
    gc, gd = rn(L, B, Q, 6), rn(L, B, Q, 2)
    # keep raw = (c_4 + c_5) img_h away from the clamp's kink: an offender becomes a tiny box (fp64, from the inputs alone)
    for _ in range(4):
        r64 = _framework(t, F64, "cpu", gc, gd)
        raw = (r64["coord"][..., 4] + r64["coord"][..., 5]) * t["img_h"].double().view(1, -1, 1)
        near = (raw - 1).abs() <= FLOOR
        if not bool(near.any()):
            break
        t["delta"][..., 4:] = torch.where(near[..., None], torch.full_like(t["delta"][..., 4:], -9.0), t["delta"][..., 4:])
    else:
        raise PremiseError("%s/%s: (c_4 + c_5) img_h stays on the clamp's kink" % (name, kind))
    for key in ("init_ref", "inter"):
        x = t[key].double()
        if bool((((x - EPS).abs() <= FLOOR * EPS) | (((1 - x) - EPS).abs() <= FLOOR * EPS)).any()):
            raise PremiseError("%s/%s: a reference on the eps kink of inverse_sigmoid" % (name, kind))
    c = Case()
    c.name, c.kind, c.t, c.gc, c.gd, c.ref = name, kind, t, gc, gd, r64
    c.scale, c.aux = magnitudes(t, gc, gd, r64)
    coord = r64["coord"]
    if kind == "saturated" and L * B * Q >= 40 and not (bool((coord == 0).any() or (t["delta"] == -100).any()) and bool((coord == 1).any()) and float(t["depth_reg"][..., 0].abs().max()) > 25):
        raise PremiseError("saturated: no coordinate at exactly 0 / 1 or no depth_reg near +-30")
    if kind == "refs01" and B * Q * nd0 >= 40:
        x = t["init_ref"]
        if not (bool((x == 0).any()) and bool((x == 1).any()) and bool(((x < 0) | (x > 1)).any())):
            raise PremiseError("refs01: no reference at 0, at 1 or outside [0, 1]")
        at01 = (x == 0) | (x == 1)
        gz = r64["g_delta"][0, ..., :nd0][at01]                                # (autograd's log and divide round: 1 to 1e-12)
        if not bool((c.aux["slope"][at01] == 1).all()) or not bool(((r64["g_init_ref"][at01] - gz).abs() <= 1e-12 * gz.abs()).all()):
            raise PremiseError("refs01: autograd's derivative of inverse_sigmoid at 0 and 1 is not 1")
    if kind == "tiny_boxes" and not bool((c.aux["passes"] == 0).any()):
        raise PremiseError("tiny_boxes: nothing on the clamp's flat side")
    if kind == "borders" and L * B * Q >= 40:
        cx, cy = coord[..., 0], coord[..., 1]
        for want in ((0, 0), (0, 1), (1, 0), (1, 1)):
            if not bool(((cx.round() == want[0]) & ((cx - want[0]).abs() < 1e-30) & ((cy - want[1]).abs() < 1e-30)).any()):
                raise PremiseError("borders: no centre in the corner %s" % (want,))
    if kind == "one_cell":
        hx, hy, _, _ = _hats(coord[:, 0].reshape(-1, 6)[:, :2], H, W)
        if int(((hx > 0).any(0)).sum()) > 2 or int(((hy > 0).any(0)).sum()) > 2:
            raise PremiseError("one_cell: the centres of image 0 spread over more than one footprint")
    return c


def check_always(tag, t, got, failures, gd=None):
    if gd is not None and not torch.equal(got["g_depth_reg"][..., 1], gd[..., 1]):
        failures.append(tag + ": g_depth_reg[..., 1] is not g_depth[..., 1]")
    if not torch.equal(got["depth"][..., 1], t["depth_reg"][..., 1]):
        failures.append(tag + ": depth_ave[..., 1] is not depth_reg[..., 1]")
    if not bool((got["g_size3d"][..., 1:] == 0).all()):
        failures.append(tag + ": g_size3d[..., 1:] != 0")


def check_unused_and_repeat(tag, c, got, device, backend, failures):
    t, nd0 = c.t, c.t["init_ref"].shape[-1]
    again = run(t, c.gc, c.gd, device, backend)
    diff = {k: int((again[k] != got[k]).sum()) for k in got}
    only_c, only_d = run(t, c.gc, None, device, backend), run(t, None, c.gd, device, backend)
    zeros = dict(coord_only={k: int((only_c[k] != 0).sum()) for k in ("g_size3d", "g_depth_reg", "g_depth_map")},
                 depth_only={"g_delta[:4]": int((only_d["g_delta"][..., :4] != 0).sum()), "g_init_ref[:4]": int((only_d["g_init_ref"][..., :4] != 0).sum())})
    print("head_tail_case %s  second run differs in %s; nonzeros with one output unused: %s" % (tag, diff, zeros))
    if any(diff.values()):
        failures.append("%s: two runs differ: %s" % (tag, diff))
    if any(v for d in zeros.values() for v in d.values()):
        failures.append("%s: an unused output's gradients are not exact zeros: %s" % (tag, zeros))


def check_bounded(name, kind, device, backend=None, extras=True):
    c = bounded_case(name, kind)
    tag = "%s/%s" % (name, kind)
    fw = _framework(c.t, F32, device, c.gc, c.gd)
    got = run(c.t, c.gc, c.gd, device, backend)
    figs, failures = {}, []
    for k in ("coord", "depth") + tuple("g_" + n for n in NAMES):
        if not bool(torch.isfinite(got[k]).all()):
            failures.append("%s %s is not finite" % (tag, k))
        within(tag, k, got[k], c.ref[k], fw[k], c.scale[k], figs, failures)
    print(_line(tag, figs))
    check_always(tag, c.t, got, failures, c.gd)
    if extras:
        check_unused_and_repeat(tag, c, got, device, backend, failures)
    assert not failures, "\n".join(failures)
    return figs


# ---- exact ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def exact_case(name):
    L, B, Q, H, W, nd0 = EXACT_SHAPES[name]
    if not (H % 2 and W % 2 and B >= 2):
        raise PremiseError("exact: H and W odd, two images")
    g = gen("head_tail_exact", name)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()  # noqa: E731
    t = dict(delta=torch.zeros(L, B, Q, 6), init_ref=torch.full((B, Q, nd0), 0.5), inter=torch.full((L - 1, B, Q, 6), 0.5),
             size3d=ri(1, 4, L, B, Q, 3), depth_reg=torch.randn(L, B, Q, 2, generator=g), depth_map=ri(0, 50, B, H, W),
             img_h=torch.tensor([375.0] * (B - 1) + [1.0]), focal=torch.full((B,), 512.0))
    c = Case()
    c.name, c.kind, c.t = name, "exact", t
    c.gc, c.gd = ri(-8, 8, L, B, Q, 6), torch.stack((3 * ri(-8, 8, L, B, Q), ri(-8, 8, L, B, Q)), -1)
    c.ref = _framework(t, F64, "cpu", c.gc, c.gd)
    c.scale, c.aux = magnitudes(t, c.gc, c.gd, c.ref)
    if not (bool((c.ref["coord"] == 0.5).all()) and bool((c.aux["raw"][:, B - 1] == 1).all())):
        raise PremiseError("exact: coord != 0.5 or the last image is not on the clamp's tie")
    want = torch.zeros(B, H, W, dtype=F64)
    want[:, (H - 1) // 2, (W - 1) // 2] = (c.gd.double()[..., 0] / 3).sum((0, 2))
    if not torch.equal(c.ref["g_depth_map"], want) or float((c.gd.double()[..., 0].abs() / 3).sum((0, 2)).max()) >= 2 ** 24:
        raise PremiseError("exact: the fp64 map gradient is not the integer sum at the middle cell")
    tie = c.ref["g_delta"][:, B - 1]
    if not (torch.equal(tie.float().double(), tie) and bool((tie[..., 4] != c.gc.double()[:, B - 1, :, 4] * 0.25).any())):
        raise PremiseError("exact: the tie's g_delta is not exact in fp32, or the clamp passes no gradient in fp64")
    return c


def check_exact(name, device, backend=None, extras=True):
    c = exact_case(name)
    L, B, Q, H, W, nd0 = EXACT_SHAPES[name]
    tag = "%s/exact" % name
    fw = _framework(c.t, F32, device, c.gc, c.gd)
    got = run(c.t, c.gc, c.gd, device, backend)
    figs, failures = {}, []
    for k in ("coord", "depth") + tuple("g_" + n for n in NAMES):
        within(tag, k, got[k], c.ref[k], fw[k], c.scale[k], figs, failures)
    wrong = dict(coord=int((got["coord"] != 0.5).sum()), g_depth_map=int((got["g_depth_map"].double() != c.ref["g_depth_map"]).sum()),
                 g_delta_tie=int((got["g_delta"][:, B - 1].double() != c.ref["g_delta"][:, B - 1]).sum()))
    print(_line(tag, figs) + "  pairs per image %d, cells %d; elements that differ: %s" % (L * Q, H * W, wrong))
    check_always(tag, c.t, got, failures, c.gd)
    if extras:
        check_unused_and_repeat(tag, c, got, device, backend, failures)
    assert not failures, "\n".join(failures)
    assert_bits_equal(got["coord"], torch.full((L, B, Q, 6), 0.5), tag + " coord")
    assert_bits_equal(got["g_depth_map"], c.ref["g_depth_map"].float(), tag + " g_map")
    assert_bits_equal(got["g_delta"][:, B - 1], c.ref["g_delta"][:, B - 1].float(), tag + " g_delta on the clamp's tie")


# ---- box_refine -------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def refine_case(rows, nd):
    g = gen("box_refine", rows, nd)
    delta, ref = torch.randn(rows, 6, generator=g), torch.rand(rows, nd, generator=g)
    u, v = torch.rand(rows, 6, generator=g), torch.rand(rows, nd, generator=g)
    delta = torch.where(u < 0.1, delta * 8, torch.where(u < 0.13, torch.full_like(u, -100.0), torch.where(u > 0.97, torch.full_like(u, 100.0), delta)))
    ref = torch.where(v < 0.1, torch.zeros_like(v), torch.where(v > 0.9, torch.ones_like(v), torch.where((v > 0.45) & (v < 0.5), 1.3 * ref - 0.2, ref)))
    x = ref.double()
    if bool((((x - EPS).abs() <= FLOOR * EPS) | (((1 - x) - EPS).abs() <= FLOOR * EPS)).any()):
        raise PremiseError("box_refine: a reference on the eps kink of inverse_sigmoid")
    return delta, ref


def _refine_expression(delta, ref):
    nd = ref.shape[-1]
    return (delta + F.pad(inverse_sigmoid(ref), (0, 6 - nd))).sigmoid()


def check_refine(rows, nd, device, backend=None):
    delta, ref = refine_case(rows, nd)
    want = _refine_expression(delta.double(), ref.double())
    zabs = delta.double().abs() + F.pad(inverse_sigmoid(ref.double()), (0, 6 - nd)).abs()
    scale = want + zabs * want * (1 - want)
    fw = _refine_expression(delta.to(device), ref.to(device)).cpu()
    with kernels_on(backend) as ext:
        got = ext.box_refine(delta.to(device), ref.to(device)).cpu()
        again = ext.box_refine(delta.to(device), ref.to(device)).cpu()
    tag = "box_refine/rows%d/nd%d" % (rows, nd)
    figs, failures = {}, []
    assert got.shape == (rows, 6) and got.dtype == F32
    within(tag, "out", got, want, fw, scale, figs, failures)
    print(_line(tag, figs) + "  second run differs in %d" % int((again != got).sum()))
    assert not failures, "\n".join(failures)
    assert torch.equal(again, got)
