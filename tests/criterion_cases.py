"""Cases, references and checks for the criterion kernels: the matched-pair losses (csrc/pair_losses.hip), the depth-map loss
(csrc/ddn_loss.hip) and the matching cost evaluated inside the solver (csrc/lsa.hip).  Test infrastructure: plain torch in fp64, no
kernel code; tests/test_criterion_cases_gpu.py runs the cases on the device, tests/test_criterion_cases_emulated_cpu.py through both
CPU stand-ins of tests/backends.py.

REFERENCES.  `pair_reference` evaluates the nine rows per level from an EXPLICIT assignment [L, B, G, K] (each case builds its own
valid partial matching, so no loss test depends on how the matcher breaks ties) and takes the gradients of the five prediction
tensors by autograd in fp64; `ddn_reference` does the same for the depth-map loss with num_bins = C - 1 as a parameter (box
painting with balancer.py's floor / ceil / Python-slice semantics, nearest object wins, LID bins, the +1e-6 one-hot, fg/bg weights).
Both are written in the cancellation-free forms (1 - sigmoid(x) = sigmoid(-x), 1 - p = -expm1(log p)), so that they stay references
where logits are +-30.  `anchor_pair` / `anchor_ddn` show once, on a benign case, that they are the project's own PyTorch
SetCriterion / DDNLoss (run in float64) to 1e-12 relative.

PREMISES, checked from the inputs and the fp64 reference before any kernel runs (`PremiseError`: a broken case, not a tolerance):
  * no two class logits of a row are closer than 1e-3 (class error and cardinality read an argmax);
  * every painted depth's fp64 bin index is at least 2^-11 from an integer;
  * every box corner gives the same floor / ceil in fp32 (the kernel's operation order) and fp64;
  * no predicted box corner or parameter of a matched pair equals its target's (torch splits the gradient of a min/max tie, the
    kernel does not: pair_losses_math.h).

WHAT IS ASSERTED.
Discrete results match the fp64 reference exactly: the number of correctly classified matched queries and the summed cardinality
difference behind `class_error` / `cardinality_error` (recovered from the fp32 value, which may differ from the reference by the
one or two fp32 roundings of 100 - 100 hits / n and sum / B: 2^-17 at magnitude 100 -- a count off by one moves the value by at
least 100 / 256); the exact zeros of a batch without targets; the box / dim / depth / angle gradients of unmatched rows (exact
zeros); the depth-map target bin of every pixel, read as the argmin of the pixel's gradient (the target class is the one logit the
loss pushes up; cases with benign logits only); foreground membership, read from the 13 : 1 ratio between a pixel's gradient
L1 norm and the fp64 reference's UNWEIGHTED one.
Loss values and gradients are compared against fp64, and the yardstick is the error of the project's fp32 PyTorch criterion on the
same inputs and device -- the path the kernels replace.  Per case and tensor, for the kernel and for fp32 PyTorch:
  (a) relative error of each loss entry;
  (b) max |g - g64| / max |g64| over the tensor;
  (c) the same per row (a query's entries; for the depth logits a pixel's C gradients), the row scale floored at 1e-6 x the
      tensor's scale (rows whose gradients all underflow have O(1) row-relative error in fp32 PyTorch too).
A figure's bound is max(8 x fp32 PyTorch's figure, 64 x 2^-24): 8 x because the device's native exp / log are a few ulp against
libm's one and block sums arrive by float atomics in arbitrary order; the floor because fp32 PyTorch is sometimes exact by luck.
For (a) of an entry summed from >= 1000 terms (loss_ce at B Q C >= 1000, the depth-map loss) the floor is 2^-20.  A reference entry
that is exactly 0 asks for an exact 0.  Measured figures: profiles/criterion_cases_measured.txt.  A figure above its bound is a
finding to be traced to its element, not a reason to widen the bound.
No bound is widened.  The figure closest to its bound, on the device and on both stand-ins alike, is (c) of the depth logits in
`saturated`: 4.55e-6 against fp32 PyTorch's 7.8e-7 (bound 6.2e-6).  Its element is the target class of background pixel (0, 5, 16),
p_t = 0.99255: g_t = a_t - p_t tail with tail ~ a_t cancels to 1 / 134 of its terms, and 1 - p_t itself carries 2^-24 / 0.0074 --
inherent to p held in fp32; the row is 5.7e-6 of the tensor's scale (absolute error 6e-13)."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

F32, F64 = torch.float32, torch.float64
ROWS = ("loss_ce", "loss_center", "loss_bbox", "loss_giou", "loss_depth", "loss_dim", "loss_angle", "class_error", "cardinality_error")
PRED_KEYS = ("pred_logits", "pred_boxes", "pred_3d_dim", "pred_depth", "pred_angle")
ALPHA = 0.25
FLOOR = 64.0 * 2.0 ** -24
FLOOR_LONG_SUM = 2.0 ** -20
MARGIN = 8.0
ROW_FLOOR = 1e-6


class PremiseError(AssertionError):
    """The inputs do not have the property the case was built for (a fault of the test, not of a kernel)."""


def gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * (int(k) if not isinstance(k, str) else sum(map(ord, k)))
                                             for i, k in enumerate(key)) % (2 ** 31))


# ---- figures -------------------------------------------------------------------------------------------------------------------------
def fig_a(got, ref):
    """worst relative error over loss entries; an exactly-zero reference entry asks for an exact zero (inf otherwise)."""
    got, ref = got.double().reshape(-1), ref.double().reshape(-1)
    worst = 0.0
    for x, r in zip(got.tolist(), ref.tolist()):
        e = (0.0 if x == 0.0 else math.inf) if r == 0.0 else abs(x - r) / abs(r)
        worst = max(worst, e if e == e else math.inf)
    return worst


def fig_bc(got, ref):
    """(b), (c) for a gradient tensor whose last dimension is the row."""
    got, ref = got.double(), ref.double()
    scale = float(ref.abs().max())
    err = (got - ref).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
    if scale == 0.0:
        z = 0.0 if bool((got == 0).all()) else math.inf
        return z, z
    rows = ref.abs().amax(-1).clamp(min=ROW_FLOOR * scale)
    return float(err.max()) / scale, float((err.amax(-1) / rows).max())


def bound(fig32, floor=FLOOR):
    return max(MARGIN * fig32, floor)


# ======================================================================================================================================
#  matched-pair losses
# ======================================================================================================================================
PAIR_CASES = {
    #  name              L  B  Q    G   K   C
    "single":           (1, 1, 1,   1,  1,  3),
    "short_rows":       (2, 5, 20,  1,  5,  3),    # a wave's 64 rows span four images: the cardinality ballot loop runs > 2 rounds
    "ragged":           (3, 3, 110, 11, 9,  3),    # B Q = 330: two blocks per level, the second ragged; K = 9: the second slot batch is clamped
    "full_slots":       (1, 2, 128, 2,  64, 3),    # K = 64, every slot valid, every query of the group matched
    "no_targets":       (2, 2, 22,  11, 4,  3),
    "one_empty_image":  (3, 4, 110, 11, 7,  3),
    "all_fg":           (1, 3, 66,  11, 5,  3),
    "all_bg":           (1, 3, 66,  11, 5,  3),
    "classes8":         (1, 2, 40,  1,  5,  8),    # kMaxClasses
    "saturated":        (2, 3, 66,  11, 9,  3),
    "boxes":            (1, 2, 66,  11, 9,  3),
}
GEOMETRIES = ("disjoint_x", "disjoint_y", "disjoint_xy", "nested", "containing", "tiny")


class PairCase:
    pass


def _separate_logits(x, g, mul):
    """resample the rows that hold two logits closer than 1e-3 (the argmax must not hang on the last bits)."""
    for _ in range(100):
        s = x.sort(-1).values
        bad = (s[..., 1:] - s[..., :-1]).amin(-1) < 2e-3 if x.shape[-1] > 1 else torch.zeros(x.shape[:-1], dtype=torch.bool)
        if not bool(bad.any()):
            return x
        x[bad] = torch.randn(int(bad.sum()), x.shape[-1], generator=g) * mul
    raise PremiseError("could not separate the class logits")


def _plant_geometry(name, tb, g):
    """a predicted (cx, cy, l, r, t, b) in the named relation to the target box `tb`; jittered, so that no coordinate ties."""
    j = lambda: float(torch.rand((), generator=g)) * 0.004 + 0.001           # noqa: E731
    cx, cy, l, r, t, b = (float(v) for v in tb)
    if name == "disjoint_x":
        return [cx + 0.5 + j(), cy + j(), 0.03 + j(), 0.04 + j(), 0.6 * t + j(), 0.7 * b + j()]
    if name == "disjoint_y":
        return [cx - j(), cy - 0.5 - j(), 0.6 * l + j(), 0.7 * r + j(), 0.03 + j(), 0.04 + j()]
    if name == "disjoint_xy":
        return [cx - 0.5 - j(), cy + 0.5 + j(), 0.03 + j(), 0.05 + j(), 0.02 + j(), 0.04 + j()]
    if name == "nested":
        return [cx + j(), cy - j(), 0.4 * l, 0.35 * r, 0.45 * t, 0.3 * b]
    if name == "containing":
        return [cx - j(), cy + j(), 1.7 * l, 1.6 * r, 1.8 * t, 1.5 * b]
    if name == "tiny":
        return [cx + j(), cy + j(), 5e-5, 5e-5, 5e-5, 5e-5]
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def pair_case(name):
    L, B, Q, G, K, C = PAIR_CASES[name]
    g = gen("pair", name)
    r = lambda *s: torch.rand(*s, generator=g)          # noqa: E731
    n_ = lambda *s: torch.randn(*s, generator=g)        # noqa: E731
    n = Q // G
    sat = name == "saturated"
    logit_mul = 12.0 if sat else 1.0
    logits = _separate_logits(n_(L, B, Q, C) * logit_mul, g, logit_mul)
    if name == "all_fg":
        logits[..., C - 1] = logits[..., :C - 1].amin(-1) - 1.0
    if name == "all_bg":
        logits[..., C - 1] = logits[..., :C - 1].amax(-1) + 1.0
    boxes = torch.cat((0.2 + 0.6 * r(L, B, Q, 2), 0.02 + 0.2 * r(L, B, Q, 4)), -1)
    if sat:
        boxes[..., 2:] = boxes[..., 2:] * r(L, B, Q, 4) ** 4                  # shrunk boxes
        far = r(L, B, Q) < 0.2                                                # some queries far from every target
        boxes[..., 0] = torch.where(far, boxes[..., 0] + 3.0, boxes[..., 0])
    angles = n_(L, B, Q, 24)
    if sat:
        angles[..., :12] *= 15.0
    preds = {
        "pred_logits": logits,
        "pred_boxes": boxes,
        "pred_3d_dim": 0.5 + 2.5 * r(L, B, Q, 3),
        "pred_depth": torch.cat((5 + 40 * r(L, B, Q, 1), (4.0 if sat else 1.0) * n_(L, B, Q, 1)), -1),
        "pred_angle": angles,
    }
    if name == "no_targets":
        num = torch.zeros(B, dtype=torch.int64)
    elif name == "full_slots":
        num = torch.full((B,), K, dtype=torch.int64)
    elif name == "single":
        num = torch.ones(B, dtype=torch.int64)
    else:
        num = torch.randint(1, K + 1, (B,), generator=g)
        num[0] = K
        if name == "one_empty_image":
            num[2] = 0
    gt = {
        "labels": torch.randint(0, C, (B, K), generator=g),
        "boxes": torch.cat((0.2 + 0.6 * r(B, K, 2), 0.05 + 0.2 * r(B, K, 2)), -1),
        "boxes_3d": torch.cat((0.3 + 0.4 * r(B, K, 2), 0.05 + 0.1 * r(B, K, 4)), -1),
        "depth": 5 + 40 * r(B, K),
        "size_3d": 0.8 + 2 * r(B, K, 3),
        "heading_bin": torch.randint(0, 12, (B, K), generator=g),
        "heading_res": 0.3 * n_(B, K),
        "valid": torch.arange(K)[None, :] < num[:, None],
        "num": num.to(torch.int32),
        "num_host": [int(v) for v in num],
    }
    # a valid partial matching per (level, image, group): distinct queries of the group for some of the valid slots; the slots
    # beyond num[b] hold stale query indices now and then (valid = 0 must keep them out)
    assign = torch.full((L, B, G, K), -1, dtype=torch.int64)
    for l in range(L):
        for b in range(B):
            for gi in range(G):
                perm = torch.randperm(n, generator=g) + gi * n
                k_all = int(num[b])
                m = min(k_all, n)
                slots = torch.randperm(k_all, generator=g)[:m] if k_all else torch.zeros(0, dtype=torch.int64)
                if name not in ("full_slots", "single", "boxes") and m > 1 and (l + b + gi) % 3 == 0:
                    slots = slots[:-1]                                        # leave a valid slot unmatched
                assign[l, b, gi, slots] = perm[:len(slots)]
                if k_all < K and len(slots) < n and (b + gi) % 2 == 0:
                    assign[l, b, gi, K - 1] = perm[len(slots)]                # a stale entry in a padded slot
    c = PairCase()
    if name == "boxes":
        c.geometry = {}
        for b in range(B):
            for gi in range(G):
                for k in range(K):
                    q = int(assign[0, b, gi, k])
                    if q >= 0 and bool(gt["valid"][b, k]):
                        geo = GEOMETRIES[(k + gi) % len(GEOMETRIES)]
                        preds["pred_boxes"][0, b, q] = torch.tensor(_plant_geometry(geo, gt["boxes_3d"][b, k], g))
                        c.geometry[geo] = c.geometry.get(geo, 0) + 1
    c.name, c.dims = name, (L, B, Q, G, K, C)
    c.preds, c.gt, c.assign = preds, gt, assign
    c.num_boxes = max(float(int(num.sum()) * G), 1.0)
    c.w = 0.5 + torch.arange(7 * L, dtype=F32).reshape(7, L) / (7.0 * L)     # upstream gradient of the seven weighted rows
    c.ref = pair_reference(preds, assign, gt, c.num_boxes, ALPHA, c.w)
    _pair_premises(c)
    return c


def _xyxy(b):
    cx, cy, l, r, t, bb = b.unbind(-1)
    return torch.stack((cx - l, cy - t, cx + r, cy + bb), -1)


def _matched(assign, gt):
    """index vectors (l, b, q, k) of the matched pairs."""
    ok = (assign >= 0) & gt["valid"][None, :, None, :]
    l, b, gi, k = ok.nonzero(as_tuple=True)
    return l, b, assign[l, b, gi, k], k


def pair_reference(preds, assign, gt, num_boxes, alpha, w):
    """The nine rows [9, L], the detached dimension factor [L], the gradients of sum(w * rows[:7]) w.r.t. the five prediction tensors,
    and the integer counts behind the two metric rows -- everything in fp64."""
    x, bx, dm, dp, an = (preds[k].double().clone().requires_grad_(True) for k in PRED_KEYS)
    L, B, Q, C = x.shape
    l, b, q, k = _matched(assign, gt)
    nb = float(num_boxes)
    # sigmoid focal, gamma = 2, summed over (image, query, class)
    t = torch.zeros(L, B, Q, C, dtype=F64)
    t[l, b, q, gt["labels"][b, k]] = 1.0
    ce = x.clamp(min=0) - x * t + torch.log1p(torch.exp(-x.abs()))
    one_minus_pt = torch.where(t > 0, torch.sigmoid(-x), torch.sigmoid(x))
    a_t = alpha * t + (1 - alpha) * (1 - t) if alpha >= 0 else torch.ones_like(t)
    rows = [(a_t * ce * one_minus_pt ** 2).flatten(1).sum(1) / nb]

    def per_level(v):                                                        # [pairs] -> [L]
        return torch.zeros(L, dtype=F64).index_add(0, l, v)

    pb, tb = bx[l, b, q], gt["boxes_3d"].double()[b, k]
    rows.append(per_level((pb[:, 0:2] - tb[:, 0:2]).abs().sum(-1)) / nb)
    rows.append(per_level((pb[:, 2:6] - tb[:, 2:6]).abs().sum(-1)) / nb)
    s, tt = _xyxy(pb), _xyxy(tb)
    iwh = (torch.min(s[:, 2:], tt[:, 2:]) - torch.max(s[:, :2], tt[:, :2])).clamp(min=0)
    inter = iwh[:, 0] * iwh[:, 1]
    union = (s[:, 2] - s[:, 0]) * (s[:, 3] - s[:, 1]) + (tt[:, 2] - tt[:, 0]) * (tt[:, 3] - tt[:, 1]) - inter
    hwh = (torch.max(s[:, 2:], tt[:, 2:]) - torch.min(s[:, :2], tt[:, :2])).clamp(min=0)
    hull = hwh[:, 0] * hwh[:, 1]
    rows.append(per_level(1 - (inter / union - (hull - union) / hull)) / nb)
    pd = dp[l, b, q]
    rows.append(per_level(1.4142 * torch.exp(-pd[:, 1]) * (pd[:, 0] - gt["depth"].double()[b, k]).abs() + pd[:, 1]) / nb)
    ts = gt["size_3d"].double()[b, k]
    diff = (dm[l, b, q] - ts).abs()
    s_rel, s_dim = per_level((diff / ts).sum(-1)), per_level(diff.sum(-1))
    comp = (s_dim / s_rel.clamp(min=1e-12)).detach()
    rows.append(s_rel * comp / nb)
    pa, hb = an[l, b, q], gt["heading_bin"][b, k]
    ang = torch.logsumexp(pa[:, :12], -1) - pa[:, :12].gather(-1, hb[:, None])[:, 0] \
        + (pa[:, 12:].gather(-1, hb[:, None])[:, 0] - gt["heading_res"].double()[b, k]).abs()
    rows.append(per_level(ang) / nb)
    weighted = torch.stack(rows)                                             # [7, L]
    (weighted * w.double()).sum().backward()
    with torch.no_grad():
        best = x.argmax(-1)                                                  # [L, B, Q]
        hits = torch.zeros(L, dtype=torch.int64).index_add(0, l, (best[l, b, q] == gt["labels"][b, k]).long())
        nmatch = torch.zeros(L, dtype=torch.int64).index_add(0, l, torch.ones_like(l))
        class_error = 100.0 - torch.where(nmatch > 0, hits.double() * 100.0 / nmatch.clamp(min=1).double(), torch.zeros(L, dtype=F64))
        card_diff = ((best != C - 1).sum(2) - gt["num"].long()[None]).abs().sum(1)            # [L]
        out = torch.cat((weighted.detach(), class_error[None], (card_diff.double() / B)[None]))
    matched_rows = torch.zeros(L, B, Q, dtype=torch.bool)
    matched_rows[l, b, q] = True
    grads = {key: (torch.zeros_like(v) if v.grad is None else v.grad) for key, v in zip(PRED_KEYS, (x, bx, dm, dp, an))}
    return dict(rows=out, comp=comp, grads=grads,
                hits=hits, nmatch=nmatch, card_diff=card_diff, matched_rows=matched_rows)


def _pair_premises(c):
    L, B, Q, G, K, C = c.dims
    x = c.preds["pred_logits"].double()
    if C > 1:
        s = x.sort(-1).values
        gap = float((s[..., 1:] - s[..., :-1]).amin())
        if gap < 1e-3:
            raise PremiseError("%s: two class logits of a row are %.2e apart" % (c.name, gap))
    # the assignment is a valid partial matching within each group
    n = Q // G
    for l in range(L):
        for b in range(B):
            for gi in range(G):
                a = c.assign[l, b, gi]
                a = a[(a >= 0) & c.gt["valid"][b]]
                if len(set(a.tolist())) != len(a) or (len(a) and (int(a.min()) < gi * n or int(a.max()) >= (gi + 1) * n)):
                    raise PremiseError("%s: not a matching within group %d" % (c.name, gi))
    l, b, q, k = _matched(c.assign, c.gt)
    pb, tb = c.preds["pred_boxes"][l, b, q], c.gt["boxes_3d"][b, k]
    if bool((pb == tb).any()) or bool((_xyxy(pb) == _xyxy(tb)).any()) or bool((_xyxy(pb.double()) == _xyxy(tb.double())).any()):
        raise PremiseError("%s: a predicted box coordinate equals its target's" % c.name)
    if c.name == "no_targets" and len(l):
        raise PremiseError("no_targets has pairs")
    if c.name == "full_slots" and not (len(l) == L * B * G * K and bool(c.ref["matched_rows"].all())):
        raise PremiseError("full_slots: not every slot / query is matched")
    if c.name == "all_fg" and not bool((x.argmax(-1) != C - 1).all()):
        raise PremiseError("all_fg")
    if c.name == "all_bg" and not bool((x.argmax(-1) == C - 1).all()):
        raise PremiseError("all_bg")
    if c.name == "boxes":
        if set(c.geometry) != set(GEOMETRIES):
            raise PremiseError("boxes: geometries planted: %s" % sorted(c.geometry))
        s, t = _xyxy(pb.double()), _xyxy(tb.double())
        iw, ih = torch.min(s[:, 2], t[:, 2]) - torch.max(s[:, 0], t[:, 0]), torch.min(s[:, 3], t[:, 3]) - torch.max(s[:, 1], t[:, 1])
        inside = (s[:, 0] > t[:, 0]) & (s[:, 1] > t[:, 1]) & (s[:, 2] < t[:, 2]) & (s[:, 3] < t[:, 3])
        around = (s[:, 0] < t[:, 0]) & (s[:, 1] < t[:, 1]) & (s[:, 2] > t[:, 2]) & (s[:, 3] > t[:, 3])
        for what, m in (("iw < 0 only", (iw < 0) & (ih >= 0)), ("ih < 0 only", (ih < 0) & (iw >= 0)), ("both < 0", (iw < 0) & (ih < 0)),
                        ("nested", inside), ("containing", around)):
            if not bool(m.any()):
                raise PremiseError("boxes: no pair with %s" % what)


def pair_torch(c, dtype, device):
    """The project's PyTorch SetCriterion on the case's explicit assignment: rows [9, L] and the five gradients."""
    from monodetr_amd.monodetr.monodetr import SetCriterion, _Pairs
    L, B, Q, G, K, C = c.dims
    crit = SetCriterion(C, None, {}, ALPHA, [], group_num=G)
    stacked = {k: v.to(device=device, dtype=dtype).clone().requires_grad_(True) for k, v in c.preds.items()}
    gt = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in c.gt.items()}
    gt = {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in gt.items()}
    pr = _Pairs(c.assign.to(device), gt)
    res = {}
    for loss in ("labels", "cardinality", "center", "boxes", "depths", "dims", "angles"):
        res.update(crit._get(loss, stacked, pr, c.num_boxes))
    rows = torch.stack([res[r].to(dtype) for r in ROWS])
    (rows[:7] * c.w.to(device=device, dtype=dtype)).sum().backward()
    zero = lambda v: torch.zeros_like(v) if v.grad is None else v.grad       # noqa: E731  (no pairs: a tensor may not be reached)
    return rows.detach().cpu(), {k: zero(v).cpu() for k, v in stacked.items()}


def pair_kernel(c, nb_form, device):
    """The fused kernels on the case: rows [9, L], comp [L], the five gradients (CPU tensors)."""
    from monodetr_amd.pair_losses_ext import _FusedPairLosses
    leaves = [c.preds[k].clone().to(device).requires_grad_(True) for k in PRED_KEYS]
    gt = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in c.gt.items()}
    nb = c.num_boxes if nb_form == "host" else torch.tensor(c.num_boxes, dtype=F32, device=device)
    out, comp = _FusedPairLosses.apply(*leaves, c.assign.to(device), gt, nb, ALPHA)
    (out[:7] * c.w.to(device)).sum().backward()
    return out.detach().cpu(), comp.detach().cpu(), {k: v.grad.cpu() for k, v in zip(PRED_KEYS, leaves)}


def anchor_pair(name="one_empty_image"):
    """`pair_reference` is the project's SetCriterion in float64 (values and gradients, 1e-12 relative)."""
    c = pair_case(name)
    rows, grads = pair_torch(c, F64, "cpu")
    ref = c.ref
    for i, r in enumerate(ROWS):
        # (the two metric rows are float32 in the criterion whatever the inputs' dtype: `count * 100.0 / n`, `.float()`)
        tol = 2.0 ** -17 if r in ("class_error", "cardinality_error") else 1e-12 * max(1.0, float(ref["rows"][i].abs().max()))
        assert (rows[i] - ref["rows"][i]).abs().max() <= tol, r
    for k in PRED_KEYS:
        assert float(ref["grads"][k].abs().max()) > 0
        assert (grads[k] - ref["grads"][k]).abs().max() <= 1e-12 * float(ref["grads"][k].abs().max()), k


def _pair_figures(rows, grads, ref):
    f = {}
    for i, r in enumerate(ROWS[:7]):
        f[r] = (fig_a(rows[i], ref["rows"][i]),)
    for k in PRED_KEYS:
        f[k] = fig_bc(grads[k], ref["grads"][k])
    return f


def _report(tag, fk, f32, bounds):
    for key in fk:
        print("criterion_case %s %s kernel %s torch32 %s bound %s" % (
            tag, key, "/".join("%.3e" % v for v in fk[key]), "/".join("%.3e" % v for v in f32[key]), "/".join("%.3e" % v for v in bounds[key])))


def check_pair(name, nb_form, device, backend="device"):
    """Run pair case `name` (num_boxes as a Python float: nb_form "host", or as a device tensor: "dev") and assert it."""
    c = pair_case(name)
    L, B, Q, G, K, C = c.dims
    ref = c.ref
    rows32, grads32 = pair_torch(c, F32, device)
    rows, comp, grads = pair_kernel(c, nb_form, device)
    fk, f32 = _pair_figures(rows, grads, ref), _pair_figures(rows32, grads32, ref)
    long_sum = B * Q * C >= 1000
    bounds = {key: tuple(bound(v, FLOOR_LONG_SUM if (key == "loss_ce" and long_sum) else FLOOR) for v in f32[key]) for key in fk}
    _report("pair/%s/%s/%s" % (name, nb_form, backend), fk, f32, bounds)
    # discrete results
    ce, card = rows[7].double(), rows[8].double()
    assert bool(torch.isfinite(rows).all()) and bool(torch.isfinite(comp).all())
    hits = torch.round((100.0 - ce) * ref["nmatch"].double() / 100.0).long()
    assert torch.equal(hits, ref["hits"]), ("class_error: hits", hits, ref["hits"])
    assert bool(((ce - ref["rows"][7]).abs() <= 2.0 ** -17).all()), ("class_error", ce, ref["rows"][7])
    assert torch.equal(torch.round(card * B).long(), ref["card_diff"]), ("cardinality", card * B, ref["card_diff"])
    assert bool(((card - ref["rows"][8]).abs() <= 2.0 ** -23 * ref["rows"][8].abs()).all()), ("cardinality", card, ref["rows"][8])
    un = ~ref["matched_rows"]
    for k in PRED_KEYS[1:]:
        assert bool((grads[k][un] == 0).all()), "%s: an unmatched row's gradient is not exactly 0" % k
    if name == "no_targets":
        assert bool((rows[1:7] == 0).all()) and bool((ce == 100.0).all()) and bool((rows[0] > 0).all())
    if name == "all_fg":
        assert torch.equal(ref["card_diff"], (Q - c.gt["num"].long()).abs().sum().expand(L))
    if name == "all_bg":
        assert torch.equal(ref["card_diff"], c.gt["num"].long().sum().expand(L))
    assert (comp.double() - ref["comp"]).abs().max() <= bound(0.0) * 4 * max(1.0, float(ref["comp"].abs().max()))
    # values and gradients
    for key in fk:
        for what, v, bnd in zip("a" if key in ROWS else "bc", fk[key], bounds[key]):
            assert v <= bnd, "%s (%s): %.3e > %.3e (fp32 PyTorch: %s)" % (key, what, v, bnd, f32[key])
    return rows, grads, fk, f32


def check_pair_sequence(device, backend="device"):
    """`ragged`, `short_rows`, `ragged` on the same self-cleaning workspace: (L, B) changes, so the carve-up of the workspace moves.
    Every run is checked against its own reference; the third equals the first (discrete rows exactly, losses within the bound)."""
    first = check_pair("ragged", "host", device, backend)
    check_pair("short_rows", "host", device, backend)
    third = check_pair("ragged", "host", device, backend)
    assert torch.equal(first[0][7:], third[0][7:])
    ref = pair_case("ragged").ref["rows"][:7]
    fk32 = first[3]
    for i, r in enumerate(ROWS[:7]):
        assert bool(((first[0][i].double() - third[0][i].double()).abs() <= 2 * bound(fk32[r][0], FLOOR_LONG_SUM if r == "loss_ce" else FLOOR) * ref[i].abs()).all()), r
    for k in ("pred_logits", "pred_boxes", "pred_depth", "pred_angle"):      # no sum enters these gradients: bit-identical
        assert torch.equal(first[1][k], third[1][k]), k


# ======================================================================================================================================
#  depth-map loss
# ======================================================================================================================================
DEPTH_MIN, DEPTH_MAX, FG_W, BG_W = 1e-3, 60.0, 13.0, 1.0
DDN_CASES = {
    #  name           B  C   H   W    K    layouts
    "tiny":          (1, 81, 5,  7,   1,   ("contiguous",)),
    "ragged_multi":  (3, 81, 24, 80,  6,   ("contiguous", "channels_last")),
    "c17":           (2, 17, 6,  20,  3,   ("contiguous",)),
    "c96":           (2, 96, 6,  20,  3,   ("contiguous",)),
    "c97":           (2, 97, 6,  20,  3,   ("contiguous", "channels_last")),
    "bins":          (1, 81, 2,  160, 160, ("contiguous",)),
    "range":         (1, 81, 2,  16,  8,   ("contiguous",)),
    "raster":        (2, 81, 24, 80,  10,  ("contiguous",)),
    "saturated":     (2, 81, 6,  20,  3,   ("contiguous", "channels_last")),
}
DDN_UPSTREAM = 1.7


class DdnCase:
    pass


def lid_depth(idx, nbins):
    """the depth whose LID bin index is `idx` (fp64)."""
    bs = 2 * (DEPTH_MAX - DEPTH_MIN) / (nbins * (1 + nbins))
    return DEPTH_MIN + bs * ((2 * idx + 1) ** 2 - 1) / 8


def lid_index(depth, nbins):
    bs = 2 * (DEPTH_MAX - DEPTH_MIN) / (nbins * (1 + nbins))
    return -0.5 + 0.5 * torch.sqrt(1 + 8 * (depth - DEPTH_MIN) / bs)


def _dyadic_boxes(g, B, K, W, H):
    """random (cx, cy, w, h) on multiples of 1/64: every product with W = 80 / H = 24 and every corner is exact in fp32."""
    q = lambda lo, hi: torch.randint(lo, hi + 1, (B, K), generator=g).float() / 64.0          # noqa: E731
    return torch.stack((q(0, 64), q(0, 64), q(3, 35), q(3, 35)), -1)


@functools.lru_cache(maxsize=None)
def ddn_case(name):
    B, C, H, W, K, layouts = DDN_CASES[name]
    g = gen("ddn", name)
    nb = C - 1
    logits = torch.randn(B, C, H, W, generator=g)
    valid = torch.ones(B, K, dtype=torch.bool)
    if name == "tiny":
        boxes = torch.tensor([[[0.5, 0.5, 0.5, 0.5]]])                         # 3.5 +- 1.75, 2.5 +- 1.25: columns 1..5, rows 1..3
        depth = torch.tensor([[21.3]])
    elif name in ("ragged_multi", "c17", "c96", "c97", "saturated"):
        boxes = _dyadic_boxes(g, B, K, W, H)
        depth = 2 + 55 * torch.rand(B, K, generator=g)
        depth[0, 0] = 75.0                                                     # beyond depth_max -> the extra bin
        num = torch.randint(1, K + 1, (B,), generator=g)
        num[0] = K
        valid = torch.arange(K)[None, :] < num[:, None]
        if name == "saturated":
            mul = torch.ones(B, 1, H, W)
            mul[:, :, :, 0::3] = 30.0
            mul[:, :, :, 1::3] = 8.0
            logits = logits * mul
            logits[:, 40, 2, :] += 60.0                                        # one class +60 along a row
    elif name == "bins":
        j = torch.arange(K)
        boxes = torch.stack(((j + 0.5) / W, torch.full((K,), 0.5), torch.full((K,), 0.5 / W), torch.full((K,), 0.5)), -1)[None].float()
        kk = (j // 2).double()
        idx = torch.where(j % 2 == 0, kk + 2.0 ** -10, kk + 1 - 2.0 ** -10)
        depth = lid_depth(idx, nb)[None].float()
        order = torch.randperm(K, generator=g)                                 # the slots in no particular order
        boxes, depth = boxes[:, order], depth[:, order]
    elif name == "range":
        j = torch.arange(K)
        boxes = torch.stack(((2 * j + 1) / W, torch.full((K,), 0.5), torch.full((K,), 1.5 / W), torch.full((K,), 0.5)), -1)[None].float()
        depth = torch.tensor([[0.0, 5e-4, 60.01, 75.0, math.inf, lid_depth(2.0 ** -10, nb), -3.0, 20.0]])
    elif name == "raster":
        f = lambda *v: [x / 64.0 for x in v]                                     # noqa: E731
        img0 = [f(8, 32, 8, 32),        # 0 corners exactly on integers: x 5..15, y 6..18
                f(2, 40, 20, 16),       # 1 sticks out on the left: x0 = -10 wraps to 70, the slice [70:15] is empty
                f(40, 2, 16, 20),       # 2 sticks out at the top: y0 = -3 wraps to 21, [21:5] is empty
                f(-6, 32, 4, 16),       # 3 wholly left of the image: [-10:-5] wraps to columns 70..74, rows 9..14
                f(60, 56, 24, 32),      # 4 beyond right and bottom: x 60..90, y 15..27, clipped at 80 / 24
                f(18, 32, 0, 16),       # 5 zero width at x = 22.5: floor 22, ceil 23 -- one column, rows 9..14
                f(30, 40, 12, 20),      # 6, 7 identical boxes (x 30..45, y 11.25..18.75), different depths
                f(30, 40, 12, 20),
                f(8, 32, 4, 16),        # 8 a nearer box inside box 0: x 7.5..12.5, y 9..15
                [0.0, 0.0, 0.0, 0.0]]   # 9 a padded slot: valid = 0, box zeroed as the caller does
        boxes = torch.zeros(B, K, 4)
        boxes[0] = torch.tensor(img0)
        depth = torch.ones(B, K)
        depth[0] = torch.tensor([30.0, 12.0, 14.0, 50.0, 41.0, 8.0, 35.0, 17.0, 10.0, 1.0])
        valid[0, 9] = False
        valid[1] = False                                                       # an image without objects
    else:
        raise KeyError(name)
    c = DdnCase()
    c.name, c.dims, c.layouts = name, (B, C, H, W, K), layouts
    c.logits, c.boxes, c.depth, c.valid = logits, boxes.float().contiguous(), depth.float().contiguous(), valid
    c.benign = name != "saturated"                                             # the target is the unique logit pushed up
    c.ref = ddn_reference(logits, c.boxes, c.depth, valid)
    _ddn_premises(c)
    return c


def _slice_bounds(lo, hi, n):
    start = torch.where(lo < 0, (lo + n).clamp(min=0), lo.clamp(max=n))
    stop = torch.where(hi < 0, (hi + n).clamp(min=0), hi.clamp(max=n))
    return start, stop


def _corners(boxes, H, W, dtype):
    """floor / ceil of the four corners in the kernel's operation order, evaluated in `dtype`."""
    b = boxes.to(dtype)
    cx, cy, hx, hy = b[..., 0] * W, b[..., 1] * H, 0.5 * (b[..., 2] * W), 0.5 * (b[..., 3] * H)
    return torch.floor(cx - hx).long(), torch.floor(cy - hy).long(), torch.ceil(cx + hx).long(), torch.ceil(cy + hy).long()


def ddn_reference(logits, boxes, depth, valid, alpha=ALPHA):
    """fp64: loss, d (DDN_UPSTREAM loss) / d logits, the per-pixel target bin, foreground mask and the gradient of the UNWEIGHTED
    per-pixel loss (from which a kernel's foreground weight is read back)."""
    B, C, H, W = logits.shape
    nbins = C - 1
    u1, v1, u2, v2 = _corners(boxes, H, W, F64)                                # [B, K]
    x0, x1 = _slice_bounds(u1, u2, W)
    y0, y1 = _slice_bounds(v1, v2, H)
    xs, ys = torch.arange(W).view(1, 1, 1, W), torch.arange(H).view(1, 1, H, 1)
    e = lambda t: t[:, :, None, None]                                          # noqa: E731
    cover = (xs >= e(x0)) & (xs < e(x1)) & (ys >= e(y0)) & (ys < e(y1)) & e(valid)            # [B, K, H, W]
    fg = cover.any(1)
    inf = torch.full((), math.inf, dtype=F64)
    nearest = torch.where(cover, e(depth.double()).expand_as(cover), inf).amin(1) if cover.shape[1] else torch.full((B, H, W), math.inf)
    d = torch.where(fg, nearest, torch.zeros((), dtype=F64))                   # unpainted pixels hold depth 0
    idx = lid_index(d, nbins)
    bad = ~(idx >= 0) | (idx > nbins) | ~torch.isfinite(idx)
    target = torch.where(bad, torch.full_like(idx, nbins), idx.floor()).long()
    z = logits.double().clone().requires_grad_(True)
    logp = F.log_softmax(z, 1)
    focal = -alpha * torch.expm1(logp) ** 2 * logp                             # (1 - p)^2 = expm1(log p)^2
    px = focal.gather(1, target[:, None])[:, 0] + 1e-6 * focal.sum(1)
    weights = torch.where(fg, FG_W, BG_W).double()
    loss = (px * weights).sum() / (B * H * W)
    (gw,) = torch.autograd.grad(loss * DDN_UPSTREAM, z, retain_graph=True)
    (g1,) = torch.autograd.grad(px.sum() * DDN_UPSTREAM / (B * H * W), z)
    return dict(loss=loss.detach(), grad=gw, grad_unweighted=g1, target=target, fg=fg, idx=idx, painted=torch.where(fg, nearest, inf))


def _ddn_premises(c):
    B, C, H, W, K = c.dims
    for a, b in zip(_corners(c.boxes, H, W, F32), _corners(c.boxes, H, W, F64)):
        if not torch.equal(a[c.valid], b[c.valid]):
            raise PremiseError("%s: a box corner rounds differently in fp32 and fp64" % c.name)
    idx = c.ref["idx"]
    idx = idx[torch.isfinite(idx)]
    off = float((idx - idx.round()).abs().min())
    if off < 2.0 ** -11:
        raise PremiseError("%s: a bin index is %.2e from an integer" % (c.name, off))
    t, fg = c.ref["target"], c.ref["fg"]
    if c.name == "bins":
        col = t[0, 0]
        if not (torch.equal(col, torch.arange(W) // 2) and torch.equal(t[0, 1], col) and bool(fg.all())):
            raise PremiseError("bins: column j is not in bin j // 2")
    if c.name == "range":
        want = torch.tensor([80, 80, 80, 80, 80, 0, 80, -1]).repeat_interleave(2)
        if not (bool(((t[0, 0] == want) | (want < 0)).all()) and bool(fg.all()) and 0 < int(t[0, 0, 15]) < 80):
            raise PremiseError("range: bins are %s" % t[0, 0].tolist())
    if c.name == "raster":
        want = torch.zeros(H, W, dtype=torch.bool)
        for (xa, xb, ya, yb) in ((5, 15, 6, 18), (70, 75, 9, 15), (60, 80, 15, 24), (22, 23, 9, 15), (30, 45, 11, 19), (7, 13, 9, 15)):
            want[ya:yb, xa:xb] = True
        if not (torch.equal(fg[0], want) and not bool(fg[1].any())):
            raise PremiseError("raster: the painted pixels are not the expected rectangles")
        near = lid_index(torch.tensor([10.0, 17.0, 8.0], dtype=F64), C - 1).floor().long()
        if not (int(t[0, 12, 10]) == int(near[0]) and int(t[0, 12, 40]) == int(near[1]) and int(t[0, 12, 22]) == int(near[2])):
            raise PremiseError("raster: nearest object does not win")
    if c.name in ("ragged_multi", "c17", "c96", "c97", "saturated") and not (bool(fg.any()) and bool((~fg).any()) and bool((t[fg] == C - 1).any())):
        raise PremiseError("%s: no foreground, no background or no out-of-range depth" % c.name)


def _layout(t, layout):
    return t.contiguous(memory_format=torch.channels_last) if layout == "channels_last" else t.contiguous()


def ddn_torch(c, dtype, device, layout="contiguous"):
    """The project's PyTorch DDNLoss (its painting, binning with num_bins = C - 1, focal loss and balancer): loss and gradient."""
    from monodetr_amd.monodetr.depth_predictor.ddn_loss import DDNLoss
    from monodetr_amd.utils import box_ops
    B, C, H, W, K = c.dims
    mod = DDNLoss(alpha=ALPHA, fg_weight=FG_W, bg_weight=BG_W)
    z = _layout(c.logits.to(device=device, dtype=dtype), layout).clone().requires_grad_(True)
    b, valid = c.boxes.to(device=device, dtype=dtype), c.valid.to(device)
    xyxy = box_ops.box_cxcywh_to_xyxy(torch.stack((b[..., 0] * W, b[..., 1] * H, b[..., 2] * W, b[..., 3] * H), -1))
    xyxy = torch.where(valid[..., None], xyxy, torch.zeros_like(xyxy)).reshape(-1, 4)
    depth = c.depth.to(device=device, dtype=dtype).reshape(-1)
    target = mod.bin_depths(mod.build_target_depth_from_3dcenter(z, xyxy, depth, K, valid.reshape(-1)),
                            depth_min=DEPTH_MIN, depth_max=DEPTH_MAX, num_bins=C - 1, target=True)
    loss = mod.balancer(loss=mod.loss_func(z, target), gt_boxes2d=xyxy, num_gt_per_img=K)
    (loss * DDN_UPSTREAM).backward()
    return loss.detach().cpu(), z.grad.cpu()


def ddn_kernel(c, device, layout):
    from monodetr_amd.ddn_loss_ext import fused_ddn_loss
    z = _layout(c.logits.to(device), layout).clone().requires_grad_(True)
    loss = fused_ddn_loss(z, c.boxes.to(device), c.depth.to(device), c.valid.to(device), ALPHA, FG_W, BG_W, DEPTH_MIN, DEPTH_MAX)
    (loss * DDN_UPSTREAM).backward()
    assert z.grad.stride() == z.stride()
    return loss.detach().cpu(), z.grad.cpu()


def anchor_ddn(name="ragged_multi"):
    """`ddn_reference` is the project's DDNLoss.forward in float64 (C = 81: the module hard-codes 80 bins)."""
    from monodetr_amd.monodetr.depth_predictor.ddn_loss import DDNLoss
    from monodetr_amd.utils import box_ops
    c = ddn_case(name)
    B, C, H, W, K = c.dims
    assert C == 81
    z = c.logits.double().clone().requires_grad_(True)
    b = c.boxes.double()
    xyxy = box_ops.box_cxcywh_to_xyxy(torch.stack((b[..., 0] * W, b[..., 1] * H, b[..., 2] * W, b[..., 3] * H), -1))
    xyxy = torch.where(c.valid[..., None], xyxy, torch.zeros_like(xyxy))
    loss = DDNLoss(alpha=ALPHA, fg_weight=FG_W, bg_weight=BG_W)(z, xyxy.reshape(-1, 4), K, c.depth.double().reshape(-1), valid=c.valid.reshape(-1))
    (loss * DDN_UPSTREAM).backward()
    assert abs(float(loss) - float(c.ref["loss"])) <= 1e-12 * abs(float(c.ref["loss"]))
    assert (z.grad - c.ref["grad"]).abs().max() <= 1e-12 * float(c.ref["grad"].abs().max())


def _ddn_figures(loss, grad, ref):
    rows = lambda t: t.permute(0, 2, 3, 1)                                     # noqa: E731  a pixel's C gradients are a row
    return {"loss_depth_map": (fig_a(loss, ref["loss"]),), "depth_logits": fig_bc(rows(grad), rows(ref["grad"]))}


def check_ddn(name, device, layout="contiguous", backend="device"):
    """Run depth-map case `name` twice in a row (the second call runs on the workspace the first left behind) and assert it."""
    c = ddn_case(name)
    B, C, H, W, K = c.dims
    ref = c.ref
    f32 = _ddn_figures(*ddn_torch(c, F32, device, layout), ref)
    bounds = {"loss_depth_map": (bound(f32["loss_depth_map"][0], FLOOR_LONG_SUM if B * H * W * C >= 1000 else FLOOR),),
              "depth_logits": tuple(bound(v) for v in f32["depth_logits"])}
    out = None
    for rep in range(2):
        loss, grad = ddn_kernel(c, device, layout)
        fk = _ddn_figures(loss, grad, ref)
        _report("ddn/%s/%s/%s/run%d" % (name, layout, backend, rep), fk, f32, bounds)
        assert bool(torch.isfinite(grad).all()) and bool(torch.isfinite(loss))
        g = grad.double()
        if c.benign:                                                           # the target bin: the one logit the loss pushes up
            assert torch.equal(g.argmin(1), ref["target"]), "target bins differ in %d pixels" % int((g.argmin(1) != ref["target"]).sum())
        # foreground membership from the 13 : 1 ratio of the pixel's gradient L1 norm to the reference's unweighted one
        ratio = g.abs().sum(1) / ref["grad_unweighted"].abs().sum(1)
        assert torch.equal(ratio > math.sqrt(FG_W * BG_W), ref["fg"]), "foreground membership differs"
        if c.benign:
            assert bool(((ratio / torch.where(ref["fg"], FG_W, BG_W) - 1).abs() < 1e-2).all())
        for key in fk:
            for what, v, bnd in zip("a" if key == "loss_depth_map" else "bc", fk[key], bounds[key]):
                assert v <= bnd, "%s (%s) run %d: %.3e > %.3e (fp32 PyTorch: %s)" % (key, what, rep, v, bnd, f32[key])
        out = (fk, f32)
    return out


# ======================================================================================================================================
#  matching cost inside the solver
# ======================================================================================================================================
COST_CASES = ("square64", "boxes")
COST_WEIGHTS = (2.0, 5.0, 10.0, 2.0)                                          # class, bbox, 3dcenter, giou (the shipped configuration)


@functools.lru_cache(maxsize=None)
def cost_case(name):
    """(logits [L,B,Q,C], boxes [L,B,Q,6], gt, G).  Logits stay within +-8: beyond that 1 - p + 1e-8 evaluates materially differently
    in fp32 and fp64, the fp32 value is the reference's own semantics, and an fp64 cost is no oracle."""
    if name == "square64":                                                     # n = K = 64 per group, every slot valid
        L, B, G, n, K, C = 1, 2, 2, 64, 64, 3
        g = gen("cost", name)
        r = lambda *s: torch.rand(*s, generator=g)                             # noqa: E731
        logits = (torch.randn(L, B, G * n, C, generator=g) * 2.5).clamp(-8, 8)
        boxes = torch.cat((0.2 + 0.6 * r(L, B, G * n, 2), 0.02 + 0.2 * r(L, B, G * n, 4)), -1)
        num = torch.full((B,), K, dtype=torch.int64)
        gt = {"labels": torch.randint(0, C, (B, K), generator=g),
              "boxes_3d": torch.cat((0.2 + 0.6 * r(B, K, 2), 0.02 + 0.2 * r(B, K, 4)), -1)}
    else:                                                                      # the `boxes` geometries as predictions, one group of
        c = pair_case("boxes")                                                 # 66 queries (K = 9 slots need n >= 9)
        logits, boxes, G = c.preds["pred_logits"], c.preds["pred_boxes"], 1
        gt = {"labels": c.gt["labels"], "boxes_3d": c.gt["boxes_3d"]}
        num = c.gt["num"].long()
        K = gt["labels"].shape[1]
    gt["valid"] = torch.arange(K)[None, :] < num[:, None]
    gt["num"] = num.to(torch.int32)
    if float(logits.abs().max()) > 8.0:
        raise PremiseError("%s: logits beyond +-8" % name)
    return logits, boxes, gt, G


def check_cost(name, device, backend="device"):
    """The assignment of lsa.hip with the fused cost has the optimal total cost of scipy on the fp64 cost matrix (1e-5 relative), is a
    set of distinct queries of its group, and leaves the padded slots at -1."""
    from scipy.optimize import linear_sum_assignment
    from monodetr_amd.lsa_ext import batched_assignment_fused
    from monodetr_amd.monodetr.matcher import HungarianMatcher
    logits, boxes, gt, G = cost_case(name)
    m = HungarianMatcher(*COST_WEIGHTS[:1], cost_bbox=COST_WEIGHTS[1], cost_3dcenter=COST_WEIGHTS[2], cost_giou=COST_WEIGHTS[3])
    cost = m.cost_padded(logits.double(), boxes.double(), {k: (v.double() if v.is_floating_point() else v) for k, v in gt.items()}).numpy()
    gtd = {k: v.to(device) for k, v in gt.items()}
    got = batched_assignment_fused(logits.to(device), boxes.to(device), gtd, G,
                                   (m.cost_class, m.cost_bbox, m.cost_3dcenter, m.cost_giou)).cpu().numpy()
    L, B, Q, _ = logits.shape
    n = Q // G
    worst = 0.0
    for l in range(L):
        for b in range(B):
            k = int(gt["num"][b])
            for gi in range(G):
                a = got[l, b, gi]
                assert (a[k:] == -1).all()
                if k == 0:
                    continue
                sub = cost[l, b, gi * n:(gi + 1) * n, :k]
                r, cidx = linear_sum_assignment(sub)
                mine = a[:k] - gi * n
                assert len(set(mine.tolist())) == k and mine.min() >= 0 and mine.max() < n
                ref_total, my_total = sub[r, cidx].sum(), sub[mine, np.arange(k)].sum()
                worst = max(worst, abs(ref_total - my_total) / max(1.0, abs(ref_total)))
    print("criterion_case cost/%s/%s total-cost excess %.3e (bound 1e-5)" % (name, backend, worst))
    assert worst <= 1e-5
