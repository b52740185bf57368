"""Shared cases and comparators of the detection decoder's tests (csrc/detect.hip, ``mdetr_detect_decode``): the emulated CPU
suite and the GPU suite build the same problems and hold the kernel's three outputs to the same references.

Value cases lie on lattices, so that the expected answer does not hang on a rounding: the logits of an image are a permutation
of DISTINCT multiples of 2^-6 in [-6, 2] (2^-k with the smallest k >= 6 that yields Q C distinct values where an image has more
than 513 keys: 2^-8 for 1 650, 2^-10 for 8 192 -- still thousands of fp32 ulps of the sigmoid apart), the heading bin logits of a
query a permutation of distinct multiples of 2^-6, and every generated problem is checked here, on the CPU, before anything runs:

  * the sigmoid scores of an image are pairwise distinct in fp32 (torch.topk is then well defined and equals the order rule);
  * no score is within 1e-5 of the threshold;
  * the two largest heading logits of every selected query are at least 1e-3 apart;
  * every selected angle before a wrap (alpha, ry) is at least 1e-4 from +-pi.

A seed whose problem misses a property is skipped for the next one (deterministic).  The golden problem
(``kitti_synth_dets.decode_problem``) is not on a lattice and meets the same four checks.

Tie and edge cases test the order rule alone: their selection is held to ``torch.sort(logits, stable=True, descending=True)``."""
import ctypes
import functools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kitti_synth_dets                                                            # noqa: E402
from monodetr_amd.datasets.kitti.kitti_utils import Calibration                    # noqa: E402
from monodetr_amd.helpers import decode_helper                                     # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'kitti_eval.npz')
THRESHOLD = 0.2
TOL = dict(rtol=1e-6, atol=1e-6)                      # the bar of tests/test_kitti_eval_cpu.py for this path
HEADS = ('pred_logits', 'pred_boxes', 'pred_angle', 'pred_3d_dim', 'pred_depth')

# (B, Q, C, topk): fewer keys than lanes (twice); the golden problem; topk = Q C; 66 keys, one past a wave; C = 1; the training
# query count (1 650 keys: no power of two, more than a workgroup's threads); the limit
SHAPES = [(1, 1, 3, 1), (1, 1, 3, 3), (2, 50, 3, 50), (3, 17, 3, 51), (1, 22, 3, 50), (1, 64, 1, 64), (2, 550, 3, 50), (1, 2048, 4, 50)]
GOLDEN_SHAPE = (2, 50, 3, 50)
REFUSED = [(1, 2049, 4, 50), (1, 17, 3, 52)]           # Q C > 8192; topk > Q C
TIES = ['all_equal', 'straddle', 'zeros', 'infinities', 'one_nan', 'several_nan']

_KITTI_MEAN = np.array([[1.76255119, 0.66068622, 0.84422524], [1.52563191, 1.62856739, 3.88311640], [1.73698127, 0.59706367, 1.76282397]])
_P2 = np.array([[721.54, 0, 609.56, 44.857], [0, 721.54, 172.85, 0.2164], [0, 0, 1, 0.002746]], dtype=np.float32)


class Case(object):
    """outputs: the five heads (CPU fp32 tensors); calibs: one Calibration per image; info: img_id / img_size arrays; mean [C, 3] fp64"""

    def __init__(self, name, outputs, calibs, info, mean, topk):
        self.name, self.outputs, self.calibs, self.info, self.mean, self.topk = name, outputs, calibs, info, mean, topk
        self.B, self.Q, self.C = outputs['pred_logits'].shape
        self.calib6 = np.array([[float(v) for v in (c.cu, c.cv, c.fu, c.fv, c.tx, c.ty)] for c in calibs], dtype=np.float64).reshape(self.B, 6)
        self.size = np.asarray(info['img_size'], dtype=np.float64).reshape(self.B, 2)
        # the order rule's own reference: stable descending sort of the logits (NaN first, -0 == +0, ties by ascending index)
        self.order = torch.sort(outputs['pred_logits'].reshape(self.B, -1), dim=1, stable=True, descending=True)[1][:, :topk].numpy()

    def __repr__(self):
        return self.name


def _calib(p2):
    return Calibration({'P2': p2, 'R0': np.eye(3, dtype=np.float32), 'Tr_velo2cam': np.zeros((3, 4), dtype=np.float32)})


def _frames(B, rs):
    """B frames: KITTI-like projection matrices (fp32, as the calibration files hold them) and image sizes"""
    calibs, sizes = [], []
    for _ in range(B):
        p2 = _P2.copy()
        p2[0, 0] = p2[1, 1] = np.float32(721.54 + rs.uniform(-15, 15))
        p2[0, 2], p2[1, 2] = np.float32(609.56 + rs.uniform(-6, 6)), np.float32(172.85 + rs.uniform(-8, 8))
        p2[0, 3], p2[1, 3] = np.float32(44.857 + rs.uniform(-1, 1)), np.float32(0.2164 + rs.uniform(-0.5, 0.5))
        calibs.append(_calib(p2))
        sizes.append([1242 - rs.randint(0, 20), 375 - rs.randint(0, 6)])
    return calibs, {'img_id': np.arange(B) * 3 + 1, 'img_size': np.array(sizes)}


def _other_heads(B, Q, g):
    """boxes / angle / sizes / depth in the ranges of ``decode_problem``; the heading bin logits on the 2^-6 lattice"""
    boxes = torch.cat([torch.rand(B, Q, 2, generator=g) * 0.6 + 0.2, torch.rand(B, Q, 4, generator=g) * 0.08 + 0.01], -1)
    bins = torch.stack([torch.randperm(256, generator=g)[:12] for _ in range(B * Q)]).view(B, Q, 12).float() / 64 - 2
    angle = torch.cat([bins, torch.randn(B, Q, 12, generator=g) * 0.2], -1)
    depth = torch.cat([torch.rand(B, Q, 1, generator=g) * 50 + 3, torch.randn(B, Q, 1, generator=g)], -1)
    return {'pred_boxes': boxes, 'pred_angle': angle, 'pred_3d_dim': torch.rand(B, Q, 3, generator=g) * 2 + 1, 'pred_depth': depth}


def _lattice_logits(B, n, g):
    k = 6
    while 8 * 2 ** k + 1 < n:
        k += 1
    return torch.stack([torch.randperm(8 * 2 ** k + 1, generator=g)[:n] for _ in range(B)]).double().div(2 ** k).sub(6).float()


def check_properties(case):
    """-> None, or what the problem misses.  fp64 throughout, on the CPU."""
    lg = case.outputs['pred_logits'].reshape(case.B, -1)
    score32 = lg.sigmoid()
    for b in range(case.B):
        if len(np.unique(score32[b].numpy())) != lg.shape[1]:
            return 'equal fp32 scores'
        key = np.concatenate([case.outputs['pred_boxes'][b, :, :2].numpy(), case.outputs['pred_depth'][b, :, :1].numpy()], 1)
        if len(np.unique(key, axis=0)) != case.Q:
            return 'two queries share (cx, cy, depth): the tests tell queries apart by them'
    if (lg.double().sigmoid() - THRESHOLD).abs().min() < 1e-5:
        return 'a score within 1e-5 of the threshold'
    for b in range(case.B):
        q = case.order[b] // case.C
        ang = case.outputs['pred_angle'][b, q].double().numpy()
        top2 = np.sort(ang[:, :12], axis=1)[:, -2:]
        if (top2[:, 1] - top2[:, 0]).min() < 1e-3:
            return 'heading logits closer than 1e-3'
        cls = np.argmax(ang[:, :12], axis=1)
        alpha0 = cls * (2 * np.pi / 12) + ang[np.arange(len(q)), 12 + cls]
        alpha = np.where(alpha0 > np.pi, alpha0 - 2 * np.pi, alpha0)
        bx = case.outputs['pred_boxes'][b, q].double().numpy()
        x = ((bx[:, 0] - bx[:, 2]) + (bx[:, 0] + bx[:, 3])) / 2 * case.size[b, 0]
        ry0 = alpha + np.arctan2(x - case.calib6[b, 0], case.calib6[b, 2])
        if min(np.abs(np.abs(alpha0) - np.pi).min(), np.abs(np.abs(ry0) - np.pi).min()) < 1e-4:
            return 'an angle within 1e-4 of +-pi before its wrap'
    return None


@functools.lru_cache(maxsize=None)
def value_case(shape):
    """The value problem of one (B, Q, C, topk): built once, shared by every test, never written to."""
    B, Q, C, topk = shape
    if shape == GOLDEN_SHAPE:
        outputs, p2, info = kitti_synth_dets.decode_problem()
        case = Case('golden', outputs, [_calib(p) for p in p2], info, np.zeros((3, 3)), topk)
        assert check_properties(case) is None, check_properties(case)
        return case
    for seed in range(100 * (Q * C + topk), 100 * (Q * C + topk) + 50):
        g, rs = torch.Generator().manual_seed(seed), np.random.RandomState(seed)
        outputs = dict(_other_heads(B, Q, g), pred_logits=_lattice_logits(B, Q * C, g).view(B, Q, C))
        calibs, info = _frames(B, rs)
        mean = np.stack([_KITTI_MEAN[c % 3] * (1 + 0.25 * (c // 3)) for c in range(C)])                # non-zero: a wrong class lookup shows
        case = Case('B%d_Q%d_C%d_k%d' % shape, outputs, calibs, info, mean, topk)
        if check_properties(case) is None:
            return case
    raise AssertionError('no seed gives a %s problem with the four properties' % (shape,))


@functools.lru_cache(maxsize=None)
def tie_case(kind):
    """Order-rule problems: 24 queries x 3 classes (72 keys: more than a wave), top 20."""
    B, Q, C, topk = 2, 24, 3, 20
    g, rs = torch.Generator().manual_seed(7 + TIES.index(kind)), np.random.RandomState(7)
    n = Q * C
    if kind == 'all_equal':
        lg = torch.full((B, n), -0.5)
    elif kind == 'straddle':                                       # 6 distinct values, 12 of each: ranks 13 .. 24 share one value
        lg = torch.stack([(torch.arange(n) % 6)[torch.randperm(n, generator=g)] for _ in range(B)]).float() / 4 - 1
    elif kind == 'zeros':                                          # +0 and -0 interleaved above a negative rest: 30 zeros, 20 taken
        lg = torch.full((B, n), -1.0)
        for b in range(B):
            at = torch.randperm(n, generator=g)[:30]
            lg[b, at] = torch.where(torch.arange(30) % 2 == b, torch.tensor(-0.0), torch.tensor(0.0))
    else:
        lg = _lattice_logits(B, n, g)
        if kind == 'infinities':
            lg[:, 5], lg[:, 40], lg[:, 41], lg[0, 70] = float('inf'), float('-inf'), float('inf'), float('-inf')
        elif kind == 'one_nan':
            lg[0, 33], lg[1, 0] = float('nan'), float('nan')
        else:                                                      # several, of both signs and payloads
            bits = lg.view(torch.int32)
            bits[:, 9], bits[:, 2], bits[0, 71], bits[1, 50] = 0x7FC00000, -0x400000, 0x7F800001, -1      # +qNaN, -qNaN, +sNaN, all ones
    outputs = dict(_other_heads(B, Q, g), pred_logits=lg.view(B, Q, C).contiguous())
    calibs, info = _frames(B, rs)
    case = Case('tie_' + kind, outputs, calibs, info, _KITTI_MEAN.copy(), topk)
    if kind in ('one_nan', 'several_nan'):
        assert torch.isnan(lg.gather(1, torch.from_numpy(case.order)))[:, 0].all()          # the reference puts NaN first
    return case


# ---- running the entry ---------------------------------------------------------------------------------------------------------
def run_ext(case, device='cpu', want_dets37=True, threshold=THRESHOLD):
    """Through ``detect_ext.detect_decode`` (the product's wrapper) -> numpy (rows, keep, dets37)."""
    from monodetr_amd import detect_ext
    outputs = {k: v.to(device) for k, v in case.outputs.items()}
    found = detect_ext.detect_decode(outputs, case.calib6, case.size, case.mean, threshold, case.topk, want_dets37=want_dets37)
    assert found.rows.device == outputs['pred_logits'].device and found.rows.data_ptr() == found.packed.data_ptr()
    return found.rows.cpu().numpy(), found.keep.cpu().numpy(), (found.dets37.cpu().numpy() if found.dets37 is not None else None)


def run_raw(lib, case, device, want_dets37=True, threshold=THRESHOLD):
    """The C entry itself on host arrays (``device`` -1: the serial host form; under the emulated library any other ordinal runs the kernel)."""
    heads = [np.ascontiguousarray(case.outputs[k].numpy()) for k in HEADS]
    rows = np.full((case.B, case.topk, 14), np.nan)
    keep = np.full((case.B, case.topk), 7, dtype=np.uint8)
    dets = np.full((case.B, case.topk, 37), np.nan, dtype=np.float32) if want_dets37 else None
    mean = np.ascontiguousarray(case.mean, dtype=np.float64)
    rc = lib.mdetr_detect_decode(*[a.ctypes.data for a in heads], case.calib6.ctypes.data, case.size.ctypes.data, mean.ctypes.data, case.B, case.Q,
                                 case.C, case.topk, ctypes.c_double(threshold), rows.ctypes.data, keep.ctypes.data,
                                 dets.ctypes.data if dets is not None else None, device, None)
    assert rc == 0, lib.mdetr_last_error()
    assert set(np.unique(keep)) <= {0, 1}
    return rows, keep.astype(bool), dets


# ---- comparators ---------------------------------------------------------------------------------------------------------------
def selected_flat(case, dets37):
    """The flat indices q * C + c the records were taken from: the query is the one with the record's (cx, cy, depth) -- unique per
    image (check_properties) -- the class is column 0."""
    flat = np.empty((case.B, case.topk), dtype=np.int64)
    for b in range(case.B):
        key = np.concatenate([case.outputs['pred_boxes'][b, :, :2].numpy(), case.outputs['pred_depth'][b, :, :1].numpy()], 1)
        hit = (dets37[b][:, None, [34, 35, 6]] == key[None]).all(-1)
        assert (hit.sum(1) == 1).all(), 'a record matches no query or several'
        flat[b] = hit.argmax(1) * case.C + dets37[b, :, 0].astype(np.int64)
    return flat


def check_selection(case, dets37):
    assert np.array_equal(selected_flat(case, dets37), case.order)
    assert np.array_equal(dets37[:, :, 0], (case.order % case.C).astype(np.float32))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_record(case, dets37):
    """Columns 0, 2-35 bit for bit the framework path's (and the recorded reference's on the golden problem); score and sigma
    against fp64 sigmoid / exp of the selected inputs."""
    want = decode_helper.extract_dets_from_outputs(case.outputs, K=50, topk=case.topk).numpy()
    exact = [0] + list(range(2, 36))
    assert np.array_equal(_bits(dets37[:, :, exact]), _bits(want[:, :, exact]))
    order = torch.from_numpy(case.order)
    score = case.outputs['pred_logits'].reshape(case.B, -1).double().gather(1, order).sigmoid().numpy()
    sigma = torch.exp(-case.outputs['pred_depth'][:, :, 1].double()).gather(1, order // case.C).numpy()
    err = max(np.abs(dets37[:, :, 1] - score).max(), np.abs(dets37[:, :, 36] - sigma).max())
    print('%s: score / sigma max abs error vs fp64 %.3g' % (case, err))
    assert np.allclose(dets37[:, :, 1], score, **TOL) and np.allclose(dets37[:, :, 36], sigma, **TOL)
    if case.name == 'golden':
        gold = np.load(GOLD)['decode_dets']
        assert np.array_equal(_bits(dets37[:, :, exact]), _bits(gold[:, :, exact]))
        assert np.allclose(dets37, gold, **TOL)


def check_rows(case, rows, keep, dets37, threshold=THRESHOLD):
    """Rows and keep flags against ``decode_detections`` fed the kernel's own record (and the recorded results on the golden problem)."""
    assert np.array_equal(keep, dets37[:, :, 1] >= threshold)                      # numpy compares the fp32 column with the Python float in fp32
    want = decode_helper.decode_detections(dets37.copy(), case.info, case.calibs, case.mean, threshold)
    worst = 0.0
    for b in range(case.B):
        preds = np.array(want[case.info['img_id'][b]], dtype=np.float64).reshape(-1, 14)
        got = rows[b][keep[b]]
        assert got.shape == preds.shape, (got.shape, preds.shape)
        if len(got):
            worst = max(worst, np.abs(got - preds).max())
        assert np.allclose(got, preds, **TOL)
        if case.name == 'golden':
            gold = np.load(GOLD)['decode_img%d' % case.info['img_id'][b]]
            assert got.shape == gold.shape and np.allclose(got, gold, **TOL)
    print('%s: %d of %d rows kept, max abs difference from decode_detections %.3g' % (case, keep.sum(), keep.size, worst))
    return int(keep.sum())


def check_all(case, rows, keep, dets37):
    check_selection(case, dets37)
    if not case.name.startswith('tie_'):
        check_record(case, dets37)
    return check_rows(case, rows, keep, dets37)


def check_refused_and_empty(device):
    """Beyond the limits the entry refuses (the wrapper raises with its message); an empty batch is a success that writes nothing."""
    import pytest
    from monodetr_amd import detect_ext
    for B, Q, C, topk in REFUSED:
        outputs = {k: torch.zeros(B, Q, w, device=device) for k, w in zip(HEADS, (C, 6, 24, 3, 2))}
        assert detect_ext.supported(outputs) == (Q * C <= detect_ext.MAX_KEYS)
        with pytest.raises(RuntimeError, match=r"mdetr_detect_decode failed \(code -1\)"):
            detect_ext.detect_decode(outputs, np.ones((B, 6)), np.ones((B, 2)), np.zeros((C, 3)), THRESHOLD, topk)
    outputs = {k: torch.zeros(0, 5, w, device=device) for k, w in zip(HEADS, (3, 6, 24, 3, 2))}
    found = detect_ext.detect_decode(outputs, np.ones((0, 6)), np.ones((0, 2)), np.zeros((3, 3)), THRESHOLD, 4, want_dets37=True)
    assert found.rows.shape == (0, 4, 14) and found.keep.shape == (0, 4) and found.dets37 is None
