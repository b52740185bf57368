"""csrc/detect.hip -- the REAL kernel, launcher and C-ABI entry (mdetr_detect_decode) -- on the HIP-on-CPU shim, through
monodetr_amd/detect_ext.py.  Cases and comparators are in tests/detect_cases.py; tests/test_detect_gpu.py runs the same ones on the
device."""
import ctypes

import numpy as np
import pytest
import torch

import detect_cases as D
import native_emul
from monodetr_amd import detect_ext


@pytest.fixture(scope="module")
def emul():
    return native_emul.lib()


@pytest.fixture
def backend(emul, monkeypatch):
    monkeypatch.setattr(detect_ext, "_backend", emul)
    return emul


@pytest.mark.parametrize("shape", D.SHAPES, ids=lambda s: "B%d_Q%d_C%d_k%d" % s)
def test_selection_record_rows_and_keep_flags(backend, shape):
    case = D.value_case(shape)
    rows, keep, dets37 = D.run_ext(case)
    kept = D.check_all(case, rows, keep, dets37)
    if shape[3] >= 50 and 3 * shape[3] >= shape[1] * shape[2]:        # (a third of a lattice over [-6, 2] reaches below the threshold)
        assert 0 < kept < keep.size                                # the threshold splits the ranks: both sides of the flag are exercised
    # the record is optional, and leaving it out changes nothing else
    rows2, keep2, none = D.run_ext(case, want_dets37=False)
    assert none is None and np.array_equal(rows, rows2) and np.array_equal(keep, keep2)


@pytest.mark.parametrize("kind", D.TIES)
def test_order_rule_on_ties_zeros_infinities_and_nan(backend, kind):
    case = D.tie_case(kind)
    rows, keep, dets37 = D.run_ext(case)
    D.check_all(case, rows, keep, dets37)
    nan = np.isnan(dets37[:, :, 1])
    if 'nan' in kind:
        assert nan[:, 0].all() and nan.sum() == (2 if kind == 'one_nan' else 6) and not keep[nan].any()       # first, and never kept
    else:
        assert not nan.any()


@pytest.mark.parametrize("name", ["B%d_Q%d_C%d_k%d" % s for s in D.SHAPES] + D.TIES)
def test_host_form_equals_the_kernel_exactly(emul, name):
    case = D.tie_case(name) if name in D.TIES else D.value_case(D.SHAPES[["B%d_Q%d_C%d_k%d" % s for s in D.SHAPES].index(name)])
    kernel, host = D.run_raw(emul, case, device=0), D.run_raw(emul, case, device=-1)
    for a, b in zip(kernel, host):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))          # bytes: NaN rows included


def test_refused_shapes_and_the_empty_batch(backend):
    D.check_refused_and_empty('cpu')
    # B = 0 looks at no pointer
    assert backend.mdetr_detect_decode(*[None] * 8, 0, 5, 3, 4, ctypes.c_double(0.2), None, None, None, 0, None) == 0


def test_threshold_is_compared_in_fp32(backend):
    """numpy >= 2 compares the fp32 score column with the Python float in fp32: a score equal to float32(threshold) is kept even
    though it is below the double."""
    case = D.value_case((1, 22, 3, 50))
    _, _, dets37 = D.run_ext(case)
    score = float(dets37[0, 10, 1])                                # an fp32 value, exactly representable as a double
    above = float(np.nextafter(np.float32(score), np.float32(1)))
    for thr, want in ((score, True), (score + (above - score) / 4, True), (above, False)):       # the middle one rounds to `score` in fp32
        rows, keep, again = D.run_ext(case, threshold=thr)
        assert bool(keep[0, 10]) is want and np.array_equal(keep, again[:, :, 1] >= thr)


def test_wrapper_takes_non_contiguous_heads_and_constants_of_any_kind(backend):
    case = D.value_case((3, 17, 3, 51))
    want = D.run_ext(case)
    outputs = {k: torch.cat([v, v], -1)[..., :v.shape[-1]] for k, v in case.outputs.items()}
    assert not outputs['pred_boxes'].is_contiguous() and detect_ext.supported(outputs)
    found = detect_ext.detect_decode(outputs, torch.from_numpy(case.calib6), case.size.astype(np.int64), case.mean, D.THRESHOLD, case.topk,
                                     want_dets37=True)
    for a, b in zip(want, (found.rows.numpy(), found.keep.numpy(), found.dets37.numpy())):
        assert np.array_equal(a, b)
    assert not detect_ext.supported({k: v.bfloat16() for k, v in case.outputs.items()})
    assert not detect_ext.supported(dict(case.outputs, pred_angle=case.outputs['pred_angle'][:, :, :12]))
