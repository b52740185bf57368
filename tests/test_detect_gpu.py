"""csrc/detect.hip on the device: the cases and comparators of tests/detect_cases.py (as tests/test_detect_emulated_cpu.py applies them
on the shim), the library's serial host form beside the kernel, and ``decode_batch`` against the host path it replaces."""
import numpy as np
import pytest
import torch

import detect_cases as D

pytestmark = pytest.mark.gpu
IDS = ["B%d_Q%d_C%d_k%d" % s for s in D.SHAPES]


def dev():
    return torch.device("cuda", 0)


@pytest.mark.parametrize("shape", D.SHAPES, ids=IDS)
def test_detect_selection_record_rows_and_keep_flags(shape):
    case = D.value_case(shape)
    rows, keep, dets37 = D.run_ext(case, dev())
    D.check_all(case, rows, keep, dets37)
    rows2, keep2, none = D.run_ext(case, dev(), want_dets37=False)
    assert none is None and np.array_equal(rows, rows2) and np.array_equal(keep, keep2)


@pytest.mark.parametrize("kind", D.TIES)
def test_detect_order_rule_on_ties_zeros_infinities_and_nan(kind):
    case = D.tie_case(kind)
    rows, keep, dets37 = D.run_ext(case, dev())
    D.check_all(case, rows, keep, dets37)
    nan = np.isnan(dets37[:, :, 1])
    assert nan.sum() == {'one_nan': 2, 'several_nan': 6}.get(kind, 0) and not keep[nan].any()
    assert nan[:, 0].all() or 'nan' not in kind


@pytest.mark.parametrize("name", IDS + D.TIES)
def test_detect_host_form_beside_the_kernel(name):
    """The library's device = -1 form (the host compiler's expf, a serial stable sort) meets the same references, selects the same
    pairs and keeps the same ranks as the kernel; all but the two expf columns of the record agree bit for bit."""
    from monodetr_amd import _capi
    case = D.tie_case(name) if name in D.TIES else D.value_case(D.SHAPES[IDS.index(name)])
    rows, keep, dets37 = D.run_raw(_capi.lib(), case, device=-1)
    D.check_all(case, rows, keep, dets37)
    krows, kkeep, kdets = D.run_ext(case, dev())
    exact = [0] + list(range(2, 36))
    assert np.array_equal(kkeep, keep) and np.array_equal(D._bits(kdets[:, :, exact]), D._bits(dets37[:, :, exact]))
    assert np.allclose(krows, rows, equal_nan=True, **D.TOL)


def test_detect_refused_shapes_and_the_empty_batch():
    D.check_refused_and_empty(dev())


def test_detect_decode_batch_equals_the_host_path_on_the_golden_problem():
    from monodetr_amd.helpers import decode_helper
    case = D.value_case(D.GOLDEN_SHAPE)
    outputs = {k: v.to(dev()) for k, v in case.outputs.items()}
    got = decode_helper.decode_batch(outputs, case.info, case.calibs, np.zeros((3, 3), dtype=np.float32), D.THRESHOLD, case.topk)
    dets = decode_helper.extract_dets_from_outputs(outputs, K=50, topk=case.topk)
    want = decode_helper.decode_detections(dets.cpu().numpy(), case.info, case.calibs, np.zeros((3, 3), dtype=np.float32), D.THRESHOLD)
    gold = np.load(D.GOLD)
    assert list(got) == list(want)
    for img_id in want:
        a, b = np.array(got[img_id]).reshape(-1, 14), np.array(want[img_id]).reshape(-1, 14)
        assert a.shape == b.shape == gold['decode_img%d' % img_id].shape and np.allclose(a, b, **D.TOL) and np.allclose(a, gold['decode_img%d' % img_id], **D.TOL)
        assert all(type(p[0]) is int for p in got[img_id])
