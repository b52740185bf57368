"""``Tester._detect`` and ``decode_helper.decode_batch`` around the detection decoder, under the emulated library: the device path is
taken only when asked for (``decode: device`` / MDETR_DETECT_DECODE=1) and only for outputs the kernel takes, it calls the entry
once per batch, and the result files it leads to are the host path's."""
import logging
import os

import numpy as np
import pytest
import torch

import detect_cases as D
import native_emul
from monodetr_amd import detect_ext
from monodetr_amd.helpers import tester_helper


class _Counting(object):
    """The emulated library with its detection entry counted."""

    def __init__(self, lib):
        self._lib, self.calls = lib, 0

    def mdetr_detect_decode(self, *args):
        self.calls += 1
        return self._lib.mdetr_detect_decode(*args)

    def __getattr__(self, name):
        return getattr(self._lib, name)


class _Raising(object):
    def __getattr__(self, name):
        raise AssertionError("the host path reached the detection library (%s)" % name)


@pytest.fixture
def counted(monkeypatch):
    monkeypatch.delenv("MDETR_DETECT_DECODE", raising=False)
    backend = _Counting(native_emul.lib())
    monkeypatch.setattr(detect_ext, "_backend", backend)
    return backend


def _tester(tmp_path, case, cfg, outputs=None):
    """A Tester whose model returns the case's head outputs and whose dataset serves its calibrations."""
    calibs = dict(zip(case.info['img_id'].tolist(), case.calibs))

    class _DS:
        max_objs, class_name, cls_mean_size = 50, ['Pedestrian', 'Car', 'Cyclist'], case.mean
        get_calib = staticmethod(lambda index: calibs[index])

    class _DL:
        dataset = _DS()

    class _Model:
        def __call__(self, inputs, calibs, targets, img_sizes, dn_args=0):
            return outputs if outputs is not None else case.outputs

    t = tester_helper.Tester(dict({'type': 'KITTI', 'topk': case.topk, 'threshold': D.THRESHOLD}, **cfg), _Model(), _DL(), logging.getLogger('t'),
               train_cfg={'save_path': str(tmp_path).lstrip('/')}, model_name='m')
    t.output_dir = str(tmp_path)
    batch = (torch.zeros(case.B, 3, 8, 8), torch.zeros(case.B, 3, 4), None, {k: torch.from_numpy(np.asarray(v)) for k, v in case.info.items()})
    return t, batch


def _files(tester, found, folder):
    tester.output_dir = folder
    tester.save_results(found)
    data = os.path.join(folder, 'outputs', 'data')
    return {name: open(os.path.join(data, name)).read().splitlines() for name in sorted(os.listdir(data))}


def test_decode_device_writes_the_host_paths_result_files(tmp_path, counted):
    case = D.value_case(D.GOLDEN_SHAPE)
    host, batch = _tester(tmp_path, case, {})
    device, _ = _tester(tmp_path, case, {'decode': 'device'})
    want, _ = host._detect(batch)
    assert counted.calls == 0
    got, _ = device._detect(batch)
    assert counted.calls == 1 and list(got) == list(want)
    a, b = _files(host, want, str(tmp_path / 'host')), _files(device, got, str(tmp_path / 'device'))
    assert list(a) == list(b) == ['000001.txt', '000004.txt']
    values = near_tie = 0
    for name, img_id in zip(a, want):
        assert len(a[name]) == len(b[name]) == len(want[img_id]) > 0
        for line_h, line_d, pred in zip(a[name], b[name], want[img_id]):
            th, td = line_h.split(' '), line_d.split(' ')
            assert th[:3] == td[:3] and len(th) == len(td) == 16
            for text_h, text_d, v in zip(th[3:], td[3:], pred[1:]):
                values += 1
                if abs(abs(v) * 100 % 1 - 0.5) < 1e-5 * 100:          # the host's figure within 1e-5 of a %.2f rounding tie: as numbers
                    near_tie += 1
                    assert abs(float(text_h) - float(text_d)) <= 0.01 + 1e-12
                else:
                    assert text_h == text_d, (name, line_h, line_d)
    print('%d values, %d within 1e-5 of a rounding tie' % (values, near_tie))
    assert values == 67 * 13 and near_tie <= values // 100 and near_tie == 0       # none on this fixture (the nearest is 1.1e-5 away)


def test_the_environment_variable_asks_for_the_device_path_too(tmp_path, counted, monkeypatch):
    case = D.value_case((3, 17, 3, 51))
    host, batch = _tester(tmp_path, case, {})
    want, _ = host._detect(batch)
    monkeypatch.setenv("MDETR_DETECT_DECODE", "1")
    got, _ = host._detect(batch)
    assert counted.calls == 1 and list(got) == list(want)
    for img_id in want:
        assert len(got[img_id]) == len(want[img_id]) and all(type(p[0]) is int for p in got[img_id])
        assert np.allclose(np.array(got[img_id]).reshape(-1, 14), np.array(want[img_id], dtype=np.float64).reshape(-1, 14), **D.TOL)
    monkeypatch.setenv("MDETR_DETECT_DECODE", "0")
    host._detect(batch)
    assert counted.calls == 1


def test_the_default_never_reaches_the_detection_library(tmp_path, monkeypatch):
    monkeypatch.delenv("MDETR_DETECT_DECODE", raising=False)
    monkeypatch.setattr(detect_ext, "_backend", _Raising())

    def refuse(*args, **kwargs):
        raise AssertionError("the host path reached detect_ext")
    monkeypatch.setattr(detect_ext, "supported", refuse)
    monkeypatch.setattr(detect_ext, "detect_decode", refuse)
    case = D.value_case(D.GOLDEN_SHAPE)
    for cfg in ({}, {'decode': 'host'}):
        tester, batch = _tester(tmp_path, case, cfg)
        found, _ = tester._detect(batch)
        gold = np.load(D.GOLD)
        for img_id, preds in found.items():
            assert np.allclose(np.array(preds, dtype=np.float64).reshape(-1, 14), gold['decode_img%d' % img_id], **D.TOL)


def test_bf16_and_over_limit_outputs_keep_the_host_path(tmp_path, counted):
    case = D.value_case(D.GOLDEN_SHAPE)
    bf16 = {k: v.bfloat16() for k, v in case.outputs.items()}
    g = torch.Generator().manual_seed(5)
    big = dict(D._other_heads(1, 2731, g), pred_logits=torch.randn(1, 2731, 3, generator=g))          # 8 193 keys
    big_case = D.Case('over_limit', big, case.calibs[:1], {k: v[:1] for k, v in case.info.items()}, case.mean, 50)
    for c, outputs in ((case, bf16), (big_case, big)):
        assert not detect_ext.supported(outputs)
        want, batch = _tester(tmp_path, c, {}, outputs)
        got, _ = _tester(tmp_path, c, {'decode': 'device'}, outputs)
        a, b = want._detect(batch)[0], got._detect(batch)[0]
        assert counted.calls == 0 and list(a) == list(b) and all(a[k] == b[k] and len(a[k]) > 0 for k in a)


def test_decode_batch_calls_the_entry_once_per_batch(counted):
    from monodetr_amd.helpers import decode_helper
    for shape in ((2, 550, 3, 50), (1, 64, 1, 64)):
        case, before = D.value_case(shape), counted.calls
        found = decode_helper.decode_batch(case.outputs, case.info, case.calibs, case.mean, D.THRESHOLD, case.topk)
        assert counted.calls == before + 1 and list(found) == case.info['img_id'].tolist()
        _, keep, _ = D.run_ext(case)
        assert [len(found[i]) for i in found] == keep.sum(1).tolist()
