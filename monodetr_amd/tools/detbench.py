"""Timing of the tester's tail -- head outputs on the device -> finished ``{img_id: detections}`` dict on the host -- on its two paths:

    host     decode_helper.extract_dets_from_outputs + .cpu().numpy() + decode_helper.decode_detections   (the default)
    device   decode_helper.decode_batch: one launch of csrc/detect.hip, one copy                           (``tester.decode: device``)

    python -m monodetr_amd.tools.detbench [--batch 8] [--queries 50,550] [--repeats 7] [--inner 50] [--out FILE]

Synthetic head outputs (seeded; per image about half of the ``topk`` selected rows above the score threshold), KITTI calibrations.
One sample is the host-clock time of ``inner`` consecutive tails divided by ``inner``; each tail ends with its results on the host, so
nothing is left in flight.  The two paths alternate sample by sample in one process; reported: the median of ``repeats`` samples with
[min, max], in microseconds per batch.  Before timing, the two paths' results are compared (same rows kept, values within 1e-6)."""
import argparse
import json
import math
import statistics
import time

import numpy as np
import torch

from monodetr_amd.datasets.kitti.kitti_utils import Calibration
from monodetr_amd.helpers import decode_helper

THRESHOLD, TOPK, CLASSES = 0.2, 50, 3
MEAN_SIZE = np.array([[1.76255119, 0.66068622, 0.84422524], [1.52563191, 1.62856739, 3.88311640], [1.73698127, 0.59706367, 1.76282397]])


def make_batch(B, Q, device, seed=0):
    g = torch.Generator().manual_seed(seed)
    lg = torch.randn(B, Q * CLASSES, generator=g) * 1.5
    cut = lg.topk(TOPK // 2 + 1, dim=1)[0][:, -2:].mean(1, keepdim=True)                 # between ranks 25 and 26
    logits = (lg - cut + math.log(THRESHOLD / (1 - THRESHOLD))).view(B, Q, CLASSES)
    boxes = torch.cat([torch.rand(B, Q, 2, generator=g) * 0.6 + 0.2, torch.rand(B, Q, 4, generator=g) * 0.08 + 0.01], -1)
    depth = torch.cat([torch.rand(B, Q, 1, generator=g) * 50 + 3, torch.randn(B, Q, 1, generator=g)], -1)
    outputs = {'pred_logits': logits, 'pred_boxes': boxes, 'pred_angle': torch.randn(B, Q, 24, generator=g),
               'pred_3d_dim': torch.rand(B, Q, 3, generator=g) * 2 + 1, 'pred_depth': depth}
    p2 = np.array([[721.54, 0, 609.56, 44.857], [0, 721.54, 172.85, 0.2164], [0, 0, 1, 0.002746]], dtype=np.float32)
    calibs = [Calibration({'P2': p2, 'R0': np.eye(3, dtype=np.float32), 'Tr_velo2cam': np.zeros((3, 4), dtype=np.float32)}) for _ in range(B)]
    info = {'img_id': np.arange(B), 'img_size': np.array([[1242, 375]] * B)}
    return {k: v.to(device) for k, v in outputs.items()}, calibs, info


def host_tail(outputs, calibs, info):
    dets = decode_helper.extract_dets_from_outputs(outputs=outputs, K=50, topk=TOPK)
    return decode_helper.decode_detections(dets=dets.detach().float().cpu().numpy(), info=info, calibs=calibs, cls_mean_size=MEAN_SIZE, threshold=THRESHOLD)


def device_tail(outputs, calibs, info):
    return decode_helper.decode_batch(outputs=outputs, info=info, calibs=calibs, cls_mean_size=MEAN_SIZE, threshold=THRESHOLD, topk=TOPK)


def sample(fn, args, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn(*args)
    return (time.perf_counter() - t0) / inner * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--queries", default="50,550")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("detbench: no GPU -- a timing taken anywhere else says nothing about this path")
    assert a.repeats >= 3
    device = torch.device("cuda", 0)
    result = {"batch": a.batch, "classes": CLASSES, "topk": TOPK, "threshold": THRESHOLD, "repeats": a.repeats, "inner": a.inner, "unit": "us per batch",
              "gpu": torch.cuda.get_device_name(0), "configs": []}
    for Q in (int(q) for q in a.queries.split(",")):
        args = make_batch(a.batch, Q, device)
        want, got = host_tail(*args), device_tail(*args)
        kept = sum(len(v) for v in want.values())
        assert list(want) == list(got) and all(len(want[k]) == len(got[k]) for k in want)
        assert all(np.allclose(np.array(got[k]).reshape(-1, 14), np.array(want[k], dtype=np.float64).reshape(-1, 14), rtol=1e-6, atol=1e-6) for k in want)
        for fn in (host_tail, device_tail):                         # warm both paths at this shape
            sample(fn, args, 10)
        times = {"host": [], "device": []}
        for _ in range(a.repeats):
            times["host"].append(sample(host_tail, args, a.inner))
            times["device"].append(sample(device_tail, args, a.inner))
        entry = {"queries": Q, "rows_kept": kept, "rows_selected": a.batch * TOPK}
        for tag, t in times.items():
            entry[tag] = {"median": round(statistics.median(t), 1), "min": round(min(t), 1), "max": round(max(t), 1)}
        entry["device_ahead_of_host_range"] = entry["device"]["median"] < entry["host"]["min"]
        entry["host_over_device"] = round(entry["host"]["median"] / entry["device"]["median"], 2)
        result["configs"].append(entry)
    text = json.dumps(result)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
