"""Model outputs -> KITTI detections -- mirror of ``lib/helpers/decode_helper.py`` (the two functions the tester
calls; the heat-map helpers of that file belong to centre-net style heads and are not mirrored).

``extract_dets_from_outputs`` runs on the device without host synchronisation; ``decode_detections`` is the
reference's numpy step (image-plane decoding, back-projection with the frame's calibration), vectorised per image.
``decode_batch`` is both steps as one kernel launch and one copy to the host (``detect_ext``; opt-in, see ``Tester._detect``)."""
import numpy as np
import torch

from ..datasets.utils import class2angle
from ..utils import box_ops


def extract_dets_from_outputs(outputs, K=50, topk=50):
    """Top-``topk`` (query, class) pairs by sigmoid score -> ``[B, topk, 37]``:
    label, score, 2-D centre x, y, 2-D width, height, depth, 24 heading logits / residuals, 3 dimensions,
    projected 3-D centre x, y, exp(-log-variance of depth)."""
    logits, boxes = outputs['pred_logits'], outputs['pred_boxes']
    B, Q, C = logits.shape
    scores, flat = torch.topk(logits.sigmoid().view(B, -1), topk, dim=1)
    query = (flat // C).unsqueeze(-1)
    labels = (flat % C).view(B, -1, 1)
    take = lambda t: torch.gather(t, 1, query.expand(-1, -1, t.shape[-1]))
    boxes = take(boxes)
    heading = take(outputs['pred_angle'])
    size_3d = take(outputs['pred_3d_dim'])
    depth = take(outputs['pred_depth'][:, :, 0:1])
    sigma = take(torch.exp(-outputs['pred_depth'][:, :, 1:2]))
    xywh = box_ops.box_xyxy_to_cxcywh(box_ops.box_cxcylrtb_to_xyxy(boxes))
    return torch.cat([labels, scores.view(B, -1, 1), xywh[:, :, 0:1], xywh[:, :, 1:2], xywh[:, :, 2:4], depth, heading, size_3d,
                      boxes[:, :, 0:1], boxes[:, :, 1:2], sigma], dim=2)


def get_heading_angle(heading):
    """24 values = 12 bin logits + 12 residuals -> angle in (-pi, pi]."""
    cls = np.argmax(heading[0:12])
    return class2angle(cls, heading[12:24][cls], to_label_format=True)


def decode_detections(dets, info, calibs, cls_mean_size, threshold):
    """``dets`` numpy ``[B, max_dets, 37]`` (layout above), ``info`` dict of numpy arrays (``img_id``, ``img_size``),
    ``calibs`` one ``Calibration`` per image -> ``{img_id: [[cls, alpha, x1, y1, x2, y2, h, w, l, x, y, z, ry, score], ...]}``."""
    results = {}
    for i in range(dets.shape[0]):
        d = dets[i][dets[i, :, 1] >= threshold]
        W, H = info['img_size'][i][0], info['img_size'][i][1]
        cls_id = d[:, 0].astype(np.int64)
        x, y, w, h = d[:, 2] * W, d[:, 3] * H, d[:, 4] * W, d[:, 5] * H
        depth = d[:, 6]
        dims = d[:, 31:34] + cls_mean_size[cls_id]
        loc = calibs[i].img_to_rect(d[:, 34] * W, d[:, 35] * H, depth)
        loc[:, 1] += dims[:, 0] / 2                                  # box origin: bottom centre
        preds = []
        for j in range(d.shape[0]):
            alpha = get_heading_angle(d[j, 7:31])
            ry = calibs[i].alpha2ry(alpha, x[j])
            preds.append([int(cls_id[j]), alpha, x[j] - w[j] / 2, y[j] - h[j] / 2, x[j] + w[j] / 2, y[j] + h[j] / 2]
                         + dims[j].tolist() + loc[j].tolist() + [ry, d[j, 1] * d[j, -1]])
        results[info['img_id'][i]] = preds
    return results


def decode_batch(outputs, info, calibs, cls_mean_size, threshold, topk):
    """``extract_dets_from_outputs`` + ``decode_detections`` on the device: one launch of ``mdetr_detect_decode``, one copy of the
    result rows and keep flags to the host, no per-detection Python.  Same arguments as ``decode_detections`` with the head
    ``outputs`` in place of ``dets``; same ``{img_id: [[cls, alpha, ...], ...]}`` result.  The calibration scalars are read from the
    ``Calibration`` objects, so both paths see identical numbers."""
    from .. import detect_ext
    B = outputs['pred_logits'].shape[0]
    mean = np.asarray(cls_mean_size, dtype=np.float64)
    consts = np.empty(B * 8 + mean.size, dtype=np.float64)          # calibration, image sizes, mean sizes: one copy to the device
    consts[:B * 6] = [float(v) for c in calibs for v in (c.cu, c.cv, c.fu, c.fv, c.tx, c.ty)]
    consts[B * 6:B * 8] = np.asarray(info['img_size'], dtype=np.float64).reshape(-1)
    consts[B * 8:] = mean.reshape(-1)
    dev = torch.from_numpy(consts).to(outputs['pred_logits'].device)
    found = detect_ext.detect_decode(outputs, dev[:B * 6].view(B, 6), dev[B * 6:B * 8].view(B, 2), dev[B * 8:].view(mean.shape), threshold, topk)
    host = found.packed.cpu().numpy()
    slots = B * topk
    rows, keep = host[:slots * 14 * 8].view(np.float64).reshape(B, topk, 14), host[slots * 14 * 8:].view(np.bool_).reshape(B, topk)
    results = {}
    for i in range(B):
        preds = rows[i][keep[i]].tolist()
        for p in preds:
            p[0] = int(p[0])
        results[info['img_id'][i]] = preds
    return results
