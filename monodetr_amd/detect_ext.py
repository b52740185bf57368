"""``detect_decode``: the model's head outputs -> finished KITTI detections in ONE launch (csrc/detect.hip through
``mdetr_detect_decode``, ABI 22).

The tester's tail is ``extract_dets_from_outputs`` -- a sigmoid, a top-k, six gathers, two box conversions, an exp and a 12-way cat:
some twenty framework launches on a few kilobytes -- a synchronising copy to the host, and ``decode_detections``, a Python loop over
every kept detection.  Here one workgroup per image sorts the image's Q C logits in LDS and thread j decodes rank j: the result
rows in fp64 exactly as numpy computes them from the fp32 record, a keep flag per rank, and on request the 37-float record itself.

``tester.decode: device`` in the yaml or ``MDETR_DETECT_DECODE=1`` in the environment routes ``Tester._detect`` here
(``decode_helper.decode_batch``); the default is the host path.  NOT a kernel family: nothing in the training step changes."""
import collections

import numpy as np
import torch

from . import _capi

_backend = None      # tests substitute the same kernel source built for the host (tests/native_emul.py)
MAX_KEYS = 8192      # Q * C of one image (csrc/detect.h: kDetectMaxKeys)
HEADS = (('pred_logits', None), ('pred_boxes', 6), ('pred_angle', 24), ('pred_3d_dim', 3), ('pred_depth', 2))

# rows [B, topk, 14] fp64 and keep [B, topk] bool are views of `packed` (uint8: all rows, then all flags), so one copy moves both;
# dets37 [B, topk, 37] fp32 or None
Detections = collections.namedtuple('Detections', 'rows keep dets37 packed')


def _lib():
    return _backend if _backend is not None else _capi.lib()


def supported(outputs):
    """fp32 head outputs of one batch on one device, within the kernel's limits.  (CPU tensors take the entry's serial host form.)"""
    logits = outputs.get('pred_logits')
    if not (torch.is_tensor(logits) and logits.dim() == 3 and logits.dtype == torch.float32):
        return False
    B, Q, C = logits.shape
    if not (Q >= 1 and C >= 1 and Q * C <= MAX_KEYS):
        return False
    for name, width in HEADS[1:]:
        t = outputs.get(name)
        if not (torch.is_tensor(t) and t.dtype == torch.float32 and t.device == logits.device and t.shape == (B, Q, width)):
            return False
    return True


def _f64(x, device, shape):
    t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))
    t = t.to(device=device, dtype=torch.float64).contiguous()
    assert t.shape == shape, (tuple(t.shape), shape)
    return t


def detect_decode(outputs, calib6, img_size, cls_mean_size, threshold, topk, want_dets37=False):
    """outputs: the five fp32 heads; calib6 [B, 6] (cu, cv, fu, fv, tx, ty per frame), img_size [B, 2] (W, H), cls_mean_size [C, 3]:
    tensors or arrays, taken as fp64 on the outputs' device.  -> ``Detections`` on that device.  Rank order: by logit, NaN first, ties
    by ascending query * C + class (csrc/detect_math.h).  Raises where the entry refuses (topk outside 1 .. Q C, Q C > 8192)."""
    heads = [outputs[name].contiguous() for name, _ in HEADS]
    logits = heads[0]
    B, Q, C = logits.shape
    device = logits.device
    calib6, img_size, cls_mean_size = _f64(calib6, device, (B, 6)), _f64(img_size, device, (B, 2)), _f64(cls_mean_size, device, (C, 3))
    k = max(int(topk), 0)
    slots = B * k
    packed = torch.empty(slots * 14 * 8 + slots, dtype=torch.uint8, device=device)
    rows = packed[:slots * 14 * 8].view(torch.float64).view(B, k, 14)
    keep = packed[slots * 14 * 8:].view(B, k)
    dets37 = torch.empty(B, k, 37, dtype=torch.float32, device=device) if want_dets37 and slots else None
    cuda = logits.is_cuda
    # CPU tensors: ordinal -1, the entry's serial host form -- under the emulated library 0, whose "launch" runs the kernel itself on the host
    where = device.index if cuda else (0 if _backend is not None else -1)
    rc = _lib().mdetr_detect_decode(*[t.data_ptr() for t in heads], calib6.data_ptr(), img_size.data_ptr(), cls_mean_size.data_ptr(), B, Q, C, int(topk),
                                    float(threshold), rows.data_ptr(), keep.data_ptr(), dets37.data_ptr() if dets37 is not None else None,
                                    where, torch.cuda.current_stream(device).cuda_stream if cuda else None)
    if rc != 0:
        msg = _lib().mdetr_last_error()
        raise RuntimeError("mdetr_detect_decode failed (code %d): %s" % (rc, msg.decode() if msg else "?"))
    return Detections(rows, keep.view(torch.bool), dets37, packed)
