"""``conv_stem(x, weight, shift)``: the ResNet stem -- 7x7 / stride 2 / pad 3 convolution of the 3-channel image, frozen-BN shift
and ReLU in the epilogue (csrc/conv_stem.hip through ``mdetr_conv_stem``).  The stem is frozen (lib/models/monodetr/
backbone.py:71-73): forward only; the packed weight is built once per folded weight.

With MDETR_CONV_STEM_F32=1 an fp32 image and weight take the fp32 form of the same kernel (``mdetr_conv_stem_f32``: three-way bf16
split, six product terms, fp32-accurate) and return fp32; the weight is packed as three bf16 planes (hi, mid, lo)."""
import os

import torch

from . import _capi

_backend = None               # tests substitute the CPU emulation of the same kernel source (tests/native_emul.py)
ENABLED = os.environ.get("MDETR_CONV_STEM") == "1"
# The fp32 form: a family of its own (opt-in, on no committed list), separate from ENABLED.
ENABLED_F32 = os.environ.get("MDETR_CONV_STEM_F32") == "1"
K_PACKED = 176


def _lib():
    return _backend if _backend is not None else _capi.lib()


def supported(x, weight, stride=(2, 2), padding=(3, 3), dilation=(1, 1), groups=1):
    return ((x.is_cuda or _backend is not None) and x.dim() == 4 and weight.dim() == 4 and x.dtype == torch.bfloat16
            and weight.dtype == torch.bfloat16 and tuple(weight.shape) == (64, 3, 7, 7) and x.shape[1] == 3 and tuple(stride) == (2, 2)
            and tuple(padding) == (3, 3) and tuple(dilation) == (1, 1) and groups == 1 and x.numel() > 0
            and x.is_contiguous(memory_format=torch.channels_last) and not x.requires_grad and not weight.requires_grad)


def supported_f32(x, weight, stride=(2, 2), padding=(3, 3), dilation=(1, 1), groups=1):
    """``supported`` for the fp32 form: fp32 channels_last x [B, 3, H, W] within the entry's 32-bit byte offsets (B H W 12 < 2^31) and a
    frozen fp32 [64, 3, 7, 7] weight.  False without the family MDETR_CONV_STEM_F32 -- also under the emulated kernel (tests): the
    family alone decides, so that fp32 tensors keep the library's convolution without it."""
    return (ENABLED_F32 and (x.is_cuda or _backend is not None) and x.dim() == 4 and weight.dim() == 4 and x.dtype == torch.float32
            and weight.dtype == torch.float32 and tuple(weight.shape) == (64, 3, 7, 7) and x.shape[1] == 3 and tuple(stride) == (2, 2)
            and tuple(padding) == (3, 3) and tuple(dilation) == (1, 1) and groups == 1 and 0 < x.numel() * 4 < (1 << 31)
            and x.is_contiguous(memory_format=torch.channels_last) and not x.requires_grad and not weight.requires_grad)


def pack_weight_f32(weight):
    """[64, 3, 7, 7] fp32 -> [3, 64, 176] bf16: the planes hi = bf16(w), mid = bf16(w - hi), lo = bf16(w - hi - mid) (both subtractions
    are exact in fp32), each in ``pack_weight``'s layout; the pad columns of all three are exact zeros."""
    w = weight.detach().float().permute(0, 2, 3, 1).reshape(64, 7, 21)          # [n, t, e * 3 + ch]
    hi = w.to(torch.bfloat16)
    r1 = w - hi.float()
    mid = r1.to(torch.bfloat16)
    lo = (r1 - mid.float()).to(torch.bfloat16)
    out = torch.zeros(3, 64, K_PACKED, dtype=torch.bfloat16, device=weight.device)
    for plane, part in enumerate((hi, mid, lo)):
        out[plane, :, :168].view(64, 7, 24)[:, :, :21] = part
    return out


def pack_weight(weight):
    """[64, 3, 7, 7] -> [64, 176] bf16: row n holds, per tap row t, the 21 values w[n, ch, t, e] in (e, ch) order -- the order
    of 7 consecutive channels-last pixels -- padded to 24; 8 zeros at the end."""
    w = weight.detach().permute(0, 2, 3, 1).reshape(64, 7, 21)                  # [n, t, e * 3 + ch]
    out = torch.zeros(64, K_PACKED, dtype=torch.bfloat16, device=weight.device)
    out[:, :168].view(64, 7, 24)[:, :, :21] = w.to(torch.bfloat16)
    return out


def _launch(x, packed, shift, relu=True):
    assert relu, "the stem's epilogue is shift + ReLU"
    B, _, H, W = x.shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.empty((B, 64, OH, OW), dtype=torch.bfloat16, device=x.device, memory_format=torch.channels_last)
    cuda = x.is_cuda
    rc = _lib().mdetr_conv_stem(x.data_ptr(), packed.data_ptr(), shift.data_ptr() if shift is not None else None, y.data_ptr(), B, H, W,
                                x.device.index if cuda else -1, torch.cuda.current_stream(x.device).cuda_stream if cuda else None)
    if rc != 0:
        _capi.check(rc, "mdetr_conv_stem")
    return y


def _launch_f32(x, planes, shift, relu=True):
    assert relu, "the stem's epilogue is shift + ReLU"
    B, _, H, W = x.shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.empty((B, 64, OH, OW), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    cuda = x.is_cuda
    rc = _lib().mdetr_conv_stem_f32(x.data_ptr(), planes.data_ptr(), shift.data_ptr() if shift is not None else None, y.data_ptr(), B, H, W,
                                    x.device.index if cuda else -1, torch.cuda.current_stream(x.device).cuda_stream if cuda else None)
    if rc != 0:
        _capi.check(rc, "mdetr_conv_stem_f32")
    return y


_packed = {}


def conv_stem(x, weight, shift):
    """relu(conv2d(x, weight, stride=2, padding=3) + shift); the packed form of `weight` is cached per (storage, version)."""
    if x.dtype == torch.float32 and supported_f32(x, weight):
        # the fp32 planes in a slot of their own: alternating bf16 and fp32 calls do not evict each other
        hit = _packed.get("w_f32")
        if hit is None or hit[0]() is not weight or hit[1] != weight._version or (hit[4]() is not shift if shift is not None else hit[4] is not None):
            import weakref
            hit = _packed["w_f32"] = (weakref.ref(weight), weight._version, pack_weight_f32(weight),
                                      None if shift is None else shift.float().contiguous(), None if shift is None else weakref.ref(shift))
        return _launch_f32(x, hit[2], hit[3])
    if not supported(x, weight):
        raise RuntimeError("conv_stem: needs a bf16 channels_last [B, 3, H, W] image batch and a frozen bf16 [64, 3, 7, 7] weight, or the "
                           "same in fp32 with MDETR_CONV_STEM_F32")
    # keyed by the tensor OBJECT (a weak reference: a freed tensor's address and version may come back with another weight) and its
    # version counter
    hit = _packed.get("w")
    if hit is None or hit[0]() is not weight or hit[1] != weight._version or (hit[4]() is not shift if shift is not None else hit[4] is not None):
        import weakref
        hit = _packed["w"] = (weakref.ref(weight), weight._version, pack_weight(weight), None if shift is None else shift.float().contiguous(),
                              None if shift is None else weakref.ref(shift))
    return _launch(x, hit[2], hit[3])
