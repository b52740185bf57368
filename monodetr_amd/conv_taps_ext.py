"""``conv_strided(x, weight, shift, relu)``: the stride-2 convolutions of the backbone, the fourth pyramid level and the depth
predictor -- 3x3 / stride 2 / pad 1 and 1x1 / stride 2 on a channels_last bf16 activation, with the folded frozen-BN shift (or
a trainable bias) and the ReLU in the epilogue (csrc/conv_taps.hip through ``mdetr_conv_taps``).  Forward and input gradient
run on that kernel -- the input gradient as the four pixel-parity classes of the stride-2 transpose, each a stride-1 problem
with 1x1 / 1x2 / 2x1 / 2x2 taps --, the weight gradient on csrc/conv_wgrad.hip (conv_wgrad_ext).

With MDETR_CONV_STRIDED_F32=1 fp32 tensors take the fp32 form of the same kernel for the 3x3 case (``mdetr_conv_taps_f32``,
``mdetr_conv_dgrad_s2_f32``: three-way bf16 split, fp32-accurate) and return fp32; their weight gradient is the library's unless
MDETR_CONV_WGRAD_S2_F32=1 sends it to ``mdetr_conv_wgrad_s2_f32`` (conv_wgrad_ext.supported_f32_s2)."""
import os

import torch

from . import _capi

_backend = None               # tests substitute the CPU emulation of the same kernel source (tests/native_emul.py)
ENABLED = os.environ.get("MDETR_CONV_STRIDED") == "1"
# The fp32 form: a family of its own (opt-in, on no committed list), separate from ENABLED.
ENABLED_F32 = os.environ.get("MDETR_CONV_STRIDED_F32") == "1"


def _lib():
    return _backend if _backend is not None else _capi.lib()


def supported(x, weight, stride=(2, 2), padding=(1, 1), dilation=(1, 1), groups=1):
    """x [B, C, H, W] channels_last bf16; weight [N, C, 3, 3] with padding 1 or [N, C, 1, 1] with padding 0; stride 2."""
    k = tuple(weight.shape[2:]) if weight.dim() == 4 else None
    return ((x.is_cuda or _backend is not None) and x.dim() == 4 and weight.dim() == 4 and x.dtype == torch.bfloat16
            and weight.dtype == torch.bfloat16 and tuple(stride) == (2, 2) and tuple(dilation) == (1, 1) and groups == 1
            and ((k == (3, 3) and tuple(padding) == (1, 1)) or (k == (1, 1) and tuple(padding) == (0, 0)))
            and weight.shape[1] == x.shape[1] and x.shape[1] % 64 == 0 and weight.shape[0] % 64 == 0 and x.numel() > 0
            and x.is_contiguous(memory_format=torch.channels_last) and x.data_ptr() % 16 == 0)


# The measured shape rule of the fp32 form (tools/convbench --dtype fp32 --only strided at B = 8, profiles/r11a_convbench_fp32_strided.json;
# kernel / library, us, medians of 3 captures whose spread is below 4 us on either side, layer2's forward kernel 156 - 163).  A class goes to the kernel only where it wins:
#   forward   160 / 194 at 128 -> 128 channels from 96 x 320 (layer2);  263 / 182 at 256 -> 256 from 48 x 160 (layer3, the depth predictor's
#             downsample);  381 / 170 at 512 -> 512 from 24 x 80 (layer4);  276 (8 splits; 505 unsplit) / 91 at 2048 -> 256 from 12 x 40 (the
#             fourth pyramid level): the 16-channel slab pays 6 slabs x 3 stages per 32 channels more the wider the layer
#   dX        173 / 234, 190 / 252, 199 / 257 on the three backbone sites (177 / 198 / 215 with the weight transpose the backward pass makes
#             for an fp32 weight);  165 (195 with the transpose) / 125 on the pyramid level (2048 channels of dx on 12 x 40)
# so the forward pass takes the kernel up to 128 input channels and the input gradient up to 512; a convolution neither class of which
# takes the kernel (the pyramid level) is not `supported_f32` at all.  The entries compute every shape: the kernel's tests lift the rule.
_F32_FWD_MAX_C = 128
_F32_DX_MAX_C = 512


def supported_f32(x, weight, stride=(2, 2), padding=(1, 1), dilation=(1, 1), groups=1):
    """``supported`` for the fp32 form: x [B, C, H, W] channels_last fp32, weight [N, C, 3, 3] fp32 with padding 1, stride 2 (the
    1x1 / stride-2 shortcut is a gather and a token GEMM in fp32), within the entry's 32-bit byte offsets (x.numel() < 2^29).
    N % 32 == 0 is enough for the forward pass; the input gradient takes the kernel where N % 64 == 0 (``_dx_on_kernel``) and the
    library otherwise.  The measured shape rule above decides per class (``_fwd_on_kernel``, ``_dx_on_kernel``); true where at least
    one of the two takes the kernel.  False without the family MDETR_CONV_STRIDED_F32 -- also under the emulated kernel (tests): the
    family alone decides, so that fp32 tensors keep the library's convolution (and ``conv_strided`` its refusal) without it."""
    return (ENABLED_F32 and (x.is_cuda or _backend is not None) and x.dim() == 4 and weight.dim() == 4 and x.dtype == torch.float32
            and weight.dtype == torch.float32 and tuple(stride) == (2, 2) and tuple(dilation) == (1, 1) and groups == 1
            and tuple(weight.shape[2:]) == (3, 3) and tuple(padding) == (1, 1)
            and weight.shape[1] == x.shape[1] and x.shape[1] % 64 == 0 and weight.shape[0] % 32 == 0 and 0 < x.numel() < (1 << 29)
            and (x.shape[1] <= _F32_FWD_MAX_C or (weight.shape[0] % 64 == 0 and x.shape[1] <= _F32_DX_MAX_C))
            and x.is_contiguous(memory_format=torch.channels_last) and x.data_ptr() % 16 == 0)


def _f32(t):
    return t.dtype == torch.float32


def _fwd_on_kernel(x):
    """bf16: always.  fp32: the measured shape rule (``_F32_FWD_MAX_C``)."""
    return not _f32(x) or x.shape[1] <= _F32_FWD_MAX_C


def _dx_on_kernel(dy, C):
    """bf16: always (``supported`` asks for N % 64 == 0).  fp32: mdetr_conv_dgrad_s2_f32 contracts dy's channels in whole 64s, and the
    measured shape rule (``_F32_DX_MAX_C``) on dx's C channels."""
    return not _f32(dy) or (dy.shape[1] % 64 == 0 and C <= _F32_DX_MAX_C)


def _forward_library(x, weight, shift, relu):
    """The library's forward pass inside ``_ConvStrided`` (fp32 classes the shape rule keeps off the kernel): what backbone.conv_bn
    does without the family -- the convolution, then shift and ReLU in one pass (csrc/bias_act.hip) where that family is on."""
    import torch.nn.functional as F
    from . import bias_act_ext
    if relu and shift is not None and bias_act_ext.ENABLED and (x.is_cuda or bias_act_ext._backend is not None):
        y = F.conv2d(x, weight, None, (2, 2), (1, 1))
        if bias_act_ext.supported(y, shift):
            return bias_act_ext.bias_act(y, shift, None, relu=True)
        y = y + shift.view(1, -1, 1, 1)
    else:
        y = F.conv2d(x, weight, shift, (2, 2), (1, 1))
    return torch.relu_(y) if relu else y


def _autocast(x):
    """Is autocast on for x's device type?  (The fp32 route must not take tensors the library would compute in a lower precision.)"""
    try:
        return torch.is_autocast_enabled(x.device.type)
    except TypeError:                                                  # (a torch whose query takes no device type)
        return torch.is_autocast_enabled()


def _ohwi(weight):
    """[N, C, kh, kw] -> contiguous [N, kh, kw, C] (a view when the weight is channels_last already)."""
    w = weight.permute(0, 2, 3, 1).contiguous()
    return w if w.data_ptr() % 16 == 0 else w.clone()


def _call(x, w, shift, y, dims, relu):
    cuda = x.is_cuda
    d = torch.tensor(dims, dtype=torch.int64)
    name = "mdetr_conv_taps_f32" if _f32(x) else "mdetr_conv_taps"
    rc = getattr(_lib(), name)(x.data_ptr(), w.data_ptr(), shift.data_ptr() if shift is not None else None, y.data_ptr(), d.data_ptr(),
                               1 if relu else 0, x.device.index if cuda else -1, torch.cuda.current_stream(x.device).cuda_stream if cuda else None)
    if rc != 0:
        _capi.check(rc, name)


def _split_count(B, OH, OW, N, C, k, relu):
    """Contraction splits for the forward pass, 0 = none: few output tiles (4 x 32 pixels x 32 channels each) against many channel
    slabs -- split until ~1 000 workgroups exist, at least 4 slabs of 32 channels per split."""
    from . import _tune
    if relu or k != 3 or _tune.get("conv_taps_split", "1") == "0":
        return 0
    blocks = B * ((OH + 3) // 4) * ((OW + 31) // 32) * (N // 32)
    slabs = C // 32
    if blocks >= 256 or slabs < 16:
        return 0
    ks = 1
    while ks * 2 <= 64 and blocks * ks * 2 <= 1024 and slabs % (ks * 2) == 0 and slabs // (ks * 2) >= 4:
        ks *= 2
    return ks if ks >= 2 else 0


def _forward_split(x, w_ohwi, shift, ks, dims):
    """The forward pass with the contraction split ks ways (mdetr_conv_taps_split; mdetr_conv_taps_f32_split for fp32 tensors) + one
    sum over the splits in a fixed order (csrc/colsum.hip), rounded to x's dtype."""
    B, OH, OW, N = dims[0], dims[4], dims[5], dims[6]
    cuda = x.is_cuda
    cols = B * OH * OW * N
    if cuda and _backend is None:
        from . import _workspace as W_
        part = W_.get("conv_taps_split", x.device, ks * cols * 4).view(torch.float32)[:ks * cols]
    else:
        part = torch.empty(ks * cols, dtype=torch.float32, device=x.device)
    d = torch.tensor(dims, dtype=torch.int64)
    name = "mdetr_conv_taps_f32_split" if _f32(x) else "mdetr_conv_taps_split"
    rc = getattr(_lib(), name)(x.data_ptr(), w_ohwi.data_ptr(), shift.data_ptr() if shift is not None else None, part.data_ptr(),
                               part.numel(), d.data_ptr(), ks, x.device.index if cuda else -1,
                               torch.cuda.current_stream(x.device).cuda_stream if cuda else None)
    if rc != 0:
        _capi.check(rc, name)
    part = part.view(ks, cols)
    if cuda and _backend is None:
        from .colsum_ext import column_sum, supported as colsum_ok
        y = column_sum(part, out_dtype=x.dtype) if colsum_ok(part) else part.sum(0).to(x.dtype)
    else:
        y = part.sum(0).to(x.dtype)
    return y.view(B, OH, OW, N).permute(0, 3, 1, 2)                     # [B, N, OH, OW] with channels_last strides


def _forward(x, w_ohwi, shift, relu):
    """x [B, C, H, W] channels_last, w_ohwi [N, k, k, C] -> y [B, N, OH, OW] channels_last."""
    B, C, H, W = x.shape
    N, k = w_ohwi.shape[0], w_ohwi.shape[1]
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    ks = _split_count(B, OH, OW, N, C, k, relu)
    if ks:
        return _forward_split(x, w_ohwi, shift, ks, [B, H, W, C, OH, OW, N, 2, k, k, 1, 1, 0, 1, 0, 1, 0, OH * OW * N, OW * N, N, k * k * C, k * C, C])
    y = torch.empty((B, N, OH, OW), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    pad = 1 if k == 3 else 0
    _call(x, w_ohwi, shift, y, [B, H, W, C, OH, OW, N, 2, k, k, pad, pad, 0, 1, 0, 1, 0, OH * OW * N, OW * N, N, k * k * C, k * C, C], relu)
    return y


def _input_gradient(dy, w_ohwi, H, W, w_ihwo=None):
    """dX [B, C, H, W] of the stride-2 convolution from dY [B, N, OH, OW] (channels_last): the four pixel-parity classes in one
    launch (``mdetr_conv_dgrad_s2``; ``mdetr_conv_dgrad_s2_f32`` for fp32 tensors); every element of dX is written by it."""
    B, N, OH, OW = dy.shape
    k, C = w_ohwi.shape[1], w_ohwi.shape[3]
    wt = w_ihwo                                                         # [C, k, k, N]: made with the weight (csrc/wfold.hip) ...
    if wt is None or wt.shape != (C, k, k, N) or not wt.is_contiguous() or wt.dtype != w_ohwi.dtype:
        wt = w_ohwi.permute(3, 1, 2, 0).contiguous()                    # ... or one small copy here
    dx = torch.empty((B, C, H, W), dtype=dy.dtype, device=dy.device, memory_format=torch.channels_last)
    cuda = dy.is_cuda
    name = "mdetr_conv_dgrad_s2_f32" if _f32(dy) else "mdetr_conv_dgrad_s2"
    rc = getattr(_lib(), name)(dy.data_ptr(), wt.data_ptr(), dx.data_ptr(), B, OH, OW, N, H, W, C, k, dy.device.index if cuda else -1,
                               torch.cuda.current_stream(dy.device).cuda_stream if cuda else None)
    if rc != 0:
        _capi.check(rc, name)
    return dx


class _ConvStrided(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, shift, relu, hand_out_token=False):
        w = _ohwi(weight)
        sh = None if shift is None else shift.float().contiguous()
        y = _forward(x, w, sh, relu) if _fwd_on_kernel(x) else _forward_library(x, weight, sh, relu)
        ctx.relu = bool(relu)
        ctx.shift_dtype = None if shift is None else shift.dtype
        ctx.w_ihwo = getattr(weight, "_mdetr_ihwo", None)
        ctx.relu_token = None
        if relu and hand_out_token:
            from .monodetr.linear import ReluToken
            ctx.relu_token = y._mdetr_relu_token = ReluToken()         # the one consumer of y may take over this ReLU's backward mask
        ctx.save_for_backward(x, weight, w, *((y,) if relu else ()))
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, weight, w = ctx.saved_tensors[:3]
        if ctx.relu and not (ctx.relu_token is not None and ctx.relu_token.premasked):
            dy = torch.ops.aten.threshold_backward(dy, ctx.saved_tensors[3], 0.0)
        dy = dy.contiguous(memory_format=torch.channels_last)
        k = weight.shape[2]
        pad = (1, 1) if k == 3 else (0, 0)
        dx = dw = ds = None
        if ctx.needs_input_grad[0]:
            if _dx_on_kernel(dy, x.shape[1]):
                dx = _input_gradient(dy, w, x.shape[2], x.shape[3], ctx.w_ihwo)
            else:
                dx = torch.ops.aten.convolution_backward(dy, x, weight, None, (2, 2), pad, (1, 1), False, (0, 0), 1, (True, False, False))[0]
        if ctx.needs_input_grad[1]:
            from . import conv_wgrad_ext
            # (fp32: the stride-2 form of the weight-gradient kernel where its family is on -- whichever route forward and dX took)
            if conv_wgrad_ext.supported(x, dy, k, 2) or (k == 3 and weight.dtype == torch.float32 and conv_wgrad_ext.supported_f32_s2(x, dy)):
                dw = conv_wgrad_ext.weight_gradient(x, dy, k, 2, weight.dtype, like=weight)
            else:
                dw = torch.ops.aten.convolution_backward(dy, x, weight, None, (2, 2), pad, (1, 1), False, (0, 0), 1, (False, True, False))[1]
        if ctx.shift_dtype is not None and ctx.needs_input_grad[2]:
            dy2 = dy.permute(0, 2, 3, 1).reshape(-1, dy.shape[1])
            if dy2.is_cuda and _backend is None:
                from .colsum_ext import column_sum, supported as colsum_ok
                od = ctx.shift_dtype if ctx.shift_dtype in (torch.float32, torch.bfloat16) else torch.float32       # (one rounding, no cast launch)
                ds = column_sum(dy2, out_dtype=od) if colsum_ok(dy2) else dy2.float().sum(0)
            else:
                ds = dy2.float().sum(0)
            ds = ds.to(ctx.shift_dtype)
        return dx, dw, ds, None, None


def conv_strided(x, weight, shift=None, relu=False, hand_out_token=False):
    """act(conv2d(x, weight, stride=2, padding=1 (3x3) / 0 (1x1)) + shift[None, :, None, None])."""
    if not supported(x, weight, padding=(1, 1) if weight.shape[2] == 3 else (0, 0)) and not supported_f32(x, weight):
        raise RuntimeError("conv_strided: needs a bf16 channels_last activation with C % 64 == 0 and a bf16 [N, C, 3, 3] / [N, C, 1, 1] weight with "
                           "N % 64 == 0, or the same in fp32 with a [N, C, 3, 3] weight")
    return _ConvStrided.apply(x, weight, shift, relu, hand_out_token)


class ConvStrided(torch.nn.Conv2d):
    """nn.Conv2d (same parameters, same state_dict keys) whose forward takes the kernel when MDETR_CONV_STRIDED=1 (bf16) or
    MDETR_CONV_STRIDED_F32=1 (fp32) and the call qualifies, and nn.Conv2d's otherwise (monodetr.py:87-92, depth_predictor.py:29-31:
    3x3 / stride 2 / pad 1 with a bias)."""

    def forward(self, x):
        if ENABLED_F32 and x.dtype == self.weight.dtype and not torch.is_autocast_enabled() and not _autocast(x) \
                and self.padding_mode == "zeros" and supported_f32(x, self.weight, self.stride, self.padding, self.dilation, self.groups):
            return conv_strided(x, self.weight, self.bias, relu=False)
        if ENABLED and x.dtype == self.weight.dtype and not torch.is_autocast_enabled() and self.padding_mode == "zeros" \
                and supported(x, self.weight, self.stride, self.padding, self.dilation, self.groups):
            return conv_strided(x, self.weight, self.bias, relu=False)
        return super().forward(x)
