"""``weight_gradient(x, dy, k, stride, dtype)``: dW of a 3x3 (stride 1 / 2, pad 1) or 1x1 (stride 2) convolution from the
channels_last bf16 activation and output gradient (csrc/conv_wgrad.hip through ``mdetr_conv_wgrad``: split-K over pixel tiles
on the matrix cores; the per-chunk partial gradients are added in a fixed order by csrc/colsum.hip, one rounding).  fp32 operands
of a 3x3 / stride-1 convolution take the fp32 form of the kernel (``mdetr_conv_wgrad_f32``, MDETR_CONV_WGRAD_F32=1), those of a
3x3 / stride-2 convolution its stride-2 sibling (``mdetr_conv_wgrad_s2_f32``, MDETR_CONV_WGRAD_S2_F32=1)."""
import os

import torch

from . import _capi

_backend = None               # tests substitute the CPU emulation of the same kernel source (tests/native_emul.py)
# MDETR_CONV_WGRAD=1: the hand-written convolutions (conv3x3_ext, conv_taps_ext) take their weight gradient from this kernel
# instead of the library's (MIOpen igemm_wrw)
ENABLED = os.environ.get("MDETR_CONV_WGRAD") == "1"


def _lib():
    return _backend if _backend is not None else _capi.lib()


def supported(x, dy, k, stride):
    return ((ENABLED or _backend is not None) and (x.is_cuda or _backend is not None) and x.dim() == 4 and dy.dim() == 4 and x.dtype == torch.bfloat16 and dy.dtype == torch.bfloat16
            and ((k == 3 and stride in (1, 2)) or (k == 1 and stride in (1, 2))) and x.shape[1] % 64 == 0 and dy.shape[1] % 32 == 0
            and x.numel() > 0 and dy.numel() > 0 and x.is_contiguous(memory_format=torch.channels_last)
            and dy.is_contiguous(memory_format=torch.channels_last) and x.data_ptr() % 16 == 0 and dy.data_ptr() % 16 == 0)


# Which fp32 shape classes take the kernel: tools/convbench --dtype fp32 --only wgrad (profiles/r10a_convbench_fp32_wgrad.json; kernel +
# chunk sum against aten.convolution_backward, B = 8, medians of 3 captures [min, max], us):
#   layer1   64 ch, 96 x 320   208.4 [208.0, 210.6]  against  184.3 [178.7, 192.9]   behind: N = 64 fills half of the 128-row dY block
#   layer2  128 ch, 48 x 160   118.9 [118.2, 119.2]  against  164.4 [159.7, 171.5]   ahead
#   layer3  256 ch, 24 x 80    111.9 [111.7, 113.1]  against  163.7 [160.9, 172.4]   ahead (the depth head's 3x3 is this problem)
#   layer4  512 ch, 12 x 40    188.6 [187.7, 188.7]  against  163.6 [161.9, 167.3]   behind: 4 x 8 weight blocks x 3 tap rows leave 2 chunks,
#                                                                                   192 workgroups of 24 tiles each on 256 CUs
# A class whose median is not ahead of the library's own [min, max] goes back to the library: fewer than 128 output channels, or more
# than 8 (128 n x 64 c) weight blocks (layer3 has 8, layer4 32; nothing between them was measured, so nothing between them is admitted).
_F32_MIN_N = 128
_F32_MAX_BLOCKS = 8


def supported_f32(x, dy, k, stride):
    """fp32 channels_last operands of a 3x3 / stride-1 convolution within the entry's limits (C % 64 == 0, N % 32 == 0, 16-byte aligned,
    B H W C and B H W N below 2^29 elements, 9 N C below 2^28) and the measured shape rule above, with the family MDETR_CONV_WGRAD_F32
    on -- also under the emulated kernel (tests): the family alone decides, so that fp32 convolutions keep the library's weight
    gradient without it."""
    return (ENABLED_CONV_F32 and (x.is_cuda or _backend is not None) and x.dim() == 4 and dy.dim() == 4 and x.dtype == torch.float32
            and dy.dtype == torch.float32 and k == 3 and stride == 1 and x.shape[1] % 64 == 0 and dy.shape[1] % 32 == 0
            and x.numel() > 0 and dy.numel() > 0 and x.shape[0] == dy.shape[0] and tuple(x.shape[2:]) == tuple(dy.shape[2:])
            and x.numel() < (1 << 29) and dy.numel() < (1 << 29) and dy.shape[1] * 9 * x.shape[1] < (1 << 28)
            and dy.shape[1] >= _F32_MIN_N and ((dy.shape[1] + 127) // 128) * (x.shape[1] // 64) <= _F32_MAX_BLOCKS
            and x.is_contiguous(memory_format=torch.channels_last) and dy.is_contiguous(memory_format=torch.channels_last)
            and x.data_ptr() % 16 == 0 and dy.data_ptr() % 16 == 0)


# Which fp32 STRIDE-2 shape classes take the kernel (mdetr_conv_wgrad_s2_f32): tools/convbench --dtype fp32 --only wgrad, the stride-2 rows
# (profiles/r14a_convbench_fp32_wgrad_s2.json; kernel + chunk sum against aten.convolution_backward at stride 2, B = 8, medians of 3 captures
# [min, max], us):
#   layer2.0.conv2  128 -> 128 from 96 x 320   142.4 [141.9, 144.1]  against  172.0 [168.3, 177.3]   ahead  (4 blocks of 64 n x 64 c, 42 chunks)
#   layer3.0.conv2  256 -> 256 from 48 x 160   142.7 [141.2, 142.9]  against  166.3 [162.9, 175.1]   ahead  (16 blocks, 10 chunks; the depth
#                                                                                                   predictor's downsample is this problem)
#   layer4.0.conv2  512 -> 512 from 24 x 80    194.6 [194.0, 195.3]  against  169.8 [164.8, 174.2]   behind: 64 blocks x 3 tap rows leave 2 chunks,
#                                                                                                   384 workgroups on 512 places
# A class whose median is not ahead of the library's own [min, max] stays on the library: more than 16 (64 n x 64 c) weight blocks (layer3.0
# has 16, layer4.0 64; nothing between them was measured, so nothing between them is admitted).  Nothing below 128 output channels was
# measured either -- the model has no such site -- so nothing below is admitted.
_F32_S2_MIN_N = 128
_F32_S2_MAX_BLOCKS = 16


def supported_f32_s2(x, dy):
    """fp32 channels_last operands of a 3x3 / stride-2 / pad-1 convolution (x [B, C, H, W], dy [B, N, (H - 1) // 2 + 1, (W - 1) // 2 + 1]) within
    the entry's limits (C % 64 == 0, N % 32 == 0, 16-byte aligned, both operands below 2^29 elements, 9 N C below 2^28) and the measured
    shape rule above, with the family MDETR_CONV_WGRAD_S2_F32 on -- also under the emulated kernel (tests): the family alone decides, so
    that the fp32 strided convolutions keep the library's weight gradient without it."""
    return (ENABLED_CONV_S2_F32 and (x.is_cuda or _backend is not None) and x.dim() == 4 and dy.dim() == 4 and x.dtype == torch.float32
            and dy.dtype == torch.float32 and x.shape[1] % 64 == 0 and dy.shape[1] % 32 == 0
            and x.numel() > 0 and dy.numel() > 0 and x.shape[0] == dy.shape[0]
            and tuple(dy.shape[2:]) == ((x.shape[2] - 1) // 2 + 1, (x.shape[3] - 1) // 2 + 1)
            and x.numel() < (1 << 29) and dy.numel() < (1 << 29) and dy.shape[1] * 9 * x.shape[1] < (1 << 28)
            and dy.shape[1] >= _F32_S2_MIN_N and ((dy.shape[1] + 63) // 64) * (x.shape[1] // 64) <= _F32_S2_MAX_BLOCKS
            and x.is_contiguous(memory_format=torch.channels_last) and dy.is_contiguous(memory_format=torch.channels_last)
            and x.data_ptr() % 16 == 0 and dy.data_ptr() % 16 == 0)


# Weight AND bias gradients of token-wise linear layers over tens of thousands of rows (the encoder's 81 600, the backbone's 1x1
# convolutions) as the 1x1 case of this kernel, the bias gradient riding along (mdetr_token_wgrad), instead of the library's batched
# split-K product + chunk sum + two-launch column sum: 53 -> 43 us at [81 600, 256] x [81 600, 256], 49 -> 28-36 us on the backbone's
# and the depth head's shapes (profiles/r04q_wgradbench.json).
TOKEN_ROUTE = True
# MDETR_TWGRAD_F32=1: the same two gradients of FP32 token matrices through the fp32 form of csrc/twgrad.hip (mdetr_token_wgrad_f32:
# operands split three ways into bf16, six matrix-instruction terms -- fp32-accurate) instead of the library's batched product + chunk
# sum + column sum.  A family of its own: separate from ENABLED (MDETR_CONV_WGRAD) and from linear._TGEMM_F32.  Opt-in, on no committed list.
ENABLED_F32 = os.environ.get("MDETR_TWGRAD_F32") == "1"
# MDETR_CONV_WGRAD_F32=1: the weight gradient of the FP32 stride-1 3x3 convolutions through the fp32 form of csrc/conv_wgrad.hip
# (mdetr_conv_wgrad_f32: operands split three ways into bf16, six matrix-instruction terms -- fp32-accurate) instead of the library's
# (MIOpen igemm_wrw / CK bwd_weight).  Consulted in conv3x3_ext._Conv3x3.backward only, so in the step it acts together with
# MDETR_CONV3X3_F32.  A family of its own, opt-in, on no committed list.
ENABLED_CONV_F32 = os.environ.get("MDETR_CONV_WGRAD_F32") == "1"
# MDETR_CONV_WGRAD_S2_F32=1: the weight gradient of the FP32 3x3 / stride-2 convolutions through conv_wgrad_s2_f32_kernel
# (mdetr_conv_wgrad_s2_f32: the same split and six terms on a tile of its own) instead of the library's.  Consulted in
# conv_taps_ext._ConvStrided.backward only, so in the step it acts together with MDETR_CONV_STRIDED_F32.  A family of its own, opt-in,
# on no committed list.
ENABLED_CONV_S2_F32 = os.environ.get("MDETR_CONV_WGRAD_S2_F32") == "1"
# MDETR_TWGRAD_GROUPED=1: inside chunk_sums.deferred() the bf16 token weight gradients of at most small_wgrad_ext.MAX_ROWS rows are
# registered and launched together at the next flush (mdetr_token_wgrad_grouped: one launch per kernel instantiation), ahead of the
# chunk sums that read their partials -- the same partials, bit for bit.  kernel_families decides; DESIGN.md 3.4.
GROUPED = os.environ.get("MDETR_TWGRAD_GROUPED") == "1"


def _chunk_sum_route(chunk_sums, cuda, cols, dtype):
    """Do the partials go to chunk_sums.chunk_sum (which defers or launches at once)?  On the GPU inside ``deferred()`` only -- outside it
    the column-sum kernel adds them out of the shared workspace; with the emulated kernel (tests) whenever the family is on, so that
    the sums of a backward pass that may not defer still run the kernel."""
    if cols % 4 != 0 or dtype not in (torch.float32, torch.bfloat16):
        return False
    return chunk_sums.deferring() if cuda and chunk_sums._backend is None else chunk_sums._backend is not None and chunk_sums.ENABLED


def token_weight_gradient(x2, dy2, dtype, bias=False):
    """(dW [N, K], db [N] or None) = (dy2^T x2, column sums of dy2) for token matrices x2 [T, K], dy2 [T, N] (both bf16 or both fp32, contiguous
    rows): the 1x1 case of the convolution weight-gradient kernel, the bias gradient riding along on the dy operand that
    is already in LDS -- one kernel + one sum over its chunks for both gradients (the library route: a batched split-K product, a
    chunk sum, and a two-launch column sum that reads dy a second time)."""
    T, K = x2.shape
    N = dy2.shape[1]
    lib = _lib()
    if x2.dtype != dy2.dtype or x2.dtype not in (torch.bfloat16, torch.float32):
        raise RuntimeError("token_wgrad: operands of one dtype, bf16 or fp32 (got %s, %s)" % (x2.dtype, dy2.dtype))
    # fp32 operands: the fp32 form of the kernel (three-way bf16 split), same partials and chunk sums
    entry = "mdetr_token_wgrad_f32" if x2.dtype == torch.float32 else "mdetr_token_wgrad"
    chunks = getattr(lib, entry + "_chunks")(T, K, N)
    if chunks <= 0:
        raise RuntimeError("token_wgrad: unsupported problem")
    cols = N * K + (N if bias else 0)
    cuda = x2.is_cuda
    from . import chunk_sums
    batched = _chunk_sum_route(chunk_sums, cuda, cols, dtype)
    if cuda and _backend is None and not batched:
        from . import _workspace as W_
        part = W_.get("conv_wgrad", x2.device, chunks * cols * 4).view(torch.float32)[:chunks * cols]
    else:                                            # (a deferred sum reads its partials later: they get a buffer of their own)
        part = torch.empty(chunks * cols, dtype=torch.float32, device=x2.device)
    from .small_wgrad_ext import MAX_ROWS
    if GROUPED and batched and x2.dtype == torch.bfloat16 and T <= MAX_ROWS and chunk_sums.deferring_producers():
        # a short token axis: the launch is nearly all boundary and nothing waits for it -- it goes out with the next flush, grouped
        chunk_sums.register_producer(x2, dy2, part, bias)
    else:
        rc = getattr(lib, entry)(x2.data_ptr(), dy2.data_ptr(), part.data_ptr(), part.numel(), T, K, N, 1 if bias else 0,
                                 x2.device.index if cuda else -1, torch.cuda.current_stream(x2.device).cuda_stream if cuda else None)
        if rc != 0:
            _capi.check(rc, entry)
    part = part.view(chunks, cols)
    if batched:
        both = chunk_sums.chunk_sum(part, dtype)     # one launch for all the iteration's weight gradients (chunk_sums.flush)
    elif cuda and _backend is None:
        from .colsum_ext import column_sum, supported as colsum_ok
        out_dt = dtype if dtype in (torch.float32, torch.bfloat16) else torch.float32
        both = (column_sum(part, out_dtype=out_dt) if colsum_ok(part) else part.sum(0)).to(dtype)
    else:
        both = part.sum(0).to(dtype)
    return both[:N * K].view(N, K), (both[N * K:] if bias else None)


def token_supported(x2, dy2):
    """bf16 token matrices with contiguous rows whose widths are multiples of 8 (csrc/twgrad.hip).  With MDETR_TUNE="twgrad=0" (tests: the
    1x1 case of csrc/conv_wgrad.hip behind the same entry point) that kernel's narrower rules apply."""
    T = x2.shape[0]
    ok = (TOKEN_ROUTE and (ENABLED or _backend is not None) and x2.dtype == torch.bfloat16 and dy2.dtype == torch.bfloat16 and x2.is_contiguous()
          and dy2.is_contiguous() and (x2.is_cuda or _backend is not None) and x2.data_ptr() % 16 == 0 and dy2.data_ptr() % 16 == 0
          and T * max(x2.shape[1], dy2.shape[1]) * 2 < (1 << 31))
    from . import _tune
    if _tune.get("twgrad") == "0":
        # (narrow outputs waste that kernel's 128-row dy block; a weight of more than 64 (128 x 64) blocks leaves too few chunks)
        return ok and T % 8 == 0 and x2.shape[1] % 64 == 0 and dy2.shape[1] % 32 == 0 and dy2.shape[1] >= 128 \
            and ((dy2.shape[1] + 127) // 128) * (x2.shape[1] // 64) <= 64
    return ok and x2.shape[1] % 8 == 0 and dy2.shape[1] % 8 == 0


def token_supported_f32(x2, dy2):
    """fp32 token matrices with contiguous rows whose widths are multiples of 8 (the fp32 form of csrc/twgrad.hip), with the family
    MDETR_TWGRAD_F32 on -- also under the emulated kernel (tests): the family alone decides, so that fp32 layers keep the library route without it."""
    T = x2.shape[0]
    return (TOKEN_ROUTE and ENABLED_F32 and x2.dtype == torch.float32 and dy2.dtype == torch.float32 and x2.dim() == 2
            and dy2.dim() == 2 and T > 0 and x2.is_contiguous() and dy2.is_contiguous() and (x2.is_cuda or _backend is not None)
            and x2.data_ptr() % 16 == 0 and dy2.data_ptr() % 16 == 0 and T * max(x2.shape[1], dy2.shape[1]) < (1 << 29)
            and x2.shape[1] % 8 == 0 and dy2.shape[1] % 8 == 0 and x2.shape[1] > 0 and dy2.shape[1] > 0)


def _stolen(like, N, C, k):
    """Does AccumulateGrad keep a [N, C, k, k] gradient with channels_last strides for the leaf ``like`` as it is (same strides wherever a
    dimension is longer than 1)?  Otherwise it copies the gradient into the parameter's layout -- it READS it inside the backward pass."""
    if like is None or not like.is_leaf:
        return True                                  # (an intermediate -- a folded weight --: its consumer flushes before it reads)
    want = (k * k * C, 1, k * C, C)
    return tuple(like.shape) == (N, C, k, k) and all(n == 1 or a == b for n, a, b in zip(like.shape, like.stride(), want))


def weight_gradient(x, dy, k, stride, dtype=torch.bfloat16, like=None):
    """x [B, C, H, W], dy [B, N, OH, OW] (channels_last, both bf16 or -- k = 3, stride 1 or 2 -- both fp32) -> dW [N, C, k, k] in ``dtype``
    (channels_last strides).
    like: the weight the gradient is for; a leaf whose strides are not the result's gets its sum at once, never deferred (chunk_sums.py)."""
    B, C, H, W = x.shape
    _, N, OH, OW = dy.shape
    lib = _lib()
    if x.dtype != dy.dtype or x.dtype not in (torch.bfloat16, torch.float32):
        raise RuntimeError("conv_wgrad: operands of one dtype, bf16 or fp32 (got %s, %s)" % (x.dtype, dy.dtype))
    # fp32 operands: the fp32 forms of the kernel (three-way bf16 split; 3x3 / stride 2 has an entry of its own), same partials and chunk sums
    entry = "mdetr_conv_wgrad" if x.dtype != torch.float32 else "mdetr_conv_wgrad_s2_f32" if (k, stride) == (3, 2) else "mdetr_conv_wgrad_f32"
    chunks = getattr(lib, entry + "_chunks")(B, H, W, C, OH, OW, N, k, stride)
    if chunks <= 0:
        raise RuntimeError("conv_wgrad: unsupported problem")
    cols = N * k * k * C
    cuda = x.is_cuda
    from . import chunk_sums
    batched = _chunk_sum_route(chunk_sums, cuda, cols, dtype)
    if cuda and _backend is None and not batched:
        from . import _workspace as W_
        part = W_.get("conv_wgrad", x.device, chunks * cols * 4).view(torch.float32)[:chunks * cols]
    else:
        part = torch.empty(chunks * cols, dtype=torch.float32, device=x.device)
    rc = getattr(lib, entry)(x.data_ptr(), dy.data_ptr(), part.data_ptr(), part.numel(), B, H, W, C, OH, OW, N, k, stride,
                             x.device.index if cuda else -1, torch.cuda.current_stream(x.device).cuda_stream if cuda else None)
    if rc != 0:
        _capi.check(rc, entry)
    part = part.view(chunks, cols)
    if batched:
        dw = chunk_sums.chunk_sum(part, dtype, defer=_stolen(like, N, C, k))
    elif cuda and _backend is None:
        from .colsum_ext import column_sum, supported as colsum_ok
        out_dt = dtype if dtype in (torch.float32, torch.bfloat16) else torch.float32
        dw = (column_sum(part, out_dtype=out_dt) if colsum_ok(part) else part.sum(0)).to(dtype)
    else:
        dw = part.sum(0).to(dtype)
    return dw.view(N, k, k, C).permute(0, 3, 1, 2)                       # [N, C, k, k] with channels_last strides
