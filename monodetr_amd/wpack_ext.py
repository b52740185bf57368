"""``pack_sites`` / ``level_positions``: the per-iteration re-assembly of parameters as ONE launch each (csrc/wpack.hip through
``mdetr_pack_params`` / ``mdetr_level_pos``).

The transformer packs projections that act on the same input into one GEMM: every ``MSDeformAttn`` concatenates its sampling-offset
and attention-weight projections (256 + 128 rows, monodetr/ops/modules/ms_deform_attn.py), every decoder layer sums its content and
position projections in weight space and concatenates the two sums (monodetr/depthaware_transformer.py).  As framework calls that
is two ``cat`` per deformable-attention module and four ``add`` + two ``cat`` per decoder layer, every forward pass, for tensors that only
change in the optimizer step: 30 launches of ~5 us.  Here every row block of every packed parameter is one JOB of a grouped
elementwise kernel -- ``dst = src0`` or ``dst = src0 + src1``, rounded once, bit for bit what ``cat`` / ``+`` give -- and the whole
forward pass takes one launch.  The backward computes nothing: each source gets the row block of the packed gradient as a view.

``level_positions``: the encoder's position tensor cat_l(sine_l + level_embed[l]) as ONE [S, C] tensor from one launch; with an
unpadded batch and the (cached, constant) sine encoding it is the same for every image, so the batch axis is a stride-0 view."""
import ctypes
import os

import torch

from . import _capi

# MDETR_PARAM_PACK=1 (kernel_families decides: committed)
ENABLED = os.environ.get("MDETR_PARAM_PACK") == "1"
_backend = None      # tests substitute the same kernel source built for the host (tests/native_emul.py)
MAX_LEVELS = 8       # level boundaries travel as kernel arguments (csrc/wpack.h: kPosLevels)


class _Job(ctypes.Structure):
    """mdetr_pack_job (include/monodetr_amd.h)"""
    _fields_ = [("dst", ctypes.c_void_p), ("src0", ctypes.c_void_p), ("src1", ctypes.c_void_p), ("elements", ctypes.c_int64),
                ("dtype", ctypes.c_int32), ("reserved", ctypes.c_int32)]


def _lib():
    return _backend if _backend is not None else _capi.lib()


def _code(dtype):
    return _capi.MDETR_BF16 if dtype == torch.bfloat16 else _capi.MDETR_F32


def _where(t):
    cuda = t.is_cuda
    return (t.device.index if cuda else -1), (torch.cuda.current_stream(t.device).cuda_stream if cuda else None)


def available(like):
    """Is the family on and `like` where the kernels run (the device, or the host with the emulated library)?"""
    return ENABLED and (like.is_cuda or _backend is not None) and not torch.is_autocast_enabled()


def blocks_supported(blocks):
    """blocks: the row blocks of ONE packed tensor, each a tuple of one source or of two to be added: dense bf16 / fp32 tensors of one
    dtype on one device with the same trailing shape, the members of a pair of the same shape."""
    first = blocks[0][0]
    for block in blocks:
        if len(block) not in (1, 2) or block[-1].shape != block[0].shape:
            return False
        for t in block:
            if not (t.dtype == first.dtype and t.dtype in (torch.float32, torch.bfloat16) and t.device == first.device and t.dim() >= 1
                    and t.shape[1:] == first.shape[1:] and t.is_contiguous() and (t.is_cuda or _backend is not None)):
                return False
    return True


def launch(jobs):
    """jobs: [(dst, src0, src1 or None)] -- dense tensors of one dtype per job; dst may be a row block of a larger tensor."""
    arr = (_Job * len(jobs))()
    for q, (dst, src0, src1) in zip(arr, jobs):
        q.dst, q.src0, q.src1 = dst.data_ptr(), src0.data_ptr(), (src1.data_ptr() if src1 is not None else None)
        q.elements, q.dtype, q.reserved = src0.numel(), _code(dst.dtype), 0
    device, stream = _where(jobs[0][0])
    rc = _lib().mdetr_pack_params(ctypes.cast(arr, ctypes.c_void_p), len(jobs), device, stream)
    if rc != 0:
        msg = _lib().mdetr_last_error()
        raise RuntimeError("mdetr_pack_params failed (code %d): %s" % (rc, msg.decode() if msg else "?"))


class _PackParams(torch.autograd.Function):
    """plan: per packed tensor the row blocks as tuples of one or two indices into `params`.  -> the packed tensors, new
    allocations every call (a saved packed weight must not alias the next iteration's).  Backward: block r of a packed gradient,
    as a view, to the block's source -- to both members of a summed pair, each its own view of the same rows (as `_SummedPair`).
    `chunk_sums.flush()` first, where `_SummedPair` has it: a packed gradient may be a registered, not yet computed chunk sum.
    A packed tensor nobody used (the decoder's, when only the encoder ran) has no gradient: its sources get None."""

    @staticmethod
    def forward(ctx, plan, *params):
        outs, jobs = [], []
        for blocks in plan:
            like = params[blocks[0][0]]
            out = torch.empty((sum(params[b[0]].shape[0] for b in blocks),) + tuple(like.shape[1:]), dtype=like.dtype, device=like.device)
            row = 0
            for b in blocks:
                n = params[b[0]].shape[0]
                jobs.append((out[row:row + n], params[b[0]], params[b[1]] if len(b) == 2 else None))
                row += n
            outs.append(out)
        launch(jobs)
        ctx.plan = plan
        ctx.rows = [[params[b[0]].shape[0] for b in blocks] for blocks in plan]
        ctx.nparams = len(params)
        ctx.set_materialize_grads(False)
        return tuple(outs)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *gouts):
        from . import chunk_sums
        chunk_sums.flush()
        grads = [None] * ctx.nparams
        for blocks, rows, g in zip(ctx.plan, ctx.rows, gouts):
            if g is None:
                continue
            row = 0
            for b, n in zip(blocks, rows):
                for i in b:
                    grads[i] = g[row:row + n]     # a view of its own per source: AccumulateGrad clones a tensor something else holds
                row += n
        return (None,) + tuple(grads)


def pack_sites(sites):
    """sites: [(key, weight_blocks, bias_blocks)] with the blocks as `blocks_supported` takes them.  -> {key: (weight, bias)} for
    the sites the kernel takes (the others keep their own code), all from ONE launch."""
    params, plan, keys = [], [], []
    for key, wblocks, bblocks in sites:
        if not (blocks_supported(wblocks) and blocks_supported(bblocks)):
            continue
        for blocks in (wblocks, bblocks):
            idx = []
            for block in blocks:
                idx.append(tuple(range(len(params), len(params) + len(block))))
                params.extend(block)
            plan.append(tuple(idx))
        keys.append(key)
    if not keys:
        return {}
    outs = _PackParams.apply(tuple(plan), *params)
    return {key: (outs[2 * i], outs[2 * i + 1]) for i, key in enumerate(keys)}


def level_pos_supported(sine, level_embed, counts, out_dtype):
    """sine [S, C] and level_embed [L, C], fp32 / bf16 (dense), S == sum(counts), L == len(counts) <= 8, C a multiple of 8, 16-byte
    aligned tensors, fp32 / bf16 result."""
    return (available(sine) and sine.dtype in (torch.float32, torch.bfloat16) and sine.dim() == 2 and sine.is_contiguous()
            and level_embed.dim() == 2 and level_embed.is_contiguous() and level_embed.device == sine.device
            and level_embed.dtype in (torch.float32, torch.bfloat16) and out_dtype in (torch.float32, torch.bfloat16)
            and level_embed.shape == (len(counts), sine.shape[1]) and 0 < len(counts) <= MAX_LEVELS and sum(counts) == sine.shape[0]
            and all(n > 0 for n in counts) and sine.shape[1] % 8 == 0 and sine.data_ptr() % 16 == 0 and level_embed.data_ptr() % 16 == 0)


@torch.no_grad()
def level_positions(sine, level_embed, counts, out_dtype):
    """-> [S, C] in out_dtype: out[s] = sine[s] + level_embed[level of s], bit for bit ``(sine_l + level_embed[l]).to(out_dtype)``."""
    out = torch.empty(sine.shape, dtype=out_dtype, device=sine.device)
    device, stream = _where(sine)
    rc = _lib().mdetr_level_pos(sine.data_ptr(), _code(sine.dtype), level_embed.data_ptr(), _code(level_embed.dtype), out.data_ptr(), _code(out_dtype),
                                (ctypes.c_int64 * len(counts))(*counts), len(counts), sine.shape[1], device, stream)
    if rc != 0:
        msg = _lib().mdetr_last_error()
        raise RuntimeError("mdetr_level_pos failed (code %d): %s" % (rc, msg.decode() if msg else "?"))
    return out
