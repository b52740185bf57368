"""The chunk sums of the split weight-gradient kernels (csrc/twgrad.hip, csrc/conv_wgrad.hip), batched.

Those kernels cut their contraction over the tokens / pixels into chunks and leave fp32 partials ``[chunks, cols]`` that are added
in chunk order (deterministic, one rounding).  Added right away that is one small launch per weight gradient -- 159 of them in the
round-5 iteration, ~6 us each, mostly fill and drain.  Inside ``deferred()`` (``helpers/step_helper.TrainIteration`` wraps every
backward call in it) the sum is only REGISTERED: the caller gets the result tensor at once, its values arrive with ``flush()`` --
ONE launch of ``mdetr_chunk_sums`` for up to 48 gradients -- when the context closes, or earlier where something reads a deferred
result (the frozen-BN unfold of the backbone's weight gradients, monodetr/backbone.py).  The arithmetic is the same sum in the same
order.  Outside the context every sum runs immediately.

What makes the deferral safe -- the invariant, and who enforces it.  A registered result may be HELD but not READ before its flush.
Autograd holds it: a weight gradient leaves its autograd function only towards the parameter's AccumulateGrad node, which stores
the tensor without reading it -- provided the parameter has no ``.grad`` yet, carries no hook, and has the strides of the arriving
gradient.  Everything else reads, and is closed in one of three ways:

* the readers inside the product's own backward functions (the frozen-BN unfold, the decoder's concatenations, the fp32-bias
  conversion of monodetr/linear.py) call ``flush()`` first;
* ``deferred(module)`` -- the form ``TrainIteration._backward`` / ``_backward_backbone`` use -- asks ``reader_inside_backward``
  before it opens: a DistributedDataParallel wrapper (its reducer copies every gradient into a bucket as it arrives), a parameter
  with a tensor hook or a post-accumulate hook (``dist_helper.BucketedGradSync`` hangs one on every parameter), a parameter that
  still has a ``.grad`` (AccumulateGrad adds into it) turn the deferral OFF for that backward pass: every sum is then launched at
  once, as outside the context.  The second half of a cut backward pass (``held="verify"``) legitimately starts with the first
  half's gradients in place; it defers, and raises afterwards if one of those was accumulated into;
* ``conv_wgrad_ext.weight_gradient(..., like=weight)`` computes at once the gradient of a leaf weight whose strides differ from the
  channels-last result's (AccumulateGrad would copy it into the parameter's layout).

The PRODUCERS of the short partial sets are deferred too (family MDETR_TWGRAD_GROUPED).  A token weight gradient over at most
``small_wgrad_ext.MAX_ROWS`` rows of bf16 operands (the decoder's 4 400-row layers, layer4's 3 840-row products: ~30 launches of ~11 us
per step, nine tenths of each fill, drain and launch boundary) is, inside ``deferred()``, only REGISTERED as well
(``register_producer``): ``flush()`` first sends every registered producer -- ``mdetr_token_wgrad_grouped``, one launch per kernel
instantiation and per 32 jobs, each job planned as a launch of its own, so the partials have the same bits -- and then the sums that
read them.  Every ``flush()`` that guaranteed values to a reader before still does.  Longer token axes stay launched at once: their
kernels are 20 - 45 us of real work, and holding their 42 - 126 MB operands until a flush would cost the captured graph's pool
gigabytes for ~2 us each.

The second invariant, which the deferred producers add.  A registered OPERAND (x2, dy2) may be held but must not be WRITTEN before its
flush.  The registration keeps both alive, so their storage cannot be handed out again by the allocator; what remains is a writer in
place.  The audit of the backward pass (round 17), writer by writer:

* ``tgemm``'s accumulating form (``res is out``) is used by tools/gemmbench.py only; ``linear._input_gradient`` adds the residual
  path's gradient inside the product but writes a NEW tensor, and so do the masked tails (``tgemm_masked``), ``bias_act_ext``'s
  backward (``dx = empty_like(y)``; a badly laid out ``dy`` is COPIED), the LayerNorm, attention, MSDA and convolution backwards;
* the shared scratch buffers of ``_workspace`` hold partials and kernel workspaces, never a tensor that travels as a gradient or is
  saved for backward, so no operand lives in memory that a later call reuses;
* the forward pass's in-place ReLUs (backbone.py) have run before the backward pass begins, and a saved activation is not written
  afterwards (autograd's version counter would raise for the framework's own functions);
* the autograd engine adds gradients in place only into a buffer it holds the SOLE reference to, and only while a node's inputs are
  still being collected: a gradient has its final value when its node runs, and from then on the registration holds a second
  reference, so a later fan-in sum that meets the same tensor (a backward that passes its gradient through) is computed out of place.

``VERIFY`` (tests) keeps a clone of both operands at registration and raises at the flush unless each still equals its clone;
tests/test_twgrad_grouped_routing_cpu.py holds the routing on the emulated kernels, tests/test_twgrad_grouped_gpu.py runs a token MLP and
a decoder layer with POISON and VERIFY on.

The flat and the two-part gradient exchange (``FlatGradSync``, ``SplitGradSync``) and the optimizer run after the context has closed.
A bare ``deferred()`` checks nothing: the caller vouches for its consumers.  tests/test_deferred_sums_emulated_cpu.py holds the
invariant for every consumer on the CPU emulation of the kernels, tests/test_grad_exchange_gpu.py for the exchanges of the whole
model."""
import ctypes
import os
import threading

import torch

from . import _capi

# MDETR_CHUNK_SUMS=1 (kernel_families decides): batch the sums; off = every sum its own launch, as in round 5
ENABLED = os.environ.get("MDETR_CHUNK_SUMS") == "1"
# tests: a registered result is filled with NaN until its flush, so that anything reading it too early shows (a recycled buffer
# otherwise tends to hold last iteration's -- plausible -- values)
POISON = False
# tests: a registered producer keeps a clone of both operands; the flush raises unless they still equal them (the second invariant)
VERIFY = False
# tests: every sum at once, through the same kernel (the reference the batched results must equal bit for bit)
IMMEDIATE = False
_backend = None               # tests substitute the CPU emulation of the same kernel source (tests/native_emul.py)
_lock = threading.RLock()     # (registrations come from autograd's device thread, flush() from either)
_depth = 0
_pending = []                 # (part [chunks, cols] fp32, out [cols]); both stay referenced until the flush
_producers = []               # (x2 [T, K] bf16, dy2 [T, N] bf16, part fp32 [chunks * cols], bias, clones or None); all referenced until the flush


class _Job(ctypes.Structure):
    _fields_ = [("part", ctypes.c_void_p), ("out", ctypes.c_void_p), ("cols", ctypes.c_int64), ("chunks", ctypes.c_int32), ("out_dtype", ctypes.c_int32)]


class _PitchedJob(ctypes.Structure):
    """mdetr_chunk_job_pitched: a column range [chunks, cols] of a wider partial set whose rows are `pitch` floats apart."""
    _fields_ = [("part", ctypes.c_void_p), ("out", ctypes.c_void_p), ("cols", ctypes.c_int64), ("pitch", ctypes.c_int64), ("chunks", ctypes.c_int32),
                ("out_dtype", ctypes.c_int32)]


class _TwgradJob(ctypes.Structure):
    """mdetr_twgrad_job"""
    _fields_ = [("x", ctypes.c_void_p), ("dy", ctypes.c_void_p), ("part", ctypes.c_void_p), ("part_elems", ctypes.c_int64), ("T", ctypes.c_int64),
                ("K", ctypes.c_int32), ("N", ctypes.c_int32), ("with_bias", ctypes.c_int32), ("pad_", ctypes.c_int32)]


def _pitch(part):
    return part.stride(0) if part.shape[0] > 1 else part.shape[1]


def _lib():
    return _backend if _backend is not None else _capi.lib()


def supported(part, out_dtype):
    """Contiguous fp32 partials [chunks, cols], or a column range of such a set (``wide[:, c0:c0 + cols]``: unit column stride, rows a
    multiple of 4 floats apart, the first element 16-byte aligned)."""
    return ((part.is_cuda or _backend is not None) and part.dim() == 2 and part.dtype == torch.float32 and part.shape[0] > 0
            and part.shape[1] > 0 and part.shape[1] % 4 == 0 and part.stride(1) == 1 and _pitch(part) % 4 == 0 and _pitch(part) >= part.shape[1]
            and part.data_ptr() % 16 == 0 and out_dtype in (torch.float32, torch.bfloat16))


def _launch(jobs):
    pitched = any(_pitch(part) != part.shape[1] for part, _ in jobs)
    arr = ((_PitchedJob if pitched else _Job) * len(jobs))()
    for q, (part, out) in zip(arr, jobs):
        q.part, q.out, q.cols, q.chunks = part.data_ptr(), out.data_ptr(), part.shape[1], part.shape[0]
        q.out_dtype = _capi.MDETR_BF16 if out.dtype == torch.bfloat16 else _capi.MDETR_F32
        if pitched:
            q.pitch = _pitch(part)
    dev = jobs[0][0].device
    entry = _lib().mdetr_chunk_sums_pitched if pitched else _lib().mdetr_chunk_sums
    rc = entry(ctypes.cast(arr, ctypes.c_void_p), len(jobs), dev.index if dev.type == "cuda" else -1,
               torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else None)
    if rc != 0:
        msg = _lib().mdetr_last_error()
        raise RuntimeError("mdetr_chunk_sums failed (code %d): %s" % (rc, msg.decode() if msg else "?"))


def _launch_producers(jobs):
    """One call of mdetr_token_wgrad_grouped for the registered producers of one device (on the current stream)."""
    arr = (_TwgradJob * len(jobs))()
    for q, (x2, dy2, part, bias, _) in zip(arr, jobs):
        q.x, q.dy, q.part, q.part_elems = x2.data_ptr(), dy2.data_ptr(), part.data_ptr(), part.numel()
        q.T, q.K, q.N, q.with_bias = x2.shape[0], x2.shape[1], dy2.shape[1], 1 if bias else 0
    dev = jobs[0][0].device
    rc = _twgrad_lib().mdetr_token_wgrad_grouped(ctypes.cast(arr, ctypes.c_void_p), len(jobs), dev.index if dev.type == "cuda" else -1,
                                                 torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else None)
    if rc != 0:
        msg = _twgrad_lib().mdetr_last_error()
        raise RuntimeError("mdetr_token_wgrad_grouped failed (code %d): %s" % (rc, msg.decode() if msg else "?"))


def _twgrad_lib():
    """The library the producers' single launches come from (conv_wgrad_ext's: tests substitute the emulation there)."""
    from . import conv_wgrad_ext
    return conv_wgrad_ext._lib()


def deferring_producers():
    """Would ``register_producer`` hold a producer until the next flush?  (As ``chunk_sum`` decides for the sums: the family on, inside
    ``deferred()``, not in the tests' IMMEDIATE mode -- a sum that runs at once needs its partials at once.)"""
    return ENABLED and _depth > 0 and not IMMEDIATE


def register_producer(x2, dy2, part, bias):
    """The token weight gradient of (x2 [T, K], dy2 [T, N]) -- bf16, contiguous -- into the partials `part` (fp32, a tensor of its own of
    mdetr_token_wgrad_chunks(T, K, N) * (N K + (N if bias))) floats), launched with the next ``flush()`` ahead of the sums.  The caller
    has asked ``deferring_producers()`` and registers the chunk sum of `part` right after.  The operands must not be written before the
    flush (the second invariant, module docstring)."""
    with _lock:
        _producers.append((x2, dy2, part, bool(bias), (x2.clone(), dy2.clone()) if VERIFY else None))


def chunk_sum(part, out_dtype=torch.float32, defer=True):
    """part [chunks, cols] fp32 -> [cols] in out_dtype = the chunks added in order.  Inside ``deferred()`` the values arrive at the
    next ``flush()``; `part` must then be a tensor of its own (not a shared scratch buffer): it is read later.  defer=False: this
    sum now, whatever the context (its consumer reads it inside the backward pass).  `part` may be a column range of a wider set
    (the LayerNorm sites' gamma / beta halves, add_ln_ext.py): each range gets a result tensor of its own.  More than 128 chunks
    are added by 32 row lanes (csrc/colsum.hip); which form a job takes depends on its chunk count alone, deferred or not."""
    if not supported(part, out_dtype):
        raise RuntimeError("chunk_sum: needs fp32 partials [chunks, cols] (contiguous, or a column range of such), cols a multiple of 4, 16-byte aligned")
    out = torch.empty(part.shape[1], dtype=out_dtype, device=part.device)
    with _lock:
        if defer and ENABLED and _depth > 0 and not IMMEDIATE:
            if POISON:
                out.fill_(float("nan"))
            _pending.append((part, out))
            return out
    _launch([(part, out)])
    return out


def deferring():
    return ENABLED and _depth > 0


def flush():
    """Compute every registered sum now (on the current stream of the calling thread -- the stream the producers ran on): first the
    registered producers, grouped, then the sums that read their partials."""
    with _lock:
        prods = list(_producers)
        del _producers[:]
        jobs = list(_pending)
        del _pending[:]
    if prods:
        for x2, dy2, _, _, clones in prods:
            if clones is not None and not (torch.equal(x2, clones[0]) and torch.equal(dy2, clones[1])):
                raise RuntimeError("chunk_sums.flush: an operand of a registered weight gradient was written between its registration and the flush")
        by_dev = {}
        for j in prods:
            by_dev.setdefault(j[0].device, []).append(j)
        for group in by_dev.values():
            _launch_producers(group)
    if jobs:
        by_dev = {}
        for j in jobs:
            by_dev.setdefault(j[0].device, []).append(j)
        for group in by_dev.values():
            _launch(group)


def reader_inside_backward(module=None, params=None, held="refuse"):
    """Why the chunk sums of a backward pass into ``module``'s (or ``params``') parameters must NOT be deferred -- a short reason --,
    or None: nothing that is visible from here reads a weight gradient before the flush.  held="verify": parameters that already
    have a ``.grad`` are not a reason (``deferred`` checks afterwards that none of them was touched)."""
    if module is not None:
        from torch.nn.parallel import DistributedDataParallel
        if isinstance(module, DistributedDataParallel):
            return "DistributedDataParallel copies each gradient into its bucket during the backward pass"
        if params is None:
            params = module.parameters()
    for p in params or ():
        if not p.requires_grad:
            continue
        if p._backward_hooks or p._post_accumulate_grad_hooks:
            return "a parameter carries a gradient hook"
        if held == "refuse" and p.grad is not None:
            return "a parameter still has a .grad: the new gradient is added to it during the backward pass"
    return None


class deferred:
    """``with deferred(model): loss.backward()`` -- chunk sums registered inside are computed together when the block ends (also when
    it ends with an exception: no registered result stays unwritten).  With ``module`` / ``params`` the block defers only if
    ``reader_inside_backward`` finds no reason against it (``self.reason``); otherwise it changes nothing and every sum inside is
    launched at once.  held="verify" (the second half of a cut backward pass): gradients that exist already must come out of the
    block untouched -- a parameter that received gradient in both halves was accumulated from an unwritten sum, and that raises."""

    def __init__(self, module=None, params=None, held="refuse"):
        self.reason = None
        self._held = ()
        if (module is not None or params is not None) and ENABLED and not IMMEDIATE:       # (nothing is deferred otherwise: nothing to ask)
            params = list(module.parameters() if params is None else params)
            self.reason = reader_inside_backward(module, params, held)
            if self.reason is None and held == "verify":
                self._held = [(p, p.grad, p.grad._version) for p in params if p.requires_grad and p.grad is not None]

    def __enter__(self):
        global _depth
        if self.reason is None:
            with _lock:
                _depth += 1
        return self

    def __exit__(self, *exc):
        global _depth
        if self.reason is not None:
            return False
        with _lock:
            _depth -= 1
            last = _depth == 0
        if last:
            flush()
        if exc[0] is None and any(p.grad is not g or g._version != v for p, g, v in self._held):
            raise RuntimeError("chunk_sums.deferred(held='verify'): a parameter that had a gradient before this backward pass received "
                               "another one inside it -- it was added from a sum that was not computed yet")
        return False
