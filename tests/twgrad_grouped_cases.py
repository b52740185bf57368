"""Job lists and checks for mdetr_token_wgrad_grouped (csrc/twgrad.hip's grouped kernel): test infrastructure, shared by
tests/test_twgrad_grouped_emulated_cpu.py (the kernel source on the HIP-on-CPU shim) and tests/test_twgrad_grouped_gpu.py.

What can go wrong in a grouped launch and is put here on purpose: a workgroup finding the wrong job or the wrong index inside it (jobs
of different grids, one of them with dead workgroups: a chunk count that is no multiple of 8), a job table longer than one launch
holds (kTwgradJobs + 1 jobs), jobs of different kernel instantiations in one call (each its own launch, in an order that is not the
caller's), the two-wave-group instantiation (MDETR_TUNE twgrad_kg=2), ragged last slabs and ragged column tiles.

The checks: the partials of a grouped call are ``torch.equal`` to those of one mdetr_token_wgrad call per job -- directly and after
mdetr_chunk_sums, fp32 and bf16 --, and on small-integer operands (tests/exact_cases.py: every partial sum an integer below 2^24,
exact in fp32 in any order) the summed result equals the fp64 product rounded once."""
import ctypes

import torch

import exact_cases as E

K_TWGRAD_JOBS = 32                    # csrc/twgrad.hip's kTwgradJobs
TS = (1024, 1031, 1100)               # exactly 32 slabs; a ragged last slab; 35 slabs -> 7 chunks of 5: one dead workgroup in eight
KNS = ((64, 64), (128, 64), (256, 256), (136, 72))      # 64 x 64; 64 (n) x 128 (c); 128 x 128, four tiles; 128 x 128, two tiles, ragged in both

# (T, K, N, with_bias)
ALL_SHAPES = [(T, K, N, (i + j) % 2 == 0) for i, T in enumerate(TS) for j, (K, N) in enumerate(KNS)]
ALL_SHAPES_OTHER_BIAS = [(T, K, N, not b) for T, K, N, b in ALL_SHAPES if (K, N) != (256, 256)]
# the four instantiations of one wave group interleaved (64 -> 128 is the fourth: 128 (n) x 64 (c)), so no launch has the caller's order
MIXED = [(1100, 64, 64, True), (1024, 256, 256, False), (1031, 128, 64, True), (1024, 64, 128, True), (1100, 136, 72, True),
         (1031, 64, 64, False), (1100, 64, 128, False), (1024, 128, 64, False)]
ONE_MORE_THAN_THE_CAP = [(1100 if i % 3 == 0 else 1024, 64, 64, i % 2 == 0) for i in range(K_TWGRAD_JOBS + 1)]
DEAD_WORKGROUPS = [(1100, 64, 64, True), (1024, 64, 64, True), (1100, 64, 64, False)]
TWO_WAVE_GROUPS = [(1024, 256, 256, True), (1100, 136, 72, True), (1031, 256, 256, False)]


class Job(ctypes.Structure):
    """mdetr_twgrad_job"""
    _fields_ = [("x", ctypes.c_void_p), ("dy", ctypes.c_void_p), ("part", ctypes.c_void_p), ("part_elems", ctypes.c_int64), ("T", ctypes.c_int64),
                ("K", ctypes.c_int32), ("N", ctypes.c_int32), ("with_bias", ctypes.c_int32), ("pad_", ctypes.c_int32)]


def _where(dev):
    if dev.type == "cuda":
        return dev.index or 0, torch.cuda.current_stream(dev).cuda_stream
    return -1, None


def err(lib):
    return ctypes.string_at(lib.mdetr_last_error()).decode()


def operands(T, K, N, kind, dev):
    """kind "ints": tests/exact_cases.py's integer operands (shared, never written); "randn": N(0, 1) / N(0, 0.25) rounded to bf16."""
    if kind == "ints":
        x, dy = E.wgrad_operands(T, K, N)[:2]
    else:
        g = E.gen(T, K, N, 17)
        x, dy = torch.randn(T, K, generator=g).to(E.BF16), (torch.randn(T, N, generator=g) * 0.5).to(E.BF16)
    return x.to(dev), dy.to(dev)


def chunks_of(lib, T, K, N):
    c = lib.mdetr_token_wgrad_chunks(T, K, N)
    assert c >= 1
    return c


def single(lib, dev, x, dy, bias):
    """One mdetr_token_wgrad call -> partials [chunks, N K (+ N)]."""
    (T, K), N = x.shape, dy.shape[1]
    part = torch.full((chunks_of(lib, T, K, N), N * K + (N if bias else 0)), float("nan"), device=dev)
    idx, stream = _where(dev)
    rc = lib.mdetr_token_wgrad(x.data_ptr(), dy.data_ptr(), part.data_ptr(), part.numel(), T, K, N, 1 if bias else 0, idx, stream)
    assert rc == 0, err(lib)
    return part


def grouped(lib, dev, ops):
    """One mdetr_token_wgrad_grouped call for [(x, dy, bias)] -> the jobs' partials."""
    parts, arr = [], (Job * len(ops))()
    for q, (x, dy, bias) in zip(arr, ops):
        (T, K), N = x.shape, dy.shape[1]
        part = torch.full((chunks_of(lib, T, K, N), N * K + (N if bias else 0)), float("nan"), device=dev)
        parts.append(part)
        q.x, q.dy, q.part, q.part_elems, q.T, q.K, q.N, q.with_bias = x.data_ptr(), dy.data_ptr(), part.data_ptr(), part.numel(), T, K, N, 1 if bias else 0
    idx, stream = _where(dev)
    rc = lib.mdetr_token_wgrad_grouped(ctypes.cast(arr, ctypes.c_void_p), len(ops), idx, stream)
    assert rc == 0, err(lib)
    return parts


def summed(lib, dev, part, dtype):
    """mdetr_chunk_sums on one partial set, at once (the chunk sum the step registers behind the producer)."""
    from monodetr_amd import chunk_sums
    was = chunk_sums._backend
    chunk_sums._backend = lib if dev.type == "cpu" else None
    try:
        return chunk_sums.chunk_sum(part, dtype, defer=False)
    finally:
        chunk_sums._backend = was


def check(lib, dev, jobs, kind, want_dead=False, want_launches=None):
    """The grouped call on `jobs` against one single call per job: equal partials, equal sums; kind "ints": the sums equal fp64."""
    ops = [operands(T, K, N, kind, dev) + (b,) for T, K, N, b in jobs]
    if want_dead:
        assert any(chunks_of(lib, T, K, N) % 8 for T, K, N, _ in jobs)                 # (the grid is rounded up to whole eights of chunks)
    got = grouped(lib, dev, ops)
    for (T, K, N, b), (x, dy, _), part in zip(jobs, ops, got):
        what = "T=%d K=%d N=%d bias=%s (%s)" % (T, K, N, b, kind)
        assert not torch.isnan(part).any(), what + ": a chunk left part of its partial unwritten"
        want = single(lib, dev, x, dy, b)
        assert torch.equal(part, want), what + ": partials differ from the single launch's"
        for dtype in (E.F32, E.BF16):
            s = summed(lib, dev, part, dtype)
            assert torch.equal(s, summed(lib, dev, want, dtype)), what
            if kind == "ints":
                _, _, rw, mw, rb, mb = E.wgrad_operands(T, K, N)
                E.assert_bits_equal(s[:N * K].view(N, K), E.expected(rw, mw, dtype, what=what), what + " dW -> %s" % dtype)
                if b:
                    E.assert_bits_equal(s[N * K:], E.expected(rb, mb, dtype, what=what), what + " db -> %s" % dtype)
    return got


def check_validation(lib, dev):
    """What the grouped entry refuses, with a message, before anything is launched: a null pointer, a short partial buffer, a shape
    the kernel does not take -- each in the LAST job of a list whose other jobs are fine."""
    good = [operands(1024, 64, 64, "randn", dev) + (True,), operands(1031, 64, 64, "randn", dev) + (False,)]
    idx, stream = _where(dev)

    def call(mutate):
        arr = (Job * len(good))()
        keep = []
        for q, (x, dy, bias) in zip(arr, good):
            (T, K), N = x.shape, dy.shape[1]
            part = torch.zeros((chunks_of(lib, T, K, N), N * K + (N if bias else 0)), device=dev)
            keep.append(part)
            q.x, q.dy, q.part, q.part_elems, q.T, q.K, q.N, q.with_bias = x.data_ptr(), dy.data_ptr(), part.data_ptr(), part.numel(), T, K, N, 1 if bias else 0
        mutate(arr[len(good) - 1])
        rc = lib.mdetr_token_wgrad_grouped(ctypes.cast(arr, ctypes.c_void_p), len(good), idx, stream)
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)
        return rc, err(lib), keep

    rc, msg, _ = call(lambda q: None)
    assert rc == 0, msg
    for field in ("x", "dy", "part"):
        rc, msg, keep = call(lambda q: setattr(q, field, None))
        assert rc != 0 and "null pointer" in msg, (field, rc, msg)
        assert all(float(p.abs().max()) == 0 for p in keep)                             # nothing ran: the first job's partials are untouched
    rc, msg, keep = call(lambda q: setattr(q, "part_elems", q.part_elems - 1))
    assert rc != 0 and "floats" in msg and "needed" in msg, (rc, msg)
    assert all(float(p.abs().max()) == 0 for p in keep)
    rc, msg, keep = call(lambda q: setattr(q, "K", 60))                                 # K % 8 != 0
    assert rc != 0 and msg, (rc, msg)
    rc, msg, keep = call(lambda q: setattr(q, "T", 0))
    assert rc != 0 and msg, (rc, msg)
    assert lib.mdetr_token_wgrad_grouped(None, 0, idx, stream) == 0                     # no jobs: nothing to do
    assert lib.mdetr_token_wgrad_grouped(None, 2, idx, stream) != 0
