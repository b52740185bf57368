"""Deferred chunk sums (monodetr_amd/chunk_sums.py) under EVERY way a weight gradient is consumed, on the real kernel sources
(csrc/twgrad.hip, csrc/conv_wgrad.hip, csrc/colsum.hip's mdetr_chunk_sums) running on the HIP-on-CPU shim, driven by the product's
``TrainIteration`` and its gradient exchanges (tests/deferred_stack.py: a Conv3x3, a strided convolution, three token-linear layers).

A deferred result is memory that is not written until the flush; ``chunk_sums.POISON`` fills it with NaN so that a reader inside the
backward pass shows.  For each consumer, three consecutive iterations (a reader that only exists from the second iteration on -- the
bucketed exchange's hooks, a retained ``.grad`` -- shows there):

* no gradient holds a non-finite value;
* deferred and immediate gradients are ``torch.equal``: the same kernel adds the same partials in the same order on one thread;
* the immediate run's weight gradients are held to fp64 products / ``gemm_bounds.conv2d_f64`` on the operands the kernels were given:
  |err| <= 2^-8 |ref| + 4 sqrt(K) 2^-23 mag  (one bf16 rounding of an fp32 accumulation of K exact products);
* what reached ``chunk_sums`` is what the case EXPECTS: "deferred" -- all five sums of a backward pass registered and computed by
  flushes of more than one job --, or "off" -- nothing registered, five launches of one job --: the consumer reads inside the
  backward pass and ``chunk_sums.deferred`` / ``conv_wgrad_ext.weight_gradient`` must have refused to defer for it."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

import deferred_stack as ds
import gemm_bounds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDER = ["lins.2", "lins.1", "lins.0", "down", "conv"]                # the order in which a backward pass produces the weight gradients


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _child(rank, consumer, port, out):
    """One rank, gloo: the exchanges need a process group; it lives and dies in this child process."""
    import sys
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1")
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        torch.save({mode: ds.run_case(consumer, mode) for mode in ("deferred", "immediate")}, out)
    finally:
        dist.destroy_process_group()


def both_modes(consumer, tmp_path, group):
    if not group:
        return {mode: ds.run_case(consumer, mode) for mode in ("deferred", "immediate")}
    out = os.path.join(str(tmp_path), "case.pt")
    mp.spawn(_child, args=(consumer, _free_port(), out), nprocs=1, join=True)
    return torch.load(out, weights_only=False)


def assert_reference(calls):
    """The results of the immediate run's weight-gradient calls against fp64 on the same bf16 operands."""
    assert [c[0] for c in calls] == ["token"] * ds.LINEARS + ["conv", "conv"]
    assert all(c[5] > 1 for c in calls), [c[5] for c in calls]       # every one of them is a sum over several chunks
    ulp = 2.0 ** -8
    for kind, x, dy, dw, extra, chunks in calls:
        if kind == "token":
            x64, dy64, K = x.double(), dy.double(), x.shape[0]
            ref, mag = dy64.t() @ x64, dy64.abs().t() @ x64.abs()
            rb, mb = dy64.sum(0), dy64.abs().sum(0)
            assert bool(((extra.double() - rb).abs() <= ulp * rb.abs() + 4 * K ** 0.5 * 2.0 ** -23 * mb + 1e-30).all()), "bias gradient"
        else:
            k, stride = extra
            K = dy.shape[0] * dy.shape[2] * dy.shape[3]
            w0 = torch.zeros(dy.shape[1], x.shape[1], k, k, dtype=torch.float64, requires_grad=True)
            ref, = torch.autograd.grad((gemm_bounds.conv2d_f64(x.double(), w0, stride=stride, padding=k // 2) * dy.double()).sum(), w0)
            mag, = torch.autograd.grad((gemm_bounds.conv2d_f64(x.double().abs(), w0, stride=stride, padding=k // 2) * dy.double().abs()).sum(), w0)
        assert dw.dtype == torch.bfloat16 and dw.shape == ref.shape
        err = (dw.double() - ref).abs()
        assert bool((err <= ulp * ref.abs() + 4 * K ** 0.5 * 2.0 ** -23 * mag + 1e-30).all()), (kind, float(err.max()))
        assert float(ref.abs().max()) > 0


def assert_case(res, expect, summed=False):
    """expect: per iteration "deferred" | "off" | (registered, launches).  summed: ``.grad`` accumulates over the iterations."""
    (gd, sd, nd), (gi, si, ni) = res["deferred"], res["immediate"]
    assert len(gd) == len(gi) == len(expect) >= 3
    assert nd["route"] == "_ConvStridedBackward" and nd["conv_route"] == "_Conv3x3Backward"      # the kernels' autograd functions, not the library's
    for it, want in enumerate(expect):
        assert set(gd[it]) == set(gi[it]) and len(gd[it]) == 2 * ds.SUMS
        bad = [n for n in gd[it] if not torch.isfinite(gd[it][n].float()).all()]
        assert not bad, "iteration %d: non-finite gradient in %s" % (it, bad)
        assert not [n for n in gi[it] if not torch.isfinite(gi[it][n].float()).all()]
        for n in gi[it]:
            assert torch.equal(gd[it][n], gi[it][n]), "iteration %d: %s differs between the deferred and the immediate run" % (it, n)
        got = (sd[it]["registered"], sd[it]["launches"])
        if want == "deferred":
            assert got[0] == ds.SUMS and sum(got[1]) == ds.SUMS and min(got[1]) > 1, got
        elif want == "off":
            assert got == (0, [1] * ds.SUMS), got
        else:
            assert got == want, got
        assert (si[it]["registered"], si[it]["launches"]) == (0, [1] * ds.SUMS)
        assert_reference(si[it]["calls"])
        # ... and those checked results are what the parameters hold
        for name, call in zip(ORDER, si[it]["calls"]):
            want_w = call[3] if not (summed and it) else None
            if want_w is not None:
                assert torch.equal(gi[it][name + ".weight"], want_w), name
    return gd, gi, nd


@pytest.mark.timeout(600)
@pytest.mark.parametrize("consumer,group,expect", [
    ("none", False, "deferred"),               # .grad cleared to None, nothing attached: AccumulateGrad takes the registered tensors over
    ("flat", True, "deferred"),                # FlatGradSync.sync() after the backward pass: after the flush
    ("split", True, "deferred"),               # SplitGradSync start / start / finish around the cut backward pass: each start after its flush
    ("bucketed", True, "off"),                 # BucketedGradSync: post-accumulate hooks read p.grad inside the backward pass
    ("ddp_view", True, "off"),                 # torch DDP, gradient_as_bucket_view=True: the reducer copies each gradient as it arrives
    ("ddp_copy", True, "off"),                 # ... and with gradient_as_bucket_view=False
    ("hooks", False, "off"),                   # a tensor hook on one weight, a post-accumulate hook reading p.grad on another
])
def test_every_consumer_of_the_gradients_sees_computed_sums(consumer, group, expect, tmp_path):
    res = both_modes(consumer, tmp_path, group)
    gd, gi, notes = assert_case(res, [expect] * 3)
    if consumer == "split":
        # the order of TrainIteration._step: [upper backward] start [backbone backward] start finish -- each half is one deferred block
        # whose flush comes before that half's start() reads the gradients: 3 sums above the cut, 2 below
        assert [seen["launches"] for seen in res["deferred"][1]] == [[ds.LINEARS, 2]] * 3
    if consumer == "bucketed":
        assert notes["buckets"] >= 2
    if consumer == "hooks":
        assert len(notes["hook_saw"]) == 3
        for it, seen in enumerate(notes["hook_saw"]):                  # what the hook read inside the backward pass is the gradient
            assert torch.equal(seen, gi[it]["lins.0.weight"])


def test_a_retained_grad_turns_the_deferral_off_for_the_passes_that_add_to_it():
    """Two more backward passes without clearing ``.grad``: AccumulateGrad adds the arriving gradient to the kept one -- a read.  The
    first pass (no .grad yet) defers, the following ones must not; the result is the sum of the single-pass gradients."""
    res = {mode: ds.run_case("retained", mode) for mode in ("deferred", "immediate")}
    gd, gi, _ = assert_case(res, ["deferred", "off", "off"], summed=True)
    single, _, _ = ds.run_case("none", "immediate")
    acc = {n: g.clone() for n, g in single[0].items()}
    for it in (1, 2):
        for n in acc:
            acc[n] += single[it][n]                                    # (bf16 addition, the order AccumulateGrad adds in)
            assert torch.equal(gd[it][n], acc[n]), (it, n)


def test_a_weight_that_is_not_channels_last_gets_its_sum_at_once():
    """The parameter NCHW-contiguous, the kernel's result with channels_last strides: conv3x3_ext takes the call all the same (its
    ``supported`` looks at the activation's layout only), and AccumulateGrad copies the gradient into the parameter's layout inside
    the backward pass.  ``weight_gradient(..., like=weight)`` computes that one sum at once; the other four stay deferred."""
    res = {mode: ds.run_case("nchw_weight", mode) for mode in ("deferred", "immediate")}
    _, _, notes = assert_case(res, [(ds.SUMS - 1, [1, ds.SUMS - 1])] * 3)
    C = ds.CH
    assert notes["grad_strides"]["conv.weight"] == (9 * C, 9, 3, 1) and notes["grad_strides"]["down.weight"] == (9 * C, 1, 3 * C, C)


def test_an_exception_in_the_backward_pass_leaves_nothing_registered_and_nothing_unwritten():
    from monodetr_amd import chunk_sums
    out = {}
    for mode in ("deferred", "immediate"):
        with ds.emulated(mode), ds.Probe() as probe:
            model = ds.Stack()
            it, _ = ds.make_iteration("none", model)
            model.interrupt = True
            with pytest.raises(ds.Interrupted):
                it._step(ds.batch(40))
            assert chunk_sums._pending == [] and chunk_sums._depth == 0
            seen = probe.take()
            first = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
            # the two layers whose backward ran before the exception: their sums were registered and the exit of the block computed them
            assert set(first) == {"lins.2.weight", "lins.2.bias", "lins.1.weight", "lins.1.bias"}
            assert (seen["registered"], seen["launches"]) == ((2, [2]) if mode == "deferred" else (0, [1, 1]))
            for call in seen["calls"]:
                assert torch.isfinite(call[3].float()).all() and torch.isfinite(call[4].float()).all()
            model.interrupt = False
            it._step(ds.batch(41))                                      # the next backward pass works, and defers again
            seen = probe.take()
            assert (seen["registered"], seen["launches"]) == ((ds.SUMS, [ds.SUMS]) if mode == "deferred" else (0, [1] * ds.SUMS))
            out[mode] = (first, {n: p.grad.detach().clone() for n, p in model.named_parameters()}, seen["calls"])
    for a, b in zip(out["deferred"][:2], out["immediate"][:2]):
        assert set(a) == set(b)
        for n in a:
            assert torch.isfinite(a[n].float()).all() and torch.equal(a[n], b[n]), n
    assert_reference(out["immediate"][2])


def test_the_check_names_its_reason_and_the_cut_pass_refuses_a_second_contribution():
    """chunk_sums.reader_inside_backward on its own (what TrainIteration's backward passes ask), and held="verify": a parameter that
    received gradient in both halves of a cut backward pass was accumulated from an unwritten sum -- that raises instead of training on."""
    from monodetr_amd import chunk_sums
    from torch.nn.parallel import DistributedDataParallel
    lin = torch.nn.Linear(4, 4)
    assert chunk_sums.reader_inside_backward(lin) is None
    lin.weight.grad = torch.zeros(4, 4)
    assert "still has a .grad" in chunk_sums.reader_inside_backward(lin)
    assert chunk_sums.reader_inside_backward(lin, held="verify") is None
    lin.weight.grad = None
    h = lin.bias.register_hook(lambda g: g)
    assert "hook" in chunk_sums.reader_inside_backward(lin)
    h.remove()
    assert chunk_sums.reader_inside_backward(lin) is None
    h = lin.bias.register_post_accumulate_grad_hook(lambda p: None)
    assert "hook" in chunk_sums.reader_inside_backward(params=[lin.bias])
    h.remove()
    ddp = DistributedDataParallel.__new__(DistributedDataParallel)      # (the type is what is asked; no process group needed for that)
    assert "DistributedDataParallel" in chunk_sums.reader_inside_backward(ddp)
    was = chunk_sums.ENABLED
    chunk_sums.ENABLED = True
    try:
        with chunk_sums.deferred(lin) as d:
            assert d.reason is None and chunk_sums.deferring()
        lin.weight.grad = torch.zeros(4, 4)
        with chunk_sums.deferred(lin) as d:
            assert d.reason is not None and not chunk_sums.deferring()
        with chunk_sums.deferred(lin, held="verify"):
            assert chunk_sums.deferring()
        with pytest.raises(RuntimeError, match="received another one"):
            with chunk_sums.deferred(lin, held="verify"):
                lin(torch.ones(2, 4)).sum().backward()
        assert chunk_sums._depth == 0 and chunk_sums._pending == []
    finally:
        chunk_sums.ENABLED = was


def test_no_shape_the_convolution_kernel_takes_has_a_sum_that_chunk_sums_refuses():
    """``chunk_sums.chunk_sum`` needs cols % 4 == 0 and raises otherwise; ``token_weight_gradient`` asks before it defers,
    ``weight_gradient`` now asks too.  Through csrc/conv_wgrad.hip the question never arises: its entry point takes C % 64 == 0 and
    N % 32 == 0 only, so cols = N k k C is a multiple of 2048 -- over a grid of small shapes, every problem ``mdetr_conv_wgrad`` accepts
    is one ``conv_wgrad_ext.supported`` accepts and has cols % 4 == 0, and every other one fails inside ``deferred()`` with an error
    from the kernel's own argument check, nothing registered."""
    import itertools
    from monodetr_amd import chunk_sums, conv_wgrad_ext
    taken = 0
    with ds.emulated("deferred") as L:
        for C, N, k, stride in itertools.product((8, 32, 63, 64, 66, 128), (1, 3, 16, 31, 32, 33, 64), (1, 3), (1, 2)):
            H = W = 4
            OH = (H + 2 * (k // 2) - k) // stride + 1
            x = torch.randn(1, C, H, W).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
            dy = torch.randn(1, N, OH, OH).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
            chunks = L.mdetr_conv_wgrad_chunks(1, H, W, C, OH, OH, N, k, stride)
            cols = N * k * k * C
            part = torch.zeros(max(chunks, 1) * cols)
            rc = L.mdetr_conv_wgrad(x.data_ptr(), dy.data_ptr(), part.data_ptr(), part.numel(), 1, H, W, C, OH, OH, N, k, stride, -1, None)
            if rc == 0:
                taken += 1
                assert chunks > 0 and cols % 4 == 0 and conv_wgrad_ext.supported(x, dy, k, stride), (C, N, k, stride)
                assert chunk_sums.supported(part.view(chunks, cols), torch.bfloat16)
            else:
                assert C % 64 or N % 32 or (k, stride) == (1, 1), (C, N, k, stride)
                with chunk_sums.deferred():
                    with pytest.raises(RuntimeError):
                        conv_wgrad_ext.weight_gradient(x, dy, k, stride)
                    assert chunk_sums._pending == []
            if cols % 4:
                assert rc != 0
    assert taken >= 12
