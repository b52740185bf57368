"""The deferred PRODUCERS of the short token weight gradients (monodetr_amd/chunk_sums.py: register_producer / flush; family
MDETR_TWGRAD_GROUPED in conv_wgrad_ext.token_weight_gradient) on the real kernel sources running on the HIP-on-CPU shim: what is
registered and what is not, when the values arrive, in which order a flush launches, and the test-only VERIFY mode that holds the
second invariant (a registered operand is not written before its flush)."""
import contextlib

import pytest
import torch

import native_emul

T, K, N = 1031, 64, 64


@contextlib.contextmanager
def emulated(grouped=True, poison=True, verify=False):
    from monodetr_amd import chunk_sums, conv_wgrad_ext
    L = native_emul.lib()
    saved = [(m, a, getattr(m, a)) for m, a in ((chunk_sums, "_backend"), (conv_wgrad_ext, "_backend"), (chunk_sums, "ENABLED"), (chunk_sums, "POISON"),
                                                (chunk_sums, "VERIFY"), (chunk_sums, "IMMEDIATE"), (conv_wgrad_ext, "GROUPED"))]
    try:
        chunk_sums._backend = conv_wgrad_ext._backend = L
        chunk_sums.ENABLED, chunk_sums.POISON, chunk_sums.VERIFY, chunk_sums.IMMEDIATE, conv_wgrad_ext.GROUPED = True, poison, verify, False, grouped
        assert not chunk_sums._producers and not chunk_sums._pending
        yield chunk_sums, conv_wgrad_ext
    finally:
        del chunk_sums._producers[:]
        del chunk_sums._pending[:]
        for m, a, v in saved:
            setattr(m, a, v)


def operands(seed=0, T=T, K=K, N=N, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(T, K, generator=g).to(dtype), (torch.randn(T, N, generator=g) * 0.5).to(dtype)


@pytest.fixture(scope="module")
def reference():
    """(dW, db) in fp32 of the operands of seeds 0 and 1, launched at once, family off: computed once, never written."""
    out = {}
    with emulated(grouped=False) as (cs, cw):
        for seed in (0, 1):
            out[seed] = cw.token_weight_gradient(*operands(seed), torch.float32, bias=True)
    return out


def test_a_registered_result_is_nan_until_the_flush_and_right_after_it(reference):
    with emulated() as (cs, cw):
        x, dy = operands(0)
        with cs.deferred():
            dw, db = cw.token_weight_gradient(x, dy, torch.float32, bias=True)
            assert len(cs._producers) == 1 and len(cs._pending) == 1
            assert torch.isnan(dw).all() and torch.isnan(db).all()
        assert not cs._producers and not cs._pending
        assert torch.equal(dw, reference[0][0]) and torch.equal(db, reference[0][1])


def test_the_family_off_launches_the_producer_at_once_and_defers_only_the_sum(reference):
    with emulated(grouped=False) as (cs, cw):
        x, dy = operands(0)
        with cs.deferred():
            dw, db = cw.token_weight_gradient(x, dy, torch.float32, bias=True)
            assert not cs._producers and len(cs._pending) == 1
        assert torch.equal(dw, reference[0][0]) and torch.equal(db, reference[0][1])


def test_a_reader_side_flush_gets_computed_values(reference):
    """linear._weight_bias_grads with an fp32 bias beside a bf16 weight converts both gradients -- it READS them -- and calls flush()
    first: inside deferred() the caller receives values, and an earlier registration is computed by the same flush."""
    from monodetr_amd.monodetr import linear
    with emulated() as (cs, cw):
        x0, dy0 = operands(0)
        x1, dy1 = operands(1)
        weight = torch.zeros(N, K, dtype=torch.bfloat16)
        with cs.deferred():
            dw0, db0 = cw.token_weight_gradient(x0, dy0, torch.float32, bias=True)
            assert torch.isnan(dw0).all() and len(cs._producers) == 1
            dw1, db1 = linear._weight_bias_grads(x1, dy1, weight, True, True, bias_dtype=torch.float32)
            assert not cs._producers and not cs._pending
            assert dw1.dtype == torch.bfloat16 and db1.dtype == torch.float32
            assert torch.equal(dw1, reference[1][0].to(torch.bfloat16)) and torch.equal(db1, reference[1][1])
            assert torch.equal(dw0, reference[0][0]) and torch.equal(db0, reference[0][1])


def test_a_flush_launches_the_producers_before_the_sums(reference):
    with emulated() as (cs, cw):
        order = []
        producers, sums = cs._launch_producers, cs._launch
        cs._launch_producers = lambda jobs: (order.append(("producers", len(jobs))), producers(jobs))[1]
        cs._launch = lambda jobs: (order.append(("sums", len(jobs))), sums(jobs))[1]
        try:
            with cs.deferred():
                got = [cw.token_weight_gradient(*operands(s), torch.float32, bias=True) for s in (0, 1, 0)]
                assert order == []
        finally:
            cs._launch_producers, cs._launch = producers, sums
        assert order == [("producers", 3), ("sums", 3)]
        for s, (dw, db) in zip((0, 1, 0), got):
            assert torch.equal(dw, reference[s][0]) and torch.equal(db, reference[s][1])


def test_outside_deferred_and_with_a_refusing_module_the_launch_is_immediate(reference):
    with emulated() as (cs, cw):
        x, dy = operands(0)
        dw, db = cw.token_weight_gradient(x, dy, torch.float32, bias=True)
        assert not cs._producers and not cs._pending and torch.equal(dw, reference[0][0]) and torch.equal(db, reference[0][1])
        module = torch.nn.Linear(4, 4)
        module.weight.grad = torch.zeros_like(module.weight)                 # a retained .grad: AccumulateGrad would read the new gradient
        with cs.deferred(module) as d:
            assert d.reason is not None
            dw, db = cw.token_weight_gradient(x, dy, torch.float32, bias=True)
            assert not cs._producers and not cs._pending and torch.equal(dw, reference[0][0]) and torch.equal(db, reference[0][1])
        cs.IMMEDIATE = True                                                  # (the tests' reference mode: every sum at once, so every producer too)
        with cs.deferred():
            dw, db = cw.token_weight_gradient(x, dy, torch.float32, bias=True)
            assert not cs._producers and not cs._pending and torch.equal(dw, reference[0][0])


def test_an_exception_inside_the_block_still_flushes(reference):
    with emulated() as (cs, cw):
        x, dy = operands(1)
        with pytest.raises(KeyError):
            with cs.deferred():
                dw, db = cw.token_weight_gradient(x, dy, torch.float32, bias=True)
                assert torch.isnan(dw).all()
                raise KeyError("stop")
        assert not cs._producers and not cs._pending
        assert torch.equal(dw, reference[1][0]) and torch.equal(db, reference[1][1])


def test_verify_raises_when_a_registered_operand_is_written_before_the_flush(reference):
    with emulated(verify=True) as (cs, cw):
        x, dy = operands(0)
        with cs.deferred():                                                  # untouched operands: VERIFY is silent
            dw, db = cw.token_weight_gradient(x, dy, torch.float32, bias=True)
        assert torch.equal(dw, reference[0][0]) and torch.equal(db, reference[0][1])
        for which in ("dy", "x"):
            x, dy = operands(0)
            with pytest.raises(RuntimeError, match="written between its registration and the flush"):
                with cs.deferred():
                    cw.token_weight_gradient(x, dy, torch.float32, bias=True)
                    (dy if which == "dy" else x)[5, 3] += 1.0                # an in-place writer inside the backward pass
            assert not cs._producers


def test_long_token_axes_and_fp32_operands_never_register():
    from monodetr_amd.small_wgrad_ext import MAX_ROWS
    with emulated(poison=False) as (cs, cw):
        with cs.deferred():
            x, dy = operands(2, T=MAX_ROWS, K=64, N=64)
            cw.token_weight_gradient(x, dy, torch.float32, bias=True)
            assert len(cs._producers) == 1                                   # the last row count of the class
            x, dy = operands(2, T=MAX_ROWS + 8, K=64, N=64)
            dw, db = cw.token_weight_gradient(x, dy, torch.float32, bias=True)
            assert len(cs._producers) == 1 and len(cs._pending) == 2         # launched at once; its sum deferred as before
            xf, dyf = operands(3, dtype=torch.float32)
            cw.token_weight_gradient(xf, dyf, torch.float32, bias=True)
            assert len(cs._producers) == 1 and len(cs._pending) == 3
        ref = dy.double().t() @ x.double()
        assert float((dw.double() - ref).abs().max()) <= 1e-3 * float(ref.abs().max())
