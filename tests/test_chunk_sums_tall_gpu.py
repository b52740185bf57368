"""Tall and pitched jobs of the grouped chunk sums (csrc/colsum.hip: mdetr_chunk_sums_pitched) on the device -- the cases of
tests/chunk_sums_tall_cases.py, as tests/test_chunk_sums_tall_emulated_cpu.py runs them on the shim -- and the gamma / beta gradients
of ``_AddLayerNorm`` registered as two such jobs, against fp64 and against the column-sum route they replace."""
import pytest
import torch

import chunk_sums_tall_cases as T

pytestmark = pytest.mark.gpu


def test_chunk_sums_tall_integer_partials_sum_exactly_in_both_forms():
    T.check_exact(torch.device("cuda"))


def test_chunk_sums_tall_random_partials_stay_within_the_summation_bound():
    T.check_random(torch.device("cuda"))


def test_chunk_sums_tall_grouped_jobs_equal_the_single_launches_bit_for_bit():
    T.check_grouped_equals_single(torch.device("cuda"))


def test_fused_add_layernorm_sums_deferred_and_poisoned_equal_the_immediate_ones():
    T.check_ln_stack(torch.device("cuda"))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [128, 256, 512])
@pytest.mark.parametrize("rows", [1, 5, 4 * 1024 + 3])
def test_fused_add_layernorm_deferred_parameter_gradients_match_fp64(rows, C, dtype):
    """gamma / beta gradients of one site, registered (deferred) and launched at once (immediate): equal bits; against the fp64 sums
    of dy * xhat and dy within the bar of tests/test_colsum_gpu.py (2e-5 sqrt(rows) + 1e-6 max|ref| for fp32 results, 2^-7 max|ref|
    for bf16 ones); and within the same bar of the column-sum route outside the context."""
    from monodetr_amd import add_ln_ext
    g = T.gen("ln", rows, C)
    a, b, dy = (torch.randn(rows, C, generator=g).to(dtype).cuda() for _ in range(3))

    def grads(mode):
        gamma = (1 + 0.1 * torch.randn(C, generator=T.gen("g", C))).to(dtype).cuda().requires_grad_(True)
        beta = (0.1 * torch.randn(C, generator=T.gen("b", C))).to(dtype).cuda().requires_grad_(True)
        with T.chunk_sums_on(poison=mode == "deferred", immediate=mode == "immediate") as cs:
            y = add_ln_ext.fused_add_layernorm(a, b, gamma, beta, 1e-5, 0.0)
            if mode == "outside":
                y.backward(dy)
            else:
                with cs.deferred(params=[gamma, beta]) as d:
                    assert d.reason is None
                    y.backward(dy)
        return gamma, beta

    (g_def, b_def), (g_imm, b_imm), (g_out, b_out) = grads("deferred"), grads("immediate"), grads("outside")
    assert g_def.grad.dtype == b_def.grad.dtype == dtype
    assert torch.equal(g_def.grad, g_imm.grad) and torch.equal(b_def.grad, b_imm.grad)
    s = (a.float() + b.float()).to(dtype).double()
    xhat = (s - s.mean(1, keepdim=True)) / (s.var(1, unbiased=False, keepdim=True) + 1e-5).sqrt()
    for got, out, ref in ((g_def.grad, g_out.grad, (dy.double() * xhat).sum(0)), (b_def.grad, b_out.grad, dy.double().sum(0))):
        bar = 2.0 ** -7 * ref.abs().max() if dtype == torch.bfloat16 else 2e-5 * rows ** 0.5 + 1e-6 * ref.abs().max()
        print("rows %d C %d %s: error %.3g (column-sum route %.3g), bar %.3g" % (rows, C, dtype, float((got.double() - ref).abs().max()),
                                                                                float((out.double() - ref).abs().max()), float(bar)))
        assert (got.double() - ref).abs().max() <= bar
        assert (out.double() - ref).abs().max() <= bar
