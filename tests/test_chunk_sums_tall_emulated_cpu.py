"""Tall and pitched jobs of the grouped chunk sums (csrc/colsum.hip: mdetr_chunk_sums_pitched) on the HIP-on-CPU shim, through
monodetr_amd/chunk_sums.py, and the LayerNorm sites' gamma / beta sums registered with them (monodetr_amd/add_ln_ext.py).  The cases
and their bounds are in tests/chunk_sums_tall_cases.py; tests/test_chunk_sums_tall_gpu.py runs the same ones on the device."""
import pytest
import torch

import chunk_sums_tall_cases as T
import native_emul

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def emul():
    return native_emul.lib()


def test_integer_partials_sum_exactly_in_both_forms(emul):
    T.check_exact(CPU, emul)


def test_random_partials_stay_within_the_summation_bound(emul):
    T.check_random(CPU, emul)


def test_grouped_jobs_equal_the_single_launches_bit_for_bit(emul):
    T.check_grouped_equals_single(CPU, emul)


def test_layernorm_sums_deferred_and_poisoned_equal_the_immediate_ones(emul):
    """Two LayerNorm sites, three iterations, registered results filled with NaN until the flush: AccumulateGrad has to take each of
    the four results over without reading it."""
    T.check_ln_stack(CPU, emul)


def test_the_form_follows_from_the_chunk_count_alone_and_bad_jobs_are_refused(emul):
    with T.chunk_sums_on(emul) as cs:
        wide = torch.randn(200, 64)
        assert cs.supported(wide[:, 32:], torch.float32) and cs.supported(wide[:, :32], torch.bfloat16)
        assert not cs.supported(wide[:, 2:34], torch.float32)              # first element not 16-byte aligned
        assert not cs.supported(wide[:, 0:30], torch.float32)              # 30 columns
        assert not cs.supported(wide.t(), torch.float32)                   # columns not unit-stride
        with pytest.raises(RuntimeError, match="chunk_sum: needs"):
            cs.chunk_sum(wide[:, 2:34], torch.float32)
        # without the parameter gradients' context the LayerNorm sums keep the column-sum route: nothing reaches _launch
        assert not cs.deferring()
