"""The three-way bf16 split form of csrc/sgemm.hip (MDETR_SGEMM_SPLIT) on the GPU: the cases of tests/sgemm_split_cases.py."""
import pytest
import torch

import sgemm_split_cases as C

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


@pytest.mark.parametrize("tune", C.TUNES)
def test_exact_groups_in_the_split_form(monkeypatch, tune):
    monkeypatch.setenv("MDETR_TUNE", tune)
    C.check_exact_groups(DEV, monkeypatch)


@pytest.mark.parametrize("tune", C.TUNES[1:])
@pytest.mark.parametrize("mode", C.MODES)
def test_every_geometry_bit_for_bit(monkeypatch, mode, tune):
    monkeypatch.setenv("MDETR_TUNE", tune)
    for kind in C.KINDS:
        for shape in (C.TN_SHAPES if mode == "tn" else C.SHAPES):
            C.check_split_case(DEV, mode, kind, shape)


@pytest.mark.parametrize("mode", C.MODES)
@pytest.mark.parametrize("kind", C.KINDS)
def test_split_cases_bit_for_bit(mode, kind):
    for shape in (C.TN_SHAPES if mode == "tn" else C.SHAPES):
        C.check_split_case(DEV, mode, kind, shape)


@pytest.mark.parametrize("mode", ["nt", "tn"])
def test_a_bf16_operand_takes_three_terms_and_stays_exact(mode):
    for shape in (C.TN_SHAPES if mode == "tn" else C.SHAPES):
        C.check_three_term_case(DEV, mode, shape)


@pytest.mark.parametrize("x_dtype", [torch.bfloat16, torch.float32])
def test_heads_groups_on_random_operands_vs_float64(x_dtype):
    C.check_heads_groups_bounded(DEV, 150, x_dtype)


@pytest.mark.parametrize("x_dtype", [torch.bfloat16, torch.float32])
def test_tn_at_the_step_s_contraction_split_vs_float64_and_twice_the_same(x_dtype):
    C.check_tn_bounded(DEV, 4400, x_dtype, full=True)        # the ten weight gradients of a level: the split count of the step
    C.check_tn_bounded(DEV, 4400, x_dtype, full=False)       # few tiles: the largest split count


def test_the_unflagged_call_is_still_the_fmaf_chain():
    C.check_unflagged_is_the_fmaf_chain(DEV)


def test_heads_level_with_a_bf16_input_takes_the_split_form():
    C.check_heads_level_split(DEV)
