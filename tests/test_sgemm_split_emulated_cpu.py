"""The three-way bf16 split form of csrc/sgemm.hip (MDETR_SGEMM_SPLIT) on the HIP-on-CPU shim: the cases of tests/sgemm_split_cases.py
through the unmodified kernel source (tests/native_emul.py); tests/test_sgemm_split_gpu.py runs the same cases on the GPU."""
import pytest
import torch

import native_emul
import sgemm_split_cases as C

CPU = torch.device("cpu")


@pytest.fixture()
def emul(monkeypatch):
    from monodetr_amd import sgemm_ext
    monkeypatch.setattr(sgemm_ext, "_backend", native_emul.lib())


@pytest.mark.parametrize("tune", C.TUNES)
def test_exact_groups_in_the_split_form(emul, monkeypatch, tune):
    monkeypatch.setenv("MDETR_TUNE", tune)
    C.check_exact_groups(CPU, monkeypatch)


@pytest.mark.parametrize("tune", C.TUNES[1:])
@pytest.mark.parametrize("mode", C.MODES)
def test_every_geometry_bit_for_bit(emul, monkeypatch, mode, tune):
    monkeypatch.setenv("MDETR_TUNE", tune)
    for shape in C.SHAPES[1:4]:
        C.check_split_case(CPU, mode, "int", shape)


@pytest.mark.parametrize("mode", C.MODES)
@pytest.mark.parametrize("kind", C.KINDS)
def test_split_cases_bit_for_bit(emul, mode, kind):
    for shape in (C.TN_SHAPES if mode == "tn" else C.SHAPES):
        C.check_split_case(CPU, mode, kind, shape)


@pytest.mark.parametrize("mode", ["nt", "tn"])
def test_a_bf16_operand_takes_three_terms_and_stays_exact(emul, mode):
    for shape in (C.TN_SHAPES if mode == "tn" else C.SHAPES):
        C.check_three_term_case(CPU, mode, shape)


@pytest.mark.parametrize("x_dtype", [torch.bfloat16, torch.float32])
def test_heads_groups_on_random_operands_vs_float64(emul, x_dtype):
    C.check_heads_groups_bounded(CPU, 150, x_dtype)


@pytest.mark.parametrize("x_dtype", [torch.bfloat16, torch.float32])
def test_tn_across_the_contraction_split_vs_float64_and_twice_the_same(emul, x_dtype):
    C.check_tn_bounded(CPU, 4400, x_dtype, full=False)       # (a light group: the emulation runs one lane at a time)


def test_the_unflagged_call_is_still_the_fmaf_chain(emul):
    C.check_unflagged_is_the_fmaf_chain(CPU)


def test_tune_key_overrides_the_flag(emul, monkeypatch):
    g = C.X.gen(7)
    a, w = C.X.full_mantissa(g, (70, 64)), C.X.full_mantissa(g, (33, 64))
    exact, split = C.product(CPU, "nt", a, w, False), C.product(CPU, "nt", a, w, True)
    assert not torch.equal(exact, split)
    monkeypatch.setenv("MDETR_TUNE", "sgemm_split=0")
    assert torch.equal(C.product(CPU, "nt", a, w, True), exact)
    monkeypatch.setenv("MDETR_TUNE", "sgemm_split=1")
    assert torch.equal(C.product(CPU, "nt", a, w, False), split)


def test_heads_level_with_a_bf16_input_takes_the_split_form(emul):
    C.check_heads_level_split(CPU)
