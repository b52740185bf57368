"""The MSDA prologue cases of tests/prologue_cases.py -- exact-arithmetic rows, peaked / shifted / edge rows against fp64, the
packed form, views at an odd storage offset, bf16 against fp32 I/O -- through the real csrc/msda_prologue.hip kernels on the
HIP-on-CPU shim (tests/native_emul.py), as tests/test_prologue_cases_gpu.py runs them on the device; and the anchor check of the fp64
reference.  The bounds and what is asserted are in prologue_cases.py."""
import pytest
import torch

import native_emul
import prologue_cases as C

BF16, F32 = torch.bfloat16, torch.float32
IDS = {BF16: "bf16", F32: "fp32"}


@pytest.fixture(scope="module")
def emul():
    return native_emul.lib()


def test_prologue_reference_is_the_module_formulation_in_float64():
    C.anchor()


def test_every_combination_of_the_cross_product_is_reached():
    """The thinned list still pairs every kind with every form, and every R and I/O type with every reference-point layout and type."""
    for name, shape in C.SHAPES.items():
        for R in (2, 6):
            for io in (F32, BF16):
                combos = C.thinned(name, R, io)
                assert {(k, f) for k, _, _, f in combos} == {(k, f) for k in C.kinds(R, io) for f in C.forms(shape)}
                assert {(e, r) for _, e, r, _ in combos} == {(e, r) for e in (False, True) for r in (F32, BF16)}


@pytest.mark.parametrize("io", [F32, BF16], ids=IDS.get)
@pytest.mark.parametrize("R", [2, 6])
@pytest.mark.parametrize("name", list(C.SHAPES))
def test_emulated_prologue_exact_rows(emul, name, R, io):
    for expanded in (False, True):
        for rdt in (F32, BF16):
            for form in C.forms(C.SHAPES[name]):
                C.check_exact(name, R, expanded, rdt, io, form, "cpu", emul)


@pytest.mark.parametrize("io", [F32, BF16], ids=IDS.get)
@pytest.mark.parametrize("R", [2, 6])
@pytest.mark.parametrize("name", list(C.SHAPES))
def test_emulated_prologue_against_fp64(emul, name, R, io):
    for kind, expanded, rdt, form in C.thinned(name, R, io):
        C.check_bounded(name, kind, R, expanded, rdt, io, form, "cpu", emul)
