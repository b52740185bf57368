"""The MSDA prologue cases of tests/prologue_cases.py on the device: csrc/msda_prologue.hip on one unit, 592 units (two blocks and
a ragged third), M = 5, LP = 16 without L = P = 4, the generic path, LP = 64 and LP = 1; 2- and 6-component reference points, full or
an expanded view, fp32 or bf16; fp32 and bf16 I/O; the two-tensor form, the packed form and views at an odd storage offset; on
exact-arithmetic rows and, against fp64, on benign, peaked, shifted, large-offset, extreme-extent and edge rows.
tests/test_prologue_cases_emulated_cpu.py runs the same cases on the CPU emulation; the bounds and what is asserted are in
prologue_cases.py.  Every case prints its figures before it asserts."""
import pytest
import torch

import prologue_cases as C

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
IDS = {BF16: "bf16", F32: "fp32"}


@pytest.mark.parametrize("io", [F32, BF16], ids=IDS.get)
@pytest.mark.parametrize("R", [2, 6])
@pytest.mark.parametrize("name", list(C.SHAPES))
def test_msda_prologue_kernel_exact_rows(name, R, io):
    for expanded in (False, True):
        for rdt in (F32, BF16):
            for form in C.forms(C.SHAPES[name]):
                C.check_exact(name, R, expanded, rdt, io, form, "cuda")


@pytest.mark.parametrize("io", [F32, BF16], ids=IDS.get)
@pytest.mark.parametrize("R", [2, 6])
@pytest.mark.parametrize("name", list(C.SHAPES))
def test_msda_prologue_kernel_against_fp64(name, R, io):
    for kind, expanded, rdt, form in C.thinned(name, R, io):
        C.check_bounded(name, kind, R, expanded, rdt, io, form, "cuda")
