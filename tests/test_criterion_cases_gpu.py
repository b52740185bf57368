"""The criterion cases of tests/criterion_cases.py on the device: csrc/pair_losses.hip at one row, rows spread over four images per
wave, ragged blocks, clamped slot batches, K = 64, no targets, both cardinality extremes, kMaxClasses, saturated inputs and every
GIoU branch, each with num_boxes as a float and as a device tensor, and across a change of (L, B) on the same workspace;
csrc/ddn_loss.hip at a ragged block, C = 17 / 96 / 97 (partial 16-batch, full register array, the from-memory path), every bin edge
with a guard band, out-of-range depths, the box rasterisation and saturated logits, each twice in a row; the matching cost of
csrc/lsa.hip on a square 64 x 64 problem and on the planted box geometries.  tests/test_criterion_cases_emulated_cpu.py runs the same
cases on the CPU stand-ins; the bounds and what is asserted are in criterion_cases.py.  Every case prints its figures before it asserts."""
import pytest

import criterion_cases as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("nb_form", ["host", "dev"])
@pytest.mark.parametrize("name", list(C.PAIR_CASES))
def test_pair_losses(name, nb_form):
    C.check_pair(name, nb_form, "cuda")


def test_pair_losses_when_the_workspace_carve_up_moves():
    C.check_pair_sequence("cuda")


@pytest.mark.parametrize("name,layout", [(n, l) for n, v in C.DDN_CASES.items() for l in v[5]])
def test_ddn_loss(name, layout):
    C.check_ddn(name, "cuda", layout)


@pytest.mark.parametrize("name", C.COST_CASES)
def test_matching_cost_in_the_solver(name):
    C.check_cost(name, "cuda")
