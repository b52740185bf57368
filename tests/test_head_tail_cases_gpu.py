"""The head-tail cases of tests/head_tail_cases.py on the device: csrc/head_tail.hip on a single query and cell, the training
geometry with 2- and 6-component initial references, 2100 and 3300 (level, query) pairs per image (the second LDS batch of the map
gradient), 35 cells (a partial last workgroup), three images on a narrow map, H = 1 and W = 1; an exact-arithmetic case with the
clamp's tie; against fp64 on benign and saturated inputs, references at 0 / 1 / outside [0, 1], tiny boxes, centres on the borders and
corners, every centre of an image in one cell, and a depth map with zero rows; box_refine on 1, 257 and 1100 rows.
tests/test_head_tail_cases_emulated_cpu.py runs the same cases on the CPU emulation; the bounds and what is asserted are in
head_tail_cases.py.  Every case prints its figures before it asserts."""
import pytest

import head_tail_cases as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(C.EXACT_SHAPES))
def test_head_tail_exact_centres(name):
    C.check_exact(name, "cuda")


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("name", list(C.SHAPES))
def test_head_tail_against_fp64(name, kind):
    C.check_bounded(name, kind, "cuda")


@pytest.mark.parametrize("nd", [2, 6])
@pytest.mark.parametrize("rows", C.REFINE_ROWS)
def test_head_tail_box_refine_against_fp64(rows, nd):
    C.check_refine(rows, nd, "cuda")
