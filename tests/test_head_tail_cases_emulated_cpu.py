"""The head-tail cases of tests/head_tail_cases.py -- the exact-arithmetic case with the clamp's tie, saturated inputs, references on
the clamps of inverse_sigmoid, centres on borders and corners, the second LDS batch and the partial last workgroup of the map
gradient, H = 1 and W = 1, box_refine -- through the real csrc/head_tail.hip kernels on the HIP-on-CPU shim (tests/native_emul.py), as
tests/test_head_tail_cases_gpu.py runs them on the device; and the anchor check of the map gradient's fp64 form.  The bounds and what
is asserted are in head_tail_cases.py.  The shim runs a workgroup's threads as fibers and is deterministic by construction: the
second run and the two runs with one output unused are made on the maps below 1000 cells (240 workgroups of the map gradient per run
on 24 x 80), for every kind, as the device makes them at every shape."""
import pytest

import head_tail_cases as C
import native_emul


@pytest.fixture(scope="module")
def emul():
    return native_emul.lib()


def test_map_gradient_reference_is_grid_sample_in_float64():
    C.anchor()


@pytest.mark.parametrize("name", list(C.EXACT_SHAPES))
def test_emulated_head_tail_exact_centres(emul, name):
    H, W = C.EXACT_SHAPES[name][3:5]
    C.check_exact(name, "cpu", emul, extras=H * W < 1000)


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("name", list(C.SHAPES))
def test_emulated_head_tail_against_fp64(emul, name, kind):
    H, W = C.SHAPES[name][3:5]
    C.check_bounded(name, kind, "cpu", emul, extras=H * W < 1000)


@pytest.mark.parametrize("nd", [2, 6])
@pytest.mark.parametrize("rows", C.REFINE_ROWS)
def test_emulated_head_tail_box_refine_against_fp64(emul, rows, nd):
    C.check_refine(rows, nd, "cpu", emul)
