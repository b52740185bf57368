"""The criterion cases of tests/criterion_cases.py -- edge shapes, saturated inputs, depth-bin edges, box rasterisation, the matching
cost -- through both CPU stand-ins of tests/backends.py ("host": the shared *_math.h arithmetic; "emul": the real pair_losses.hip /
ddn_loss.hip / lsa.hip kernels with the ballot loop and the last-block finalisation, on the HIP-on-CPU shim), as
tests/test_criterion_cases_gpu.py runs them on the device; and the anchor checks of the two fp64 references.  The bounds and what is
asserted are in criterion_cases.py."""
import pytest

import backends
import criterion_cases as C


@pytest.fixture(params=backends.BACKENDS)
def backend(request):
    from monodetr_amd import ddn_loss_ext, lsa_ext, pair_losses_ext
    pair_losses_ext._backend = ddn_loss_ext._backend = lsa_ext._backend = backends.get(request.param)
    yield request.param
    pair_losses_ext._backend = ddn_loss_ext._backend = lsa_ext._backend = None


def test_every_case_holds_its_premises():
    """Building a case checks its premises (PremiseError): argmax gaps, bin-index guard band, fp32 == fp64 box corners, no box
    coordinate ties, and that the case reaches what it was built for."""
    for name in C.PAIR_CASES:
        C.pair_case(name)
    for name in C.DDN_CASES:
        C.ddn_case(name)
    for name in C.COST_CASES:
        C.cost_case(name)


def test_pair_reference_is_the_pytorch_criterion_in_float64():
    C.anchor_pair()


def test_ddn_reference_is_the_pytorch_ddn_loss_in_float64():
    C.anchor_ddn()


@pytest.mark.parametrize("nb_form", ["host", "dev"])
@pytest.mark.parametrize("name", list(C.PAIR_CASES))
def test_emulated_pair_losses(backend, name, nb_form):
    C.check_pair(name, nb_form, "cpu", backend)


def test_emulated_pair_losses_when_the_workspace_carve_up_moves(backend):
    C.check_pair_sequence("cpu", backend)


@pytest.mark.parametrize("name,layout", [(n, l) for n, v in C.DDN_CASES.items() for l in v[5]])
def test_emulated_ddn_loss(backend, name, layout):
    C.check_ddn(name, "cpu", layout, backend)


@pytest.mark.parametrize("name", C.COST_CASES)
def test_emulated_matching_cost_in_the_solver(backend, name):
    C.check_cost(name, "cpu", backend)
