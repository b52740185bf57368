"""The exact lattice cases of tests/msda_lattice_cases.py on the device, through monodetr_amd.msda_ext: forward (fp32, bf16), gather
indices, the fp32 backward through msda_bwd = fused / tiled / atomic, and the one-pass backward in its seven launch variants with fp32 and
bf16 grad_value -- the full product of tile plans, variants and near / far / contention sets on the 255- and 640-cell pyramids, the
cross-attention and degenerate-map calls, a 2550-cell pyramid under the default plan (core tiles next to whole-level chunks) and the
generic kernels.  Everything is compared bit for bit with the fp64 reference (one documented bound: msda_lattice_cases.py).
tests/test_msda_lattice_cases_emulated_cpu.py runs a thinned product on the CPU emulation."""
import pytest
import torch

import msda_lattice_cases as C

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
SELF = {"tiny": (2, 3), "small": (1, 2), "odd": (1, 2)}                      # (B, M) of the self-attention calls
CROSS = {"tiny": (2, 3, 50), "small": (2, 2, 50), "odd": (2, 3, 37)}         # (B, M, Lq)


@pytest.fixture(scope="module")
def be():
    return C.DeviceBackend()


def _run(c, be, monkeypatch):
    print(C.describe(c))
    C.check_routes(c, be, monkeypatch)
    for variant in C.VARIANTS:
        C.check_variant(c, be, variant, monkeypatch)


@pytest.mark.parametrize("plan", list(C.PLANS))
@pytest.mark.parametrize("geom", list(SELF))
def test_msda_self_attention_every_plan_variant_and_set(be, monkeypatch, geom, plan):
    B, M = SELF[geom]
    for kind in C.sets_for(geom, plan, None):
        _run(C.case(geom, B, M, None, kind, plan), be, monkeypatch)


@pytest.mark.parametrize("plan", list(C.PLANS))
@pytest.mark.parametrize("geom", list(CROSS))
def test_msda_cross_attention_every_plan_and_variant(be, monkeypatch, geom, plan):
    B, M, Lq = CROSS[geom]
    _run(C.case(geom, B, M, Lq, "any", plan), be, monkeypatch)


@pytest.mark.parametrize("kind", ["near", "far"])
def test_msda_core_tiles_next_to_whole_level_chunks_under_the_default_plan(be, monkeypatch, kind):
    _run(C.case("big", 1, 8, None, kind, "default"), be, monkeypatch)


@pytest.mark.parametrize("D,dtype", [(16, F32), (30, F64)], ids=["D16-fp32", "D30-fp64"])
def test_msda_generic_kernels(be, monkeypatch, D, dtype):
    C.set_plan(monkeypatch, "default")
    C.check_generic(be, D, dtype)
