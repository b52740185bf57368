"""The exact lattice cases of tests/msda_lattice_cases.py through the real csrc/msda.hip, csrc/msda_tiled.hip and csrc/msda_fused.hip on
the HIP-on-CPU shim (tests/native_emul.py): forward, gather indices and the backward routes against the fp64 reference, bit for bit.
A thinned product -- every tile plan, every launch variant and every set at least once (asserted below); the device run
(tests/test_msda_lattice_cases_gpu.py) takes the full product.  The emulation additionally reads Header.far: 0 on every near set.
What is placed, the premises and the one bounded output are in msda_lattice_cases.py."""
import pytest
import torch

import msda_lattice_cases as C
import native_emul

F32, F64 = torch.float32, torch.float64

#        geometry, B, M, Lq, set, plan, variant
THINNED = [
    ("tiny", 1, 2, None, "near", "tiles_chunks", (512, 8, 2)),
    ("tiny", 1, 2, None, "far", "tiles_only", (1024, 8, 2)),
    ("tiny", 1, 2, None, "far", "whole", (1024, 4, 2)),
    ("tiny", 1, 2, None, "near", "default", (1024, 2, 2)),
    ("tiny", 1, 2, None, "contention", "one_chunk", (768, 4, 2)),          # 1020 contributions: one repeated pass
    ("small", 1, 2, None, "contention", "one_chunk", (768, 4, 4)),         # 2560: three
    ("small", 1, 2, None, "far", "tiles_chunks", "fp32"),
    ("small", 2, 3, 50, "any", "tiles_only", (768, 4, 2)),                 # cross-attention: every block scans every query
    ("odd", 2, 3, 37, "any", "whole", "fp32"),
    ("odd", 1, 2, None, "far", "tiles_only", (1024, 4, 2)),
    ("odd", 1, 2, None, "near", "tiles_only", (512, 8, 2)),
]


@pytest.fixture(scope="module")
def be():
    return C.EmulatedBackend(native_emul.lib())


def test_reference_is_the_fp64_oracle_on_random_floats():
    C.anchor()


def test_the_thinned_product_reaches_every_plan_variant_and_set():
    assert {t[5] for t in THINNED} == set(C.PLANS)
    assert {t[6] for t in THINNED} == set(C.VARIANTS)
    assert {t[4] for t in THINNED} == {"near", "far", "any", "contention"}
    assert {t[0] for t in THINNED} == {"tiny", "small", "odd"} and {t[1] for t in THINNED} == {1, 2} and {t[2] for t in THINNED} == {2, 3}


def test_premises_hold_for_the_sets_only_the_device_runs():
    """The cases the device run adds (cheap: operands, reference and premises only): every plan x set of the two self-attention
    pyramids and the GPU-only pyramid under the default plan."""
    for geom, B, M in (("tiny", 2, 3), ("small", 1, 2)):
        for plan in C.PLANS:
            for kind in C.sets_for(geom, plan, None):
                C.case(geom, B, M, None, kind, plan)
    for kind in C.sets_for("big", "default", None):
        c = C.case("big", 1, 8, None, kind, "default")
        assert sorted(lv.mode for lv in c.models[32]) == [0, 1, 1, 1]         # level 0 in core tiles next to whole-level chunks


@pytest.mark.parametrize("geom,B,M,Lq,kind,plan", [("tiny", 1, 2, None, "near", "tiles_chunks"), ("small", 2, 3, 50, "any", "tiles_only"),
                                                   ("odd", 1, 2, None, "far", "tiles_only")])
def test_emulated_forward_indices_and_backward_routes(be, monkeypatch, geom, B, M, Lq, kind, plan):
    c = C.case(geom, B, M, Lq, kind, plan)
    print(C.describe(c))
    C.check_routes(c, be, monkeypatch)


@pytest.mark.parametrize("geom,B,M,Lq,kind,plan,variant", THINNED, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_emulated_one_pass_backward(be, monkeypatch, geom, B, M, Lq, kind, plan, variant):
    c = C.case(geom, B, M, Lq, kind, plan)
    print(C.describe(c))
    C.check_variant(c, be, variant, monkeypatch)


@pytest.mark.parametrize("D,dtype", [(16, F32), (30, F64)], ids=["D16-fp32", "D30-fp64"])
def test_emulated_generic_kernels(be, monkeypatch, D, dtype):
    C.set_plan(monkeypatch, "default")
    C.check_generic(be, D, dtype)
