"""The normalisation cases of tests/norm_cases.py -- exact-arithmetic rows and groups, dropout, offset / constant / tiny / big rows,
the ReLU mask -- through the real csrc/add_ln.hip and csrc/group_norm.hip kernels on the HIP-on-CPU shim (tests/native_emul.py), as
tests/test_norm_cases_gpu.py runs them on the device; and the anchor checks of the two fp64 references.  The bounds and what is
asserted are in norm_cases.py.  The shim runs a workgroup's threads as fibers, so the shapes are the smaller part of the device's:
the 4 101-row LayerNorm case for one width per I/O type, GroupNorm tensors up to 2^19 elements."""
import pytest
import torch

import native_emul
import norm_cases as N

BF16, F32 = torch.bfloat16, torch.float32
IDS = {BF16: "bf16", F32: "fp32"}


@pytest.fixture(scope="module")
def emul():
    return native_emul.lib()


def test_ln_reference_is_the_framework_operator_in_float64():
    N.anchor_ln()


def test_gn_reference_is_the_framework_operator_in_float64():
    N.anchor_gn()


LN_EXACT = [(R, C, io, pdt) for R in N.LN_EXACT_ROWS[:-1] for C in N.LN_WIDTHS for io in (F32, BF16) for pdt in (F32, BF16)] + \
    [(4101, 512, F32, F32), (4101, 256, BF16, BF16), (4101, 128, BF16, F32)]


@pytest.mark.parametrize("R,C,io,pdt", LN_EXACT, ids=lambda v: IDS.get(v, str(v)))
def test_emulated_layernorm_exact_rows(emul, R, C, io, pdt):
    N.check_ln_exact(R, C, io, pdt, "cpu", emul)


@pytest.mark.parametrize("io", [F32, BF16], ids=IDS.get)
@pytest.mark.parametrize("C", N.LN_WIDTHS)
@pytest.mark.parametrize("name", list(N.LN_BOUNDED))
def test_emulated_layernorm_against_fp64(emul, name, C, io):
    N.check_ln_bounded(name, C, io, F32, "cpu", emul)


@pytest.mark.parametrize("io", [F32, BF16], ids=IDS.get)
@pytest.mark.parametrize("name,C", [("p01", 256), ("mixed", 128), ("constant", 512)])
def test_emulated_layernorm_against_fp64_with_bf16_parameters(emul, name, C, io):
    N.check_ln_bounded(name, C, io, BF16, "cpu", emul)


@pytest.mark.parametrize("io", [F32, BF16], ids=IDS.get)
@pytest.mark.parametrize("C", N.LN_WIDTHS)
def test_emulated_layernorm_mask_is_the_same_for_a_host_and_a_device_seed(emul, C, io):
    N.check_ln_seed_forms(C, io, "cpu", emul)


@pytest.mark.parametrize("io", [F32, BF16], ids=IDS.get)
@pytest.mark.parametrize("C", N.LN_WIDTHS)
def test_emulated_layernorm_of_a_view_at_an_odd_storage_offset(emul, C, io):
    N.check_ln_bounded("p01", C, io, F32, "cpu", emul, odd_view=True)


def _gn_exact_params():
    """Every (C, HW, N) of the device's list within 600 000 elements -- left out here: (64, 4096, 3), (256, 2048 | 2049, 3),
    (256, 4096, 1 | 3), (2048, 128 | 257, 3), (2048, 2048 | 2049 | 4096, 1 | 3); the single-image shapes up to 70 000 elements in all
    three dtype combinations, the others in one each."""
    shapes = sorted(set(N.gn_exact_shapes(N.GN_HW, 600000) + N.gn_exact_shapes(N.GN_HW_POW2, 600000)))
    out = []
    for C, HW, n in shapes:
        every = C * HW * n <= 70000 and n == 1
        out += [(C, HW, n) + dt for k, dt in enumerate(N.GN_DTYPES) if every or k == (C + HW + n) % 3]
    return out


@pytest.mark.parametrize("C,HW,n,io,pdt", _gn_exact_params(), ids=lambda v: IDS.get(v, str(v)))
def test_emulated_group_norm_exact_groups(emul, C, HW, n, io, pdt):
    N.check_gn_exact(C, HW, n, io, pdt, "cpu", emul)


def _gn_bounded_params():
    """plain: every shape and dtype combination; offset / constant: every shape in fp32, the 768-group shape in bf16 (norm_cases.py:
    one such group among 768 keeps the guard band under its cap)."""
    out = []
    for name in N.GN_BOUNDED:
        for io, pdt in N.GN_DTYPES:
            for variant in ("plain", "offset", "constant"):
                if variant == "plain" or io == F32 or name == "groups768":
                    out.append((name, variant, io, pdt))
    return out


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("name,variant,io,pdt", _gn_bounded_params(), ids=lambda v: IDS.get(v, str(v)))
def test_emulated_group_norm_against_fp64(emul, name, variant, io, pdt, relu):
    N.check_gn_bounded(name, io, pdt, variant, relu, "cpu", emul)
