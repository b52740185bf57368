"""The normalisation cases of tests/norm_cases.py on the device: csrc/add_ln.hip on exact-arithmetic rows (one row, a partial
workgroup, 4 101 rows: two rows per backward wave and a ragged last block; every width, I/O and parameter type; the gamma / beta sums
through the column sum and through the deferred chunk sums), under dropout 0 .. 0.999 with a host and a device seed, on offset,
constant, tiny and big rows, a batch mixing them, and a view at an odd storage offset; csrc/group_norm.hip on exact-arithmetic groups
(C = 8 .. 2048, 1 .. 4 096 pixels: one and 256 row lanes, chunks shorter than the lanes, 32 chunks, a last chunk of one row), on
offset and constant groups, and its ReLU mask.  tests/test_norm_cases_emulated_cpu.py runs the same cases on the CPU emulation; the
bounds and what is asserted are in norm_cases.py.  Every case prints its figures before it asserts."""
import pytest
import torch

import norm_cases as N

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
IDS = {BF16: "bf16", F32: "fp32"}


@pytest.mark.parametrize("pdt", [F32, BF16], ids=IDS.get)
@pytest.mark.parametrize("io", [F32, BF16], ids=IDS.get)
@pytest.mark.parametrize("C", N.LN_WIDTHS)
@pytest.mark.parametrize("R", N.LN_EXACT_ROWS)
def test_layernorm_exact_rows(R, C, io, pdt):
    N.check_ln_exact(R, C, io, pdt, "cuda")


@pytest.mark.parametrize("io", [F32, BF16], ids=IDS.get)
@pytest.mark.parametrize("C", N.LN_WIDTHS)
@pytest.mark.parametrize("name", list(N.LN_BOUNDED))
def test_layernorm_against_fp64(name, C, io):
    N.check_ln_bounded(name, C, io, F32, "cuda")


@pytest.mark.parametrize("io", [F32, BF16], ids=IDS.get)
@pytest.mark.parametrize("name,C", [("p01", 256), ("mixed", 128), ("constant", 512)])
def test_layernorm_against_fp64_with_bf16_parameters(name, C, io):
    N.check_ln_bounded(name, C, io, BF16, "cuda")


@pytest.mark.parametrize("io", [F32, BF16], ids=IDS.get)
@pytest.mark.parametrize("C", N.LN_WIDTHS)
def test_layernorm_mask_is_the_same_for_a_host_and_a_device_seed(C, io):
    N.check_ln_seed_forms(C, io, "cuda")


@pytest.mark.parametrize("io", [F32, BF16], ids=IDS.get)
@pytest.mark.parametrize("C", N.LN_WIDTHS)
def test_layernorm_of_a_view_at_an_odd_storage_offset(C, io):
    N.check_ln_bounded("p01", C, io, F32, "cuda", odd_view=True)


def _gn_exact_params():
    """Every (C, HW, N) of C in {8, 64, 256, 2048}, HW in {1, 63, 64, 65, 128, 257, 2048, 2049, 4096}, N in {1, 3}, except
    (2048, 2048, 3), (2048, 2049, 3) and (2048, 4096, 3) (12.6 - 25 M elements: N = 1 runs at those three).  Shapes up to 70 000
    elements run all three dtype combinations, the larger ones one each, in turn by (C + HW + N) % 3."""
    shapes = sorted(set(N.gn_exact_shapes(N.GN_HW, 1 << 22) + N.gn_exact_shapes(N.GN_HW_POW2, 1 << 22)))
    shapes += [(2048, HW, 1) for HW in (2049, 4096) if (2048, HW, 1) not in shapes]
    out = []
    for C, HW, n in shapes:
        every = C * HW * n <= 70000
        out += [(C, HW, n) + dt for k, dt in enumerate(N.GN_DTYPES) if every or k == (C + HW + n) % 3]
    return out


@pytest.mark.parametrize("C,HW,n,io,pdt", _gn_exact_params(), ids=lambda v: IDS.get(v, str(v)))
def test_group_norm_exact_groups(C, HW, n, io, pdt):
    N.check_gn_exact(C, HW, n, io, pdt, "cuda")


def _gn_bounded_params():
    out = []
    for name in N.GN_BOUNDED:
        for io, pdt in N.GN_DTYPES:
            for variant in ("plain", "offset", "constant"):
                if variant == "plain" or io == F32 or name == "groups768":
                    out.append((name, variant, io, pdt))
    return out


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("name,variant,io,pdt", _gn_bounded_params(), ids=lambda v: IDS.get(v, str(v)))
def test_group_norm_against_fp64(name, variant, io, pdt, relu):
    N.check_gn_bounded(name, io, pdt, variant, relu, "cuda")
