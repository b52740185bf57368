"""The exact-arithmetic cases of tests/exact_cases.py through the REAL kernel sources on the HIP-on-CPU shim (tests/native_emul.py), at
the smallest shape per entry point, and the helper's own premise checks.  Integer operands below 2^24 make every partial sum exact in
fp32, so each result is compared for EQUALITY with the fp64 value rounded once; tests/test_exact_products_gpu.py runs the same cases
(and the larger shapes) on the GPU."""
import pytest
import torch

import exact_cases as X
import native_emul
from conftest import tune

CPU = torch.device("cpu")
EXTS = ("tgemm_ext", "bias_act_ext", "conv_wgrad_ext", "small_wgrad_ext", "sgemm_ext", "conv3x3_ext", "conv_taps_ext", "conv_stem_ext",
        "decimate_ext")


@pytest.fixture()
def emul(monkeypatch):
    import importlib
    lib = native_emul.lib()
    for name in EXTS:
        monkeypatch.setattr(importlib.import_module("monodetr_amd." + name), "_backend", lib)
    return lib


# ---- the helper itself ------------------------------------------------------------------------------------------------------------------
def test_rounding_shares_and_the_expected_value_on_known_numbers():
    ref = torch.tensor([256.0, 257.0, 258.0, 259.0, 261.0, -257.0, -259.0, 513.0, 514.0, 3.0], dtype=torch.float64)
    inexact, tie = X.bf16_rounding_shares(ref)
    assert (inexact, tie) == (0.7, 0.6)                                 # 257 259 261 -257 -259 513 514 need rounding; all of them but 513 are ties
    want = X.expected(ref, ref.abs(), torch.bfloat16, wide=True)
    assert want.tolist() == [256.0, 256.0, 258.0, 260.0, 260.0, -256.0, -260.0, 512.0, 512.0, 3.0]      # ties to even
    with pytest.raises(X.PremiseError):
        X.expected(ref + 0.5, ref.abs() + 1, torch.float32)            # not integers
    with pytest.raises(X.PremiseError):
        X.expected(ref, ref.abs() + 2.0 ** 24, torch.float32)          # beyond the cap
    small = torch.arange(200, dtype=torch.float64)
    with pytest.raises(X.PremiseError):
        X.expected(small, small, torch.bfloat16, wide=True)            # nothing to round
    with pytest.raises(X.PremiseError):
        X.expected(small, small, torch.float32, zeros_of=small + 1)    # no zeros


def test_assert_bits_equal_reports_count_index_values_and_ulps():
    want = torch.tensor([[1.0, 2.0], [256.0, -3.0]], dtype=torch.bfloat16)
    X.assert_bits_equal(want.clone(), want)
    X.assert_bits_equal(torch.tensor([0.0, float("nan")]), torch.tensor([-0.0, float("nan")]))
    got = want.clone()
    got[1, 0] = 260.0
    with pytest.raises(AssertionError, match=r"1 of 4 elements differ; first at \(1, 0\): got 260.0, want 256.0; largest difference 2 ulp of bfloat16"):
        X.assert_bits_equal(got, want, "x")
    with pytest.raises(AssertionError, match="1 ulp of float32"):
        X.assert_bits_equal(torch.tensor([1.0 + 2.0 ** -23]), torch.tensor([1.0]))
    with pytest.raises(AssertionError):
        X.assert_bits_equal(torch.tensor([float("nan")]), torch.tensor([1.0]))


@pytest.mark.parametrize("T,K,N", X.TGEMM_SHAPES)
def test_every_case_of_the_table_meets_its_premises(T, K, N):
    """The operands of every tgemm / split case at every shape of the GPU file: `expected` and `split_case` raise otherwise."""
    for nn in (False, True):
        for kind in ("wide", "narrow"):
            a, w, b, r = X.tgemm_operands(T, K, N, nn, kind)
            ref, mag = X.product_f64(a, w, nn, b, None)
            X.expected(ref.clamp(min=0), mag, torch.bfloat16, wide=kind == "wide", zeros_of=ref if kind == "narrow" else None, what=kind)
        for kind in ("a", "w", "int"):
            X.split_case(T, K, N, nn, kind)


# ---- csrc/tgemm.hip ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nn", [False, True])
@pytest.mark.parametrize("tile,pf,shape", [("128x128", "2", 0), ("128x64", "1", 1), ("64x128", "2", 1), ("64x64", "1", 1), ("128x128", "1", 1)])
def test_tgemm_bf16_exact(emul, monkeypatch, tile, pf, shape, nn):
    tune(monkeypatch, tgemm_tile=tile, tgemm_pf=pf)
    T, K, N = X.TGEMM_SHAPES[shape]
    for variant, kind in X.TGEMM_VARIANTS:
        X.check_tgemm(CPU, T, K, N, nn, variant, kind)
    for with_res in (False, True):
        X.check_tgemm_masked(CPU, T, K, N, with_res)


F32_VARIANTS = [("plain", "wide"), ("bias_f32", "wide"), ("res", "wide"), ("accum", "wide"), ("relu", "narrow"), ("dropout", "narrow")]


@pytest.mark.parametrize("nn", [False, True])
@pytest.mark.parametrize("tile,pf,shape", [("128x128", "2", 0), ("64x64", "1", 1), ("128x64", "2", 1), ("128x128", "1", 1)])
def test_tgemm_f32_exact(emul, monkeypatch, tile, pf, shape, nn):
    tune(monkeypatch, tgemm_f32_tile=tile, tgemm_f32_pf=pf)
    T, K, N = X.TGEMM_SHAPES[shape]
    for kind in ("a", "w", "int"):
        X.check_tgemm_split(CPU, T, K, N, nn, kind)
    for variant, kind in F32_VARIANTS:
        X.check_tgemm(CPU, T, K, N, nn, variant, kind, torch.float32)
    for with_res in (False, True):
        X.check_tgemm_masked(CPU, T, K, N, with_res, torch.float32)


# ---- weight gradients over token rows -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,T,K,N", [("1", 136, 72, 264), ("1", 136, 64, 64), ("0", 136, 64, 128)])
def test_token_weight_gradient_exact(emul, monkeypatch, form, T, K, N):
    tune(monkeypatch, twgrad=form)
    assert X.check_token_wgrad(CPU, T, K, N)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_small_wgrad_exact(emul, dtype):
    X.check_small_wgrad(CPU, 130, 64, 64, dtype)


def test_sgemm_grouped_exact(emul):
    X.check_sgemm_nt(CPU)
    X.check_sgemm_nn(CPU)
    X.check_sgemm_tn(CPU, 37)


# ---- convolutions -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,C,N", [(2, 5, 7, 64, 32), (1, 5, 9, 64, 64)])
def test_conv3x3_exact(emul, monkeypatch, B, H, W, C, N):
    X.check_conv3x3(CPU, B, H, W, C, N, monkeypatch)


@pytest.mark.parametrize("B,H,W,C,N,k,split", [(2, 7, 10, 64, 64, 3, False), (1, 8, 9, 64, 64, 1, False), (1, 8, 8, 512, 64, 3, True)])
def test_conv_strided_exact(emul, monkeypatch, B, H, W, C, N, k, split):
    X.check_conv_strided(CPU, B, H, W, C, N, k, monkeypatch, expect_split=split)


@pytest.mark.parametrize("k,stride", [(3, 1), (3, 2), (1, 2)])
def test_conv_wgrad_exact(emul, monkeypatch, k, stride):
    X.check_conv_wgrad(CPU, 2, 9, 11, 64, 32, k, stride, monkeypatch)


def test_conv_stem_exact(emul):
    X.check_conv_stem(CPU, 2, 18, 40)


def test_decimate_and_pointwise_conv_exact(emul, monkeypatch):
    X.check_decimate_pointwise(CPU, monkeypatch)
