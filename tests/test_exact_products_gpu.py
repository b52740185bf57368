"""Every matrix-product and convolution kernel of the repository on the GPU against an answer that is known to the BIT
(tests/exact_cases.py): integer operands whose partial sums stay below 2^24 are exact in fp32 in any summation order and any split
of the contraction, so each result must EQUAL the fp64 value rounded once to the output dtype -- no tolerance.  The operand sets put
bf16 rounding ties, pre-activations and mask elements that are exactly 0, and (for the fp32 form of csrc/tgemm.hip) every term of the
three-way split where random floats under a statistical bound never look.  Shapes come from the kernels' tile constants: below one
tile, a tile plus a ragged rest, several contraction slabs with a ragged last one; nothing near the workload's sizes.
tests/test_exact_products_emulated_cpu.py runs the same cases through the kernel sources on the CPU."""
import pytest
import torch

import exact_cases as X
from conftest import tune

pytestmark = pytest.mark.gpu

F32_VARIANTS = [("plain", "wide"), ("bias_f32", "wide"), ("res", "wide"), ("accum", "wide"), ("relu", "narrow"), ("dropout", "narrow")]


def dev():
    return torch.device("cuda", 0)


# ---- csrc/tgemm.hip ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,K,N", X.TGEMM_SHAPES)
@pytest.mark.parametrize("nn", [False, True])
@pytest.mark.parametrize("pf", ["1", "2"])
@pytest.mark.parametrize("tile", ["128x128", "128x64", "64x128", "64x64"])
def test_exact_tgemm_bf16_every_tile_pipeline_and_tail(monkeypatch, tile, pf, nn, T, K, N):
    tune(monkeypatch, tgemm_tile=tile, tgemm_pf=pf)
    for variant, kind in X.TGEMM_VARIANTS:
        X.check_tgemm(dev(), T, K, N, nn, variant, kind)


@pytest.mark.parametrize("T,K,N", X.TGEMM_SHAPES)
@pytest.mark.parametrize("with_res", [False, True])
def test_exact_tgemm_masked_bf16_zero_mask_elements(T, K, N, with_res):
    X.check_tgemm_masked(dev(), T, K, N, with_res)


@pytest.mark.parametrize("T,K,N", X.TGEMM_SHAPES)
@pytest.mark.parametrize("nn", [False, True])
@pytest.mark.parametrize("pf", ["1", "2"])
@pytest.mark.parametrize("tile", ["64x64", "128x64", "128x128"])
def test_exact_tgemm_f32_split_terms_and_tails(monkeypatch, tile, pf, nn, T, K, N):
    """(a) full-mantissa a x one-hot w, (b) one-hot a x full-mantissa w, (c) 11-bit x 10-bit integers; then the epilogue variants and the
    masked tail on integer data."""
    tune(monkeypatch, tgemm_f32_tile=tile, tgemm_f32_pf=pf)
    for kind in ("a", "w", "int"):
        X.check_tgemm_split(dev(), T, K, N, nn, kind)
    for variant, kind in F32_VARIANTS:
        X.check_tgemm(dev(), T, K, N, nn, variant, kind, torch.float32)
    if nn:
        for with_res in (False, True):
            X.check_tgemm_masked(dev(), T, K, N, with_res, torch.float32)


# ---- weight gradients over token rows ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,N", [(64, 64), (72, 264), (128, 128), (264, 72), (64, 128)])
@pytest.mark.parametrize("T", [136, 4408])
@pytest.mark.parametrize("form", ["1", "0"])
def test_exact_token_weight_gradient(monkeypatch, form, T, K, N):
    from monodetr_amd import conv_wgrad_ext
    tune(monkeypatch, twgrad=form)
    monkeypatch.setattr(conv_wgrad_ext, "ENABLED", True)
    if not X.check_token_wgrad(dev(), T, K, N):
        pytest.skip("this form does not take the shape")


@pytest.mark.parametrize("T,N,K", [(130, 64, 64), (4400, 128, 256)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_exact_small_wgrad(T, N, K, dtype):
    X.check_small_wgrad(dev(), T, N, K, dtype)


# ---- csrc/sgemm.hip ---------------------------------------------------------------------------------------------------------------------
def test_exact_sgemm_grouped_nt_with_every_tail():
    X.check_sgemm_nt(dev())


def test_exact_sgemm_grouped_nn_contraction_over_several_tensors():
    X.check_sgemm_nn(dev())


@pytest.mark.parametrize("T", [37, 550])
def test_exact_sgemm_grouped_tn_with_column_sums(T):
    X.check_sgemm_tn(dev(), T)


# ---- convolutions -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,C,N", [(2, 5, 7, 64, 32), (1, 13, 45, 64, 64), (2, 9, 33, 128, 64)])
def test_exact_conv3x3_forward_input_gradient_and_weight_gradient(monkeypatch, B, H, W, C, N):
    X.check_conv3x3(dev(), B, H, W, C, N, monkeypatch)


@pytest.mark.parametrize("B,H,W,C,N,k,split", [(2, 7, 10, 64, 64, 3, False), (1, 13, 18, 128, 64, 3, False), (1, 8, 8, 512, 64, 3, True),
                                               (1, 8, 9, 64, 64, 1, False), (2, 7, 12, 128, 128, 1, False)])
def test_exact_conv_strided_forward_input_gradient_and_weight_gradient(monkeypatch, B, H, W, C, N, k, split):
    X.check_conv_strided(dev(), B, H, W, C, N, k, monkeypatch, expect_split=split)


@pytest.mark.parametrize("B,H,W,C,N,k,stride", [(2, 9, 11, 64, 32, 3, 1), (2, 9, 11, 64, 32, 3, 2), (2, 9, 11, 64, 32, 1, 2), (1, 16, 20, 128, 96, 3, 1)])
def test_exact_conv_wgrad_direct(monkeypatch, B, H, W, C, N, k, stride):
    X.check_conv_wgrad(dev(), B, H, W, C, N, k, stride, monkeypatch)


@pytest.mark.parametrize("B,H,W", [(1, 37, 75), (2, 18, 40)])
def test_exact_conv_stem(B, H, W):
    X.check_conv_stem(dev(), B, H, W)


def test_exact_decimate_and_pointwise_conv(monkeypatch):
    X.check_decimate_pointwise(dev(), monkeypatch)
