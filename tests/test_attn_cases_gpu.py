"""The attention cases of tests/attn_cases.py on the device: integer scores to the bit (both dtypes, every mask geometry, ragged sizes,
the row maximum in the first tile / the last full tile / the ragged tail, dropout 0.5), random and peaked logits (standard deviation
1, 8, 30) forward and backward against fp64 -- bf16 within 2^-7 A of the rounding model, fp32 within the derived bound -- and the
two-group key split (MDETR_TUNE attn_ksplit=1, bf16, >= 256 keys).  tests/test_attn_cases_emulated_cpu.py runs the same cases on the
shim; the bounds and their derivation are in attn_cases.py.  Every case prints its measured figures before it asserts."""
import pytest
import torch

import attn_cases as C
from conftest import tune

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
IDS = {BF16: "bf16", F32: "fp32"}


def _fused():
    from monodetr_amd.attn_ext import fused_attention
    return fused_attention


@pytest.mark.parametrize("dtype", [F32, BF16], ids=IDS.get)
@pytest.mark.parametrize("name", list(C.INTEGER_CASES))
def test_integer_scores_forward_to_the_bit(name, dtype):
    C.check_integer_forward(_fused(), name, dtype, "cuda")


@pytest.mark.parametrize("dtype", [F32, BF16], ids=IDS.get)
@pytest.mark.parametrize("name", list(C.RANDOM_CASES))
def test_random_and_peaked_within_the_rounding_model(name, dtype):
    C.check_random(_fused(), name, dtype, "cuda")


@pytest.mark.parametrize("name", ["wide_std8", "wide_std30", "wide_lead96"])
def test_key_split_on_the_peaked_and_masked_cases(name, monkeypatch):
    """attn_ksplit=1 (the launcher reads it per call): 330 keys = 5 tiles + 10 keys in 2 x 3 trips, group 1's last tile all padding;
    with `lead96` group 0 starts on a fully masked tile."""
    tune(monkeypatch, attn_ksplit="1")
    C.check_random(_fused(), name, BF16, "cuda")


@pytest.mark.parametrize("name", ["Lk330", "Lk330_lead96"])
def test_key_split_integer_scores_to_the_bit(name, monkeypatch):
    tune(monkeypatch, attn_ksplit="1")
    C.check_integer_forward(_fused(), name, BF16, "cuda")
