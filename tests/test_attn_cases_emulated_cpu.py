"""The attention cases of tests/attn_cases.py -- integer scores to the bit, random and peaked logits against fp64 with a rounding model,
the mask geometries -- through the CPU emulation of csrc/attn.hip (tests/native_emul.py), as tests/test_attn_cases_gpu.py runs them on
the device.  The bounds and their derivation are in attn_cases.py."""
import pytest
import torch

import attn_cases as C
import native_emul
from conftest import tune

BF16, F32 = torch.bfloat16, torch.float32
IDS = {BF16: "bf16", F32: "fp32"}


def _ext(defines=()):
    from monodetr_amd import attn_ext
    attn_ext._backend = native_emul.lib(defines)
    return attn_ext


@pytest.fixture
def ext():
    e = _ext()
    yield e
    e._backend = None


@pytest.fixture
def ext_remap():
    e = _ext(("MDETR_ATTN_STAGE_REMAP=1",))
    yield e
    e._backend = None


def test_closed_form_reference_equals_autograd_and_the_dropout_threshold_is_the_kernels():
    """attn_cases' closed-form fp64 gradients against autograd through `reference`, with a mask and dropout; and the restated
    threshold: float32(0.1) 2^32 = 429496736, which the double 0.1 misses by 7."""
    c = C.random_case("dropout_lead96", F32)
    q, k, v = (t.double().requires_grad_(True) for t in (c.q, c.k, c.v))
    out = C.reference(q, k, v, c.H, c.kpm, c.keep, float(torch.tensor(c.p, dtype=F32)), scale=c.scale)   # (the C float the kernels get)
    out.backward(c.go.double())
    for got, name in ((out.detach(), "out"), (q.grad, "dq"), (k.grad, "dk"), (v.grad, "dv")):
        assert (got - c.truth[name]).abs().max() <= 1e-12 * max(1.0, c.truth[name].abs().max().item()), name
    import numpy as np
    assert int(float(np.float32(0.1)) * 4294967296.0) == 429496736 and int(0.1 * 4294967296.0) == 429496729
    keep = C.keep_mask(C.RND_SEED, 2, 2, 70, 200, 0.1)
    assert abs(keep.double().mean().item() - 0.9) < 0.01


@pytest.mark.parametrize("dtype", [F32, BF16], ids=IDS.get)
@pytest.mark.parametrize("name", list(C.INTEGER_CASES))
def test_emulated_integer_scores_forward_to_the_bit(ext, name, dtype):
    C.check_integer_forward(ext.fused_attention, name, dtype, "cpu")


@pytest.mark.parametrize("dtype", [F32, BF16], ids=IDS.get)
@pytest.mark.parametrize("name", list(C.RANDOM_CASES))
def test_emulated_random_and_peaked_within_the_rounding_model(ext, name, dtype):
    C.check_random(ext.fused_attention, name, dtype, "cpu")


@pytest.mark.parametrize("dtype", [F32, BF16], ids=IDS.get)
def test_emulated_stage_remap_build_on_a_mask_geometry(ext_remap, dtype):
    C.check_integer_forward(ext_remap.fused_attention, "lead96", dtype, "cpu")
    C.check_random(ext_remap.fused_attention, "dropout_lead96", dtype, "cpu")


@pytest.mark.parametrize("name", ["wide_std8", "wide_std30", "wide_lead96"])
def test_emulated_key_split_on_the_peaked_and_masked_cases(ext, name, monkeypatch):
    """attn_ksplit=1: two 4-wave groups walk half of the key tiles each (330 keys = 5 tiles + 10 keys in 2 x 3 trips: group 1's last
    tile is all padding; with `lead96` group 0 starts on a fully masked tile) and merge (m, l, acc) through LDS."""
    tune(monkeypatch, attn_ksplit="1")
    C.check_random(ext.fused_attention, name, BF16, "cpu")


@pytest.mark.parametrize("name", ["Lk330", "Lk330_lead96"])
def test_emulated_key_split_integer_scores_to_the_bit(ext, name, monkeypatch):
    """The merge of the two key ranges scales by powers of two here: still exact."""
    tune(monkeypatch, attn_ksplit="1")
    C.check_integer_forward(ext.fused_attention, name, BF16, "cpu")
