"""mdetr_msda_backward_to on the HIP-on-CPU shim: the one-pass MSDA backward (csrc/msda_fused.hip) writing grad_value in bf16, for fp32
and bf16 value / grad_out, against the same entry writing fp32 -- bit for bit where no corner leaves a block's reach, within one
bf16 ulp where the side buffer is folded in.  tests/test_msda_bf16_grad_value_gpu.py makes the same comparisons on the device."""
import ctypes

import pytest
import torch

import msda_grad_value_cases as C
import native_emul
from conftest import tune

TINY = [(8, 24), (4, 12), (2, 6), (1, 3)]             # S = 255; 4 x 8 tiles split level 0 into 2 x 3, levels 2 and 3 are chunked


def backward_to(p, elem, gv_dtype):
    """-> grad_value (gv_dtype), grad_loc, grad_attn, the workspace header's `far` word."""
    L = native_emul.lib()
    B, S, M, D = p["value"].shape
    Lq = p["loc"].shape[1]
    value, grad_out = (p["value"], p["grad_out"]) if elem == torch.float32 else (p["value"].to(elem), p["grad_out"].to(elem))
    gv = torch.full((B, S, M, D), 9.0, dtype=gv_dtype)
    gl, ga = torch.full_like(p["loc"], 7.0), torch.full_like(p["attn"], 5.0)
    n = L.mdetr_msda_backward_workspace_bytes(0, p["shapes"].data_ptr(), p["level_start"].data_ptr(), B, S, M, D, 4, Lq, 4)
    assert n > 0
    ws = torch.randint(0, 255, (n,), dtype=torch.uint8)                      # a fresh workspace holds anything
    code = lambda dt: 2 if dt == torch.bfloat16 else 0                        # noqa: E731
    rc = L.mdetr_msda_backward_to(code(elem), code(gv_dtype), value.data_ptr(), p["loc"].data_ptr(), p["attn"].data_ptr(), grad_out.data_ptr(),
                                  gv.data_ptr(), gl.data_ptr(), ga.data_ptr(), B, S, M, D, 4, Lq, 4, p["shapes"].data_ptr(),
                                  p["level_start"].data_ptr(), ws.data_ptr(), n, 0, None)
    assert rc == 0, ctypes.string_at(L.mdetr_last_error())
    return gv, gl, ga, int(ws[8:12].view(torch.int32).item())


@pytest.mark.parametrize("elem", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("Lq", [None, 50])
def test_bf16_grad_value_is_the_fp32_one_rounded_once(monkeypatch, elem, Lq):
    tune(monkeypatch, msda_tile_h=4, msda_tile_w=8, msda_reach=3, msda_whole_level_cells=30, msda_chunks=3)
    p = C.near_problem(1, 2, Lq, TINY, 1.4, seed=11)                          # |offset| + 1.5 <= reach
    gv32, gl32, ga32, far32 = backward_to(p, elem, torch.float32)
    gv16, gl16, ga16, far16 = backward_to(p, elem, torch.bfloat16)
    assert far32 == 0 and far16 == 0
    assert gv16.dtype == torch.bfloat16 and torch.equal(gv16, gv32.to(torch.bfloat16))
    assert torch.equal(gl16, gl32) and torch.equal(ga16, ga32)
    assert float(gv32.abs().max()) > 0


@pytest.mark.parametrize("elem", [torch.float32, torch.bfloat16])
def test_bf16_grad_value_with_the_side_buffer_is_within_one_ulp(monkeypatch, elem):
    """Uniform locations, gradients of one sign: the core value is rounded, the side buffer added, the sum rounded again -- at most
    one bf16 ulp from the fp32 result rounded once.  With both signs the first rounding can exceed the cancelled sum's ulp: held
    to the bound of msda_grad_value_cases.assert_far_path_bound instead (measured here: 0.64 / 0.75 of that bound, on
    results that cancel to nearly nothing and then lie tens of thousands of bf16 grid steps from the fp32 result rounded once)."""
    tune(monkeypatch, msda_tile_h=4, msda_tile_w=8, msda_reach=2, msda_whole_level_cells=30, msda_chunks=3)
    p = C.uniform_problem(1, 2, None, TINY, seed=12, positive=True)
    gv32, gl32, ga32, far32 = backward_to(p, elem, torch.float32)
    gv16, gl16, ga16, far16 = backward_to(p, elem, torch.bfloat16)
    assert far32 == 1 and far16 == 1                                          # the case is what it claims to be
    assert C.ulps_apart(gv16, gv32.to(torch.bfloat16)) <= 1
    assert torch.equal(gl16, gl32) and torch.equal(ga16, ga32)
    q = C.uniform_problem(1, 2, None, TINY, seed=12)
    mv32, ml32, ma32, far32 = backward_to(q, elem, torch.float32)
    mv16, ml16, ma16, far16 = backward_to(q, elem, torch.bfloat16)
    assert far32 == 1 and far16 == 1
    C.assert_far_path_bound(mv16, mv32, gv32)                                 # (p is q with |grad_out|)
    assert torch.equal(ml16, ml32) and torch.equal(ma16, ma32)


def test_a_geometry_the_one_pass_kernel_does_not_take_is_refused_and_nothing_is_written():
    L = native_emul.lib()
    p = C.uniform_problem(1, 2, 9, TINY, seed=1)
    B, S, M, D = p["value"].shape
    gv = torch.full((B, S, M, D), 9.0, dtype=torch.bfloat16)
    gl, ga = torch.full_like(p["loc"], 7.0), torch.full_like(p["attn"], 5.0)
    rc = L.mdetr_msda_backward_to(0, 2, p["value"].data_ptr(), p["loc"].data_ptr(), p["attn"].data_ptr(), p["grad_out"].data_ptr(), gv.data_ptr(),
                                  gl.data_ptr(), ga.data_ptr(), B, S, M, D, 4, 9, 4, p["shapes"].data_ptr(), p["level_start"].data_ptr(), None, 0, 0, None)
    assert rc == -4 and b"one-pass" in ctypes.string_at(L.mdetr_last_error())
    assert bool((gv == 9.0).all()) and bool((gl == 7.0).all())
    assert L.mdetr_msda_backward_to(1, 2, *([None] * 7), B, S, M, D, 4, 9, 4, None, None, None, 0, 0, None) == -1
