"""mdetr_detect_decode at the C boundary of the built library, without a GPU: what it refuses (with a message, before it looks at a
pointer), the ABI version, and its serial host form (device = -1) on the golden problem."""
import ctypes

import numpy as np
import pytest

import detect_cases as D


@pytest.fixture(scope="module")
def lib():
    from monodetr_amd import _capi, build
    build.build()
    return _capi.lib()


def _call(lib, ptrs, B, Q, C, topk, outs=(64, 64, None), device=0):
    return lib.mdetr_detect_decode(*ptrs, B, Q, C, topk, ctypes.c_double(0.2), *outs, device, None)


def test_abi_version_is_22(lib):
    from monodetr_amd import _capi
    assert lib.mdetr_abi_version() == 22 == _capi.ABI_VERSION and "mdetr_detect_decode" in _capi.SIGNATURES


def test_bad_arguments_return_the_argument_error_with_a_message(lib):
    some = [64] * 8                                                # never dereferenced: every call below is refused first
    for B, Q, C, topk, word in ((1, 50, 3, 0, b"topk=0"), (1, 50, 3, -1, b"topk=-1"), (1, 50, 3, 151, b"topk=151"), (1, 2049, 4, 50, b"Q * C <= 8192"),
                                (1, 8193, 1, 1, b"Q * C <= 8192"), (1, 65536, 65536, 1, b"Q * C <= 8192"), (-1, 50, 3, 50, b"B=-1"), (1, 0, 3, 1, b"Q=0"),
                                (1, 50, 0, 1, b"C=0")):
        assert _call(lib, some, B, Q, C, topk) == -1 and word in lib.mdetr_last_error(), (B, Q, C, topk, lib.mdetr_last_error())
        assert _call(lib, some, B, Q, C, topk, device=-1) == -1
    for missing in range(8):
        ptrs = [None if i == missing else 64 for i in range(8)]
        assert _call(lib, ptrs, 1, 50, 3, 50) == -1 and b"null pointer" in lib.mdetr_last_error()
    for outs in ((None, 64, None), (64, None, None)):
        assert _call(lib, some, 1, 50, 3, 50, outs=outs) == -1 and b"null pointer" in lib.mdetr_last_error()
    assert _call(lib, [66] + [64] * 7, 1, 50, 3, 50) == -3 and b"aligned" in lib.mdetr_last_error()          # an fp32 pointer off by 2
    assert _call(lib, [64] * 5 + [68] + [64] * 2, 1, 50, 3, 50) == -3                                          # an fp64 pointer off by 4
    assert _call(lib, some, 1, 50, 3, 50, device=-2) == -1 and b"device" in lib.mdetr_last_error()
    # an empty batch succeeds, looks at no pointer and needs no device
    assert _call(lib, [None] * 8, 0, 50, 3, 50, outs=(None, None, None)) == 0
    assert _call(lib, [None] * 8, 0, 50, 3, 151, outs=(None, None, None)) == -1                                # (limits still hold)


def test_host_form_of_the_built_library_on_the_golden_problem(lib):
    case = D.value_case(D.GOLDEN_SHAPE)
    rows, keep, dets37 = D.run_raw(lib, case, device=-1)
    assert D.check_all(case, rows, keep, dets37) == 67             # 32 + 35 recorded detections
    rows2, keep2, none = D.run_raw(lib, case, device=-1, want_dets37=False)
    assert none is None and np.array_equal(rows, rows2) and np.array_equal(keep, keep2)
