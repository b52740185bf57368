"""csrc/wpack.hip -- the REAL kernel sources, launchers and C-ABI entries (mdetr_pack_params / mdetr_level_pos) -- on the HIP-on-CPU
shim, through monodetr_amd/wpack_ext.py.  The cases are in tests/wpack_cases.py; tests/test_wpack_gpu.py runs the same ones on the
device."""
import pytest
import torch

import native_emul
import wpack_cases as W

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def emul():
    return native_emul.lib()


def test_every_size_alignment_and_form_in_one_call_equals_cat_and_add(emul):
    W.check_sizes_alignments_and_both_forms(CPU, emul)


def test_adjacent_row_blocks_of_one_tensor_leave_their_neighbours_alone(emul):
    W.check_adjacent_blocks_of_one_tensor(CPU, emul)


def test_one_job_more_than_the_cap_takes_a_second_launch(emul):
    W.check_one_job_more_than_the_cap(CPU, emul)


def test_bf16_sums_are_rounded_once(emul):
    W.check_bf16_sums_round_once(CPU, emul)


def test_the_entries_refuse_what_the_kernels_cannot_take(emul):
    W.check_entry_refuses_bad_jobs(emul)


def test_pack_sites_forward_and_the_views_of_its_backward(emul):
    W.check_pack_sites_autograd(CPU, emul)


def test_level_positions_equal_the_framework_expression_and_padding_keeps_it(emul):
    W.check_level_positions(CPU, emul)


def test_the_family_is_listed_switched_and_off_by_default():
    from monodetr_amd import kernel_families as kf, wpack_ext
    assert "MDETR_PARAM_PACK" in kf.ALL_SWITCHES and "MDETR_PARAM_PACK" in kf.SWITCH_TESTS
    assert "MDETR_PARAM_PACK" in kf.COMMITTED_SWITCHES["bf16"]
    try:
        kf.apply_switches({"MDETR_PARAM_PACK"})
        assert wpack_ext.ENABLED and not wpack_ext.available(torch.zeros(1))                       # on, but nothing runs it on the host
        kf.apply_switches(set())
        assert not wpack_ext.ENABLED
    finally:
        kf.apply_switches(set())
