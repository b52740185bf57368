"""The LDS row pitch of conv3x3_f32_kernel (csrc/conv3x3.hip: 40 bf16 = 20 dwords per row of a 32-channel slab) under the bank model
of tests/test_lds_bank_model_cpu.py: the ds_read_b128 fragment reads of every tile shape -- 16 consecutive rows for the weights and
the 32-wide blocks, the rotated row sets of the narrow blocks at a halo pitch = 8 (mod 16) pixels -- are conflict-free, because row i
starts at bank quad 5 i (mod 16) and i -> 5 i is a bijection there.  A 48-element pitch (6 i mod 16) would not be."""
import pytest

from test_lds_bank_model_cpu import B128_READ_GROUPS, worst_conflict

K_PAD = 40                                                             # kPadF


def halo_row(lane, wc, gc):
    """LDS row of the halo pixel a lane of wave 0 reads for tap (0, 0): Tile<WC, GC>'s pitch and the kernel's pixel numbering."""
    col = lane & 31
    halo_w = gc * wc + 2
    pitch = halo_w if wc == 32 else (24 if halo_w <= 24 else 40)
    pin = ((col & 15) + 8 * (col >> 4)) & 15 if wc == 16 else col % wc
    return (col // wc) * pitch + pin


@pytest.mark.parametrize("wc,gc", [(32, 1), (16, 1), (16, 2), (8, 4), (8, 2)])
def test_halo_fragment_reads_are_conflict_free(wc, gc):
    for tap_shift in range(3):                                         # (tap column s moves every lane by one row)
        for ks in range(2):
            addr = lambda l: 2 * ((halo_row(l, wc, gc) + tap_shift) * K_PAD + 8 * (l >> 5) + 16 * ks)     # noqa: E731
            assert worst_conflict(addr, 16, B128_READ_GROUPS, 64) == 1, (wc, gc, tap_shift, ks)


def test_weight_fragment_reads_are_conflict_free_and_the_model_tells_a_bad_pitch():
    assert worst_conflict(lambda l: 2 * ((l & 31) * K_PAD + 8 * (l >> 5)), 16, B128_READ_GROUPS, 64) == 1
    assert worst_conflict(lambda l: 2 * ((l & 31) * 48 + 8 * (l >> 5)), 16, B128_READ_GROUPS, 64) > 1
