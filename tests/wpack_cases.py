"""The cases of csrc/wpack.hip (mdetr_pack_params, mdetr_level_pos) shared by tests/test_wpack_emulated_cpu.py (the kernel source on
the HIP-on-CPU shim) and tests/test_wpack_gpu.py (the device).  The expected values are the framework's: ``torch.cat`` / ``+`` /
today's level-position expression on the same inputs, compared with ``torch.equal``."""
import contextlib

import torch

GUARD = 1234.0
SIZES = (0, 1, 7, 8, 9, 128, 81, 256 * 256 + 3)       # the last one: 33 workgroups' worth of bf16 pieces and a ragged tail
CAP = 48                                               # csrc/wpack.h: kPackJobs


@contextlib.contextmanager
def wpack_on(backend=None, enabled=True):
    from monodetr_amd import wpack_ext
    saved = (wpack_ext.ENABLED, wpack_ext._backend)
    wpack_ext.ENABLED = enabled
    if backend is not None:
        wpack_ext._backend = backend
    try:
        yield wpack_ext
    finally:
        wpack_ext.ENABLED, wpack_ext._backend = saved


def gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * (int(k) + 17) for i, k in enumerate(key)) % (2 ** 31))


def values(n, dtype, g):
    """Mixed magnitudes: sums that cancel, sums that round."""
    x = torch.randn(n, generator=g) * torch.exp2(torch.randint(-6, 7, (n,), generator=g).float())
    return x.to(dtype)


def carve(n, dtype, dev, misalign, fill=None, g=None):
    """A dense [n] tensor that starts `misalign` elements behind a 16-byte boundary, with 16 guard elements either side -> (buffer, view)."""
    buf = torch.full((n + misalign + 48,), GUARD, dtype=dtype, device=dev)
    assert buf.data_ptr() % 16 == 0
    view = buf[16 + misalign:16 + misalign + n]
    if g is not None:
        view.copy_(values(n, dtype, g).to(dev))
    return buf, view


def check_sizes_alignments_and_both_forms(dev, backend=None):
    """Every size x {copy, sum} x {bf16, fp32} x destination / source offsets from a 16-byte boundary, ALL in one call (so bf16 and
    fp32, src1 NULL and non-NULL share launches, and the list is longer than the per-launch cap); guards stay untouched."""
    with wpack_on(backend) as wp:
        jobs, want = [], []
        for k, n in enumerate(SIZES):
            for dtype in (torch.bfloat16, torch.float32):
                per16 = 16 // dtype.itemsize
                for summed in (False, True):
                    for dmis, smis in ((0, 0), (81 % per16, 0), (3, 3), (0, 1)):
                        g = gen(k, dtype.itemsize, summed, dmis, smis)
                        dbuf, dst = carve(n, dtype, dev, dmis)
                        _, s0 = carve(n, dtype, dev, smis, g=g)
                        _, s1 = carve(n, dtype, dev, (smis * 2) % per16, g=g) if summed else (None, None)
                        jobs.append((dst, s0, s1))
                        want.append((dbuf, dst, s0 + s1 if summed else s0.clone(), (n, dtype, summed, dmis, smis)))
        assert len(jobs) > CAP
        wp.launch(jobs)
        for dbuf, dst, ref, what in want:
            assert torch.equal(dst, ref), what
            assert bool((dbuf[:16 + what[3]] == GUARD).all()) and bool((dbuf[16 + what[3] + what[0]:] == GUARD).all()), what


def check_adjacent_blocks_of_one_tensor(dev, backend=None):
    """[W_a; W_b] and the bias block that starts at element 81 of its packed tensor: two jobs write adjacent slices; what lies before,
    between (nothing) and behind them is left alone."""
    with wpack_on(backend) as wp:
        for dtype in (torch.bfloat16, torch.float32):
            g = gen(81, dtype.itemsize)
            a, b = values(81, dtype, g).to(dev), values(47, dtype, g).to(dev)
            buf = torch.full((5 + 81 + 47 + 5,), GUARD, dtype=dtype, device=dev)
            wp.launch([(buf[5:86], a, None), (buf[86:133], b, None)])
            assert torch.equal(buf[5:133], torch.cat((a, b), 0))
            assert bool((buf[:5] == GUARD).all()) and bool((buf[133:] == GUARD).all())
            wa, wb = values(81 * 8, dtype, g).view(81, 8).to(dev), values(47 * 8, dtype, g).view(47, 8).to(dev)
            wa2, wb2 = values(81 * 8, dtype, g).view(81, 8).to(dev), values(47 * 8, dtype, g).view(47, 8).to(dev)
            out = torch.full((128, 8), GUARD, dtype=dtype, device=dev)
            wp.launch([(out[:81], wa, wa2), (out[81:], wb, wb2)])
            assert torch.equal(out, torch.cat((wa + wa2, wb + wb2), 0))


def check_one_job_more_than_the_cap(dev, backend=None):
    with wpack_on(backend) as wp:
        g = gen(49)
        srcs = [values(9 + i, torch.bfloat16 if i % 2 else torch.float32, g).to(dev) for i in range(CAP + 1)]
        outs = [torch.full_like(s, GUARD) for s in srcs]
        wp.launch([(o, s, None) for o, s in zip(outs, srcs)])
        for i, (o, s) in enumerate(zip(outs, srcs)):
            assert torch.equal(o, s), i


def check_bf16_sums_round_once(dev, backend=None):
    """Ties (to even, both ways), a sum just above a tie, cancellation down to the last bit and to zero, overflow to infinity:
    a second rounding anywhere on the way would show."""
    e = 2.0 ** -8
    pairs = [(1.0, e), (1.0 + 2 * e, e), (1.0, e * (1 + 2.0 ** -7)), (1.0, -e / 2), (258.0, -256.0), (1.0 + 2 * e, -1.0), (3.0e38, 3.0e38),
             (3.0e38, -3.0e38), (2.0 ** -126, 2.0 ** -133), (0.0, -0.0), (1.0e-3, 1.0e3), (-1.0 - 2 * e, -e)]
    a = torch.tensor([p[0] for p in pairs], dtype=torch.bfloat16, device=dev)
    b = torch.tensor([p[1] for p in pairs], dtype=torch.bfloat16, device=dev)
    assert float(a[0] + b[0]) == 1.0 and float(a[1] + b[1]) == 1.0 + 4 * e and float(a[2] + b[2]) == 1.0 + 2 * e     # (what the framework gives)
    g = gen(7)
    a, b = torch.cat((a, values(4096, torch.bfloat16, g).to(dev))), torch.cat((b, values(4096, torch.bfloat16, g).to(dev)))
    b[100:200] = -a[100:200] * (1 + 2.0 ** -7)                                                  # large cancellation
    with wpack_on(backend) as wp:
        for mis in (0, 1):
            _, dst = carve(a.numel(), torch.bfloat16, dev, mis)
            wp.launch([(dst, a, b)])
            ref = a + b
            assert torch.equal(dst.view(torch.int16), ref.view(torch.int16)), mis                     # (bits: -0.0, infinities)


def check_entry_refuses_bad_jobs(backend):
    import ctypes
    from monodetr_amd import wpack_ext
    L = backend
    x = torch.zeros(32)
    job = (wpack_ext._Job * 1)()
    job[0].dst, job[0].src0, job[0].src1, job[0].elements, job[0].dtype = x.data_ptr(), x.data_ptr(), None, 8, 1       # MDETR_F64
    ptr = ctypes.cast(job, ctypes.c_void_p)
    assert L.mdetr_pack_params(ptr, 0, -1, None) == 0
    assert L.mdetr_pack_params(ptr, 1, -1, None) != 0 and b"mdetr_pack_params" in ctypes.string_at(L.mdetr_last_error())
    job[0].dtype, job[0].src0 = 0, x.data_ptr() + 2
    assert L.mdetr_pack_params(ptr, 1, -1, None) != 0                                           # fp32 source not 4-byte aligned
    job[0].src0, job[0].elements = x.data_ptr(), -1
    assert L.mdetr_pack_params(ptr, 1, -1, None) != 0
    job[0].elements, job[0].dst = 8, None
    assert L.mdetr_pack_params(ptr, 1, -1, None) != 0
    job[0].elements = 0
    assert L.mdetr_pack_params(ptr, 1, -1, None) == 0                                           # an empty job needs no pointers
    counts = (ctypes.c_int64 * 1)(4)
    assert L.mdetr_level_pos(x.data_ptr(), 0, x.data_ptr(), 0, x.data_ptr(), 0, counts, 1, 12, -1, None) != 0       # C % 8
    assert L.mdetr_level_pos(x.data_ptr(), 0, x.data_ptr(), 0, x.data_ptr(), 0, counts, 9, 8, -1, None) != 0        # levels
    assert L.mdetr_level_pos(x.data_ptr() + 4, 0, x.data_ptr(), 0, x.data_ptr(), 0, counts, 1, 8, -1, None) != 0    # alignment


def check_pack_sites_autograd(dev, backend=None):
    """`pack_sites` on a concatenated site and a summed one: the packed tensors equal cat / + of the sources, the backward hands each
    source its row block of the packed gradient (a pair the same block twice), and a site whose packed tensors go unused gets None."""
    with wpack_on(backend) as wp:
        for dtype in (torch.bfloat16, torch.float32):
            g = gen(3, dtype.itemsize)
            mk = lambda *shape: values(int(torch.tensor(shape).prod()), dtype, g).view(*shape).to(dev).requires_grad_(True)
            wa, wb, ba, bb = mk(16, 8), mk(8, 8), mk(16), mk(8)
            q = [mk(9, 8) for _ in range(4)] + [mk(9) for _ in range(4)]
            unused = [mk(4, 8), mk(4, 8), mk(4), mk(4)]
            sites = [("cat", ((wa,), (wb,)), ((ba,), (bb,))),
                     ("sum", ((q[0], q[1]), (q[2], q[3])), ((q[4], q[5]), (q[6], q[7]))),
                     ("unused", ((unused[0],), (unused[1],)), ((unused[2],), (unused[3],))),
                     ("refused", ((wa,), (wb.float() if dtype == torch.bfloat16 else wb.bfloat16(),)), ((ba,), (bb,)))]
            packed = wp.pack_sites(sites)
            assert set(packed) == {"cat", "sum", "unused"}                                      # mixed dtypes: the site keeps its own code
            w, b = packed["cat"]
            assert torch.equal(w, torch.cat((wa, wb), 0)) and torch.equal(b, torch.cat((ba, bb), 0))
            sw, sb = packed["sum"]
            assert torch.equal(sw, torch.cat((q[0] + q[1], q[2] + q[3]), 0)) and torch.equal(sb, torch.cat((q[4] + q[5], q[6] + q[7]), 0))
            gw, gb, gsw, gsb = (values(t.numel(), dtype, g).view(t.shape).to(dev) for t in (w, b, sw, sb))
            torch.autograd.backward([w, b, sw, sb], [gw, gb, gsw, gsb])
            assert torch.equal(wa.grad, gw[:16]) and torch.equal(wb.grad, gw[16:]) and torch.equal(ba.grad, gb[:16]) and torch.equal(bb.grad, gb[16:])
            for i, (grad, lo) in enumerate(((gsw, 0), (gsw, 0), (gsw, 9), (gsw, 9), (gsb, 0), (gsb, 0), (gsb, 9), (gsb, 9))):
                assert torch.equal(q[i].grad, grad[lo:lo + 9]), i
            assert all(u.grad is None for u in unused)


LEVELS = [(3, 5), (2, 3), (1, 2), (1, 1)]


def sine_levels(dev, C, B, padded=False):
    """The sine encodings of LEVELS as the model gets them: from PositionEmbeddingSine, for masks built unpadded (or not)."""
    from monodetr_amd.monodetr.position_encoding import PositionEmbeddingSine
    from monodetr_amd.utils.misc import NestedTensor, mark_no_padding
    pe = PositionEmbeddingSine(C // 2, normalize=True)
    out = []
    for H, W in LEVELS:
        mask = torch.zeros(B, H, W, dtype=torch.bool, device=dev)
        out.append((pe, NestedTensor(None, mask if padded else mark_no_padding(mask))))
    return out


def level_expression(embed, dtype, pos):
    return torch.cat([p.flatten(2).transpose(1, 2) + embed[l].view(1, 1, -1) for l, p in enumerate(pos)], 1).to(dtype)


def check_level_positions(dev, backend=None):
    """LEVELS, C = 8 and 256, every pairing of an fp32 / bf16 encoding (the bf16 one as backbone.Joiner casts and keeps it) with an
    fp32 / bf16 embedding and result: one [S, C] tensor with a stride-0 batch axis, equal to today's expression; the gradient of the
    embedding equal to today's; a padded batch takes today's path."""
    from monodetr_amd.monodetr.backbone import Joiner
    from monodetr_amd.monodetr.depthaware_transformer import _LevelPos

    class Stages(torch.nn.Module):
        strides, num_channels = [8], [8]

    B, S = 3, sum(h * w for h, w in LEVELS)
    for C in (8, 256):
        levels = sine_levels(dev, C, B)
        joiner = Joiner(Stages(), levels[0][0])
        for pos_dtype in (torch.float32, torch.bfloat16):
            for dtype in (torch.float32, torch.bfloat16):
                g = gen(C, pos_dtype.itemsize, dtype.itemsize)
                embed_on, embed_off = (torch.randn(len(LEVELS), C, generator=g.manual_seed(5)).to(dtype).to(dev).requires_grad_(True) for _ in range(2))
                dy = torch.randn(B, S, C, generator=g).to(dtype).to(dev)
                with wpack_on(backend) as wp:
                    pos = [joiner._as(x, pe(x), pos_dtype) for pe, x in levels]
                    assert all(p.dtype == pos_dtype and p._mdetr_sine_const for p in pos)
                    out = _LevelPos.apply(embed_on, dtype, *pos)
                    again = _LevelPos.apply(embed_on, dtype, *[joiner._as(x, pe(x), pos_dtype) for pe, x in levels])
                    assert out.shape == (B, S, C) and out.stride() == (0, C, 1) and out.dtype == dtype, (out.shape, out.stride())
                    assert again.data_ptr() != out.data_ptr() and torch.equal(again, out)       # a new tensor per call, the cached encoding
                    out.backward(dy)
                with wpack_on(backend, enabled=False):
                    ref = _LevelPos.apply(embed_off, dtype, *pos)
                    assert ref.stride() == (S * C, C, 1)
                    ref.backward(dy)
                assert torch.equal(ref, level_expression(embed_off.detach(), dtype, pos))
                assert torch.equal(out, ref), (C, pos_dtype, dtype)
                assert torch.equal(embed_on.grad, embed_off.grad), (C, pos_dtype, dtype)
        with wpack_on(backend):
            padded = [pe(x) for pe, x in sine_levels(dev, C, B, padded=True)]
            embed = torch.randn(len(LEVELS), C).to(dev)
            out = _LevelPos.apply(embed, torch.float32, *padded)
            assert out.stride() == (S * C, C, 1) and torch.equal(out, level_expression(embed, torch.float32, padded))
