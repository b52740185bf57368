"""Shared by tests/test_chunk_sums_tall_emulated_cpu.py and tests/test_chunk_sums_tall_gpu.py: the jobs of ``mdetr_chunk_sums_pitched``
(csrc/colsum.hip) on either side of the tall form's threshold (more than 128 chunks: 32 row lanes per 32 columns), as contiguous
partial sets and as a column range of a set twice as wide, and a two-site LayerNorm stack whose gamma / beta sums are registered.

Exact cases follow tests/exact_cases.py: the partials are integers small enough that every partial sum stays below 2^24, so the
fp32 sum is exact in ANY order and the kernel's result has to equal it bit for bit (one rounding for a bf16 result)."""
import contextlib
import zlib

import torch

CHUNKS = (1, 5, 64, 65, 128, 129, 1024)          # 128 | 129: the threshold between the two forms; 64 | 65: inside the serial form
COLS = (4, 512, 1028)                            # one thread's quad; the widest LayerNorm half; no multiple of either form's tile
AMP = 8191                                       # 1024 chunks * 8191 < 2^23: every partial sum is an exact fp32 integer


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def part_of(data, pitched):
    """The job's partials: `data` itself, or the right half of a set twice as wide (pitch = 2 cols, column offset = cols)."""
    if not pitched:
        return data
    wide = torch.full((data.shape[0], 2 * data.shape[1]), float("nan"), dtype=data.dtype, device=data.device)   # (the other half must not be read)
    wide[:, data.shape[1]:] = data
    return wide[:, data.shape[1]:]


def cases():
    return [(ch, co, pitched) for ch in CHUNKS for co in COLS for pitched in (False, True)]


def integer_partials(chunks, cols, dev):
    return torch.randint(-AMP, AMP + 1, (chunks, cols), generator=gen("int", chunks, cols)).float().to(dev)


def random_partials(chunks, cols, dev):
    return (torch.randn(chunks, cols, generator=gen("rnd", chunks, cols)) + 0.25).to(dev)


@contextlib.contextmanager
def chunk_sums_on(backend=None, poison=False, immediate=False):
    from monodetr_amd import chunk_sums
    saved = (chunk_sums.ENABLED, chunk_sums.POISON, chunk_sums.IMMEDIATE, chunk_sums._backend)
    chunk_sums.ENABLED, chunk_sums.POISON, chunk_sums.IMMEDIATE = True, poison, immediate
    if backend is not None:
        chunk_sums._backend = backend
    try:
        yield chunk_sums
    finally:
        chunk_sums.ENABLED, chunk_sums.POISON, chunk_sums.IMMEDIATE, chunk_sums._backend = saved


def check_exact(dev, backend=None):
    """Every case, fp32 and bf16 result, launched singly: bit equality with the exact sum."""
    with chunk_sums_on(backend) as cs:
        for chunks, cols, pitched in cases():
            data = integer_partials(chunks, cols, dev)
            part = part_of(data, pitched)
            want = data.double().sum(0)
            assert float(want.abs().max()) < 2 ** 24
            for dt in (torch.float32, torch.bfloat16):
                assert cs.supported(part, dt)
                got = cs.chunk_sum(part, dt)
                assert got.dtype == dt and got.shape == (cols,)
                assert torch.equal(got, want.float().to(dt)), (chunks, cols, pitched, dt)


def check_random(dev, backend=None):
    """Random fp32 partials against the fp64 sum: each of the `chunks` additions rounds once, so a column is off by at most
    chunks * 2^-24 * sum |x| in whatever order it is added; the bf16 result is the fp32 result rounded once."""
    with chunk_sums_on(backend) as cs:
        for chunks, cols, pitched in cases():
            data = random_partials(chunks, cols, dev)
            part = part_of(data, pitched)
            got = cs.chunk_sum(part, torch.float32)
            err = (got.double() - data.double().sum(0)).abs()
            bound = chunks * 2.0 ** -24 * data.double().abs().sum(0)
            print("chunks %d cols %d pitched %d: worst error / bound = %.3g" % (chunks, cols, pitched, float((err / bound).max())))
            assert bool((err <= bound).all()), (chunks, cols, pitched, float((err / bound).max()))
            assert torch.equal(cs.chunk_sum(part, torch.bfloat16), got.to(torch.bfloat16)), (chunks, cols, pitched)


def check_grouped_equals_single(dev, backend=None):
    """All cases registered inside ONE ``deferred()`` block, between jobs of the weight gradients' shape (more than one launch of 48
    jobs, tall and serial jobs mixed in each): every result equals the one its job gives launched alone."""
    with chunk_sums_on(backend) as cs:
        parts, dts = [], []
        for i, (chunks, cols, pitched) in enumerate(cases()):
            parts.append(part_of(random_partials(chunks, cols, dev), pitched))
            dts.append(torch.bfloat16 if i % 2 else torch.float32)
            if i % 3 == 0:
                parts.append(random_partials(16 + i, 2052, dev))
                dts.append(torch.float32 if i % 2 else torch.bfloat16)
        launches, real = [], cs._launch

        def counted(jobs):
            launches.append(len(jobs))
            return real(jobs)

        cs._launch = counted
        try:
            with cs.deferred():
                outs = [cs.chunk_sum(p, dt) for p, dt in zip(parts, dts)]
                assert len(cs._pending) == len(parts) and launches == []
            assert launches == [len(parts)] and len(parts) > 48
        finally:
            cs._launch = real
        for i, (p, dt, o) in enumerate(zip(parts, dts, outs)):
            assert torch.equal(o, cs.chunk_sum(p, dt)), (i, tuple(p.shape), p.stride())


class LnStack(torch.nn.Module):
    """Two residual LayerNorm sites (csrc/add_ln.hip through add_ln_ext.residual_layernorm), 256 and 128 wide; 600 rows give 150
    partial rows, a tall job for each of the four sums."""

    def __init__(self, dtype):
        super().__init__()
        self.n1, self.n2 = torch.nn.LayerNorm(256), torch.nn.LayerNorm(128)
        with torch.no_grad():
            for n in (self.n1, self.n2):
                n.weight.add_(0.1 * torch.randn(n.weight.shape, generator=gen("w", n.weight.numel())))
                n.bias.add_(0.1 * torch.randn(n.bias.shape, generator=gen("b", n.bias.numel())))
        self.to(dtype)

    def forward(self, a, b, c):
        from monodetr_amd import add_ln_ext
        y = add_ln_ext.residual_layernorm(a, b, self.n1, None)
        return add_ln_ext.residual_layernorm(y[:, :128].contiguous(), c, self.n2, None), y


def run_ln_stack(dev, dtype, mode, backend=None, iters=3, rows=600):
    """`iters` backward passes of the stack inside ``chunk_sums.deferred(model)`` -> per iteration {name: gradient}, and the number of
    jobs per chunk-sum launch.  mode "deferred": registered results hold NaN until the flush; "immediate": each sum at once."""
    from monodetr_amd import add_ln_ext
    saved = (add_ln_ext.ENABLED, add_ln_ext._backend)
    add_ln_ext.ENABLED = True
    if backend is not None:
        add_ln_ext._backend = backend
    try:
        with chunk_sums_on(backend, poison=mode == "deferred", immediate=mode == "immediate") as cs:
            model = LnStack(dtype).to(dev)
            launches, real = [], cs._launch

            def counted(jobs):
                launches.append(len(jobs))
                return real(jobs)

            cs._launch = counted
            grads = []
            try:
                for it in range(iters):
                    a, b = (torch.randn(rows, 256, generator=gen("ab", it, k)).to(dtype).to(dev) for k in range(2))
                    c = torch.randn(rows, 128, generator=gen("c", it)).to(dtype).to(dev)
                    for p in model.parameters():
                        p.grad = None
                    z, y = model(a, b, c)
                    loss = (z.float() * 0.01).sum() + (y.float() ** 2).sum() * 1e-3
                    with cs.deferred(model) as d:
                        assert d.reason is None
                        loss.backward()
                    grads.append({n: p.grad.detach().clone() for n, p in model.named_parameters()})
            finally:
                cs._launch = real
            return grads, launches
    finally:
        add_ln_ext.ENABLED, add_ln_ext._backend = saved


def check_ln_stack(dev, backend=None):
    for dtype in (torch.float32, torch.bfloat16):
        want, single = run_ln_stack(dev, dtype, "immediate", backend)
        got, grouped = run_ln_stack(dev, dtype, "deferred", backend)
        assert single == [1] * 12 and grouped == [4] * 3, (single, grouped)          # four sums per backward pass: singly | one launch
        for it in range(3):
            assert set(got[it]) == set(want[it]) and len(got[it]) == 4
            for n in want[it]:
                assert got[it][n].dtype == dtype and bool(torch.isfinite(got[it][n]).all()), (it, n)
                assert torch.equal(got[it][n], want[it][n]), (it, n)
