"""Cases for the fp32 form of csrc/twgrad.hip (mdetr_token_wgrad_f32), shared by tests/test_twgrad_f32_emulated_cpu.py (the real
source on the HIP-on-CPU shim) and tests/test_twgrad_f32_gpu.py (test infrastructure).

Exact cases come from `exact_cases.split_case` BY TRANSPOSITION: split_case(N, T, C, False, kind) gives a [N, T], w_nk [C, T] and
want = a w_nk^T [N, C]; with dy = a^T [T, N] and x = w_nk^T [T, C] the weight gradient dW = dy^T x IS that product, known to the bit:
  "a"    full-mantissa dY against a one-hot +-2^e X: dW is a scaled copy of a dY row (dy.hi / mid / lo x x.hi);
  "w"    the mirror image (dy.hi x x.hi / mid / lo); every dY column holds one +-2^e, so db is that value;
  "int"  11-bit x 10-bit integers (mid x mid and the cross terms); db is an integer sum below 2^24.
One more db case: a single full-mantissa value per dY column (all three ones-MFMA planes).  Small integers
(`exact_cases.wgrad_operands`) are exact in any summation order.  Every premise is checked from the operands and the fp64 reference
alone; `PremiseError` is the guard."""
import functools

import torch

from exact_cases import CAP, F32, PremiseError, expected, full_mantissa, gen, split_case, wgrad_operands
from gemm_bounds import assert_product_close

TILES = ("64x64", "128x64", "64x128", "128x128")                  # MDETR_TUNE twgrad_f32_tile: every tile the launcher instantiates (BN x BC)
SHAPES = [(33, 8, 8), (136, 64, 32), (264, 64, 256), (300, 264, 72), (1000, 128, 160), (4101, 256, 256)]      # (T, C, N)
EXACT_SHAPES = [(33, 8, 8), (300, 264, 72), (4101, 256, 256)]
KINDS = ("a", "w", "int")


def partials(lib, x, dy, with_bias):
    """The raw entry on operands wherever they live -> fp32 [chunks, N C (+ N)], pre-filled with NaN: every chunk must write every element."""
    T, C = x.shape
    N = dy.shape[1]
    chunks = lib.mdetr_token_wgrad_f32_chunks(T, C, N)
    assert chunks >= 1, (T, C, N, chunks)
    cols = N * C + (N if with_bias else 0)
    part = torch.full((chunks, cols), float("nan"), device=x.device)
    cuda = x.is_cuda
    rc = lib.mdetr_token_wgrad_f32(x.data_ptr(), dy.data_ptr(), part.data_ptr(), part.numel(), T, C, N, 1 if with_bias else 0,
                                   x.device.index if cuda else -1, torch.cuda.current_stream(x.device).cuda_stream if cuda else None)
    assert rc == 0, lib.mdetr_last_error()
    assert not bool(torch.isnan(part).any()), "a chunk left elements of its partial unwritten"
    return part


def chunk_order_sum(part):
    """The chunks added in order, in fp32 (what csrc/colsum.hip does for up to 128 chunks)."""
    tot = part[0].clone()
    for c in range(1, part.shape[0]):
        tot += part[c]
    return tot


@functools.lru_cache(maxsize=None)
def random_case(T, C, N):
    """x [T, C], dy [T, N] fp32 and the fp64 values / magnitudes of dW and db.  Shared: never written to."""
    g = gen(T, C, N, 9)
    x = torch.randn(T, C, generator=g) * 0.5
    dy = torch.randn(T, N, generator=g) * 0.2
    return x, dy, dy.double().t() @ x.double(), dy.double().abs().t() @ x.double().abs(), dy.double().sum(0), dy.double().abs().sum(0)


def assert_close(dw, db, case, T, what):
    _, _, rw, mw, rb, mb = case
    assert dw.dtype == F32
    assert_product_close(dw.cpu(), rw, mw, T, what + " dW")
    if db is not None:
        assert_product_close(db.cpu(), rb, mb, T, what + " db")


@functools.lru_cache(maxsize=None)
def exact_case(T, C, N, kind):
    """-> (x [T, C], dy [T, N], want dW [N, C] fp32, want db [N] fp32 or None, fp64 db, sum |dy|)."""
    a, w_nk, want = split_case(N, T, C, False, kind)
    dy, x = a.t().contiguous(), w_nk.t().contiguous()
    if not bool((want.double() == dy.double().t() @ x.double()).all()):
        raise PremiseError("twgrad f32 %s: the transposed case is not the product" % kind)
    rb, mb = dy.double().sum(0), dy.double().abs().sum(0)
    db = None
    if kind in ("w", "int"):
        db = rb.float()
        exact = bool((db.double() == rb).all())
        if kind == "w":
            exact = exact and bool(((dy != 0).sum(0) == 1).all())              # one +-2^e per column
        else:
            exact = exact and float(mb.max()) < CAP and bool((rb == rb.round()).all())
        if not exact:
            raise PremiseError("twgrad f32 %s: db is not exact in fp32 (max sum |dy| %g)" % (kind, float(mb.max())))
    return x, dy, want, db, rb, mb


@functools.lru_cache(maxsize=None)
def db_single_case(T, C, N):
    """dY with ONE full-mantissa value per column, every other entry zero: db[n] is that value bit for bit -- it needs the lo, mid and
    hi ones-MFMA planes.  x: small integers (dW is not asserted here)."""
    g = gen(T, C, N, 77)
    v = full_mantissa(g, (N,))
    rows = torch.randint(0, T, (N,), generator=g)
    dy = torch.zeros(T, N)
    dy[rows, torch.arange(N)] = v
    low = (v.view(torch.int32) & 0xFF) != 0                                     # (bits that only the .lo part of the split carries)
    if int(low.sum()) < max(1, int(0.75 * N)) or not bool(torch.isfinite(v).all()):
        raise PremiseError("db single case: values without low mantissa bits")
    x = torch.randint(-3, 4, (T, C), generator=g).float()
    return x, dy, v.clone()


def integer_case(T, C, N):
    """Small integers: exact in any order -> (x, dy, want dW, want db)."""
    x, dy, rw, mw, rb, mb = wgrad_operands(T, C, N, F32)
    return x, dy, expected(rw, mw, F32, what="twgrad f32 integers dW"), expected(rb, mb, F32, what="twgrad f32 integers db")
