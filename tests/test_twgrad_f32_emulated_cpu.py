"""The fp32 form of csrc/twgrad.hip -- the REAL kernel source, launcher and C-ABI entry (mdetr_token_wgrad_f32) -- on the HIP-on-CPU
shim: the three-way bf16 split on the way into LDS, three row-major planes per operand read by the transposing fragments, six terms per
k-step and three ones-products for the bias gradient; every tile shape, ragged T / N / C, several chunks per tile.  Against fp64
products of the same fp32 operands within the fp32-accumulation bound (tests/gemm_bounds.py), and bit for bit on the exact cases
(tests/twgrad_f32_cases.py)."""
import ctypes

import pytest
import torch

import native_emul
import twgrad_f32_cases as X
from conftest import tune
from exact_cases import assert_bits_equal
from gemm_bounds import assert_product_close

CPU = torch.device("cpu")


def lib():
    L = native_emul.lib()
    L.mdetr_token_wgrad_f32                                            # (AttributeError without the feature: every test here needs the entry)
    return L


@pytest.fixture
def backend(monkeypatch):
    from monodetr_amd import conv_wgrad_ext
    monkeypatch.setattr(conv_wgrad_ext, "_backend", lib())
    return conv_wgrad_ext


@pytest.mark.parametrize("T,C,N", X.SHAPES)
def test_twgrad_f32_source_on_the_cpu_shim(monkeypatch, T, C, N):
    tune(monkeypatch, twgrad_f32_tile=None, twgrad_wgs=None)
    L = lib()
    case = X.random_case(T, C, N)
    x, dy = case[0], case[1]
    both = X.chunk_order_sum(X.partials(L, x, dy, True))
    X.assert_close(both[:N * C].view(N, C), both[N * C:], case, T, "T=%d C=%d N=%d" % (T, C, N))
    alone = X.chunk_order_sum(X.partials(L, x, dy, False))
    assert alone.numel() == N * C and torch.equal(alone, both[:N * C])     # with_bias = 0: the identical dW


@pytest.mark.parametrize("tile", X.TILES)
@pytest.mark.parametrize("kind", X.KINDS)
@pytest.mark.parametrize("T,C,N", X.EXACT_SHAPES)
def test_twgrad_f32_exact_split_cases(monkeypatch, backend, T, C, N, kind, tile):
    tune(monkeypatch, twgrad_f32_tile=tile)
    x, dy, want, want_db, rb, mb = X.exact_case(T, C, N, kind)
    what = "twgrad f32 %s T=%d C=%d N=%d tile %s" % (kind, T, C, N, tile)
    dw, db = backend.token_weight_gradient(x, dy, torch.float32, bias=True)
    assert_bits_equal(dw, want, what + " dW")
    if want_db is not None:
        assert_bits_equal(db, want_db, what + " db")
    else:
        assert_product_close(db, rb, mb, T, what + " db")


@pytest.mark.parametrize("tile", X.TILES)
@pytest.mark.parametrize("T,C,N", X.EXACT_SHAPES)
def test_twgrad_f32_exact_bias_gradient_and_integers(monkeypatch, backend, T, C, N, tile):
    tune(monkeypatch, twgrad_f32_tile=tile)
    what = "twgrad f32 T=%d C=%d N=%d tile %s" % (T, C, N, tile)
    x, dy, want_db = X.db_single_case(T, C, N)
    _, db = backend.token_weight_gradient(x, dy, torch.float32, bias=True)
    assert_bits_equal(db, want_db, what + " db of one full-mantissa value per column")
    x, dy, want, want_db = X.integer_case(T, C, N)
    dw, db = backend.token_weight_gradient(x, dy, torch.float32, bias=True)
    assert_bits_equal(dw, want, what + " integer dW")
    assert_bits_equal(db, want_db, what + " integer db")


def test_twgrad_f32_chunking_is_a_partition(monkeypatch):
    """More workgroups asked for than slabs allow: every chunk keeps at least one slab (no partial stays NaN), the sum over the chunks
    is the whole product; the chunk count follows the key."""
    L = lib()
    case = X.random_case(700, 64, 64)
    tune(monkeypatch, twgrad_wgs=None, twgrad_f32_tile=None)
    few = L.mdetr_token_wgrad_f32_chunks(700, 64, 64)
    tune(monkeypatch, twgrad_wgs="8192")
    many = L.mdetr_token_wgrad_f32_chunks(700, 64, 64)
    assert 1 <= few and 1 < many <= (700 + 31) // 32, (few, many)
    part = X.partials(L, case[0], case[1], True)
    assert part.shape[0] == many
    both = X.chunk_order_sum(part)
    X.assert_close(both[:64 * 64].view(64, 64), both[64 * 64:], case, 700, "chunked")


def test_twgrad_f32_argument_errors_name_the_entry():
    L = lib()
    x, dy = torch.zeros(64, 16), torch.zeros(64, 8)
    part = torch.zeros(L.mdetr_token_wgrad_f32_chunks(64, 16, 8) * (8 * 16 + 8))

    def call(xp, dyp, pp, floats, T, C, N):
        rc = L.mdetr_token_wgrad_f32(xp, dyp, pp, floats, T, C, N, 1, -1, None)
        return rc, ctypes.string_at(L.mdetr_last_error()).decode()

    MDETR_E_ARG = -1                                                   # include/monodetr_amd.h
    assert call(x.data_ptr(), dy.data_ptr(), part.data_ptr(), part.numel(), 64, 16, 8)[0] == 0
    for bad, needle in (((None, dy.data_ptr(), part.data_ptr(), part.numel(), 64, 16, 8), "null pointer"),
                        ((x.data_ptr(), dy.data_ptr(), None, part.numel(), 64, 16, 8), "null pointer"),
                        ((x.data_ptr(), dy.data_ptr(), part.data_ptr(), part.numel(), 64, 12, 8), "C % 8 == 0"),
                        ((x.data_ptr() + 4, dy.data_ptr(), part.data_ptr(), part.numel(), 32, 16, 8), "16-byte aligned"),
                        ((x.data_ptr(), dy.data_ptr(), part.data_ptr(), part.numel() - 1, 64, 16, 8), "partial buffer")):
        rc, msg = call(*bad)
        assert rc == MDETR_E_ARG and msg.startswith("mdetr_token_wgrad_f32:") and needle in msg, (bad, rc, msg)
    assert L.mdetr_token_wgrad_f32_chunks(64, 12, 8) == 0 and L.mdetr_token_wgrad_f32_chunks(0, 16, 8) == 0
