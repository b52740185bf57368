"""Cases for the stride-2 fp32 form of csrc/conv_wgrad.hip (mdetr_conv_wgrad_s2_f32; test infrastructure shared by
tests/test_conv_wgrad_s2_f32_emulated_cpu.py, tests/test_conv_wgrad_s2_f32_routing_cpu.py and tests/test_conv_wgrad_s2_f32_gpu.py).  Every
premise is checked from the operands and the fp64 reference alone, before any kernel runs (`PremiseError` otherwise).

    dW[n, t, e, c] = sum_{b, r, q} dY[b, r, q, n] X[b, 2 r + t - 1, 2 q + e - 1, c]        OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1

The kinds are those of tests/conv_wgrad_f32_cases.py on this formula -- the assertion is bit equality with the fp64 value, which is itself
an fp32 number:
  "x"    full-mantissa x against a dy that holds, per output channel n, ONE +-2^e (e in -8 .. 8) at one output pixel of the whole batch:
         dW[n, t, e, c] = 2^e x[b, 2 r + t - 1, 2 q + e - 1, c], an exact 0 where the tap leaves the image (required to occur) -- pins the
         de-interleaved window, the padding and both transposes to the bit;
  "dy"   the mirror image: full-mantissa dy against an x with one +-2^e pixel per input channel;
  "int"  dense integer dy, |dy| < 2^11, against an integer x (|x| < 2^10) with at most 4 non-zero pixels per input channel: an input pixel
         meets a tap at most once, so sum |dy||x| < 2^23 per element;
  small integers: exact_cases.conv_case(.., 3, 2, "wide") cast to fp32.
With one product per element, or integers below 2^24 throughout, the per-chunk partials and their sum are exact in ANY order.

Random case: x ~ 0.5 randn, dy ~ randn against the fp64 weight gradient within gemm_bounds' fp32 bound at K = B OH OW, the bound every other
fp32 form is held to.

`wgrad(x, dy) -> dW [N, C, 3, 3] fp32` is the route under test: conv_wgrad_ext.weight_gradient directly (`direct`), or the backward pass of
conv_taps_ext.conv_strided with the weight-gradient route recorded (`through_conv_strided`)."""
import functools

import torch

from conv_wgrad_f32_cases import _low_bits, _one_pixel_per_channel, _pow2, record_routes  # noqa: F401  (record_routes: for the runners)
from exact_cases import F32, PremiseError, assert_bits_equal, cl, conv_case, expected, full_mantissa, gen
from gemm_bounds import assert_product_close, conv2d_f64

# The kernel's tile (csrc/conv_wgrad.hip, conv_wgrad_s2_f32_kernel): 8 output rows x 8 output columns, 64 n x 64 c per workgroup, one
# workgroup per tap row; without the tune key it aims for 512 workgroups.
TILE_ROWS, TILE_COLS, N_BLOCK, C_BLOCK = 8, 8, 64, 64

# (B, H, W, C, N) of the INPUT: the smallest shapes that reach each mechanism
SHAPES = [
    (3, 3, 3, 64, 32),        # 2 x 2 output: image smaller than a tile, every tap crosses a border, N below one n block
    (2, 6, 37, 64, 64),       # even H; odd W: column 2 q + 1 of the last output column is outside; OW = 19: three column tiles, the last 3 wide
    (1, 33, 32, 128, 160),    # OH = 17: three bands, the last 1 row; even W; two c blocks; three n blocks, the last 32 wide
    (2, 18, 80, 192, 256),    # 9 x 40 outputs: 2 x 2 x 5 = 20 pixel tiles, 3 x 4 x 3 = 36 workgroups per chunk; with conv_wgrad_wgs=64 ONE
]                             # chunk walks all 20 tiles (the single LDS buffer is reused, the prefetch wraps); by default 14 chunks
WRAP_SHAPE, WRAP_WGS = SHAPES[3], 64
KINDS = ("x", "dy", "int")


def out_hw(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def tiles(shape):
    """Pixel tiles of a problem, from the tile size the kernel documents."""
    B, H, W, _, _ = shape
    OH, OW = out_hw(H, W)
    return B * ((OH + TILE_ROWS - 1) // TILE_ROWS) * ((OW + TILE_COLS - 1) // TILE_COLS)


def expected_chunks(shape, wgs):
    """geometry() of csrc/conv_wgrad.hip: target / (3 tap rows x n blocks x c blocks), between 1 and the number of tiles."""
    _, _, _, C, N = shape
    base = 3 * ((N + N_BLOCK - 1) // N_BLOCK) * (C // C_BLOCK)
    return max(1, min(tiles(shape), (wgs or 512) // base))


def wgrad_f64(x64, dy64):
    """The fp64 weight gradient [N, C, 3, 3] of conv2d(x, w, stride=2, padding=1) for the output gradient dy (autograd through conv2d_f64)."""
    w = torch.zeros(dy64.shape[1], x64.shape[1], 3, 3, dtype=torch.float64, device=x64.device, requires_grad=True)
    y = conv2d_f64(x64, w, stride=2, padding=1)
    if tuple(y.shape) != tuple(dy64.shape):
        raise PremiseError("dy %s is not the output map %s of x %s" % (tuple(dy64.shape), tuple(y.shape), tuple(x64.shape)))
    return torch.autograd.grad(y, w, dy64)[0]


@functools.lru_cache(maxsize=None)
def exact_case(B, H, W, C, N, kind):
    """-> (x [B, C, H, W], dy [B, N, OH, OW], want [N, C, 3, 3]), channels_last fp32; shared by every test that asks for the same key:
    never written to."""
    g = gen(B, H, W, C, N, ord(kind[0]), 79)
    OH, OW = out_hw(H, W)
    what = "conv_wgrad s2 f32 %s B=%d H=%d W=%d C=%d N=%d" % (kind, B, H, W, C, N)
    if kind == "x":
        x, dy = full_mantissa(g, (B, C, H, W)), _one_pixel_per_channel(g, B, N, OH, OW, _pow2(g, (N,)))
        _low_bits(x, what)
    elif kind == "dy":
        x, dy = _one_pixel_per_channel(g, B, C, H, W, _pow2(g, (C,))), full_mantissa(g, (B, N, OH, OW))
        _low_bits(dy, what)
    else:
        dy = torch.randint(-2047, 2048, (B, N, OH, OW), generator=g).float()
        x = torch.zeros(B, C, H, W)
        for _ in range(4):
            x += _one_pixel_per_channel(g, B, C, H, W, torch.randint(-1023, 1024, (C,), generator=g).float()) * (x == 0)
        x = x.clamp(-1023, 1023)
        if int((x != 0).sum((0, 2, 3)).max()) > 4:
            raise PremiseError(what + ": more than 4 non-zero pixels in a channel")
        if not bool((dy.abs() >= 256).any()) or not bool((x.abs() >= 256).any()):
            raise PremiseError(what + ": no operand beyond 8 bits")
    ref = wgrad_f64(x.double(), dy.double())
    if kind == "int":
        mag = wgrad_f64(x.double().abs(), dy.double().abs())
        if not float(mag.max()) < 2.0 ** 23:
            raise PremiseError(what + ": sum |dy||x| = %g" % float(mag.max()))
        want = expected(ref, mag, F32, what=what)
        if not bool((want != 0).any()):
            raise PremiseError(what + ": no product")
    else:
        terms = wgrad_f64((x != 0).double(), (dy != 0).double())
        if float(terms.max()) > 1.0:
            raise PremiseError(what + ": %d products meet in one element" % int(terms.max()))
        want = ref.to(F32)                                              # ONE product of an fp32 number and a power of two: exact in fp64
        if not bool((want.double() == ref).all()) or not bool(torch.isfinite(want).all()):
            raise PremiseError(what + ": the expected value is not an fp32 number")
        if not bool((want != 0).any()) or (kind == "x" and not bool((terms == 0).any())):
            raise PremiseError(what + ": no product / no tap outside the image")
    return cl(x), cl(dy), cl(want)


def lift_shape_rule(conv_wgrad_ext, monkeypatch):
    """conv_wgrad_ext.supported_f32_s2 sends the shape classes in which the library measured faster back to it (_F32_S2_MIN_N,
    _F32_S2_MAX_BLOCKS: a rule about speed).  The entry computes them all the same; the tests of the kernel lift the rule."""
    monkeypatch.setattr(conv_wgrad_ext, "_F32_S2_MIN_N", 0)
    monkeypatch.setattr(conv_wgrad_ext, "_F32_S2_MAX_BLOCKS", 1 << 30)


def direct(ext):
    """conv_wgrad_ext.weight_gradient on fp32 operands at stride 2, asked through supported_f32_s2 first."""
    def wgrad(x, dy):
        assert ext.supported_f32_s2(x, dy) and not ext.supported_f32(x, dy, 3, 2) and not ext.supported(x, dy, 3, 2)
        return ext.weight_gradient(x, dy, 3, 2, F32)
    return wgrad


def through_conv_strided(conv_taps_ext, calls):
    """The weight gradient as the backward pass of conv_taps_ext.conv_strided produces it; asserts it came from the entry, once, on fp32
    operands, and that the library was not asked for a weight gradient."""
    def wgrad(x, dy):
        w = torch.zeros(dy.shape[1], x.shape[1], 3, 3, device=x.device).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        y = conv_taps_ext.conv_strided(x, w, None, relu=False)
        del calls[:]
        y.backward(dy)
        assert calls == [("entry", F32, F32)], calls
        return w.grad
    return wgrad


def check_exact(wgrad, dev, shape, kinds=KINDS, tag=""):
    B, H, W, C, N = shape
    for kind in kinds:
        x, dy, want = exact_case(B, H, W, C, N, kind)
        dw = wgrad(x.to(dev), dy.to(dev))
        assert dw.dtype == F32 and tuple(dw.shape) == (N, C, 3, 3) and dw.is_contiguous(memory_format=torch.channels_last)
        assert_bits_equal(dw, want, "%s dW %s %s" % (kind, shape, tag))


def check_small_integers(wgrad, dev, shape, tag=""):
    B, H, W, C, N = shape
    what = "conv_wgrad s2 f32 integers %s %s" % (shape, tag)
    c = conv_case(B, H, W, C, N, 3, 2, "wide")
    dw = wgrad(c["x"].float().to(dev), c["dy"].float().to(dev))
    assert_bits_equal(dw, cl(expected(c["gw"], c["mw"], F32, what=what)), what)


def random_operands(shape, dev):
    B, H, W, C, N = shape
    OH, OW = out_hw(H, W)
    g = torch.Generator(device=dev).manual_seed(B * 1000 + H * W + C + N + 2)
    x = (torch.randn(B, H, W, C, device=dev, generator=g) * 0.5).permute(0, 3, 1, 2)
    return x, torch.randn(B, OH, OW, N, device=dev, generator=g).permute(0, 3, 1, 2)


@functools.lru_cache(maxsize=None)
def _random_reference_cpu(shape):
    x, dy = random_operands(shape, "cpu")
    return wgrad_f64(x.double(), dy.double()), wgrad_f64(x.double().abs(), dy.double().abs())


def random_reference(shape, dev):
    """(ref, mag) in fp64 on `dev`; the CPU ones are computed once per shape and shared."""
    if torch.device(dev).type == "cpu":
        return _random_reference_cpu(shape)
    x, dy = random_operands(shape, dev)
    return wgrad_f64(x.double(), dy.double()), wgrad_f64(x.double().abs(), dy.double().abs())


def check_random(wgrad, dev, shape, tag="", twice=False):
    """dW against fp64 within the fp32-accumulation bound at K = B OH OW; twice: a second call returns the same bits (no atomics)."""
    B, H, W, C, N = shape
    OH, OW = out_hw(H, W)
    x, dy = random_operands(shape, dev)
    ref, mag = random_reference(shape, dev)
    dw = wgrad(x, dy)
    assert_product_close(dw, ref, mag, B * OH * OW, "conv_wgrad s2 f32 random dW %s %s" % (shape, tag))
    if twice:
        assert torch.equal(wgrad(x, dy), dw)
    return dw
