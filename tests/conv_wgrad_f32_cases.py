"""Cases for the fp32 form of csrc/conv_wgrad.hip (mdetr_conv_wgrad_f32; test infrastructure shared by
tests/test_conv_wgrad_f32_emulated_cpu.py, tests/test_conv_wgrad_f32_routing_cpu.py and tests/test_conv_wgrad_f32_gpu.py).  Every premise
is checked from the operands and the fp64 reference alone, before any kernel runs (`PremiseError` otherwise).

    dW[n, t, e, c] = sum_{b, r, q} dY[b, r, q, n] X[b, r + t - 1, q + e - 1, c]

Exact cases -- the assertion is bit equality with the fp64 value, which is itself an fp32 number:
  "x"    full-mantissa x against a dy that holds, per output channel n, ONE +-2^e (e in -8 .. 8) at one pixel of the whole batch:
         dW[n, t, e, c] = 2^e x[b, r + t - 1, q + e - 1, c], an exact 0 where the tap leaves the image -- needs x.hi / x.mid / x.lo
         against dy.hi, and pins tap addressing, padding and both transposes to the bit;
  "dy"   the mirror image: full-mantissa dy against an x with one +-2^e pixel per input channel;
  "int"  dense integer dy, |dy| < 2^11, against an integer x (|x| < 2^10) with at most 4 non-zero pixels per input channel:
         sum |dy||x| < 2^23 per element;
  small integers: exact_cases.conv_case's "wide" set cast to fp32.
With one product per element, or integers below 2^24 throughout, the per-chunk partials and their sum are exact in ANY order: the
equality holds through every chunk count and every chunk-sum route.

Random case: x ~ 0.5 randn, dy ~ randn against the fp64 weight gradient (autograd through conv2d_f64) within gemm_bounds' fp32 bound at
K = B H W, the bound the other fp32 forms are held to (the three dropped split terms are <= 2 2^-24 per product, inside it).

`wgrad(x, dy) -> dW [N, C, 3, 3] fp32` is the route under test: conv_wgrad_ext.weight_gradient directly (`direct`), or the backward pass
of conv3x3_ext.conv3x3 with the weight-gradient route recorded (`through_conv3x3`)."""
import functools

import torch

from exact_cases import F32, PremiseError, assert_bits_equal, cl, conv_case, expected, full_mantissa, gen
from gemm_bounds import assert_product_close, conv2d_f64

# (B, H, W, C, N): the smallest shapes that reach each mechanism of the 128 n x 64 c workgroup with 8-row x 16-column pixel tiles
SHAPES = [
    (3, 3, 3, 64, 32),        # image smaller than a tile, every tap crosses a border, N below one n block
    (2, 5, 37, 64, 64),       # three column tiles, the last 5 wide; a ragged band
    (1, 17, 16, 128, 160),    # three bands, the last 1 row; two c blocks; a ragged second n block
    (2, 9, 40, 192, 256),     # 12 pixel tiles; with conv_wgrad_wgs=64 on 3 chunks: four tiles per chunk, the pipeline wraps and the
]                             # single LDS buffer is reused; with the default key one tile per chunk (chunks == units)
WRAP_SHAPE, WRAP_WGS, WRAP_CHUNKS, WRAP_UNITS = SHAPES[3], 64, 3, 12
KINDS = ("x", "dy", "int")


def _pow2(g, shape):
    return torch.exp2(torch.randint(-8, 9, shape, generator=g).float()) * (torch.randint(0, 2, shape, generator=g).float() * 2 - 1)


def _one_pixel_per_channel(g, B, A, H, W, values):
    """[B, A, H, W] with ONE non-zero per channel, at a random pixel of the whole batch."""
    t = torch.zeros(B, A, H, W)
    t[torch.randint(0, B, (A,), generator=g), torch.arange(A), torch.randint(0, H, (A,), generator=g), torch.randint(0, W, (A,), generator=g)] = values
    return t


def wgrad_f64(x64, dy64):
    """The fp64 weight gradient [N, C, 3, 3] of conv2d(x, w, padding=1) for the output gradient dy (autograd through conv2d_f64)."""
    w = torch.zeros(dy64.shape[1], x64.shape[1], 3, 3, dtype=torch.float64, device=x64.device, requires_grad=True)
    return torch.autograd.grad(conv2d_f64(x64, w, padding=1), w, dy64)[0]


def _low_bits(t, what):
    if float(((t.contiguous().view(torch.int32) & 0xFF) != 0).float().mean()) < 0.9:
        raise PremiseError(what + ": operand without low mantissa bits")


@functools.lru_cache(maxsize=None)
def exact_case(B, H, W, C, N, kind):
    """-> (x [B, C, H, W], dy [B, N, H, W], want [N, C, 3, 3]), channels_last fp32; shared by every test that asks for the same key:
    never written to."""
    g = gen(B, H, W, C, N, ord(kind[0]), 77)
    what = "conv_wgrad f32 %s B=%d H=%d W=%d C=%d N=%d" % (kind, B, H, W, C, N)
    if kind == "x":
        x, dy = full_mantissa(g, (B, C, H, W)), _one_pixel_per_channel(g, B, N, H, W, _pow2(g, (N,)))
        _low_bits(x, what)
    elif kind == "dy":
        x, dy = _one_pixel_per_channel(g, B, C, H, W, _pow2(g, (C,))), full_mantissa(g, (B, N, H, W))
        _low_bits(dy, what)
    else:
        dy = torch.randint(-2047, 2048, (B, N, H, W), generator=g).float()
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
    """conv_wgrad_ext.supported_f32 sends the shape classes in which the library measured faster back to it (_F32_MIN_N,
    _F32_MAX_BLOCKS: a rule about speed).  The entry computes them all the same; the tests of the kernel lift the rule."""
    monkeypatch.setattr(conv_wgrad_ext, "_F32_MIN_N", 0)
    monkeypatch.setattr(conv_wgrad_ext, "_F32_MAX_BLOCKS", 1 << 30)


def direct(ext):
    """conv_wgrad_ext.weight_gradient on fp32 operands, asked through supported_f32 first."""
    def wgrad(x, dy):
        assert ext.supported_f32(x, dy, 3, 1) and not ext.supported(x, dy, 3, 1)
        return ext.weight_gradient(x, dy, 3, 1, F32)
    return wgrad


def record_routes(conv_wgrad_ext, monkeypatch):
    """-> list that receives ("entry", x dtype, dy dtype) per conv_wgrad_ext.weight_gradient call and ("library", mask) per
    aten.convolution_backward call."""
    calls, real_w, real_c = [], conv_wgrad_ext.weight_gradient, torch.ops.aten.convolution_backward

    def weight_gradient(x, dy, *a, **k):
        calls.append(("entry", x.dtype, dy.dtype))
        return real_w(x, dy, *a, **k)

    def convolution_backward(*a):
        calls.append(("library", tuple(a[-1])))
        return real_c(*a)
    monkeypatch.setattr(conv_wgrad_ext, "weight_gradient", weight_gradient)
    monkeypatch.setattr(torch.ops.aten, "convolution_backward", convolution_backward)
    return calls


def through_conv3x3(conv3x3_ext, calls):
    """The weight gradient as the backward pass of conv3x3_ext.conv3x3 produces it; asserts it came from the entry, once, on fp32
    operands, and that the library was not asked for a weight gradient."""
    def wgrad(x, dy):
        w = torch.zeros(dy.shape[1], x.shape[1], 3, 3, device=x.device).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        y = conv3x3_ext.conv3x3(x, w, None, relu=False)
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
    what = "conv_wgrad f32 integers %s %s" % (shape, tag)
    c = conv_case(B, H, W, C, N, 3, 1, "wide")
    dw = wgrad(c["x"].float().to(dev), c["dy"].float().to(dev))
    assert_bits_equal(dw, cl(expected(c["gw"], c["mw"], F32, what=what)), what)


def random_operands(shape, dev):
    B, H, W, C, N = shape
    g = torch.Generator(device=dev).manual_seed(B * 1000 + H * W + C + N)
    x = (torch.randn(B, H, W, C, device=dev, generator=g) * 0.5).permute(0, 3, 1, 2)
    return x, torch.randn(B, H, W, N, device=dev, generator=g).permute(0, 3, 1, 2)


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
    """dW against fp64 within the fp32-accumulation bound at K = B H W; twice: a second call returns the same bits (no atomics)."""
    B, H, W, C, N = shape
    x, dy = random_operands(shape, dev)
    ref, mag = random_reference(shape, dev)
    dw = wgrad(x, dy)
    assert_product_close(dw, ref, mag, B * H * W, "conv_wgrad f32 random dW %s %s" % (shape, tag))
    if twice:
        assert torch.equal(wgrad(x, dy), dw)
    return dw
