"""Cases for the fp32 form of csrc/conv3x3.hip (mdetr_conv3x3_f32; test infrastructure shared by tests/test_conv3x3_f32_emulated_cpu.py
and tests/test_conv3x3_f32_gpu.py).  Every premise is checked from the operands and the fp64 reference alone, before any kernel runs
(`PremiseError` otherwise).

Exact cases -- the assertion is bit equality with the fp64 value, which is itself an fp32 number:
  "x"    full-mantissa activation against a weight with ONE +-2^e (e in -8 .. 8) per output channel at a random (tap row, tap column,
         input channel): y is a shifted, scaled copy of an x channel with exact zeros where the tap leaves the image -- needs x.hi / x.mid
         / x.lo against w.hi, and pins tap addressing and padding to the bit;
  "w"    an activation that is non-zero only at pixels with r % 3 == 1 and c % 3 == 1 (one +-2^e channel each) against a full-mantissa
         weight: every 3 x 3 window holds at most one such pixel, so y[b, r, c, n] = s w[n, t, s, k];
  "int"  |x| < 2^11 dense against a weight with at most 4 non-zeros (|w| < 2^10) per output channel: sum |x||w| < 2^23;
  small integers: exact_cases.conv_case's "wide" and "narrow" sets cast to fp32 (plain, with shift, shift + ReLU, dx, masked dx).
For the input gradient the same kinds are built on (dy, w): one non-zero per INPUT channel of w.

Random case: x ~ 0.5 randn, w ~ randn / (3 sqrt(C)), shift ~ 0.5 randn against conv2d_f64 within gemm_bounds' fp32 bound at K = 9 C (the
bound the two other fp32 forms are held to; the three dropped split terms are <= 2 2^-24 per product, inside it)."""
import functools

import torch

from exact_cases import F32, PremiseError, assert_bits_equal, cl, conv_case, expected, full_mantissa, gen
from gemm_bounds import assert_product_close, conv2d_f64

# (B, H, W, C, N): the smallest shapes that reach each mechanism
SHAPES = [
    (3, 3, 3, 64, 32),        # image smaller than any tile, every tap crosses a border, NB = 1; dx on the library (N % 64 != 0)
    (2, 5, 37, 64, 64),       # two column tiles (the second 5 wide), two row tiles (the second 1 high)
    (1, 6, 80, 192, 96),      # six slabs: the ring runs dry and refills; N = 96 leaves a half-empty output block; dx on the library
    (1, 9, 40, 64, 160),      # ragged last channel group, W = 40; dx on the library (N = 160 is not a multiple of 64)
    (1, 4, 8, 64, 384),       # three channel groups at NB = 4 / six at NB = 2: plain numbering, not the XCD one
    (1, 9, 32, 64, 512),      # XCD numbering padded past the tile count
    (2, 7, 43, 128, 128),     # ragged in H and W, four slabs: the shape of the every-tile sweep
]
SWEEP_SHAPE = (2, 7, 43, 128, 128)
TILES = [321, 161, 162, 84, 82]           # 10 WC + GC of every tile shape the launcher builds
NBS = [1, 2]                              # ... and every output-channel width
KINDS = ("x", "w", "int")


def dx_on_kernel(C, N):
    """conv3x3_ext._Conv3x3.backward: the input gradient is the kernel on (dy, w') when dy's channels are a multiple of 64."""
    return N % 64 == 0 and C % 32 == 0


def _pow2(g, shape):
    return torch.exp2(torch.randint(-8, 9, shape, generator=g).float()) * (torch.randint(0, 2, shape, generator=g).float() * 2 - 1)


def _one_per_channel(g, N, C, per_input):
    """[N, C, 3, 3] with one +-2^e per output channel (per input channel with per_input) at a random place."""
    w = torch.zeros(N, C, 3, 3)
    if per_input:
        c = torch.arange(C)
        w[torch.randint(0, N, (C,), generator=g), c, torch.randint(0, 3, (C,), generator=g), torch.randint(0, 3, (C,), generator=g)] = _pow2(g, (C,))
    else:
        n = torch.arange(N)
        w[n, torch.randint(0, C, (N,), generator=g), torch.randint(0, 3, (N,), generator=g), torch.randint(0, 3, (N,), generator=g)] = _pow2(g, (N,))
    return w


def _sparse_pixels(g, B, C, H, W):
    """[B, C, H, W], non-zero only at pixels (r % 3 == 1, c % 3 == 1): one +-2^e channel each."""
    a = torch.zeros(B, C, H, W)
    rows, cols = torch.arange(1, H, 3), torch.arange(1, W, 3)
    b, r, c = torch.meshgrid(torch.arange(B), rows, cols, indexing="ij")
    b, r, c = b.reshape(-1), r.reshape(-1), c.reshape(-1)
    a[b, torch.randint(0, C, b.shape, generator=g), r, c] = _pow2(g, b.shape)
    return a


def _few_per_channel(g, N, C, per_input):
    """[N, C, 3, 3] integers |w| < 2^10, at most 4 non-zeros per output channel (per input channel with per_input)."""
    w = torch.zeros(N, C, 3, 3)
    for _ in range(4):
        if per_input:
            c = torch.arange(C)
            w[torch.randint(0, N, (C,), generator=g), c, torch.randint(0, 3, (C,), generator=g), torch.randint(0, 3, (C,), generator=g)] = \
                torch.randint(-1023, 1024, (C,), generator=g).float()
        else:
            n = torch.arange(N)
            w[n, torch.randint(0, C, (N,), generator=g), torch.randint(0, 3, (N,), generator=g), torch.randint(0, 3, (N,), generator=g)] = \
                torch.randint(-1023, 1024, (N,), generator=g).float()
    return w


def _low_bits(t, what):
    if float(((t.contiguous().view(torch.int32) & 0xFF) != 0).float().mean()) < 0.9:
        raise PremiseError(what + ": operand without low mantissa bits")


def _conv_or_grad(a64, w64, grad):
    """conv(a, w) -- or, with grad, the input gradient of conv(., w) for the output gradient a -- in fp64."""
    if not grad:
        return conv2d_f64(a64, w64, padding=1)
    B, N, H, W = a64.shape
    z = torch.zeros(B, w64.shape[1], H, W, dtype=torch.float64, requires_grad=True)
    return torch.autograd.grad(conv2d_f64(z, w64, padding=1), z, a64)[0]


@functools.lru_cache(maxsize=None)
def exact_case(B, H, W, C, N, kind, grad=False):
    """-> (a, w [N, C, 3, 3], want): a = x [B, C, H, W] and want = conv(x, w) [B, N, H, W]; with grad a = dy [B, N, H, W] and want = dx.
    All channels_last fp32; shared by every test that asks for the same key: never written to."""
    g = gen(B, H, W, C, N, ord(kind[0]), int(grad))
    what = "conv3x3 f32 %s%s B=%d H=%d W=%d C=%d N=%d" % (kind, " dx" if grad else "", B, H, W, C, N)
    A = N if grad else C                                                # channels of the activation operand
    if kind == "x":
        a, w = full_mantissa(g, (B, A, H, W)), _one_per_channel(g, N, C, grad)
        _low_bits(a, what)
    elif kind == "w":
        a, w = _sparse_pixels(g, B, A, H, W), full_mantissa(g, (N, C, 3, 3))
        _low_bits(w, what)
    else:
        a, w = torch.randint(-2047, 2048, (B, A, H, W), generator=g).float(), _few_per_channel(g, N, C, grad)
        if not bool((a.abs() >= 256).any()) or not bool((w.abs() >= 256).any()):
            raise PremiseError(what + ": no operand beyond 8 bits")
    ref = _conv_or_grad(a.double(), w.double(), grad)
    if kind == "int":
        mag = _conv_or_grad(a.double().abs(), w.double().abs(), grad)
        if not float(mag.max()) < 2.0 ** 23:
            raise PremiseError(what + ": sum |x||w| = %g" % float(mag.max()))
        want = expected(ref, mag, F32, what=what)
    else:
        terms = _conv_or_grad((a != 0).double(), (w != 0).double(), grad)
        if float(terms.max()) > 1.0:
            raise PremiseError(what + ": %d products meet in one element" % int(terms.max()))
        want = ref.to(F32)                                              # ONE product of an fp32 number and a power of two: exact in fp64
        if not bool((want.double() == ref).all()) or not bool(torch.isfinite(want).all()):
            raise PremiseError(what + ": the expected value is not an fp32 number")
        if not bool((want != 0).any()) or (kind == "x" and min(H, W) >= 3 and not bool((terms == 0).any())):
            raise PremiseError(what + ": no product / no tap outside the image")
    return cl(a), cl(w), cl(want)


def record_launches(ext, monkeypatch):
    """-> list that receives (dtype, mirror, masked) of every conv3x3_ext._launch."""
    calls, real = [], ext._launch

    def launch(x_cl, w_ohwi, shift, relu, mirror=False, mask=None):
        calls.append((x_cl.dtype, bool(mirror), mask is not None))
        return real(x_cl, w_ohwi, shift, relu, mirror=mirror, mask=mask)
    monkeypatch.setattr(ext, "_launch", launch)
    return calls


def check_exact(ext, dev, shape, kinds=KINDS, tag=""):
    """Forward and (where the kernel takes it) input gradient of the exact kinds, bit for bit."""
    B, H, W, C, N = shape
    for kind in kinds:
        x, w, want = exact_case(B, H, W, C, N, kind)
        assert ext.supported_f32(x.to(dev), w.to(dev))
        y = ext.conv3x3(x.to(dev), w.to(dev), None, relu=False)
        assert y.dtype == F32 and y.is_contiguous(memory_format=torch.channels_last)
        assert_bits_equal(y, want, "%s forward %s %s" % (kind, shape, tag))
        if dx_on_kernel(C, N):
            dy, w, want = exact_case(B, H, W, C, N, kind, True)
            xr = torch.zeros(B, C, H, W).contiguous(memory_format=torch.channels_last).to(dev).requires_grad_(True)
            ext.conv3x3(xr, w.to(dev), None, relu=False).backward(dy.to(dev))
            assert_bits_equal(xr.grad, want, "%s dx %s %s" % (kind, shape, tag))


def check_small_integers(ext, dev, shape, calls):
    """exact_cases.conv_case's integer sets in fp32: plain, with shift, shift + ReLU (narrow: exact-zero pre-activations), dx through the
    mirrored taps and dx masked by an in_token (narrow: zero inputs under non-zero gradients)."""
    from monodetr_amd.monodetr.linear import ReluToken
    B, H, W, C, N = shape
    tag = "conv3x3 f32 integers %s " % (shape,)
    c = conv_case(B, H, W, C, N, 3, 1, "wide")
    x, w, dy, shift = c["x"].float().to(dev), c["w"].float().to(dev), c["dy"].float().to(dev), c["shift"].to(dev)
    noshift = c["pre"] - c["shift"].double().view(1, -1, 1, 1)
    assert_bits_equal(ext.conv3x3(x, w, None, relu=False), expected(noshift, c["mpre"], F32, what=tag), tag + "plain")
    xr = x.clone().requires_grad_(True)
    y = ext.conv3x3(xr, w, shift, relu=False)
    assert_bits_equal(y, expected(c["pre"], c["mpre"], F32, what=tag), tag + "shift")
    del calls[:]
    y.backward(dy)
    on_kernel = dx_on_kernel(C, N)
    assert calls == ([(F32, True, False)] if on_kernel else []), (shape, calls)     # the kernel's dx, or the library's: never silently the other
    if on_kernel:
        assert_bits_equal(xr.grad, expected(c["gx"], c["mx"], F32, what=tag + "dx"), tag + "dx (mirrored taps)")
    n = conv_case(B, H, W, C, N, 3, 1, "narrow")
    x, w, dy = n["x"].float().to(dev), n["w"].float().to(dev), n["dy"].float().to(dev)
    want = expected(n["pre"].clamp(min=0), n["mpre"], F32, zeros_of=n["pre"], what=tag + "narrow")
    assert_bits_equal(ext.conv3x3(x, w, n["shift"].to(dev), relu=True), want, tag + "shift + relu")
    if on_kernel:
        token = ReluToken()
        xr = x.clone().requires_grad_(True)
        y = ext.conv3x3(xr, w, None, relu=False, in_token=token)
        del calls[:]
        y.backward(dy)
        assert token.premasked and calls == [(F32, True, True)], calls
        xm = n["x"].double()
        if not bool(((xm == 0) & (n["gx"] != 0)).any()):
            raise PremiseError(tag + "no nonzero gradient under a zero input")
        want = expected(torch.where(xm <= 0, torch.zeros_like(xm), n["gx"]), n["mx"], F32, zeros_of=xm, what=tag + "masked dx")
        assert_bits_equal(xr.grad, want, tag + "dx masked by the input")


def random_operands(shape, dev):
    B, H, W, C, N = shape
    g = torch.Generator(device=dev).manual_seed(B * 1000 + H * W + C + N)
    mk = lambda *s: torch.randn(*s, device=dev, generator=g)          # noqa: E731
    x = (mk(B, H, W, C) * 0.5).permute(0, 3, 1, 2)
    w = (mk(N, 3, 3, C) / (3.0 * C ** 0.5)).permute(0, 3, 1, 2)
    return x, w, mk(N) * 0.5, mk(B, H, W, N).permute(0, 3, 1, 2)


def check_random(ext, dev, shape, tag="", twice=False):
    """y and (where the kernel takes it) dx against fp64 within the fp32-accumulation bound; fp64 on `dev`.  twice: a second call
    returns the same bits."""
    B, H, W, C, N = shape
    x, w, shift, dy = random_operands(shape, dev)
    assert x.is_contiguous(memory_format=torch.channels_last) and ext.supported_f32(x, w)
    xr = x.clone().requires_grad_(True)
    y = ext.conv3x3(xr, w, shift, relu=False)
    x64, w64 = x.double().requires_grad_(True), w.double()
    ref = conv2d_f64(x64, w64, shift.double(), padding=1)
    xa = x.double().abs().requires_grad_(True)
    mag = conv2d_f64(xa, w64.abs(), shift.double().abs(), padding=1)
    assert_product_close(y.detach(), ref.detach(), mag.detach(), 9 * C, "conv3x3 f32 random y %s %s" % (shape, tag))
    if twice:
        assert torch.equal(ext.conv3x3(x, w, shift, relu=False), y.detach())
    if dx_on_kernel(C, N):
        y.backward(dy)
        gx, = torch.autograd.grad(ref, x64, dy.double())
        mx, = torch.autograd.grad(mag, xa, dy.double().abs())
        assert_product_close(xr.grad, gx, mx, 9 * N, "conv3x3 f32 random dx %s %s" % (shape, tag))
        if twice:
            x2 = x.clone().requires_grad_(True)
            ext.conv3x3(x2, w, shift, relu=False).backward(dy)
            assert torch.equal(x2.grad, xr.grad)
