"""Cases for the fp32 form of csrc/conv_taps.hip (mdetr_conv_taps_f32, mdetr_conv_taps_f32_split, mdetr_conv_dgrad_s2_f32; test
infrastructure shared by tests/test_conv_strided_f32_emulated_cpu.py and tests/test_conv_strided_f32_gpu.py): the 3x3 / stride-2 / pad-1
convolution.  Every premise is checked from the operands and the fp64 reference alone, before any kernel runs (`PremiseError`
otherwise).

Exact cases -- the assertion is bit equality with the fp64 value, which is itself an fp32 number (the kinds of
tests/conv3x3_f32_cases.py, restated for stride 2):
  "x"    full-mantissa activation against a weight with ONE +-2^e per output channel at a random (tap row, tap column, input channel):
         y is a strided, scaled copy of an x channel with exact zeros where the tap leaves the image -- needs all three parts of x,
         and pins tap, stride and padding addressing to the bit;
  "w"    an activation that is non-zero only at pixels with r % 3 == 1 and c % 3 == 1 (one +-2^e channel each) against a full-mantissa
         weight: a 3 x 3 window holds at most one such pixel -- at most one product per output element;
  "int"  |x| < 2^11 dense against a weight with at most 4 non-zeros (|w| < 2^10) per output channel: sum |x||w| < 2^23;
  small integers: exact_cases.conv_case(..., 3, 2, "wide" / "narrow") cast to fp32 (plain, with shift, shift + ReLU, dx).
For the input gradient the same kinds are built on (dy, w): one non-zero per INPUT channel of w.

Random case: x ~ 0.5 randn, w ~ randn / (3 sqrt(C)), shift ~ 0.5 randn against conv2d_f64 within gemm_bounds.assert_product_close at
K = 9 C forward and K = 4 N for dx (a pixel of parity class (pi, pj) sums (1 + pi)(1 + pj) <= 4 taps over N channels); the three dropped
split terms are <= 2 2^-24 per product, inside it.  A second call returns the same bits."""
import functools

import torch

from conv3x3_f32_cases import _few_per_channel, _low_bits, _one_per_channel, _sparse_pixels
from exact_cases import F32, PremiseError, assert_bits_equal, cl, conv_case, expected, full_mantissa, gen
from gemm_bounds import assert_product_close, conv2d_f64, product_bound

# (B, H, W, C, N): the smallest shapes that reach each mechanism.  The forward tile is 4 (or 2) output rows x 32 output columns, its
# slab 16 channels; the input gradient's tiles are 4 x 32 pixels of one parity class, its slab 32 channels of dy.
SHAPES = [
    (3, 3, 3, 64, 32),        # image smaller than any tile, every tap crosses a border, odd H and W; dx on the library (N % 64 != 0)
    (3, 3, 3, 64, 64),        # the same image with dx on the kernel: every tap of the four parity classes crosses a border
    (2, 10, 75, 64, 64),      # 5 x 38 outputs: two column tiles and two row tiles with ragged ends; even H, odd W: four class sizes
    (2, 1, 9, 64, 64),        # H = 1: the two odd-row classes of the input gradient are empty
    (1, 5, 7, 64, 96),        # N = 96: three channel groups at NB = 1 (plain numbering), a half-empty last group at NB = 2; dx on the library
    (1, 4, 6, 192, 192),      # 12 forward slabs, 6 of the input gradient: the weight prefetch across slab boundaries; last group ragged at NB = 4
]
SWEEP_SHAPE = (1, 7, 67, 64, 192)      # 4 x 34 outputs, ragged in both directions at either tile height; N ragged at NB = 4, dx on the kernel
GEOMETRIES = [(4, 1), (4, 2), (4, 4), (2, 1), (2, 2)]      # (rows, NB) of every forward instantiation the launcher builds
DGRAD_NBS = [2, 4]                     # ... and every width of the input gradient
KINDS = ("x", "w", "int")


def dx_on_kernel(C, N):
    """conv_taps_ext._ConvStrided.backward: the input gradient is the kernel's where dy's channels are a multiple of 64."""
    return N % 64 == 0 and C % 32 == 0


def lift_shape_rule(conv_taps_ext, monkeypatch):
    """conv_taps_ext.supported_f32 sends the shape classes in which the library measured faster back to it (_F32_FWD_MAX_C,
    _F32_DX_MAX_C: a rule about speed).  The entries compute them all the same; the tests of the kernel lift the rule."""
    monkeypatch.setattr(conv_taps_ext, "_F32_FWD_MAX_C", 1 << 30)
    monkeypatch.setattr(conv_taps_ext, "_F32_DX_MAX_C", 1 << 30)


def out_hw(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def _conv_or_grad(a64, w64, grad, hw):
    """conv(a, w) at stride 2 -- or, with grad, the input gradient (an image of hw) of conv(., w) for the output gradient a -- in fp64."""
    if not grad:
        return conv2d_f64(a64, w64, stride=2, padding=1)
    z = torch.zeros(a64.shape[0], w64.shape[1], hw[0], hw[1], dtype=torch.float64, requires_grad=True)
    return torch.autograd.grad(conv2d_f64(z, w64, stride=2, padding=1), z, a64)[0]


@functools.lru_cache(maxsize=None)
def exact_case(B, H, W, C, N, kind, grad=False):
    """-> (a, w [N, C, 3, 3], want): a = x [B, C, H, W] and want = conv(x, w) [B, N, OH, OW]; with grad a = dy [B, N, OH, OW] and
    want = dx [B, C, H, W].  All channels_last fp32; shared by every test that asks for the same key: never written to."""
    g = gen(B, H, W, C, N, ord(kind[0]), int(grad), 2)
    what = "conv strided f32 %s%s B=%d H=%d W=%d C=%d N=%d" % (kind, " dx" if grad else "", B, H, W, C, N)
    OH, OW = out_hw(H, W)
    A, AH, AW = (N, OH, OW) if grad else (C, H, W)                      # the activation operand
    if kind == "x":
        a, w = full_mantissa(g, (B, A, AH, AW)), _one_per_channel(g, N, C, grad)
        _low_bits(a, what)
    elif kind == "w":
        a, w = _sparse_pixels(g, B, A, AH, AW), full_mantissa(g, (N, C, 3, 3))
        _low_bits(w, what)
    else:
        a, w = torch.randint(-2047, 2048, (B, A, AH, AW), generator=g).float(), _few_per_channel(g, N, C, grad)
        if not bool((a.abs() >= 256).any()) or not bool((w.abs() >= 256).any()):
            raise PremiseError(what + ": no operand beyond 8 bits")
    ref = _conv_or_grad(a.double(), w.double(), grad, (H, W))
    if kind == "int":
        mag = _conv_or_grad(a.double().abs(), w.double().abs(), grad, (H, W))
        if not float(mag.max()) < 2.0 ** 23:
            raise PremiseError(what + ": sum |x||w| = %g" % float(mag.max()))
        want = expected(ref, mag, F32, what=what)
    else:
        terms = _conv_or_grad((a != 0).double(), (w != 0).double(), grad, (H, W))
        if float(terms.max()) > 1.0:
            raise PremiseError(what + ": %d products meet in one element" % int(terms.max()))
        want = ref.to(F32)                                              # ONE product of an fp32 number and a power of two: exact in fp64
        if not bool((want.double() == ref).all()) or not bool(torch.isfinite(want).all()):
            raise PremiseError(what + ": the expected value is not an fp32 number")
        if kind == "x" and not bool((terms == 0).any()):
            raise PremiseError(what + ": no tap outside the image")
        if not bool((want != 0).any()) and not (kind == "w" and min(AH, AW) < 2):
            raise PremiseError(what + ": no product")
    return cl(a), cl(w), cl(want)


def record_launches(ext, monkeypatch):
    """-> list that receives (what, dtype) of every kernel launch of conv_taps_ext: "fwd", "split" or "dx"."""
    calls = []
    real_call, real_split, real_dx = ext._call, ext._forward_split, ext._input_gradient

    def call(x, w, shift, y, dims, relu):
        calls.append(("fwd", x.dtype))
        return real_call(x, w, shift, y, dims, relu)

    def split(x, w_ohwi, shift, ks, dims):
        calls.append(("split", x.dtype))
        return real_split(x, w_ohwi, shift, ks, dims)

    def dx(dy, w_ohwi, H, W, w_ihwo=None):
        calls.append(("dx", dy.dtype))
        return real_dx(dy, w_ohwi, H, W, w_ihwo)
    monkeypatch.setattr(ext, "_call", call)
    monkeypatch.setattr(ext, "_forward_split", split)
    monkeypatch.setattr(ext, "_input_gradient", dx)
    return calls


def _zeros_x(B, C, H, W, dev):
    return torch.zeros(B, C, H, W).contiguous(memory_format=torch.channels_last).to(dev).requires_grad_(True)


def check_exact(ext, dev, shape, kinds=KINDS, tag=""):
    """Forward and (where the kernel takes it) input gradient of the exact kinds, bit for bit."""
    B, H, W, C, N = shape
    for kind in kinds:
        x, w, want = exact_case(B, H, W, C, N, kind)
        assert ext.supported_f32(x.to(dev), w.to(dev))
        y = ext.conv_strided(x.to(dev), w.to(dev), None, relu=False)
        assert y.dtype == F32 and y.is_contiguous(memory_format=torch.channels_last)
        assert_bits_equal(y, want, "%s forward %s %s" % (kind, shape, tag))
        if dx_on_kernel(C, N):
            dy, w, want = exact_case(B, H, W, C, N, kind, True)
            xr = _zeros_x(B, C, H, W, dev)
            ext.conv_strided(xr, w.to(dev), None, relu=False).backward(dy.to(dev))
            assert_bits_equal(xr.grad, want, "%s dx %s %s" % (kind, shape, tag))


def check_small_integers(ext, dev, shape, calls):
    """exact_cases.conv_case's integer sets at stride 2 in fp32: plain, with shift, shift + ReLU (narrow: exact-zero pre-activations) and
    dx -- on the kernel or on the library, never silently the other."""
    B, H, W, C, N = shape
    tag = "conv strided f32 integers %s " % (shape,)
    c = conv_case(B, H, W, C, N, 3, 2, "wide")
    x, w, dy, shift = c["x"].float().to(dev), c["w"].float().to(dev), c["dy"].float().to(dev), c["shift"].to(dev)
    noshift = c["pre"] - c["shift"].double().view(1, -1, 1, 1)
    assert_bits_equal(ext.conv_strided(x, w, None, relu=False), expected(noshift, c["mpre"], F32, what=tag), tag + "plain")
    xr = x.clone().requires_grad_(True)
    y = ext.conv_strided(xr, w, shift, relu=False)
    assert_bits_equal(y, expected(c["pre"], c["mpre"], F32, what=tag), tag + "shift")
    del calls[:]
    y.backward(dy)
    on_kernel = dx_on_kernel(C, N)
    assert calls == ([("dx", F32)] if on_kernel else []), (shape, calls)
    assert_bits_equal(xr.grad, expected(c["gx"], c["mx"], F32, what=tag + "dx"), tag + "dx")     # (the library's is exact on integers too)
    n = conv_case(B, H, W, C, N, 3, 2, "narrow")
    x, w = n["x"].float().to(dev), n["w"].float().to(dev)
    want = expected(n["pre"].clamp(min=0), n["mpre"], F32, zeros_of=n["pre"], what=tag + "narrow")
    assert_bits_equal(ext.conv_strided(x, w, n["shift"].to(dev), relu=True), want, tag + "shift + relu")


def random_operands(shape, dev):
    B, H, W, C, N = shape
    OH, OW = out_hw(H, W)
    g = torch.Generator(device=dev).manual_seed(B * 1000 + H * W + C + N + 2)
    mk = lambda *s: torch.randn(*s, device=dev, generator=g)          # noqa: E731
    x = (mk(B, H, W, C) * 0.5).permute(0, 3, 1, 2)
    w = (mk(N, 3, 3, C) / (3.0 * C ** 0.5)).permute(0, 3, 1, 2)
    return x, w, mk(N) * 0.5, mk(B, OH, OW, N).permute(0, 3, 1, 2)


@functools.lru_cache(maxsize=None)
def random_reference(shape, dev):
    """-> (x, w, shift, dy, ref, mag, gx, mx): the operands and the fp64 results on `dev`; shared, never written to."""
    x, w, shift, dy = random_operands(shape, dev)
    x64, w64 = x.double().requires_grad_(True), w.double()
    ref = conv2d_f64(x64, w64, shift.double(), stride=2, padding=1)
    xa = x.double().abs().requires_grad_(True)
    mag = conv2d_f64(xa, w64.abs(), shift.double().abs(), stride=2, padding=1)
    gx, = torch.autograd.grad(ref, x64, dy.double())
    mx, = torch.autograd.grad(mag, xa, dy.double().abs())
    return x, w, shift, dy, ref.detach(), mag.detach(), gx, mx


def check_random(ext, dev, shape, tag="", twice=False):
    """y and (where the kernel takes it) dx against fp64 within the fp32-accumulation bound; fp64 on `dev`.  twice: a second call
    returns the same bits."""
    B, H, W, C, N = shape
    x, w, shift, dy, ref, mag, gx, mx = random_reference(shape, str(dev))
    assert x.is_contiguous(memory_format=torch.channels_last) and ext.supported_f32(x, w)
    xr = x.clone().requires_grad_(True)
    y = ext.conv_strided(xr, w, shift, relu=False)
    assert_product_close(y.detach(), ref, mag, 9 * C, "conv strided f32 random y %s %s" % (shape, tag))
    if twice:
        assert torch.equal(ext.conv_strided(x, w, shift, relu=False), y.detach())
    if dx_on_kernel(C, N):
        y.backward(dy)
        assert_product_close(xr.grad, gx, mx, 4 * N, "conv strided f32 random dx %s %s" % (shape, tag))
        if twice:
            x2 = x.clone().requires_grad_(True)
            ext.conv_strided(x2, w, shift, relu=False).backward(dy)
            assert torch.equal(x2.grad, xr.grad)


def taps_dims(B, H, W, C, N):
    """The 23 dims of mdetr_conv_taps / mdetr_conv_taps_f32 for the 3x3 / stride-2 / pad-1 forward on contiguous NHWC / OHWI tensors."""
    OH, OW = out_hw(H, W)
    return [B, H, W, C, OH, OW, N, 2, 3, 3, 1, 1, 0, 1, 0, 1, 0, OH * OW * N, OW * N, N, 9 * C, 3 * C, C]


def entry_forward(lib, x, w, shift, relu=False, dims=None):
    """mdetr_conv_taps_f32 on x [B, H, W, C], w [N, 3, 3, C] (contiguous fp32, CPU: the shim; CUDA: device 0) -> (rc, y [B, OH, OW, N])."""
    B, H, W, C = x.shape
    N = w.shape[0]
    OH, OW = out_hw(H, W)
    y = torch.empty(B, OH, OW, N, dtype=F32, device=x.device)
    d = torch.tensor(dims if dims is not None else taps_dims(B, H, W, C, N), dtype=torch.int64)
    cuda = x.is_cuda
    rc = lib.mdetr_conv_taps_f32(x.data_ptr(), w.data_ptr(), shift.data_ptr() if shift is not None else None, y.data_ptr(), d.data_ptr(),
                                 1 if relu else 0, x.device.index if cuda else -1, torch.cuda.current_stream(x.device).cuda_stream if cuda else None)
    return rc, y


def entry_split(lib, x, w, shift, ks):
    """mdetr_conv_taps_f32_split -> (rc, partials [ks, B, OH, OW, N])."""
    B, H, W, C = x.shape
    N = w.shape[0]
    OH, OW = out_hw(H, W)
    part = torch.full((ks, B, OH, OW, N), float("nan"), dtype=F32, device=x.device)
    d = torch.tensor(taps_dims(B, H, W, C, N), dtype=torch.int64)
    cuda = x.is_cuda
    rc = lib.mdetr_conv_taps_f32_split(x.data_ptr(), w.data_ptr(), shift.data_ptr() if shift is not None else None, part.data_ptr(), part.numel(),
                                       d.data_ptr(), ks, x.device.index if cuda else -1, torch.cuda.current_stream(x.device).cuda_stream if cuda else None)
    return rc, part


def check_split_entry(lib, dev, shape=(2, 5, 7, 128, 64), splits=(2, 4)):
    """The split entry directly at C = 128: the partials summed in order against fp64 (the random case's bound) and against the unsplit
    entry (both are within the bound of fp64, so within twice the bound of each other); split 0 alone carries the shift."""
    B, H, W, C, N = shape
    x, w, shift, _, ref, mag, _, _ = random_reference(shape, str(dev))
    xn, wn = x.permute(0, 2, 3, 1).contiguous(), w.permute(0, 2, 3, 1).contiguous()
    rc, whole = entry_forward(lib, xn, wn, shift)
    assert rc == 0
    refn, magn = ref.permute(0, 2, 3, 1), mag.permute(0, 2, 3, 1)
    assert_product_close(whole, refn, magn, 9 * C, "conv strided f32 unsplit entry %s" % (shape,))
    bound = product_bound(refn, magn, 9 * C, F32)
    for ks in splits:
        rc, part = entry_split(lib, xn, wn, shift, ks)
        assert rc == 0 and bool(torch.isfinite(part).all()), ks          # every partial element written
        total = part[0].clone()
        for s in range(1, ks):
            total += part[s]
        assert_product_close(total, refn, magn, 9 * C, "conv strided f32 split %d %s" % (ks, shape))
        assert bool(((total.double() - whole.double()).abs() <= 2 * bound).all()), ks
        rc, noshift = entry_split(lib, xn, wn, None, ks)
        assert rc == 0 and torch.equal(noshift[1:], part[1:]) and not torch.equal(noshift[0], part[0]), ks
