"""Cases for the fp32 form of csrc/conv_stem.hip (conv_stem_f32_kernel, mdetr_conv_stem_f32; test infrastructure shared by
tests/test_conv_stem_f32_emulated_cpu.py and tests/test_conv_stem_f32_gpu.py): y = relu(conv7x7 / stride 2 / pad 3 (x, w) + shift) of a
3-channel channels_last fp32 image into 64 channels.  Every premise is checked from the operands and the fp64 value alone, before any
kernel runs (`PremiseError` otherwise).

Exact cases -- the assertion is bit equality with relu(fp64 value), which is itself an fp32 number:
  "x"    full-mantissa image against a weight with ONE +-2^e per output channel at a random (input channel, tap row, tap column): every
         output is a strided, scaled copy of one image channel, or zero where the tap leaves the image -- needs all three parts of x,
         and pins tap, stride, padding and the 24-slot group addressing to the bit.  Output channels 0 and 1 take the central tap of the
         same input channel with opposite signs, so both signs occur (the ReLU is exercised) even on a 1 x 1 image;
  "w"    an image that is non-zero only at pixels with r % 7 == 3 and c % 7 == 3 (one +-2^e channel each) against a full-mantissa weight:
         a 7 x 7 window holds at most one such pixel -- at most one product per output element (needs all three parts of w);
  "int"  dense integer image |x| < 2^11 against a weight with at most 4 non-zeros (|w| < 2^10) per output channel and an integer shift
         |s| < 2^10: sum |x||w| + |s| < 2^24, every partial sum is an integer: exact in any order (mid x mid and the cross terms);
  small integers: exact_cases.conv_case(B, H, W, 3, 64, 7, 2, "wide" / "narrow") cast to fp32, shift + ReLU (narrow: exact-zero
         pre-activations).

Random case: x ~ 0.5 randn, w ~ randn / 12, shift ~ 0.3 randn against relu(conv2d_f64) within gemm_bounds.assert_product_close at
K = 147 (fp32; the three dropped split terms are <= 2 2^-24 per product, inside it).  A second call returns the same bits.

Non-finite case: the random case with one +inf (and, in a second run, one NaN) in a single pixel (r, c), c even.  Outputs whose 7 x 7 window
holds the pixel must be NaN (inf - bf16(inf) is NaN in the split).  The pad elements 21..23 of an operand group are the next pixel's
channels against zero weights, so the outputs at column (c - 4) / 2 of the rows whose windows hold row r may be NaN as well, or equal the
clean run (a documented property of the kernel, not of the convolution).  Every other output is bit-equal to the clean run."""
import functools

import torch

from conv3x3_f32_cases import _low_bits, _pow2
from exact_cases import F32, PremiseError, assert_bits_equal, cl, conv_case, expected, full_mantissa, gen
from gemm_bounds import assert_product_close, conv2d_f64

# (B, H, W): the smallest images that reach each mechanism.  A workgroup is 8 waves = 8 output rows x 32 output columns x 64 channels per
# tile over a 21-row x 70-pixel window, and walks up to 5 column tiles with the next tile's window prefetched.
SHAPES = [
    (1, 1, 1),       # one output, 48 of 49 taps outside: the window is padding but for one pixel
    (2, 5, 7),       # 3 x 4 outputs: smaller than any tile, odd sizes; the second image's byte offset
    (3, 16, 64),     # 8 x 32 outputs: exactly one full tile (all 8 waves, all 32 columns); even H and W: bottom / right padding differ from top / left
    (1, 37, 75),     # 19 x 38 outputs: three row tiles and two column tiles, both ragged (3 rows, 6 columns); the window prefetch once
    (1, 9, 330),     # 5 x 165 outputs: six column tiles = a second workgroup group along x (5 + 1 tiles), a ragged last tile, the prefetch
                     # across every tile boundary of a workgroup
]
KINDS = ("x", "w", "int")
K = 147


def out_hw(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def _conv(x64, w64, shift64=None):
    return conv2d_f64(x64, w64, shift64, stride=2, padding=3)


def _one_per_channel(g):
    """[64, 3, 7, 7] with one +-2^e per output channel at a random (ch, t, e); channels 0 and 1: the central tap of one input channel,
    opposite signs."""
    w = torch.zeros(64, 3, 7, 7)
    n = torch.arange(64)
    ch, t, e = torch.randint(0, 3, (64,), generator=g), torch.randint(0, 7, (64,), generator=g), torch.randint(0, 7, (64,), generator=g)
    v = _pow2(g, (64,))
    ch[1] = ch[0]
    t[:2] = 3
    e[:2] = 3
    v[1] = -v[1].abs() * torch.sign(v[0])
    w[n, ch, t, e] = v
    return w


def _sparse_pixels(g, B, H, W):
    """[B, 3, H, W], non-zero only at pixels (r % 7 == 3, c % 7 == 3): one +-2^e channel each."""
    a = torch.zeros(B, 3, H, W)
    b, r, c = torch.meshgrid(torch.arange(B), torch.arange(3, max(H, 3), 7), torch.arange(3, max(W, 3), 7), indexing="ij")
    b, r, c = b.reshape(-1), r.reshape(-1), c.reshape(-1)
    if b.numel():
        a[b, torch.randint(0, 3, b.shape, generator=g), r, c] = _pow2(g, tuple(b.shape))
    return a


def _few_per_channel(g):
    """[64, 3, 7, 7] integers |w| < 2^10, at most 4 non-zeros per output channel."""
    w = torch.zeros(64, 3, 7, 7)
    n = torch.arange(64)
    for _ in range(4):
        w[n, torch.randint(0, 3, (64,), generator=g), torch.randint(0, 7, (64,), generator=g), torch.randint(0, 7, (64,), generator=g)] = \
            torch.randint(-1023, 1024, (64,), generator=g).float()
    return w


@functools.lru_cache(maxsize=None)
def exact_case(B, H, W, kind):
    """-> (x [B, 3, H, W] channels_last, w [64, 3, 7, 7], shift [64] or None, want [B, 64, OH, OW] channels_last), all fp32; shared by every
    test that asks for the same key: never written to."""
    g = gen(B, H, W, ord(kind[0]), 7)
    what = "conv stem f32 %s B=%d H=%d W=%d" % (kind, B, H, W)
    shift = None
    if kind == "x":
        x, w = full_mantissa(g, (B, 3, H, W)), _one_per_channel(g)
        _low_bits(x, what)
    elif kind == "w":
        x, w = _sparse_pixels(g, B, H, W), full_mantissa(g, (64, 3, 7, 7))
        _low_bits(w, what)
    else:
        x, w = torch.randint(-2047, 2048, (B, 3, H, W), generator=g).float(), _few_per_channel(g)
        shift = torch.randint(-1023, 1024, (64,), generator=g).float()
        if not bool((x.abs() >= 256).any()) or not bool((w.abs() >= 256).any()):
            raise PremiseError(what + ": no operand beyond 8 bits")
    if kind == "int":
        ref = _conv(x.double(), w.double(), shift.double())
        mag = _conv(x.double().abs(), w.double().abs(), shift.double().abs())
        if not float(mag.max()) < 2.0 ** 24:
            raise PremiseError(what + ": sum |x||w| + |s| = %g" % float(mag.max()))
        if not bool((ref < 0).any()) or not bool((ref > 0).any()):
            raise PremiseError(what + ": one sign only")
        want = expected(ref.clamp(min=0), mag, F32, what=what)
    else:
        ref = _conv(x.double(), w.double())
        terms = _conv((x != 0).double(), (w != 0).double())
        if float(terms.max()) > 1.0:
            raise PremiseError(what + ": %d products meet in one element" % int(terms.max()))
        want = ref.clamp(min=0).to(F32)                                  # ONE product of an fp32 number and a power of two: exact in fp64
        if not bool((want.double() == ref.clamp(min=0)).all()) or not bool(torch.isfinite(want).all()):
            raise PremiseError(what + ": the expected value is not an fp32 number")
        if kind == "x":
            if not bool((terms == 0).any()):
                raise PremiseError(what + ": no tap outside the image")
            if not bool((ref < 0).any()) or not bool((ref > 0).any()):
                raise PremiseError(what + ": one sign only")
        elif not bool((want != 0).any()) and min(H, W) >= 4:                # (an image below 4 x 4 has no pixel (3, 3))
            raise PremiseError(what + ": no product")
    return cl(x), w, shift, cl(want)


def record_launches(ext, monkeypatch):
    """-> list that receives the dtype of x at every kernel launch of conv_stem_ext (either form)."""
    calls = []
    real, real_f32 = ext._launch, ext._launch_f32

    def bf16(x, packed, shift, relu=True):
        calls.append(x.dtype)
        return real(x, packed, shift, relu)

    def f32(x, planes, shift, relu=True):
        calls.append(x.dtype)
        return real_f32(x, planes, shift, relu)
    monkeypatch.setattr(ext, "_launch", bf16)
    monkeypatch.setattr(ext, "_launch_f32", f32)
    return calls


def _run(ext, dev, x, w, shift):
    x, w = x.to(dev), w.to(dev)
    assert ext.supported_f32(x, w)
    y = ext.conv_stem(x, w, None if shift is None else shift.to(dev))
    OH, OW = out_hw(x.shape[2], x.shape[3])
    assert y.dtype == F32 and tuple(y.shape) == (x.shape[0], 64, OH, OW) and y.is_contiguous(memory_format=torch.channels_last)
    return y


def check_exact(ext, dev, shape, kinds=KINDS):
    for kind in kinds:
        x, w, shift, want = exact_case(*shape, kind)
        assert_bits_equal(_run(ext, dev, x, w, shift), want, "conv stem f32 %s %s" % (kind, shape))


def check_small_integers(ext, dev, shape):
    """exact_cases.conv_case's integer sets for the stem in fp32, shift + ReLU: wide, and narrow (exact-zero pre-activations)."""
    B, H, W = shape
    for kind in ("wide", "narrow"):
        c = conv_case(B, H, W, 3, 64, 7, 2, kind)
        what = "conv stem f32 integers %s %s" % (shape, kind)
        want = expected(c["pre"].clamp(min=0), c["mpre"], F32, zeros_of=c["pre"] if kind == "narrow" else None, what=what)
        assert_bits_equal(_run(ext, dev, c["x"].float(), c["w"].float().contiguous(), c["shift"]), want, what)


def check_packed_planes(ext, dev="cpu"):
    """pack_weight_f32: hi + mid + lo == w exactly (fp64) for a full-mantissa weight, the layout is pack_weight's per plane, and the pad
    columns of all three planes are exact zeros."""
    w = full_mantissa(gen(64, 3, 7, 7), (64, 3, 7, 7)).to(dev)
    _low_bits(w.cpu(), "pack_weight_f32")
    planes = ext.pack_weight_f32(w)
    assert planes.dtype == torch.bfloat16 and tuple(planes.shape) == (3, 64, 176) and planes.is_contiguous()
    body = planes[:, :, :168].reshape(3, 64, 7, 24)
    assert bool((body[..., 21:] == 0).all()) and bool((planes[:, :, 168:] == 0).all())
    total = body[..., :21].double().sum(0).view(64, 7, 7, 3).permute(0, 3, 1, 2)           # [n, t, e, ch] -> [n, ch, t, e]
    assert bool((total == w.double()).all())
    assert bool((planes[1] != 0).any()) and bool((planes[2] != 0).any())
    assert torch.equal(planes[0], ext.pack_weight(w.to(torch.bfloat16)))                      # hi = bf16(w), in the bf16 form's layout
    assert torch.equal(ext.pack_weight_f32(cl(w)), planes)                                    # whatever the weight's strides


def random_operands(shape, dev):
    B, H, W = shape
    g = torch.Generator(device=dev).manual_seed(B * 1000 + H * W + 7)
    mk = lambda *s: torch.randn(*s, device=dev, generator=g)          # noqa: E731
    return (mk(B, H, W, 3) * 0.5).permute(0, 3, 1, 2), mk(64, 3, 7, 7) / 12.0, mk(64) * 0.3


@functools.lru_cache(maxsize=None)
def random_reference(shape, dev):
    """-> (x, w, shift, ref, mag): the operands, relu(fp64 value) and the magnitude sum |x||w| + |shift| on `dev`; shared, never written to."""
    x, w, shift = random_operands(shape, dev)
    ref = _conv(x.double(), w.double(), shift.double()).clamp_(min=0)
    mag = _conv(x.double().abs(), w.double().abs(), shift.double().abs())
    return x, w, shift, ref, mag


def check_random(ext, dev, shape, twice=False):
    """y against relu(fp64) within the fp32-accumulation bound at K = 147; fp64 on `dev`.  twice: a second call returns the same bits.  -> y"""
    x, w, shift, ref, mag = random_reference(shape, str(dev))
    assert x.is_contiguous(memory_format=torch.channels_last)
    y = _run(ext, dev, x, w, shift)
    assert_product_close(y, ref, mag, K, "conv stem f32 random %s" % (shape,))
    if twice:
        assert torch.equal(_run(ext, dev, x, w, shift), y)
    return y


def nonfinite_pixel(shape):
    """The pixel (r, c) of the non-finite case: the middle of the image, c even."""
    _, H, W = shape
    return H // 2, (W // 2) // 2 * 2


def check_nonfinite(ext, dev, shape):
    B, H, W = shape
    OH, OW = out_hw(H, W)
    x, w, shift, _, _ = random_reference(shape, str(dev))
    clean = _run(ext, dev, x, w, shift).cpu()
    assert bool(torch.isfinite(clean).all())
    r, c = nonfinite_pixel(shape)
    assert c % 2 == 0 and 0 <= r < H and 0 <= c < W
    rows = torch.arange(OH).view(-1, 1)
    cols = torch.arange(OW).view(1, -1)
    row_hit = (2 * rows - 3 <= r) & (r <= 2 * rows + 3)
    must = row_hit & (2 * cols - 3 <= c) & (c <= 2 * cols + 3)          # the 7 x 7 window holds the pixel
    may = row_hit & (cols == (c - 4) // 2) & ~must                      # the pad elements of the operand group fall on it
    excluded = int((must | may).sum())
    assert 1 <= int(must.sum()) <= 16 and excluded <= 4 * 4 + 4, (shape, int(must.sum()), excluded)
    for b in sorted({0, B - 1}):                                        # the first and the last image: the batch offset
        for value in (float("inf"), float("nan")):
            xb = x.clone()
            xb[b, 1, r, c] = value
            y = _run(ext, dev, xb, w, shift).cpu()
            tag = "conv stem f32 %s at image %d pixel (%d, %d) of %s" % (value, b, r, c, shape)
            assert bool(y[b][:, must].isnan().all()), tag
            got, want = y[b][:, may], clean[b][:, may]
            assert bool((got.isnan() | (got == want)).all()), tag
            keep = torch.ones(B, 1, OH, OW, dtype=torch.bool)
            keep[b, 0] = ~(must | may)
            keep = keep.expand(B, 64, OH, OW)
            assert_bits_equal(y[keep], clean[keep], tag + ": outputs away from the pixel")
            assert not bool(y[keep].isnan().any()), tag


def entry(lib, x, planes, shift, y, B, H, W, xp=None, wp=None, yp=None):
    """mdetr_conv_stem_f32 on CPU tensors (the shim) or device 0; pointer overrides for the refusal tests."""
    cuda = x is not None and x.is_cuda
    ptr = lambda t: None if t is None else t.data_ptr()               # noqa: E731
    return lib.mdetr_conv_stem_f32(ptr(x) if xp is None else xp, ptr(planes) if wp is None else wp, ptr(shift), ptr(y) if yp is None else yp,
                                   B, H, W, x.device.index if cuda else -1, torch.cuda.current_stream(x.device).cuda_stream if cuda else None)
