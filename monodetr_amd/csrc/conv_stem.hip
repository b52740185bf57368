// monodetr_amd/csrc/conv_stem.hip -- the ResNet stem: 7x7 / stride 2 / pad 3 convolution of the 3-channel image into 64 channels,
// frozen-BN shift + ReLU in the epilogue, as an implicit GEMM on the matrix cores (torchvision ResNet.conv1 -> bn1 -> relu behind
// lib/models/monodetr/backbone.py:93-106; frozen, so forward only).  MIOpen runs it in 116 us at B = 8, 384 x 1280
// (profiles/r02v: igemm_fwd_gtcx35 ... 256x64x8), 18.5 GFLOP: 160 TFLOP/s.
//
//   y[b, r, c, n] = relu( shift[n] + sum_{t < 7, e < 7, ch < 3} x[b, 2r + t - 3, 2c + e - 3, ch] * w[n, t, e, ch] )
//
// With 3 channels a pixel is 6 bytes: there is no 64-channel slab to stage.  The contraction index is laid out per tap ROW: the
// 7 taps x 3 channels of one input row are 21 CONSECUTIVE bf16 of the channels-last image, padded to 24 = three 8-element
// operand groups, so K = 7 x 24 = 168 (+ 8 zeros = 11 k-steps of 16).  The input window of a tile -- 13 rows x 70 pixels -- is
// copied into LDS as it lies in memory (2-byte buffer loads: zero outside the image = the padding); a lane's B operand for
// group (t, m) is the 8 bf16 at element 6 c + 8 m of window row 2 r + t: four aligned 4-byte LDS reads (12 c + 16 m bytes; the
// lanes of a half-wave are 3 banks apart: conflict-free).  The pad elements 21..23 of a group are the NEXT pixel's channels
// (finite data) against zero weights.  The packed weight [64][7][24] (+ 8 zeros) is built once by the caller -- the stem is
// frozen -- and held in LDS by the workgroup across its column tiles.
// Workgroup = 4 waves = 4 output rows x 32 output columns x 64 channels per tile, looping over kTilesPerWg column tiles.
// conv_stem_f32_kernel below is the fp32 form of the same job (three-way bf16 split, six product terms): see the comment above it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mdetr_wave.h>

#include "conv_stem.h"
#include "mdetr_split.h"
#include "msda.h"       // profile scopes

namespace mdetr {
namespace {

constexpr int kWavesS = 4, kTileWS = 32;
constexpr int kKS = 176;                  // packed contraction length: 7 x 24 + 8 zeros
constexpr int kWRow = kKS + 8;            // bf16 per weight row in LDS (23 sixteen-byte slots: odd)
constexpr int kWinRows = 2 * (kWavesS - 1) + 7;          // 13
constexpr int kWinPix = 2 * (kTileWS - 1) + 8;           // 70 pixels: 69 needed + the one the pad elements of the last lane fall on
constexpr int kWinEl = kWinPix * 3;                      // 210
constexpr int kWinRow = 216;                             // bf16 per window row in LDS
constexpr int kTilesPerWg = 5;

struct StemDims {
    int B, H, W, OH, OW, tiles_x, groups_x, tiles_y;
};

__global__ __launch_bounds__(kWavesS * 64)
void conv_stem_kernel(const __bf16 *__restrict__ x, const __bf16 *__restrict__ wp, const float *__restrict__ shift,
                      __bf16 *__restrict__ y, const StemDims d)
{
    __shared__ __attribute__((aligned(16))) __bf16 wts[64 * kWRow];
    __shared__ __attribute__((aligned(16))) unsigned short win[kWinRows * kWinRow];
    __shared__ float shift_s[64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, col = lane & 31;
    int id = blockIdx.x;
    const int gx = id % d.groups_x; id /= d.groups_x;
    const int ty = id % d.tiles_y; const int b = id / d.tiles_y;
    const int r0 = ty * kWavesS;

    for (int i = threadIdx.x; i < 64 * (kKS / 8); i += kWavesS * 64) {       // packed weight -> LDS, 16 bytes at a time
        const int n = i / (kKS / 8), piece = i - n * (kKS / 8);
        *reinterpret_cast<bf16x8 *>(wts + n * kWRow + piece * 8) = *reinterpret_cast<const bf16x8 *>(wp + n * kKS + piece * 8);
    }
    if (threadIdx.x < 64) shift_s[threadIdx.x] = shift ? shift[threadIdx.x] : 0.f;

    const mdetr_rsrc xr = make_rsrc(x, static_cast<unsigned>(static_cast<int64_t>(d.B) * d.H * d.W * 6));
    // The window of the NEXT column tile is requested while this tile's products run and stored behind the barrier: one 2-byte load
    // per thread and loop iteration straight into LDS -- the first version -- was 11 dependent round trips per tile ahead of the
    // first matrix instruction.  (A tile beyond the row reads nothing: offsets beyond the resource.)
    constexpr int kWinLoads = (kWinRows * kWinEl + kWavesS * 64 - 1) / (kWavesS * 64);
    unsigned short wreg[kWinLoads];
    auto fetch_window = [&](int tx) {
        const int c0n = tx * kTileWS;
#pragma unroll
        for (int j = 0; j < kWinLoads; ++j) {
            const int i = threadIdx.x + j * kWavesS * 64;
            const int wr = i / kWinEl, el = i - wr * kWinEl;
            const int row = 2 * r0 + wr - 3, gel = (2 * c0n - 3) * 3 + el;   // element of the image row
            const bool in = tx < d.tiles_x && i < kWinRows * kWinEl && row >= 0 && row < d.H && gel >= 0 && gel < d.W * 3;
            wreg[j] = rsrc_load_u16(xr, in ? static_cast<unsigned>((row * d.W * 3 + gel) * 2) : kRsrcOob,
                                    static_cast<unsigned>(b) * static_cast<unsigned>(d.H * d.W * 6));
        }
    };
    fetch_window(gx * kTilesPerWg);
    for (int tt = 0; tt < kTilesPerWg; ++tt) {
        const int tx = gx * kTilesPerWg + tt;
        if (tx >= d.tiles_x) break;                                          // uniform
        const int c0 = tx * kTileWS;
        __syncthreads();                                                     // the previous tile's window reads are done (and, first time, nothing)
        // window: rows 2 r0 - 3 .. + 12, elements (2 c0 - 3) * 3 .. + 209 of each
#pragma unroll
        for (int j = 0; j < kWinLoads; ++j) {
            const int i = threadIdx.x + j * kWavesS * 64;
            if (i < kWinRows * kWinEl) win[(i / kWinEl) * kWinRow + (i % kWinEl)] = wreg[j];
        }
        if (tt + 1 < kTilesPerWg) fetch_window(tx + 1);                      // in flight during the products below
        __syncthreads();

        f32x16 acc[2];
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[nb][i] = 0.f;
#pragma unroll
        for (int ks = 0; ks < kKS / 16; ++ks) {
            int gidx = 2 * ks + half;                                        // operand group (t, m) = (g / 3, g % 3)
            if (gidx > 20) gidx = 20;                                        // the 8 zero weights at the end: any finite data
            const int t = gidx / 3, m = gidx - 3 * t;
            const unsigned *src = reinterpret_cast<const unsigned *>(win + (2 * wave + t) * kWinRow + 6 * col + 8 * m);
            unsigned q[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) q[i] = src[i];
            bf16x8 xv;
            __builtin_memcpy(&xv, q, 16);
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) {
                const bf16x8 wv = *reinterpret_cast<const bf16x8 *>(wts + (nb * 32 + col) * kWRow + ks * 16 + half * 8);
                acc[nb] = mfma_bf16(wv, xv, acc[nb]);                        // Y^T[n][pixel]
            }
        }
        // epilogue: lane = pixel (row wave, column lane & 31); register quad q of block nb = channels 32 nb + 8 q + 4 half + 0..3
        const int r = r0 + wave, c = c0 + col;
        if (r < d.OH && c < d.OW) {
            __bf16 *yp = y + ((static_cast<int64_t>(b) * d.OH + r) * d.OW + c) * 64 + 4 * half;
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                for (int qd = 0; qd < 4; ++qd) {
                    bf16x4 o;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        float v = acc[nb][4 * qd + i] + shift_s[nb * 32 + 8 * qd + 4 * half + i];
                        o[i] = static_cast<__bf16>(v > 0.f ? v : 0.f);
                    }
                    *reinterpret_cast<bf16x4 *>(yp + nb * 32 + 8 * qd) = o;
                }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The fp32 form: x, shift and y are fp32; the products run on the bf16 matrix instruction through the three-way split of
// mdetr_split.h (hi + mid + lo carry the 24 significant bits of a value), as in tgemm.hip / conv3x3.hip / conv_taps.hip.  Kept from
// the kernel above: the contraction layout (per tap row 21 consecutive channels-last values padded to 24, K = 176, 11 k-steps), the
// window copied into LDS as it lies in memory through buffer-resource loads that return the zero padding, the operand address
// 6 c + 8 m of a window row and its bank argument, the next tile's window in flight during this tile's products, lane = pixel.
// What differs:
//   * a pixel is 12 bytes: one 4-byte load per window element; the element is split ONCE, between the staging registers and LDS
//     (split4), into three bf16 window PLANES with the row layout above -- the fragment reads are that kernel's, per plane;
//   * the packed weight arrives as three bf16 planes [3][64][176] (hi, mid, lo of the folded fp32 weight, split once by the caller:
//     the stem is frozen) and is held in LDS by the workgroup across its column tiles;
//   * per k-step one x triple and two weight triples feed 12 matrix instructions: lo.hi, hi.lo, mid.mid, mid.hi, hi.mid, hi.hi (small
//     terms first, the order of mdetr_split.h) into the one fp32 accumulator of each 32-channel block;
//   * the epilogue adds the shift, applies the ReLU and stores 16 bytes of fp32: no rounding but the accumulation's.  No atomics.
// An infinite pixel yields NaN (x - bf16(x)).  The pad elements 21..23 of an operand group are the NEXT pixel's channels against zero
// weights, so a non-finite pixel at column p of a window row also turns the outputs at column (p - 4) / 2 of the rows whose windows
// hold that row into NaN (0 x NaN), beyond its 7x7 receptive field.
//
// Geometry (160 KiB of LDS per CU).  The three weight planes are 3 x 64 x 184 x 2 = 70 656 B whatever the tile.  With the 4-row tile
// above (window 3 x 13 x 216 x 2 = 16 848 B) that is ONE four-wave workgroup per CU: every barrier parks the matrix cores.  Built:
// 8 waves = 8 output rows x 32 columns, a 21-row window (3 x 21 x 216 x 2 = 27 216 B), 98 128 B with the shift: one workgroup per CU,
// two waves per SIMD, so one wave's LDS reads run under the other's matrix instructions, and 2.6 window rows are staged (and split)
// per output row instead of 3.25.  The weights alone keep a second workgroup out whatever the window; a 32-channel half per workgroup
// (52 KB, three per CU) would stage and split every window twice.  kTilesPerWgF = 5 as above: at B = 8, 384 x 1280 the launch is
// 8 x 24 x 4 = 768 workgroups = three whole rounds of 256 CUs, at 512 x 1760 8 x 32 x 6 = 1 536 = six (tools/rounds.py).
constexpr int kWavesF = 8;                                   // = output rows per workgroup
constexpr int kThreadsF = kWavesF * 64;
constexpr int kWinRowsF = 2 * (kWavesF - 1) + 7;             // 21
constexpr int kTilesPerWgF = 5;
constexpr int kWPlaneF = 64 * kWRow;                         // bf16 elements of one weight plane in LDS
constexpr int kWinPlaneF = kWinRowsF * kWinRow;              // ... of one window plane
constexpr size_t kLdsF = static_cast<size_t>(3) * kWPlaneF * 2 + static_cast<size_t>(3) * kWinPlaneF * 2 + 64 * 4;
static_assert(kLdsF == 70656 + 27216 + 256, "the LDS arithmetic of the comment above");
static_assert(kLdsF <= 160 * 1024 && 2 * kLdsF > 160 * 1024, "one eight-wave workgroup per CU");
static_assert((3 * kWPlaneF * 2) % 16 == 0 && (3 * kWinPlaneF * 2) % 16 == 0, "planes and the shift start on 16-byte boundaries");
static_assert(6 * (kTileWS - 1) + 8 * 2 + 8 <= kWinEl, "the last lane's last operand group lies inside the window row");

// One 4-byte buffer-resource load (zero beyond the resource, as rsrc_load_u16).  The CPU emulation of the tests has the 2-byte load
// only and composes it: the halves are in range or out of range together, since offsets and the resource size are multiples of 4.
__device__ __forceinline__ float rsrc_load_f32(mdetr_rsrc r, unsigned lane_offset, unsigned scalar_offset)
{
#if defined(__HIPCC__)
    const unsigned u = __builtin_amdgcn_raw_buffer_load_b32(r, lane_offset, scalar_offset, 0);
#else
    const unsigned u = static_cast<unsigned>(rsrc_load_u16(r, lane_offset, scalar_offset)) |
                       (static_cast<unsigned>(rsrc_load_u16(r, lane_offset == kRsrcOob ? kRsrcOob : lane_offset + 2, scalar_offset)) << 16);
#endif
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}

__global__ __launch_bounds__(kThreadsF)
void conv_stem_f32_kernel(const float *__restrict__ x, const __bf16 *__restrict__ wp, const float *__restrict__ shift,
                          float *__restrict__ y, const StemDims d)
{
    MDETR_DYNAMIC_LDS(unsigned char, stem_f32_smem);
    __bf16 *wts = reinterpret_cast<__bf16 *>(stem_f32_smem);                 // [hi, mid, lo][64][kWRow]
    __bf16 *win = wts + 3 * kWPlaneF;                                        // [hi, mid, lo][kWinRowsF][kWinRow]
    float *shift_s = reinterpret_cast<float *>(win + 3 * kWinPlaneF);        // [64]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, col = lane & 31;
    int id = blockIdx.x;
    const int gx = id % d.groups_x; id /= d.groups_x;
    const int ty = id % d.tiles_y; const int b = id / d.tiles_y;
    const int r0 = ty * kWavesF;

    for (int i = threadIdx.x; i < 3 * 64 * (kKS / 8); i += kThreadsF) {      // packed weight planes -> LDS, 16 bytes at a time
        const int row = i / (kKS / 8), piece = i - row * (kKS / 8);          // row = plane * 64 + n
        *reinterpret_cast<bf16x8 *>(wts + row * kWRow + piece * 8) = *reinterpret_cast<const bf16x8 *>(wp + row * kKS + piece * 8);
    }
    if (threadIdx.x < 64) shift_s[threadIdx.x] = shift ? shift[threadIdx.x] : 0.f;

    // (byte offsets are fp32 bytes: B H W 12 < 2^31)
    const mdetr_rsrc xr = make_rsrc(x, static_cast<unsigned>(static_cast<int64_t>(d.B) * d.H * d.W * 12));
    const unsigned xb_off = static_cast<unsigned>(b) * static_cast<unsigned>(d.H * d.W * 12);
    // the window of the NEXT column tile, requested while this tile's products run and split behind the barrier
    constexpr int kWinLoads = (kWinRowsF * kWinEl + kThreadsF - 1) / kThreadsF;       // 9
    constexpr int kWinQuads = (kWinLoads + 3) / 4;
    float wreg[4 * kWinQuads];
#pragma unroll
    for (int j = kWinLoads; j < 4 * kWinQuads; ++j) wreg[j] = 0.f;
    auto fetch_window = [&](int tx) {
        const int c0n = tx * kTileWS;
#pragma unroll
        for (int j = 0; j < kWinLoads; ++j) {
            const int i = threadIdx.x + j * kThreadsF;
            const int wr = i / kWinEl, el = i - wr * kWinEl;
            const int row = 2 * r0 + wr - 3, gel = (2 * c0n - 3) * 3 + el;   // element of the image row
            const bool in = tx < d.tiles_x && i < kWinRowsF * kWinEl && row >= 0 && row < d.H && gel >= 0 && gel < d.W * 3;
            wreg[j] = rsrc_load_f32(xr, in ? static_cast<unsigned>((row * d.W * 3 + gel) * 4) : kRsrcOob, xb_off);
        }
    };
    fetch_window(gx * kTilesPerWgF);
    for (int tt = 0; tt < kTilesPerWgF; ++tt) {
        const int tx = gx * kTilesPerWgF + tt;
        if (tx >= d.tiles_x) break;                                          // uniform
        const int c0 = tx * kTileWS;
        __syncthreads();                                                     // the previous tile's window reads are done (and, first time, nothing)
        // window: rows 2 r0 - 3 .. + 20, elements (2 c0 - 3) * 3 .. + 209 of each; the one split of a value on its way into the planes
#pragma unroll
        for (int q = 0; q < kWinQuads; ++q) {
            const float v[4] = {wreg[4 * q], wreg[4 * q + 1], wreg[4 * q + 2], wreg[4 * q + 3]};
            bf16x4 h, m, l;
            split4(v, h, m, l);
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const int j = 4 * q + jj;
                if (j >= kWinLoads) break;
                const int i = threadIdx.x + j * kThreadsF;
                if (i < kWinRowsF * kWinEl) {
                    __bf16 *dst = win + (i / kWinEl) * kWinRow + (i % kWinEl);
                    dst[0] = h[jj]; dst[kWinPlaneF] = m[jj]; dst[2 * kWinPlaneF] = l[jj];
                }
            }
        }
        if (tt + 1 < kTilesPerWgF) fetch_window(tx + 1);                     // in flight during the products below
        __syncthreads();

        f32x16 acc[2];
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[nb][i] = 0.f;
#pragma unroll
        for (int ks = 0; ks < kKS / 16; ++ks) {
            int gidx = 2 * ks + half;                                        // operand group (t, m) = (g / 3, g % 3)
            if (gidx > 20) gidx = 20;                                        // the 8 zero weights at the end: data of this lane's own window
            const int t = gidx / 3, m = gidx - 3 * t;
            const __bf16 *src = win + (2 * wave + t) * kWinRow + 6 * col + 8 * m;
            const __bf16 *wsrc = wts + col * kWRow + ks * 16 + half * 8;
            bf16x8 xf[3], wf[3][2];                                          // planes: 0 = hi, 1 = mid, 2 = lo
#pragma unroll
            for (int p = 0; p < 3; ++p) {
                unsigned q[4];                                               // four aligned 4-byte LDS reads (12 c + 16 m bytes)
#pragma unroll
                for (int i = 0; i < 4; ++i) q[i] = reinterpret_cast<const unsigned *>(src + p * kWinPlaneF)[i];
                __builtin_memcpy(&xf[p], q, 16);
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) wf[p][nb] = *reinterpret_cast<const bf16x8 *>(wsrc + p * kWPlaneF + nb * 32 * kWRow);
            }
            constexpr int term_w[6] = {2, 0, 1, 1, 0, 0}, term_x[6] = {0, 2, 1, 0, 1, 0};     // lo.hi, hi.lo, mid.mid, mid.hi, hi.mid, hi.hi
#pragma unroll
            for (int i = 0; i < 6; ++i)
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) acc[nb] = mfma_bf16(wf[term_w[i]][nb], xf[term_x[i]], acc[nb]);       // Y^T[n][pixel]
        }
        // epilogue: lane = pixel (row wave, column lane & 31); register quad q of block nb = channels 32 nb + 8 q + 4 half + 0..3
        const int r = r0 + wave, c = c0 + col;
        if (r < d.OH && c < d.OW) {
            float *yp = y + ((static_cast<int64_t>(b) * d.OH + r) * d.OW + c) * 64 + 4 * half;
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                for (int qd = 0; qd < 4; ++qd) {
                    float o[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float v = acc[nb][4 * qd + i] + shift_s[nb * 32 + 8 * qd + 4 * half + i];
                        o[i] = !(v <= 0.f) ? v : 0.f;                          // (a NaN stays one)
                    }
                    f32x4 ov;
                    __builtin_memcpy(&ov, o, 16);
                    *reinterpret_cast<f32x4 *>(yp + nb * 32 + 8 * qd) = ov;
                }
        }
    }
}

}  // namespace

bool conv_stem_supported(int B, int H, int W, const void *x, const void *wp, const void *y)
{
    const auto al = [](const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; };
    return B > 0 && H > 0 && W > 0 && al(x, 2) && al(wp, 16) && al(y, 8) && static_cast<int64_t>(B) * H * W * 6 < (1ll << 31);
}

hipError_t conv_stem_launch(const void *x, const void *wp, const float *shift, void *y, int B, int H, int W, hipStream_t st)
{
    StemDims d;
    d.B = B; d.H = H; d.W = W;
    d.OH = (H - 1) / 2 + 1; d.OW = (W - 1) / 2 + 1;
    d.tiles_x = (d.OW + kTileWS - 1) / kTileWS;
    d.groups_x = (d.tiles_x + kTilesPerWg - 1) / kTilesPerWg;
    d.tiles_y = (d.OH + kWavesS - 1) / kWavesS;
    const int64_t blocks = static_cast<int64_t>(B) * d.tiles_y * d.groups_x;
    ProfileScope prof(9, conv_mflop(static_cast<int64_t>(B) * d.OH * d.OW, 64 * 3 * 49), st, 2.0 * B * d.OH * d.OW * 64 * 147 / 1e6,
                      (2.0 * B * (static_cast<double>(d.H) * d.W * 3 + static_cast<double>(d.OH) * d.OW * 64)) / 1e3);
    hipLaunchKernelGGL(conv_stem_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kWavesS * 64), 0, st, static_cast<const __bf16 *>(x),
                       static_cast<const __bf16 *>(wp), shift, static_cast<__bf16 *>(y), d);
    return hipGetLastError();
}

// ---- the fp32 entry ----
bool conv_stem_f32_supported(int B, int H, int W, const void *x, const void *wp, const void *y)
{
    const auto al = [](const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; };
    return B > 0 && H > 0 && W > 0 && al(x, 4) && al(wp, 16) && al(y, 16) && static_cast<int64_t>(B) * H * W * 12 < (1ll << 31);
}

hipError_t conv_stem_f32_launch(const void *x, const void *wp, const float *shift, void *y, int B, int H, int W, hipStream_t st)
{
    StemDims d;
    d.B = B; d.H = H; d.W = W;
    d.OH = (H - 1) / 2 + 1; d.OW = (W - 1) / 2 + 1;
    d.tiles_x = (d.OW + kTileWS - 1) / kTileWS;
    d.groups_x = (d.tiles_x + kTilesPerWgF - 1) / kTilesPerWgF;
    d.tiles_y = (d.OH + kWavesF - 1) / kWavesF;
    const int64_t blocks = static_cast<int64_t>(B) * d.tiles_y * d.groups_x;
    static bool attr_set[64] = {};                           // per device
    int dev_ = 0;
    if (hipGetDevice(&dev_) != hipSuccess) dev_ = -1;
    if (dev_ < 0 || dev_ >= 64 || !attr_set[dev_]) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(conv_stem_f32_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 static_cast<int>(kLdsF));
        if (e != hipSuccess) return e;
        if (dev_ >= 0 && dev_ < 64) attr_set[dev_] = true;
    }
    // (flops as above -- six matrix instructions per product term --; bytes: the fp32 image, the fp32 output, the three weight planes)
    ProfileScope prof(9, conv_mflop(static_cast<int64_t>(B) * d.OH * d.OW, 64 * 3 * 49), st, 2.0 * B * d.OH * d.OW * 64 * 147 / 1e6,
                      (4.0 * B * (static_cast<double>(d.H) * d.W * 3 + static_cast<double>(d.OH) * d.OW * 64) + 3.0 * 64 * kKS * 2) / 1e3);
    hipLaunchKernelGGL(conv_stem_f32_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kThreadsF), kLdsF, st, static_cast<const float *>(x),
                       static_cast<const __bf16 *>(wp), shift, static_cast<float *>(y), d);
    return hipGetLastError();
}

}  // namespace mdetr
