// monodetr_amd/csrc/conv_wgrad.hip -- weight gradient of the backbone's / pyramid's / depth head's 3x3 (stride 1 and 2) and
// strided 1x1 convolutions on the matrix cores: split-K over pixel tiles, both operands transposed on their way into LDS.
//
//   dW[n, t, e, c] = sum_{b, r, q} dY[b, r, q, n] * X[b, SI r + t - P, SI q + e - P, c]        (P = 1 for 3x3, 0 for 1x1)
//
// Reference: autograd of torchvision Bottleneck.conv2 / downsample (lib/models/monodetr/backbone.py:93-106), the 3x3 / stride-2
// pyramid level (monodetr.py:87-92) and the depth predictor's convolutions (depth_predictor.py:29-56), which the reference
// leaves to cuDNN.  MIOpen's igemm_wrw kernels take 71 us per 18.1-GFLOP layer here (255 TFLOP/s, profiles/r02v).
//
// The contraction index is the PIXEL, the slow axis of both channels-last operands: an MFMA lane needs 8 consecutive
// contraction values of one channel, so both operands are transposed -- in registers, an 8 x 8 bf16 block per thread (8 loads of
// 16 bytes = 8 channels of 8 rows; 32 two-word permutes; 8 stores of 16 bytes = 8 rows of 8 channels) -- on their way into LDS:
//   dYt[n][q][8 rows],   Xt[c][x column][8 rows]                       (a lane's operand = one aligned 16-byte read)
// The group of 8 contraction values is 8 ROWS of one column: a tap's column shift e then moves the read by whole 16-byte
// slots (8 consecutive columns would be shifted by 2 bytes: misaligned), and the tap's ROW shift t is taken out of the kernel's
// inner structure altogether -- a workgroup owns ONE tap row t and loads its X rows already shifted.  With SI = 2 the X columns
// are stored de-interleaved (even columns, then odd), as in conv_taps.hip.
// Workgroup = 8 waves: (tap row t, 128 output channels n, 64 input channels c, a chunk of the pixel tiles); wave w owns
// n-block w & 3 and c-block w >> 2: TS accumulator tiles D[n][c] (32 x 32) per wave, one per tap column.  A pixel tile is
// 8 output rows x kCols (16) output columns of one image = kCols / 2 MFMA k-steps (2 columns x 8 rows each).  The next tile's global loads are
// issued before the current tile's products and transposed into the single LDS buffer after them.
// Output: per-chunk partial gradients P[chunk][n][t][e][c] in fp32; colsum.hip adds the chunks in a fixed order and rounds once
// into the parameter's dtype (deterministic, no atomics).
// Algorithmic bytes = 2 B (H W C + OH OW N) + 4 TR TS N C;  flops = 2 B OH OW TR TS C N.  MFMA-bound by design.
// The fp32 form of the 3x3 / stride-1 case (mdetr_conv_wgrad_f32: fp32 x and dy, three-way bf16 split, six terms per product) is the
// sibling kernel conv_wgrad_f32_kernel further down; the fp32 form of the 3x3 / stride-2 case (mdetr_conv_wgrad_s2_f32) is
// conv_wgrad_s2_f32_kernel behind it, with a tile of its own.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <mdetr_wave.h>

#include "conv_wgrad.h"
#include "mdetr_tune.h"
#include "mdetr_transpose.h"
#include "mdetr_split.h"
#include "msda.h"      // profile scopes

namespace mdetr {
namespace {

constexpr int kThreadsG = 512;
constexpr int kNB = 128, kCB = 64;       // output / input channels per workgroup
// Columns of a pixel tile: 16.  With 32 the two transposed operand tiles take 103 - 134 KB of LDS -- one workgroup (8 waves) per CU;
// with 16 they take 54 - 70 KB and two workgroups fit.  Measured (profiles/r03s_wgrad_cols{32,16_wgs256}.json): 3x3 weight
// gradient of layer2 / 3 / 4 46 / 51 / 82 us -> 43 / 42 / 63 us at the same ~256 workgroups (more workgroups = more fp32 chunk
// partials to write and sum: 512 is slower again).
#ifndef MDETR_CONV_WGRAD_COLS
#define MDETR_CONV_WGRAD_COLS 16
#endif
constexpr int kRows = 8, kCols = MDETR_CONV_WGRAD_COLS;     // output pixels of a tile (columns: 16 or 32)
constexpr int kDyStride = kCols + 1;     // 16-byte slots per n row of dYt: odd, so the 16 lanes of a b128 group fall on distinct slots

struct WgradGeom {
    ConvWgradDims d;
    int bands, ctiles, units, chunks, nblocks, cblocks;
};

template <int SI, int TS>
__global__ __launch_bounds__(kThreadsG)
void conv_wgrad_kernel(const __bf16 *__restrict__ x, const __bf16 *__restrict__ dy, float *__restrict__ part, const WgradGeom g)
{
    constexpr int P = TS == 3 ? 1 : 0;
    // x columns of a tile in LDS: SI = 1: 32 + TS - 1 consecutive; SI = 2, 3 taps: 33 even + 32 odd; SI = 2, 1 tap: the 32 even ones
    constexpr int XC = SI == 1 ? kCols + TS - 1 : (TS == 3 ? 2 * kCols + 1 : kCols);
    constexpr int XSTRIDE = XC | 1;                                          // odd number of 16-byte slots per channel row
    constexpr int EVEN = kCols + 1;                                          // SI = 2, 3 taps: slots [0, 33) even columns, [33, 65) odd
    MDETR_DYNAMIC_LDS(unsigned char, wgrad_smem);
    bf16x8 *dyt = reinterpret_cast<bf16x8 *>(wgrad_smem);                    // [kNB][kDyStride]
    bf16x8 *xt = dyt + kNB * kDyStride;                                      // [kCB][XSTRIDE]
    const ConvWgradDims &d = g.d;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, l31 = lane & 31;
    const int nsub = wave & 3, csub = wave >> 2;
    int id = blockIdx.x;
    const int chunk = id % g.chunks; id /= g.chunks;
    const int t = id % TS; id /= TS;                                         // tap row (TR = TS)
    const int cblk = id % g.cblocks; const int nblk = id / g.cblocks;
    const int n0 = nblk * kNB, c0 = cblk * kCB;

    f32x16 acc[TS];
#pragma unroll
    for (int e = 0; e < TS; ++e)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[e][i] = 0.f;
    // the bias gradient of a token-wise linear layer rides along (d.DB): db[n] = sum over pixels of dY[.][n] is the product of the
    // dY^T operand already in LDS with a matrix of ones -- one more MFMA per k-step on the waves of the first input-channel block,
    // no second pass over dY (a separate column sum: two launches and 42 MB per 81 600-row layer)
    const bool want_db = TS == 1 && d.DB != 0 && cblk == 0 && csub == 0;       // wave-uniform
    f32x16 accb;
#pragma unroll
    for (int i = 0; i < 16; ++i) accb[i] = 0.f;
    bf16x8 ones;
#pragma unroll
    for (int i = 0; i < 8; ++i) ones[i] = static_cast<__bf16>(1.0f);

    // ---- loading tasks: one 8 x 8 block (8 rows x 8 channels) per lane.  A WAVE takes 16 columns x 4 channel pieces of one operand
    // (lane = 16 piece + column): the 16 lanes of a ds_write_b128 group then store 16 CONSECUTIVE slots of one channel row --
    // conflict-free (8 lanes = the 8 pieces of one pixel, the coalescing-friendly order, put 4 lanes on each of two bank quads:
    // 68 % of the LDS cycles were conflicts, profiles/r03b_pmc_conv.json) -- while a load instruction still covers 64 contiguous
    // bytes of each of its 16 pixels.
    constexpr int CGX = (XC + 15) / 16;                                      // column groups of the X window
    constexpr int WTASKS = 2 * CGX + 4 * (kCols / 16);                       // X: CGX x 2 piece groups; dY: (kCols / 16) x 4
    constexpr int kWavesG = kThreadsG / 64;
    constexpr int ROUNDS = (WTASKS + kWavesG - 1) / kWavesG;
    constexpr int PF = ROUNDS <= 2 ? 2 : 1;                                  // tiles in flight ahead of the products (registers: 32 per round and tile)
    bf16x8 stage[PF][ROUNDS][8];
    // Loads go through buffer resources: a lane outside the image (the convolution's padding, a ragged tile) passes an offset
    // beyond the tensor and receives zeros -- no branch, no zero fill.  Per-lane offset = the column part, scalar offset = the
    // (image, row) part; the tensors are below 2^31 bytes (checked by the launcher).
    const mdetr_rsrc xr = make_rsrc(x, static_cast<unsigned>(static_cast<int64_t>(d.B) * d.H * d.W * d.C * 2));
    const mdetr_rsrc yr = make_rsrc(dy, static_cast<unsigned>(static_cast<int64_t>(d.B) * d.OH * d.OW * d.N * 2));
    const int ci = lane & 15, pi = lane >> 4;
    // what a lane's tasks are does not depend on the tile: (column of the window / of the tile, channel byte offset) per round
    int t_rel[ROUNDS], t_ch[ROUNDS], t_dst[ROUNDS];                          // t_dst: first LDS slot (row of its piece's channel 0)
#pragma unroll
    for (int rd = 0; rd < ROUNDS; ++rd) {
        const int wt = wave + rd * kWavesG;                                  // wave-uniform
        if (wt < 2 * CGX) {
            const int slot = 16 * (wt >> 1) + ci, piece = 4 * (wt & 1) + pi;
            t_rel[rd] = slot >= XC ? -1 : (SI == 1 ? slot : (TS == 3 ? (slot < EVEN ? 2 * slot : 2 * (slot - EVEN) + 1) : 2 * slot));
            t_ch[rd] = (c0 + piece * 8) * 2;
            t_dst[rd] = piece * 8 * XSTRIDE + slot;
        } else {
            const int k = wt - 2 * CGX, col = 16 * (k >> 2) + ci, piece = 4 * (k & 3) + pi;
            t_rel[rd] = col;
            t_ch[rd] = (wt < WTASKS && n0 + piece * 8 < d.N) ? (n0 + piece * 8) * 2 : -1;
            t_dst[rd] = piece * 8 * kDyStride + col;
        }
    }
    auto fetch = [&](int u, bf16x8 (&st)[ROUNDS][8]) {                       // global loads of pixel tile u
        const int ct = u % g.ctiles; u /= g.ctiles;
        const int band = u % g.bands; const int b = u / g.bands;
        const int r0 = band * kRows, q0 = ct * kCols;
#pragma unroll
        for (int rd = 0; rd < ROUNDS; ++rd) {
            const int wt = wave + rd * kWavesG;
            if (wt < 2 * CGX) {
                const int col = SI * q0 + t_rel[rd] - P;
                const unsigned lane_off = (t_rel[rd] >= 0 && col >= 0 && col < d.W) ? static_cast<unsigned>(col * d.C * 2 + t_ch[rd]) : kRsrcOob;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int row = SI * (r0 + i) + t - P;                   // uniform
                    const bool ok = row >= 0 && row < d.H;
                    st[rd][i] = rsrc_load_bf16x8(xr, ok ? lane_off : kRsrcOob, ok ? static_cast<unsigned>((b * d.H + row) * d.W) * static_cast<unsigned>(d.C * 2) : 0u);
                }
            } else if (wt < WTASKS) {
                const int col = q0 + t_rel[rd];
                const unsigned lane_off = (col < d.OW && t_ch[rd] >= 0) ? static_cast<unsigned>(col * d.N * 2 + t_ch[rd]) : kRsrcOob;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int row = r0 + i;
                    const bool ok = row < d.OH;
                    st[rd][i] = rsrc_load_bf16x8(yr, ok ? lane_off : kRsrcOob, ok ? static_cast<unsigned>((b * d.OH + row) * d.OW) * static_cast<unsigned>(d.N * 2) : 0u);
                }
            }
        }
    };
    auto commit = [&](const bf16x8 (&st)[ROUNDS][8]) {                       // transpose the staged blocks into LDS
#pragma unroll
        for (int rd = 0; rd < ROUNDS; ++rd) {
            const int wt = wave + rd * kWavesG;
            if (wt >= WTASKS) continue;
            bf16x8 tr[8];
            transpose8x8(st[rd], tr);
            if (wt < 2 * CGX) {
                if (16 * (wt >> 1) + ci < XC) {
#pragma unroll
                    for (int q = 0; q < 8; ++q) xt[t_dst[rd] + q * XSTRIDE] = tr[q];
                }
            } else {
#pragma unroll
                for (int q = 0; q < 8; ++q) dyt[t_dst[rd] + q * kDyStride] = tr[q];
            }
        }
    };
    auto products = [&]() {
        const bf16x8 *ap = dyt + (nsub * 32 + l31) * kDyStride + half;
        const bf16x8 *bp = xt + (csub * 32 + l31) * XSTRIDE;
#pragma unroll 4
        for (int ks = 0; ks < kCols / 2; ++ks) {
            const int q = 2 * ks + half;                                     // this half-wave's column of the k-step
            const bf16x8 a = ap[2 * ks];
#pragma unroll
            for (int e = 0; e < TS; ++e) {
                int slot;
                if (SI == 1) slot = q + e;
                else if (TS == 3) slot = (e & 1) ? EVEN + q : q + (e >> 1);  // 2q + e: even -> q + e / 2, odd -> after the even ones
                else slot = q;
                acc[e] = mfma_bf16(a, bp[slot], acc[e]);                     // D[n][c] += dY^T[n][8 rows] X[8 rows][c]
            }
            if (want_db) accb = mfma_bf16(a, ones, accb);                    // every column: sum over the 16 pixels of the k-step
        }
    };

    // tile u's loads were issued PF steps before its products (registers: one set per tile in flight), one LDS buffer
    int u = chunk;
    if (u < g.units) fetch(u, stage[0]);
    if (PF == 2 && u + g.chunks < g.units) fetch(u + g.chunks, stage[PF - 1]);
    while (u < g.units) {
#pragma unroll
        for (int s_ = 0; s_ < PF; ++s_) {
            if (u >= g.units) break;
            __syncthreads();                                                 // the previous tile's LDS reads are done
            commit(stage[s_]);
            const int nu = u + PF * g.chunks;
            if (nu < g.units) fetch(nu, stage[s_]);                          // in flight during the next PF tiles' products
            __syncthreads();
            products();
            u += g.chunks;
        }
    }

    // ---- epilogue: acc[e] register r of lane l = D[n = (r & 3) + 8 (r >> 2) + 4 half][c = l & 31]
    const int c = c0 + csub * 32 + l31;
    float *pp = part + static_cast<int64_t>(chunk) * (static_cast<int64_t>(d.N) * TS * TS * d.C + (d.DB ? d.N : 0));
    if (want_db && l31 == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int n = n0 + nsub * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            if (n < d.N) pp[static_cast<int64_t>(d.N) * d.C + n] = accb[r];
        }
    }
#pragma unroll
    for (int e = 0; e < TS; ++e)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int n = n0 + nsub * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            if (n < d.N) pp[((static_cast<int64_t>(n) * TS + t) * TS + e) * d.C + c] = acc[e][r];
        }
}

template <int SI, int TS>
hipError_t launch(const void *x, const void *dy, float *part, WgradGeom g, hipStream_t st)
{
    constexpr int XC = SI == 1 ? kCols + TS - 1 : (TS == 3 ? 2 * kCols + 1 : kCols);
    constexpr size_t lds = (static_cast<size_t>(kNB) * kDyStride + static_cast<size_t>(kCB) * (XC | 1)) * 16;
    static_assert(lds <= 160 * 1024, "tile does not fit the LDS");
    auto kern = conv_wgrad_kernel<SI, TS>;
    static bool attr_set[64] = {};
    int dev_ = 0;
    if (hipGetDevice(&dev_) != hipSuccess) dev_ = -1;
    if (dev_ < 0 || dev_ >= 64 || !attr_set[dev_]) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 static_cast<int>(lds));
        if (e != hipSuccess) return e;
        if (dev_ >= 0 && dev_ < 64) attr_set[dev_] = true;
    }
    const int64_t blocks = static_cast<int64_t>(g.chunks) * TS * g.cblocks * g.nblocks;
    hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(blocks)), dim3(kThreadsG), lds, st, static_cast<const __bf16 *>(x),
                       static_cast<const __bf16 *>(dy), part, g);
    return hipGetLastError();
}

// ---- The fp32 form (mdetr_conv_wgrad_f32): x and dy fp32, 3 x 3 taps, stride 1.  A sibling kernel -- the bf16 kernel above has no
// run-time or compile-time flag for it.  The workgroup (tap row t, 128 n, 64 c, a chunk of 8 x 16 pixel tiles), the loading tasks,
// the buffer-resource loads, the single LDS buffer with the next tile's loads in flight and the partials' layout are the bf16
// kernel's.  What differs: a lane's 8 row x 8 channel block is 16 loads of 16 bytes (4 fp32 each); every piece is split once
// (split4, mdetr_split.h) into hi / mid / lo bf16 parts, each part's 8 x 8 block is transposed and stored into ITS plane of LDS --
// three planes of the bf16 kernel's row geometry (dYt 128 x 17 slots, Xt 64 x 19 slots: 3 x 54 272 = 162 816 bytes, one workgroup
// per CU) -- and a k-step reads the dY triple once and the X triple per tap column and issues the six terms
//   lo.hi  hi.lo  mid.mid  mid.hi  hi.mid  hi.hi        (dY part x X part, small ones first)
// into the ONE accumulator of that tap column.  What is dropped (mid.lo, lo.mid, lo.lo) is below 2^-24 of |dy||x| per product.
// An infinite operand yields NaN (x - bf16(x)), as in the other fp32 forms.  One tile in flight (64 staging registers).
constexpr int kCols32 = 16;                                                  // (independent of MDETR_CONV_WGRAD_COLS: three planes of 32 columns do not fit)
constexpr int kDyStride32 = kCols32 + 1, kXC32 = kCols32 + 2, kXStride32 = kXC32 | 1;
constexpr int kDyPlane32 = kNB * kDyStride32, kXPlane32 = kCB * kXStride32;  // 16-byte slots of one plane
constexpr size_t kLds32 = static_cast<size_t>(3) * (kDyPlane32 + kXPlane32) * 16;
static_assert(kLds32 == 162816 && kLds32 <= 160 * 1024, "three planes of the 128 x 64 tile: one workgroup per CU");

__global__ __launch_bounds__(kThreadsG)
void conv_wgrad_f32_kernel(const float *__restrict__ x, const float *__restrict__ dy, float *__restrict__ part, const WgradGeom g)
{
    constexpr int TS = 3;
    MDETR_DYNAMIC_LDS(unsigned char, wgrad32_smem);
    bf16x8 *dyt = reinterpret_cast<bf16x8 *>(wgrad32_smem);                  // [3 planes][kNB][kDyStride32]
    bf16x8 *xt = dyt + 3 * kDyPlane32;                                       // [3 planes][kCB][kXStride32]
    const ConvWgradDims &d = g.d;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, l31 = lane & 31;
    const int nsub = wave & 3, csub = wave >> 2;
    int id = blockIdx.x;
    const int chunk = id % g.chunks; id /= g.chunks;
    const int t = id % TS; id /= TS;                                         // tap row
    const int cblk = id % g.cblocks; const int nblk = id / g.cblocks;
    const int n0 = nblk * kNB, c0 = cblk * kCB;

    f32x16 acc[TS];
#pragma unroll
    for (int e = 0; e < TS; ++e)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[e][i] = 0.f;

    // ---- loading tasks: the bf16 kernel's (a wave = 16 columns x 4 pieces of 8 channels of one operand, lane = 16 piece + column),
    // one task per wave: waves 0 - 3 the 18 columns x 64 channels of the X window, waves 4 - 7 the 16 columns x 128 channels of dY
    constexpr int CGX = (kXC32 + 15) / 16;
    constexpr int WTASKS = 2 * CGX + 4 * (kCols32 / 16);
    static_assert(WTASKS == kThreadsG / 64, "one loading task per wave");
    bf16x8 stage[16];                                                        // 16 bytes = 4 fp32 each (the load moves bits): row i = stage[2 i], stage[2 i + 1]
    const mdetr_rsrc xr = make_rsrc(x, static_cast<unsigned>(static_cast<int64_t>(d.B) * d.H * d.W * d.C * 4));
    const mdetr_rsrc yr = make_rsrc(dy, static_cast<unsigned>(static_cast<int64_t>(d.B) * d.OH * d.OW * d.N * 4));
    const int ci = lane & 15, pi = lane >> 4;
    const bool is_x = wave < 2 * CGX;                                        // wave-uniform
    int t_rel, t_ch, t_dst;
    if (is_x) {
        const int slot = 16 * (wave >> 1) + ci, piece = 4 * (wave & 1) + pi;
        t_rel = slot >= kXC32 ? -1 : slot;
        t_ch = (c0 + piece * 8) * 4;
        t_dst = piece * 8 * kXStride32 + slot;
    } else {
        const int k = wave - 2 * CGX, col = 16 * (k >> 2) + ci, piece = 4 * (k & 3) + pi;
        t_rel = col;
        t_ch = n0 + piece * 8 < d.N ? (n0 + piece * 8) * 4 : -1;
        t_dst = piece * 8 * kDyStride32 + col;
    }
    auto fetch = [&](int u) {                                                // global loads of pixel tile u
        const int ct = u % g.ctiles; u /= g.ctiles;
        const int band = u % g.bands; const int b = u / g.bands;
        const int r0 = band * kRows, q0 = ct * kCols32;
        if (is_x) {
            const int col = q0 + t_rel - 1;
            const bool in = t_rel >= 0 && col >= 0 && col < d.W;
            const unsigned lane_off = in ? static_cast<unsigned>(col * d.C * 4 + t_ch) : 0u;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int row = r0 + i + t - 1;                              // uniform
                const bool ok = in && row >= 0 && row < d.H;
                const unsigned so = (row >= 0 && row < d.H) ? static_cast<unsigned>((b * d.H + row) * d.W) * static_cast<unsigned>(d.C * 4) : 0u;
                stage[2 * i] = rsrc_load_bf16x8(xr, ok ? lane_off : kRsrcOob, so);
                stage[2 * i + 1] = rsrc_load_bf16x8(xr, ok ? lane_off + 16u : kRsrcOob, so);
            }
        } else {
            const int col = q0 + t_rel;
            const bool in = col < d.OW && t_ch >= 0;
            const unsigned lane_off = in ? static_cast<unsigned>(col * d.N * 4 + t_ch) : 0u;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int row = r0 + i;
                const bool ok = in && row < d.OH;
                const unsigned so = row < d.OH ? static_cast<unsigned>((b * d.OH + row) * d.OW) * static_cast<unsigned>(d.N * 4) : 0u;
                stage[2 * i] = rsrc_load_bf16x8(yr, ok ? lane_off : kRsrcOob, so);
                stage[2 * i + 1] = rsrc_load_bf16x8(yr, ok ? lane_off + 16u : kRsrcOob, so);
            }
        }
    };
    auto commit = [&]() {                                                    // split once, transpose each part's block into its plane
        bf16x8 pl[3][8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                float f[4];
                __builtin_memcpy(f, &stage[2 * i + s], 16);
                bf16x4 h, m, l;
                split4(f, h, m, l);
#pragma unroll
                for (int j = 0; j < 4; ++j) { pl[0][i][4 * s + j] = h[j]; pl[1][i][4 * s + j] = m[j]; pl[2][i][4 * s + j] = l[j]; }
            }
        }
        if (is_x && t_rel < 0) return;                                       // (the window's 18 columns: lanes of the second group beyond it)
        bf16x8 *dst = is_x ? xt + t_dst : dyt + t_dst;
        const int stride = is_x ? kXStride32 : kDyStride32, plane = is_x ? kXPlane32 : kDyPlane32;
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            bf16x8 tr[8];
            transpose8x8(pl[p], tr);
#pragma unroll
            for (int q = 0; q < 8; ++q) dst[p * plane + q * stride] = tr[q];
        }
    };
    auto products = [&]() {
        const bf16x8 *ap = dyt + (nsub * 32 + l31) * kDyStride32 + half;
        const bf16x8 *bp = xt + (csub * 32 + l31) * kXStride32 + half;
        constexpr int term_y[6] = {2, 0, 1, 1, 0, 0}, term_x[6] = {0, 2, 1, 0, 1, 0};       // 0 hi, 1 mid, 2 lo
#pragma unroll 2
        for (int ks = 0; ks < kCols32 / 2; ++ks) {
            bf16x8 a[3], b[TS][3];                                           // this half-wave's column of the k-step: q = 2 ks + half
#pragma unroll
            for (int p = 0; p < 3; ++p) {
                a[p] = ap[p * kDyPlane32 + 2 * ks];
#pragma unroll
                for (int e = 0; e < TS; ++e) b[e][p] = bp[p * kXPlane32 + 2 * ks + e];
            }
#pragma unroll
            for (int k = 0; k < 6; ++k)                                      // term by term over the tap columns: every accumulator sees the order above
#pragma unroll
                for (int e = 0; e < TS; ++e) acc[e] = mfma_bf16(a[term_y[k]], b[e][term_x[k]], acc[e]);
        }
    };

    // tile u's loads were issued one step before its products; one LDS buffer
    int u = chunk;
    if (u < g.units) fetch(u);
    while (u < g.units) {
        __syncthreads();                                                     // the previous tile's LDS reads are done
        commit();
        const int nu = u + g.chunks;
        if (nu < g.units) fetch(nu);                                         // in flight during this tile's products
        __syncthreads();
        products();
        u = nu;
    }

    // ---- epilogue: the bf16 kernel's
    const int c = c0 + csub * 32 + l31;
    float *pp = part + static_cast<int64_t>(chunk) * (static_cast<int64_t>(d.N) * TS * TS * d.C);
#pragma unroll
    for (int e = 0; e < TS; ++e)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int n = n0 + nsub * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            if (n < d.N) pp[((static_cast<int64_t>(n) * TS + t) * TS + e) * d.C + c] = acc[e][r];
        }
}

hipError_t launch_f32(const void *x, const void *dy, float *part, WgradGeom g, hipStream_t st)
{
    auto kern = conv_wgrad_f32_kernel;
    static bool attr_set[64] = {};
    int dev_ = 0;
    if (hipGetDevice(&dev_) != hipSuccess) dev_ = -1;
    if (dev_ < 0 || dev_ >= 64 || !attr_set[dev_]) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 static_cast<int>(kLds32));
        if (e != hipSuccess) return e;
        if (dev_ >= 0 && dev_ < 64) attr_set[dev_] = true;
    }
    const int64_t blocks = static_cast<int64_t>(g.chunks) * 3 * g.cblocks * g.nblocks;
    hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(blocks)), dim3(kThreadsG), kLds32, st, static_cast<const float *>(x),
                       static_cast<const float *>(dy), part, g);
    return hipGetLastError();
}

// ---- The fp32 form at stride 2 (mdetr_conv_wgrad_s2_f32): x and dy fp32, 3 x 3 taps, stride 2, pad 1.  A sibling of conv_wgrad_f32_kernel --
// neither kernel above has a flag for it.  The arithmetic is that kernel's: split4 once per piece, transpose8x8 per part into the part's
// LDS plane, the six terms lo.hi hi.lo mid.mid mid.hi hi.mid hi.hi into the one accumulator of a tap column; buffer-resource loads (padding
// and ragged tiles read as zeros), one LDS buffer with the next tile's loads in flight, the partials' layout.  What differs is the tile:
// the X window of q output columns is 2 q + 1 column slots, stored de-interleaved (q + 1 even ones, then q odd ones) as in
// conv_wgrad_kernel<2, 3>, and three planes of the stride-1 geometry would take 3 x (128 x 17 + 64 x 33) x 16 = 205 824 bytes.  This
// kernel takes an 8-COLUMN pixel tile AND a 64-row n block:
//   dYt 64 n x 9 slots, Xt 64 c x 17 slots (9 even + 8 odd), three planes: 3 x (64 x 9 + 64 x 17) x 16 = 79 872 bytes
// -- half of the CU's 160 KB, so TWO workgroups of 4 waves share a CU and one's split / transpose (VALU, LDS stores) runs under the
// other's matrix instructions; either choice alone (107 520 / 153 600 bytes) leaves one workgroup per CU whose waves all wait at the
// same two barriers.  __launch_bounds__(256, 2) keeps the 256-register budget that two waves per SIMD need.
// Workgroup = 4 waves: (tap row t, 64 n, 64 c, a chunk of 8-row x 8-column pixel tiles); wave w owns n-block w & 1 and c-block w >> 1.
// A tile is 4 k-steps (2 columns x 8 rows).  Loading tasks, one per wave, lane = 8 piece + column: waves 0 - 2 the 17 window slots
// x 64 channels of X (the third wave's lanes beyond slot 16 load and store nothing), wave 3 the 8 columns x 64 channels of dY.  The 8
// lanes of a ds_write_b128 group store 8 CONSECUTIVE slots of one channel row (32 banks: conflict-free whatever the row stride); the
// rows are 9 and 17 slots apart -- odd -- so the 16 lanes of a ds_read_b128 group (16 distinct residues of l31 mod 16) fall on 16
// distinct slots of the 256-byte bank row.
constexpr int kThreadsS2 = 256;
constexpr int kNBS2 = 64, kColsS2 = 8;                                       // output channels per workgroup, columns of a pixel tile
constexpr int kDyStrideS2 = kColsS2 + 1, kXCS2 = 2 * kColsS2 + 1, kXStrideS2 = kXCS2 | 1, kEvenS2 = kColsS2 + 1;
constexpr int kDyPlaneS2 = kNBS2 * kDyStrideS2, kXPlaneS2 = kCB * kXStrideS2;            // 16-byte slots of one plane
constexpr size_t kLdsS2 = static_cast<size_t>(3) * (kDyPlaneS2 + kXPlaneS2) * 16;
static_assert(kLdsS2 == 79872 && 2 * kLdsS2 <= 160 * 1024, "three planes of the 64 x 64 tile, 8 columns: two workgroups per CU");
static_assert(kDyStrideS2 % 2 == 1 && kXStrideS2 % 2 == 1,"odd row strides: conflict-free operand reads");

__global__ __launch_bounds__(kThreadsS2, 2)
void conv_wgrad_s2_f32_kernel(const float *__restrict__ x, const float *__restrict__ dy, float *__restrict__ part, const WgradGeom g)
{
    constexpr int TS = 3;
    MDETR_DYNAMIC_LDS(unsigned char, wgrad_s2_smem);
    bf16x8 *dyt = reinterpret_cast<bf16x8 *>(wgrad_s2_smem);                 // [3 planes][kNBS2][kDyStrideS2]
    bf16x8 *xt = dyt + 3 * kDyPlaneS2;                                       // [3 planes][kCB][kXStrideS2]
    const ConvWgradDims &d = g.d;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, l31 = lane & 31;
    const int nsub = wave & 1, csub = wave >> 1;
    int id = blockIdx.x;
    const int chunk = id % g.chunks; id /= g.chunks;
    const int t = id % TS; id /= TS;                                         // tap row
    const int cblk = id % g.cblocks; const int nblk = id / g.cblocks;
    const int n0 = nblk * kNBS2, c0 = cblk * kCB;

    f32x16 acc[TS];
#pragma unroll
    for (int e = 0; e < TS; ++e)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[e][i] = 0.f;

    constexpr int CGX = (kXCS2 + 7) / 8;                                     // waves that load X: column groups of 8 slots
    static_assert(CGX + 1 == kThreadsS2 / 64, "one loading task per wave");
    bf16x8 stage[16];                                                        // 16 bytes = 4 fp32 each: row i = stage[2 i], stage[2 i + 1]
    const mdetr_rsrc xr = make_rsrc(x, static_cast<unsigned>(static_cast<int64_t>(d.B) * d.H * d.W * d.C * 4));
    const mdetr_rsrc yr = make_rsrc(dy, static_cast<unsigned>(static_cast<int64_t>(d.B) * d.OH * d.OW * d.N * 4));
    const int ci = lane & 7, pi = lane >> 3;
    const bool is_x = wave < CGX;                                            // wave-uniform
    int t_rel, t_ch, t_dst;
    if (is_x) {
        const int slot = 8 * wave + ci;                                      // slots [0, 9): window columns 0, 2, .. 16; [9, 17): 1, 3, .. 15
        t_rel = slot >= kXCS2 ? -1 : (slot < kEvenS2 ? 2 * slot : 2 * (slot - kEvenS2) + 1);
        t_ch = (c0 + pi * 8) * 4;
        t_dst = pi * 8 * kXStrideS2 + slot;
    } else {
        t_rel = ci;
        t_ch = n0 + pi * 8 < d.N ? (n0 + pi * 8) * 4 : -1;
        t_dst = pi * 8 * kDyStrideS2 + ci;
    }
    auto fetch = [&](int u) {                                                // global loads of pixel tile u
        const int ct = u % g.ctiles; u /= g.ctiles;
        const int band = u % g.bands; const int b = u / g.bands;
        const int r0 = band * kRows, q0 = ct * kColsS2;
        if (is_x) {
            const int col = 2 * q0 + t_rel - 1;
            const bool in = t_rel >= 0 && col >= 0 && col < d.W;
            const unsigned lane_off = in ? static_cast<unsigned>(col * d.C * 4 + t_ch) : 0u;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int row = 2 * (r0 + i) + t - 1;                        // uniform
                const bool ok = in && row >= 0 && row < d.H;
                const unsigned so = (row >= 0 && row < d.H) ? static_cast<unsigned>((b * d.H + row) * d.W) * static_cast<unsigned>(d.C * 4) : 0u;
                stage[2 * i] = rsrc_load_bf16x8(xr, ok ? lane_off : kRsrcOob, so);
                stage[2 * i + 1] = rsrc_load_bf16x8(xr, ok ? lane_off + 16u : kRsrcOob, so);
            }
        } else {
            const int col = q0 + t_rel;
            const bool in = col < d.OW && t_ch >= 0;
            const unsigned lane_off = in ? static_cast<unsigned>(col * d.N * 4 + t_ch) : 0u;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int row = r0 + i;
                const bool ok = in && row < d.OH;
                const unsigned so = row < d.OH ? static_cast<unsigned>((b * d.OH + row) * d.OW) * static_cast<unsigned>(d.N * 4) : 0u;
                stage[2 * i] = rsrc_load_bf16x8(yr, ok ? lane_off : kRsrcOob, so);
                stage[2 * i + 1] = rsrc_load_bf16x8(yr, ok ? lane_off + 16u : kRsrcOob, so);
            }
        }
    };
    auto commit = [&]() {                                                    // split once, transpose each part's block into its plane
        bf16x8 pl[3][8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                float f[4];
                __builtin_memcpy(f, &stage[2 * i + s], 16);
                bf16x4 h, m, l;
                split4(f, h, m, l);
#pragma unroll
                for (int j = 0; j < 4; ++j) { pl[0][i][4 * s + j] = h[j]; pl[1][i][4 * s + j] = m[j]; pl[2][i][4 * s + j] = l[j]; }
            }
        }
        if (is_x && t_rel < 0) return;                                       // (the window's 17 slots: lanes of the third group beyond them)
        bf16x8 *dst = is_x ? xt + t_dst : dyt + t_dst;
        const int stride = is_x ? kXStrideS2 : kDyStrideS2, plane = is_x ? kXPlaneS2 : kDyPlaneS2;
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            bf16x8 tr[8];
            transpose8x8(pl[p], tr);
#pragma unroll
            for (int q = 0; q < 8; ++q) dst[p * plane + q * stride] = tr[q];
        }
    };
    auto products = [&]() {
        const bf16x8 *ap = dyt + (nsub * 32 + l31) * kDyStrideS2 + half;
        const bf16x8 *bp = xt + (csub * 32 + l31) * kXStrideS2 + half;
        constexpr int term_y[6] = {2, 0, 1, 1, 0, 0}, term_x[6] = {0, 2, 1, 0, 1, 0};       // 0 hi, 1 mid, 2 lo
#pragma unroll 2
        for (int ks = 0; ks < kColsS2 / 2; ++ks) {
            bf16x8 a[3], b[TS][3];                                           // this half-wave's column of the k-step: q = 2 ks + half
#pragma unroll
            for (int p = 0; p < 3; ++p) {
                a[p] = ap[p * kDyPlaneS2 + 2 * ks];
#pragma unroll
                for (int e = 0; e < TS; ++e)                                 // window column 2 q + e: even -> slot q + e / 2, odd -> behind the even ones
                    b[e][p] = bp[p * kXPlaneS2 + 2 * ks + ((e & 1) ? kEvenS2 : (e >> 1))];
            }
#pragma unroll
            for (int k = 0; k < 6; ++k)                                      // term by term over the tap columns: every accumulator sees the order above
#pragma unroll
                for (int e = 0; e < TS; ++e) acc[e] = mfma_bf16(a[term_y[k]], b[e][term_x[k]], acc[e]);
        }
    };

    // tile u's loads were issued one step before its products; one LDS buffer
    int u = chunk;
    if (u < g.units) fetch(u);
    while (u < g.units) {
        __syncthreads();                                                     // the previous tile's LDS reads are done
        commit();
        const int nu = u + g.chunks;
        if (nu < g.units) fetch(nu);                                         // in flight during this tile's products
        __syncthreads();
        products();
        u = nu;
    }

    // ---- epilogue: the bf16 kernel's
    const int c = c0 + csub * 32 + l31;
    float *pp = part + static_cast<int64_t>(chunk) * (static_cast<int64_t>(d.N) * TS * TS * d.C);
#pragma unroll
    for (int e = 0; e < TS; ++e)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int n = n0 + nsub * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            if (n < d.N) pp[((static_cast<int64_t>(n) * TS + t) * TS + e) * d.C + c] = acc[e][r];
        }
}

hipError_t launch_s2_f32(const void *x, const void *dy, float *part, WgradGeom g, hipStream_t st)
{
    auto kern = conv_wgrad_s2_f32_kernel;
    static bool attr_set[64] = {};
    int dev_ = 0;
    if (hipGetDevice(&dev_) != hipSuccess) dev_ = -1;
    if (dev_ < 0 || dev_ >= 64 || !attr_set[dev_]) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 static_cast<int>(kLdsS2));
        if (e != hipSuccess) return e;
        if (dev_ >= 0 && dev_ < 64) attr_set[dev_] = true;
    }
    const int64_t blocks = static_cast<int64_t>(g.chunks) * 3 * g.cblocks * g.nblocks;
    hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(blocks)), dim3(kThreadsS2), kLdsS2, st, static_cast<const float *>(x),
                       static_cast<const float *>(dy), part, g);
    return hipGetLastError();
}

// cols x nb: the pixel tile's columns and the n block of the kernel served; target: the workgroups to aim for without the tune key
WgradGeom geometry(const ConvWgradDims &d, int cols = kCols, int nb = kNB, int target = 256)
{
    WgradGeom g;
    g.d = d;
    g.bands = (d.OH + kRows - 1) / kRows;
    g.ctiles = (d.OW + cols - 1) / cols;
    g.units = d.B * g.bands * g.ctiles;
    g.nblocks = (d.N + nb - 1) / nb;
    g.cblocks = d.C / kCB;
    // one workgroup per CU (104-134 KB of LDS): about 256 workgroups, each with at least one pixel tile (the fp32 stride-2 form: two
    // per CU, about 512)
    const int base = d.K * g.nblocks * g.cblocks;
    char tune_buf[16];
    if (const char *ev = tune_str("conv_wgrad_wgs", tune_buf, sizeof(tune_buf))) {                    // A/B runs: workgroups to aim for
        const int f = atoi(ev);
        if (f >= 64 && f <= 8192) target = f;
    }
    int chunks = target / (base > 0 ? base : 1);
    if (chunks < 1) chunks = 1;
    if (chunks > g.units) chunks = g.units;
    g.chunks = chunks;
    return g;
}

}  // namespace

bool conv_wgrad_supported(const ConvWgradDims &d, const void *x, const void *dy)
{
    const auto al = [](const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; };
    // (K = 1 / stride 1: the weight gradient of a token-wise linear layer, its [T, C] / [T, N] matrices viewed as a 1 x 8 x T / 8 image)
    const bool shape = (d.K == 3 && (d.SI == 1 || d.SI == 2)) || (d.K == 1 && (d.SI == 2 || d.SI == 1));
    return shape && d.B > 0 && d.H > 0 && d.W > 0 && d.OH > 0 && d.OW > 0 && d.C > 0 && d.C % 64 == 0 && d.N > 0 && d.N % 32 == 0 &&
           al(x, 16) && al(dy, 16) && static_cast<int64_t>(d.N) * d.K * d.K * d.C < (1ll << 28) &&
           static_cast<int64_t>(d.B) * d.H * d.W * d.C < (1ll << 30) && static_cast<int64_t>(d.B) * d.OH * d.OW * d.N < (1ll << 30);
}

int conv_wgrad_chunks(const ConvWgradDims &d) { return geometry(d).chunks; }

hipError_t conv_wgrad_launch(const void *x, const void *dy, float *part, const ConvWgradDims &d, hipStream_t st)
{
    const WgradGeom g = geometry(d);
    ProfileScope prof(d.K == 1 && d.SI == 1 ? 11 : 9, conv_mflop(static_cast<int64_t>(d.B) * d.OH * d.OW, static_cast<int64_t>(d.C) * d.N * d.K * d.K), st,
                      2.0 * d.B * d.OH * d.OW * d.C * d.N * d.K * d.K / 1e6,
                      (2.0 * d.B * (static_cast<double>(d.H) * d.W * d.C + static_cast<double>(d.OH) * d.OW * d.N) + 4.0 * g.chunks * d.K * d.K * d.N * d.C) / 1e3);
    if (d.K == 3) return d.SI == 1 ? launch<1, 3>(x, dy, part, g, st) : launch<2, 3>(x, dy, part, g, st);
    return d.SI == 1 ? launch<1, 1>(x, dy, part, g, st) : launch<2, 1>(x, dy, part, g, st);
}

bool conv_wgrad_f32_supported(const ConvWgradDims &d, const void *x, const void *dy)
{
    const auto al = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    // (fp32 elements: 2^29 of them are 2^31 bytes -- the 32-bit byte offsets of the buffer-resource loads)
    return d.K == 3 && d.SI == 1 && d.DB == 0 && d.B > 0 && d.H > 0 && d.W > 0 && d.OH == d.H && d.OW == d.W && d.C > 0 && d.C % 64 == 0 &&
           d.N > 0 && d.N % 32 == 0 && al(x) && al(dy) && static_cast<int64_t>(d.N) * 9 * d.C < (1ll << 28) &&
           static_cast<int64_t>(d.B) * d.H * d.W * d.C < (1ll << 29) && static_cast<int64_t>(d.B) * d.H * d.W * d.N < (1ll << 29);
}

int conv_wgrad_f32_chunks(const ConvWgradDims &d) { return geometry(d, kCols32).chunks; }

hipError_t conv_wgrad_f32_launch(const void *x, const void *dy, float *part, const ConvWgradDims &d, hipStream_t st)
{
    const WgradGeom g = geometry(d, kCols32);
    ProfileScope prof(9, conv_mflop(static_cast<int64_t>(d.B) * d.OH * d.OW, static_cast<int64_t>(d.C) * d.N * 9), st,
                      2.0 * d.B * d.OH * d.OW * d.C * d.N * 9 / 1e6,
                      (4.0 * d.B * (static_cast<double>(d.H) * d.W * d.C + static_cast<double>(d.OH) * d.OW * d.N) + 4.0 * g.chunks * 9 * d.N * d.C) / 1e3);
    return launch_f32(x, dy, part, g, st);
}

bool conv_wgrad_s2_f32_supported(const ConvWgradDims &d, const void *x, const void *dy)
{
    const auto al = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    // (sizes first: nothing below is evaluated on a problem whose 32-bit byte offsets would wrap)
    return d.K == 3 && d.SI == 2 && d.DB == 0 && d.B > 0 && d.H > 0 && d.W > 0 && d.OH == (d.H - 1) / 2 + 1 && d.OW == (d.W - 1) / 2 + 1 &&
           d.C > 0 && d.C % 64 == 0 && d.N > 0 && d.N % 32 == 0 && al(x) && al(dy) && static_cast<int64_t>(d.N) * 9 * d.C < (1ll << 28) &&
           static_cast<int64_t>(d.B) * d.H * d.W * d.C < (1ll << 29) && static_cast<int64_t>(d.B) * d.OH * d.OW * d.N < (1ll << 29);
}

// (two workgroups per CU: 512 to aim for)
int conv_wgrad_s2_f32_chunks(const ConvWgradDims &d) { return geometry(d, kColsS2, kNBS2, 512).chunks; }

hipError_t conv_wgrad_s2_f32_launch(const void *x, const void *dy, float *part, const ConvWgradDims &d, hipStream_t st)
{
    const WgradGeom g = geometry(d, kColsS2, kNBS2, 512);
    ProfileScope prof(9, conv_mflop(static_cast<int64_t>(d.B) * d.OH * d.OW, static_cast<int64_t>(d.C) * d.N * 9), st,
                      2.0 * d.B * d.OH * d.OW * d.C * d.N * 9 / 1e6,
                      (4.0 * d.B * (static_cast<double>(d.H) * d.W * d.C + static_cast<double>(d.OH) * d.OW * d.N) + 4.0 * g.chunks * 9 * d.N * d.C) / 1e3);
    return launch_s2_f32(x, dy, part, g, st);
}

}  // namespace mdetr
