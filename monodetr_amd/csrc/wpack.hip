// monodetr_amd/csrc/wpack.hip -- the transformer's packed and summed projection parameters in ONE launch per forward pass, and the
// encoder's level positions in one more.
//
// NOT a translation unit of its own: capi.hip includes this file (monodetr_amd/build.py leaves it out of its source list), so every
// build of the C ABI -- the device library and the host emulation of the tests, which compiles a fixed list of files -- has it.
//
// The reference runs one GEMM per projection (lib/models/monodetr/ops/modules/ms_deform_attn.py:138-141: sampling_offsets and
// attention_weights; depthaware_transformer.py:467-474: sa_qcontent / sa_qpos / sa_kcontent / sa_kpos).  This repository packs the
// projections of one input into one GEMM: [W_offsets; W_weights] (384 rows) in six modules, [Wqc + Wqp; Wkc + Wkp] (512 rows) in
// three decoder layers, and the biases alike.  Built with framework calls that is 2 `cat` per module and 4 `add` + 2 `cat` per
// layer, 30 launches of ~5 us per forward pass for 1.4 M elements -- every one of them fill and drain.  Here a row block of a
// packed tensor is one JOB:
//     dst[e] = src0[e]                                        (src1 == NULL: what `cat` copies)
//     dst[e] = T(float(src0[e]) + float(src1[e]))             (one rounding: what aten::add computes for bf16 and fp32)
// and one launch runs up to kPackJobs of them, bf16 and fp32 mixed.  Job descriptors travel as kernel arguments (the packed
// tensors are new allocations every iteration; a captured graph bakes the addresses into its node), a host-built table gives each
// job's first workgroup.  A workgroup owns 256 16-byte pieces of its job's destination: the destination is cut at ITS 16-byte
// boundaries, so a bias block that starts at element 81 of a packed tensor has a scalar head, aligned vector stores and a scalar
// tail; sources that do not share the destination's alignment are read element by element.  Nothing is assumed about `elements`.
//
// level_pos_kernel: out[s][c] = T(sine[s][c] + embed[level of s][c]) -- the encoder's position tensor
// cat_l(flatten(pos_l) + level_embed[l]).to(dtype) (reference depthaware_transformer.py:215-218) for ONE image; with the cached sine
// encoding of an unpadded batch every image has the same one.  The arithmetic is the framework expression's: the sum in fp32,
// rounded to bf16 where BOTH operands are bf16 (the type the framework's add produces), then converted to T.  A thread owns 8
// channels of one token.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mdetr_wave.h>

#include "wpack.h"

namespace mdetr {
namespace {

constexpr int kPackThreads = 256;

struct PackJob {
    void *dst;
    const void *src0, *src1;
    int64_t elements;
    int bf16, block0;
};
struct PackArgs {
    PackJob j[kPackJobs];
    int njobs, pad_;
};

template <typename T> struct PackVec;
template <> struct PackVec<__bf16> { typedef bf16x8 type; };
template <> struct PackVec<float> { typedef f32x4 type; };

__device__ __forceinline__ float pack_sum(float a, float b) { return a + b; }
__device__ __forceinline__ __bf16 pack_sum(__bf16 a, __bf16 b) { return static_cast<__bf16>(static_cast<float>(a) + static_cast<float>(b)); }

__device__ __forceinline__ bf16x8 pack_gather(const __bf16 *p)
{
    bf16x8 v;
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = p[k];
    return v;
}
__device__ __forceinline__ f32x4 pack_gather(const float *p)
{
    f32x4 v;
    v.x = p[0]; v.y = p[1]; v.z = p[2]; v.w = p[3];
    return v;
}
__device__ __forceinline__ bf16x8 pack_sum(bf16x8 a, bf16x8 b)
{
    bf16x8 v;
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = pack_sum(a[k], b[k]);
    return v;
}
__device__ __forceinline__ f32x4 pack_sum(f32x4 a, f32x4 b)
{
    f32x4 v;
    v.x = a.x + b.x; v.y = a.y + b.y; v.z = a.z + b.z; v.w = a.w + b.w;
    return v;
}

// elements of `dst` before its first 16-byte boundary (the pointer is aligned to its element: pack_params_check)
__host__ __device__ inline int64_t pack_head(const void *dst, int64_t elements, int esize)
{
    const int64_t head = static_cast<int64_t>((16u - (reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u) / esize;
    return head < elements ? head : elements;
}

// workgroup `r` of a job: pieces [256 r, 256 r + 256) of the aligned body; workgroup 0 also the head and the tail
template <typename T>
__device__ __forceinline__ void pack_job(const PackJob &J, int r)
{
    typedef typename PackVec<T>::type V;
    constexpr int N = 16 / static_cast<int>(sizeof(T));
    T *dst = static_cast<T *>(J.dst);
    const T *s0 = static_cast<const T *>(J.src0), *s1 = static_cast<const T *>(J.src1);
    const int64_t n = J.elements, head = pack_head(dst, n, sizeof(T)), nvec = (n - head) / N, tail = head + nvec * N;
    const int t = threadIdx.x;
    if (r == 0) {                                                // (uniform) at most N - 1 elements on either side
        int64_t e = -1;
        if (t < head) e = t;
        else if (t >= 32 && tail + (t - 32) < n) e = tail + (t - 32);
        if (e >= 0) dst[e] = s1 ? pack_sum(s0[e], s1[e]) : s0[e];
    }
    const int64_t v = static_cast<int64_t>(r) * kPackThreads + t;
    if (v >= nvec) return;
    const int64_t e = head + v * N;
    // (uniform per job) a source with the destination's alignment is read in 16-byte pieces as well
    const bool vec0 = (reinterpret_cast<uintptr_t>(s0 + head) & 15u) == 0;
    V a = vec0 ? *reinterpret_cast<const V *>(s0 + e) : pack_gather(s0 + e);
    if (s1) {
        const bool vec1 = (reinterpret_cast<uintptr_t>(s1 + head) & 15u) == 0;
        a = pack_sum(a, vec1 ? *reinterpret_cast<const V *>(s1 + e) : pack_gather(s1 + e));
    }
    *reinterpret_cast<V *>(dst + e) = a;
}

__global__ __launch_bounds__(kPackThreads)
void pack_params_kernel(const PackArgs a)
{
    const int b = static_cast<int>(blockIdx.x);
    int i = 0;
    while (i + 1 < a.njobs && b >= a.j[i + 1].block0) ++i;       // (uniform: a scalar loop over <= 48 entries; empty jobs own no workgroup)
    const PackJob J = a.j[i];
    if (J.bf16) pack_job<__bf16>(J, b - J.block0);
    else pack_job<float>(J, b - J.block0);
}

inline int64_t pack_job_blocks(const mdetr_pack_job &q)
{
    if (q.elements <= 0) return 0;
    const int esize = q.dtype == MDETR_BF16 ? 2 : 4;
    const int64_t nvec = (q.elements - pack_head(q.dst, q.elements, esize)) / (16 / esize);
    const int64_t blocks = (nvec + kPackThreads - 1) / kPackThreads;
    return blocks > 0 ? blocks : 1;                              // head and tail alone still need their workgroup
}

struct PosArgs {
    const void *sine, *embed;
    void *out;
    int64_t start[kPosLevels + 1];                               // first token of each level; start[levels] = S
    int levels, C, sine_bf16, embed_bf16, out_bf16;
};

__global__ __launch_bounds__(kPackThreads)
void level_pos_kernel(const PosArgs a)
{
    const int pieces = a.C / 8;
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kPackThreads + threadIdx.x;
    if (i >= a.start[a.levels] * pieces) return;
    const int64_t s = i / pieces;
    const int c = static_cast<int>(i - s * pieces) * 8;
    int l = 0;
    while (l + 1 < a.levels && s >= a.start[l + 1]) ++l;
    const int64_t ooff = s * a.C + c;
    float v[8];
    if (a.sine_bf16) {
        const bf16x8 p = *reinterpret_cast<const bf16x8 *>(static_cast<const __bf16 *>(a.sine) + ooff);
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = static_cast<float>(p[k]);
    } else {
        const float *p = static_cast<const float *>(a.sine) + ooff;
        const f32x4 lo = *reinterpret_cast<const f32x4 *>(p), hi = *reinterpret_cast<const f32x4 *>(p + 4);
        v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w; v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
    }
    const int64_t eoff = static_cast<int64_t>(l) * a.C + c;
    if (a.embed_bf16) {
        const bf16x8 e = *reinterpret_cast<const bf16x8 *>(static_cast<const __bf16 *>(a.embed) + eoff);
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] += static_cast<float>(e[k]);
    } else {
        const float *q = static_cast<const float *>(a.embed) + eoff;
        const f32x4 e0 = *reinterpret_cast<const f32x4 *>(q), e1 = *reinterpret_cast<const f32x4 *>(q + 4);
        v[0] += e0.x; v[1] += e0.y; v[2] += e0.z; v[3] += e0.w; v[4] += e1.x; v[5] += e1.y; v[6] += e1.z; v[7] += e1.w;
    }
    if (a.sine_bf16 && a.embed_bf16) {                           // (uniform) the framework's add of two bf16 tensors is a bf16 tensor
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = static_cast<float>(static_cast<__bf16>(v[k]));
    }
    if (a.out_bf16) {
        bf16x8 o;
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = static_cast<__bf16>(v[k]);
        *reinterpret_cast<bf16x8 *>(static_cast<__bf16 *>(a.out) + ooff) = o;
    } else {
        f32x4 o0, o1;
        o0.x = v[0]; o0.y = v[1]; o0.z = v[2]; o0.w = v[3]; o1.x = v[4]; o1.y = v[5]; o1.z = v[6]; o1.w = v[7];
        float *o = static_cast<float *>(a.out) + ooff;
        *reinterpret_cast<f32x4 *>(o) = o0;
        *reinterpret_cast<f32x4 *>(o + 4) = o1;
    }
}

}  // namespace

const char *pack_params_check(const mdetr_pack_job *jobs, int njobs)
{
    if (!jobs || njobs <= 0) return "no jobs";
    for (int i = 0; i < njobs; ++i) {
        const mdetr_pack_job &q = jobs[i];
        if (q.dtype != MDETR_F32 && q.dtype != MDETR_BF16) return "dtype must be MDETR_F32 or MDETR_BF16";
        if (q.elements < 0) return "negative element count";
        if (q.elements == 0) continue;
        if (!q.dst || !q.src0) return "null pointer";
        const uintptr_t mask = q.dtype == MDETR_BF16 ? 1 : 3;
        if ((reinterpret_cast<uintptr_t>(q.dst) & mask) || (reinterpret_cast<uintptr_t>(q.src0) & mask) || (reinterpret_cast<uintptr_t>(q.src1) & mask))
            return "pointer not aligned to its element";
        if (pack_job_blocks(q) > (1 << 24)) return "job too long";
    }
    return nullptr;
}

hipError_t pack_params_launch(const mdetr_pack_job *jobs, int njobs, hipStream_t st)
{
    for (int first = 0; first < njobs; first += kPackJobs) {
        PackArgs a;
        const int n = njobs - first < kPackJobs ? njobs - first : kPackJobs;
        int blocks = 0;
        for (int i = 0; i < kPackJobs; ++i) {
            PackJob &J = a.j[i];
            if (i < n) {
                const mdetr_pack_job &q = jobs[first + i];
                J.dst = q.dst; J.src0 = q.src0; J.src1 = q.src1; J.elements = q.elements; J.bf16 = q.dtype == MDETR_BF16; J.block0 = blocks;
                blocks += static_cast<int>(pack_job_blocks(q));
            } else {
                J.dst = nullptr; J.src0 = J.src1 = nullptr; J.elements = 0; J.bf16 = 0; J.block0 = blocks;
            }
        }
        a.njobs = n; a.pad_ = 0;
        if (blocks == 0) continue;
        hipLaunchKernelGGL(pack_params_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kPackThreads), 0, st, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t level_pos_launch(const void *sine, bool sine_bf16, const void *embed, bool embed_bf16, void *out, bool out_bf16, const int64_t *counts,
                            int levels, int C, hipStream_t st)
{
    PosArgs a;
    a.sine = sine; a.embed = embed; a.out = out;
    a.levels = levels; a.C = C; a.sine_bf16 = sine_bf16; a.embed_bf16 = embed_bf16; a.out_bf16 = out_bf16;
    int64_t s = 0;
    for (int l = 0; l <= kPosLevels; ++l) {
        a.start[l] = s;
        if (l < levels) s += counts[l];
    }
    const int64_t blocks = (s * (C / 8) + kPackThreads - 1) / kPackThreads;
    if (blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(level_pos_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kPackThreads), 0, st, a);
    return hipGetLastError();
}

}  // namespace mdetr
