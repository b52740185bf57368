// monodetr_amd/csrc/msda.h -- internal launcher declarations (see msda.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>

namespace mdetr {

// Element types of `value` / `out` / `grad_out` on the fast path: float, or bf16 for a bf16 model body
// (rows of 32 channels = 64 bytes, a lane's 4 channels = one 8-byte access; arithmetic stays fp32).
template <typename E> struct Elem;
template <> struct Elem<float> {
    static constexpr int kBytes = 4;
    typedef float4 Raw;                                   // 4 channels as loaded; widen() when consumed (keeps batches of loads compact)
    static __device__ __forceinline__ Raw loadr(const char *p) { return *reinterpret_cast<const float4 *>(p); }
    static __device__ __forceinline__ float4 widen(const Raw &r) { return r; }
    static __device__ __forceinline__ float load1(const float *p) { return *p; }
    static __device__ __forceinline__ float4 load4(const char *p) { return *reinterpret_cast<const float4 *>(p); }
    static __device__ __forceinline__ void store4(char *p, const float4 &v) { *reinterpret_cast<float4 *>(p) = v; }
};
template <> struct Elem<__hip_bfloat16> {
    static constexpr int kBytes = 2;
    typedef uint2 Raw;
    static __device__ __forceinline__ Raw loadr(const char *p) { return *reinterpret_cast<const uint2 *>(p); }
    static __device__ __forceinline__ float4 widen(const Raw &u)
    {
        return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xFFFF0000u),
                           __uint_as_float(u.y << 16), __uint_as_float(u.y & 0xFFFF0000u));
    }
    static __device__ __forceinline__ float load1(const __hip_bfloat16 *p) { return __bfloat162float(*p); }
    static __device__ __forceinline__ float4 load4(const char *p)
    {
        const uint2 u = *reinterpret_cast<const uint2 *>(p);                    // bf16 -> fp32 is a 16-bit shift
        return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xFFFF0000u),
                           __uint_as_float(u.y << 16), __uint_as_float(u.y & 0xFFFF0000u));
    }
    static __device__ __forceinline__ void store4(char *p, const float4 &v)
    {
        __hip_bfloat16 h[4] = {__float2bfloat16(v.x), __float2bfloat16(v.y), __float2bfloat16(v.z), __float2bfloat16(v.w)};
        *reinterpret_cast<uint2 *>(p) = *reinterpret_cast<const uint2 *>(h);
    }
};

// dtype: 0 = f32, 1 = f64 (MDETR_F32 / MDETR_F64 of include/monodetr_amd.h)
bool msda_fast_path(int dtype, int D, int L, int P);

hipError_t msda_forward_launch(int dtype, const void *value, const int64_t *shapes, const int64_t *lstart,
                               const void *loc, const void *attn, void *out,
                               int B, int S, int M, int D, int L, int Lq, int P, hipStream_t st);

hipError_t msda_backward_launch(int dtype, const void *value, const int64_t *shapes, const int64_t *lstart,
                                const void *loc, const void *attn, const void *grad_out,
                                void *grad_value, void *grad_loc, void *grad_attn,
                                int B, int S, int M, int D, int L, int Lq, int P, hipStream_t st);

// Extended backward: with host copies of the level geometry and a workspace, the self-attention
// (Lq == S) fp32 D == 32 case takes the tile-privatised grad_value path of msda_tiled.hip.
hipError_t msda_backward_launch_ex(int dtype, const void *value, const int64_t *shapes, const int64_t *lstart,
                                   const void *loc, const void *attn, const void *grad_out,
                                   void *grad_value, void *grad_loc, void *grad_attn,
                                   int B, int S, int M, int D, int L, int Lq, int P,
                                   const int64_t *shapes_host, const int64_t *lstart_host,
                                   void *workspace, int64_t workspace_bytes, hipStream_t st);

// Mixed-precision operator for a bf16 model body: `value`, `out` and `grad_out` in bf16, sampling locations,
// attention weights and every gradient output in fp32 (fp32 accumulation throughout).  D = 32, L = P = 4 only;
// other shapes return hipErrorNotSupported (the caller widens to fp32 and takes the ordinary path).
hipError_t msda_forward_bf16_launch(const void *value, const int64_t *shapes, const int64_t *lstart,
                                    const float *loc, const float *attn, void *out,
                                    int B, int S, int M, int D, int L, int Lq, int P, hipStream_t st);
hipError_t msda_backward_bf16_launch(const void *value, const int64_t *shapes, const int64_t *lstart,
                                     const float *loc, const float *attn, const void *grad_out,
                                     float *grad_value, float *grad_loc, float *grad_attn,
                                     int B, int S, int M, int D, int L, int Lq, int P,
                                     const int64_t *shapes_host, const int64_t *lstart_host,
                                     void *workspace, int64_t workspace_bytes, hipStream_t st);

int64_t msda_tiled_workspace_bytes(const int64_t *shapes_h, const int64_t *start_h, int B, int S, int M, int D, int L, int Lq, int P);

hipError_t msda_tiled_grad_value_launch(const int64_t *shapes_h, const int64_t *start_h,
                                        const float *loc, const float *attn, const void *grad_out, float *grad_value,
                                        void *workspace, int64_t workspace_bytes,
                                        int B, int S, int M, int D, int L, int Lq, int P, bool absmax_ready, hipStream_t st,
                                        int grad_out_dtype = 0 /* 0 = f32, 2 = bf16 (needs absmax_ready) */);

// msda_fused.hip: the whole backward (all three gradients) in one pass, self-attention over the pyramid or cross-attention
// with few queries; D = 32.  elem_dtype 0: value / grad_out fp32, 2: bf16.  Writes every output completely.
int64_t msda_fused_workspace_bytes(const int64_t *shapes_h, const int64_t *start_h, int B, int S, int M, int D, int L, int Lq, int P);
hipError_t msda_backward_fused_launch(const int64_t *shapes_h, const int64_t *start_h, const void *value, const float *loc,
                                      const float *attn, const void *grad_out, void *grad_value, float *grad_loc, float *grad_attn,
                                      void *workspace, int64_t workspace_bytes, int B, int S, int M, int D, int L, int Lq, int P,
                                      int elem_dtype, hipStream_t st, int gv_dtype = 0 /* grad_value alone: 0 = f32, 2 = bf16 */);
// The one-pass backward with grad_value written as gv_dtype (0 = f32, 2 = bf16) -- the type its consumer reads -- for fp32
// (elem_dtype 0) or bf16 (2) value / grad_out.  No other strategy writes bf16: hipErrorNotSupported where the geometry does not
// qualify, and nothing has been written then.
hipError_t msda_backward_to_launch(int elem_dtype, int gv_dtype, const void *value, const float *loc, const float *attn,
                                   const void *grad_out, void *grad_value, float *grad_loc, float *grad_attn,
                                   int B, int S, int M, int D, int L, int Lq, int P,
                                   const int64_t *shapes_host, const int64_t *lstart_host,
                                   void *workspace, int64_t workspace_bytes, hipStream_t st);

// msda_cpu.hip: host implementation (every pointer a HOST pointer); dtype 0 = f32, 1 = f64
void msda_forward_cpu(int dtype, const void *value, const int64_t *shapes, const int64_t *lstart, const void *loc,
                      const void *attn, void *out, int B, int S, int M, int D, int L, int Lq, int P);
void msda_backward_cpu(int dtype, const void *value, const int64_t *shapes, const int64_t *lstart, const void *loc,
                       const void *attn, const void *grad_out, void *grad_value, void *grad_loc, void *grad_attn,
                       int B, int S, int M, int D, int L, int Lq, int P);

hipError_t msda_indices_launch(int dtype, const int64_t *shapes, const void *loc, int32_t *idx,
                               int B, int M, int L, int Lq, int P, hipStream_t st);

// Zero `bytes` bytes at p with a store kernel.  Used instead of hipMemsetAsync: inside a captured
// hipGraph the memset NODE of a large, freshly mapped buffer was observed to leave stale data after
// the process mapped more device memory between replays (gradients of the first MSDA backward of a
// replay came back ~1e9); kernel nodes are not affected.
hipError_t zero_fill_launch(void *p, int64_t bytes, hipStream_t st);

// event-pair profiling of kernel launches (capi.hip owns the storage)
void profile_begin(int kind, int Lq, hipStream_t st);
void profile_end(hipStream_t st);
// one event pair around the launches of a scope.  kind 9 = a hand-written convolution, key = its MFLOP (2 x MACs / 1e6): what
// bench.py's `mfma` object sums into TFLOP/s against the dense bf16 MFMA peak
// ... and the useful work of the launches inside the scope (MFLOP, algorithmic KB): what bench.py's `families` divide by the
// families' kernel times.  kinds: 10 token GEMM, 11 token weight gradient, 12 column sum, 13 residual LayerNorm, 14 bias / activation
// tails, 15 GroupNorm, 16 small-T weight gradient, 17 MSDA prologue, 18 AdamW, 19 gathers / pooling, 20 frozen-BN weight fold
void profile_work(double mflop, double kbytes);
struct ProfileScope {
    hipStream_t s;
    ProfileScope(int kind, int64_t key, hipStream_t st) : s(st) { profile_begin(kind, static_cast<int>(key > 0x7fffffff ? 0x7fffffff : key), st); }
    ProfileScope(int kind, int64_t key, hipStream_t st, double mflop, double kbytes) : s(st)
    {
        profile_begin(kind, static_cast<int>(key > 0x7fffffff ? 0x7fffffff : key), st);
        profile_work(mflop, kbytes);
    }
    ~ProfileScope() { profile_end(s); }
};
inline int64_t conv_mflop(int64_t out_pixels, int64_t macs_per_pixel) { return (2 * out_pixels * macs_per_pixel + 500000) / 1000000; }

}  // namespace mdetr
