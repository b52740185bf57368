// monodetr_amd/csrc/detect.hip -- head outputs -> finished KITTI detections in ONE launch: the top-k (query, class) selection of
// extract_dets_from_outputs and the per-detection arithmetic of decode_detections (helpers/decode_helper.py; the reference's
// lib/helpers/decode_helper.py:8-110 runs the second half in a Python loop on the host).
//
// NOT a translation unit of its own: capi.hip includes this file (monodetr_amd/build.py leaves it out of its source list), so every
// build of the C ABI -- the device library and the host emulation of the tests, which compiles a fixed list of files -- has it.
//
// One workgroup per image, two steps.
//   Selection.  The image's n = Q C logits become 64-bit keys (detect_math.h: order word of the logit high, complemented flat index
//     low) in LDS, padded with 0 -- below every real key -- to the next power of two N, and a bitonic network sorts them descending:
//     log2 N (log2 N + 1) / 2 compare-exchange passes of N / 2 pairs, a barrier after each.  The keys are distinct, so the result
//     does not depend on the network: NaN first, then descending logit with -0 == +0, equal logits by ascending flat index -- what
//     torch.topk(sigmoid(logits)) returns wherever that is well defined, and what a stable descending sort of the logits returns
//     everywhere.
//   Decode.  Thread j < topk turns rank j into its result row, keep flag and (if asked) 37-float record: detect_decode_one.
// Latency-bound by construction: a batch is a handful of workgroups over a few kilobytes each; the passes (36 for the configured
// 150 keys, 91 at the 8 192-key limit) are what a launch costs.  Plain vector loads and stores, no atomics, no scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "detect.h"
#include "detect_math.h"

namespace mdetr {
namespace {

constexpr int kDetectThreads = 1024;

__device__ __forceinline__ void detect_rank(const DetectArgs &a, int b, int j, uint32_t flat)
{
    const int q = static_cast<int>(flat) / a.C, label = static_cast<int>(flat) - q * a.C;
    const int64_t bq = static_cast<int64_t>(b) * a.Q + q, out = static_cast<int64_t>(b) * a.topk + j;
    const bool keep = detect_decode_one(a.logits[bq * a.C + label], label, a.boxes + bq * 6, a.angle + bq * 24, a.dim + bq * 3, a.depth + bq * 2,
                                        a.calib + b * 6, a.size + b * 2, a.mean, a.threshold, a.recs ? a.recs + out * kDetectRecord : nullptr,
                                        a.rows + out * kDetectRow);
    a.keep[out] = keep ? 1 : 0;
}

__global__ __launch_bounds__(kDetectThreads)
void detect_decode_kernel(const DetectArgs a, const int N)
{
    __shared__ unsigned long long keys[kDetectMaxKeys];
    const int b = static_cast<int>(blockIdx.x), t = static_cast<int>(threadIdx.x), T = static_cast<int>(blockDim.x);
    const int n = a.Q * a.C;
    const float *lg = a.logits + static_cast<int64_t>(b) * n;
    for (int i = t; i < N; i += T) keys[i] = i < n ? detect_key(lg[i], static_cast<uint32_t>(i)) : 0ull;
    __syncthreads();
    for (int k = 2; k <= N; k <<= 1) {                           // (uniform) runs of k: descending where bit k of the position is clear
        for (int s = k >> 1; s > 0; s >>= 1) {
            for (int p = t; p < (N >> 1); p += T) {
                const int i = ((p & ~(s - 1)) << 1) | (p & (s - 1)), l = i | s;      // pair p of this pass: positions i < l, s apart
                const unsigned long long x = keys[i], y = keys[l];
                if ((i & k) == 0 ? x < y : x > y) { keys[i] = y; keys[l] = x; }
            }
            __syncthreads();
        }
    }
    for (int j = t; j < a.topk; j += T) detect_rank(a, b, j, detect_key_index(keys[j]));
}

}  // namespace

hipError_t detect_decode_launch(const DetectArgs &a, hipStream_t st)
{
    const int n = a.Q * a.C;
    int N = 1;
    while (N < n) N <<= 1;
    const int threads = std::min(kDetectThreads, std::max(64, N >> 1));             // a thread per pair up to the block limit; whole waves
    hipLaunchKernelGGL(detect_decode_kernel, dim3(static_cast<unsigned>(a.B)), dim3(static_cast<unsigned>(threads)), 0, st, a, N);
    return hipGetLastError();
}

void detect_decode_host(const DetectArgs &a)
{
    const int n = a.Q * a.C;
    std::vector<uint32_t> order(static_cast<size_t>(n));
    for (int b = 0; b < a.B; ++b) {
        const float *lg = a.logits + static_cast<int64_t>(b) * n;
        for (int i = 0; i < n; ++i) order[i] = static_cast<uint32_t>(i);
        std::stable_sort(order.begin(), order.end(), [lg](uint32_t x, uint32_t y) { return detect_order_word(lg[x]) > detect_order_word(lg[y]); });
        for (int j = 0; j < a.topk; ++j) {
            const int q = static_cast<int>(order[j]) / a.C, label = static_cast<int>(order[j]) - q * a.C;
            const int64_t bq = static_cast<int64_t>(b) * a.Q + q, out = static_cast<int64_t>(b) * a.topk + j;
            a.keep[out] = detect_decode_one(lg[order[j]], label, a.boxes + bq * 6, a.angle + bq * 24, a.dim + bq * 3, a.depth + bq * 2, a.calib + b * 6,
                                            a.size + b * 2, a.mean, a.threshold, a.recs ? a.recs + out * kDetectRecord : nullptr,
                                            a.rows + out * kDetectRow) ? 1 : 0;
        }
    }
}

}  // namespace mdetr
