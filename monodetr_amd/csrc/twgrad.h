// monodetr_amd/csrc/twgrad.h -- internal launcher declarations (see twgrad.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mdetr {

// bf16 x [T, C] (row stride ldx), dy [T, N] (row stride ldy); C % 8 == 0, N % 8 == 0; 16-byte aligned
bool twgrad_supported(int64_t T, int C, int N, int64_t ldx, int64_t ldy, const void *x, const void *dy);
int twgrad_chunks(int64_t T, int C, int N);
// part: fp32 [chunks][N * C (+ N with_db)]: per-chunk partial dW (row n, column c) followed by the chunk's partial db
hipError_t twgrad_launch(const void *x, const void *dy, float *part, int64_t T, int C, int N, int64_t ldx, int64_t ldy, bool with_db,
                         hipStream_t st);
// The same launches for several problems at once (contiguous rows: ldx = C, ldy = N), each planned as a launch of its own -- the same
// chunks (twgrad_chunks), partial layout and bits -- carried by one launch per kernel instantiation and per 32 jobs.
struct TwgradJob {
    const void *x, *dy;
    float *part;
    int64_t T;
    int C, N, with_db;
};
hipError_t twgrad_grouped_launch(const TwgradJob *jobs, int njobs, hipStream_t st);

// The fp32 form: fp32 x [T, C], dy [T, N] (row strides % 4 == 0), same partial layout; C % 8 == 0, N % 8 == 0; 16-byte aligned;
// T ld < 2^29 elements (byte offsets fit 32 bits)
bool twgrad_f32_supported(int64_t T, int C, int N, int64_t ldx, int64_t ldy, const void *x, const void *dy);
int twgrad_f32_chunks(int64_t T, int C, int N);
hipError_t twgrad_f32_launch(const void *x, const void *dy, float *part, int64_t T, int C, int N, int64_t ldx, int64_t ldy, bool with_db,
                             hipStream_t st);

}  // namespace mdetr
