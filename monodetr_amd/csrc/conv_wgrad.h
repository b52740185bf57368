// monodetr_amd/csrc/conv_wgrad.h -- internal launcher declarations (see conv_wgrad.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mdetr {

// x [B, H, W, C] bf16, dy [B, OH, OW, N] bf16 (both contiguous, 16-byte aligned), K x K taps (K = 3: pad 1, stride SI in {1, 2};
// K = 1: pad 0, stride 2), C % 64 == 0, N % 32 == 0.  part: fp32 [chunks][N][K][K][C], chunks = conv_wgrad_chunks(d).
struct ConvWgradDims {
    int B, H, W, C;
    int OH, OW, N;
    int K, SI;
    int DB = 0;       // 1 (K = 1, SI = 1 only): every chunk also carries the column sums of dy -- the bias gradient of a token-wise linear
                      // layer -- as N more floats behind its [N][C] block: part is [chunks][N * C + N]
};

bool conv_wgrad_supported(const ConvWgradDims &d, const void *x, const void *dy);
int conv_wgrad_chunks(const ConvWgradDims &d);
hipError_t conv_wgrad_launch(const void *x, const void *dy, float *part, const ConvWgradDims &d, hipStream_t st);

// The fp32 form (conv_wgrad_f32_kernel): x and dy fp32, K = 3, SI = 1 (OH = H, OW = W), DB = 0 only; B H W C and B H W N below 2^29
// elements.  Operands are split into three bf16 parts on their way into LDS (mdetr_split.h): an infinite operand yields NaN.
// Same partials: fp32 [chunks][N][3][3][C], chunks = conv_wgrad_f32_chunks(d).
bool conv_wgrad_f32_supported(const ConvWgradDims &d, const void *x, const void *dy);
int conv_wgrad_f32_chunks(const ConvWgradDims &d);
hipError_t conv_wgrad_f32_launch(const void *x, const void *dy, float *part, const ConvWgradDims &d, hipStream_t st);

// The fp32 form at stride 2 (conv_wgrad_s2_f32_kernel): x and dy fp32, K = 3, SI = 2 (OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1), DB = 0 only;
// B H W C and B OH OW N below 2^29 elements.  The same split, the same six terms, the same partials: fp32 [chunks][N][3][3][C],
// chunks = conv_wgrad_s2_f32_chunks(d).
bool conv_wgrad_s2_f32_supported(const ConvWgradDims &d, const void *x, const void *dy);
int conv_wgrad_s2_f32_chunks(const ConvWgradDims &d);
hipError_t conv_wgrad_s2_f32_launch(const void *x, const void *dy, float *part, const ConvWgradDims &d, hipStream_t st);

}  // namespace mdetr
