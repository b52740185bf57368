// monodetr_amd/csrc/detect.h -- internal launcher declarations (see detect.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mdetr {

constexpr int kDetectMaxKeys = 8192;                             // Q * C of one image: the sort runs in one workgroup's LDS

struct DetectArgs {
    const float *logits, *boxes, *angle, *dim, *depth;          // [B, Q, C] [B, Q, 6] [B, Q, 24] [B, Q, 3] [B, Q, 2]
    const double *calib, *size, *mean;                           // [B, 6] [B, 2] [C, 3]
    double *rows;                                                // [B, topk, 14]
    uint8_t *keep;                                               // [B, topk]
    float *recs;                                                 // [B, topk, 37] or NULL
    int B, Q, C, topk;
    float threshold;
};

// One workgroup per image: sort the Q C keys, decode the first topk.  1 <= topk <= Q C <= kDetectMaxKeys, B >= 1.
hipError_t detect_decode_launch(const DetectArgs &a, hipStream_t st);
// The same results from a serial stable sort and the same arithmetic on the host; every pointer is host memory.
void detect_decode_host(const DetectArgs &a);

}  // namespace mdetr
