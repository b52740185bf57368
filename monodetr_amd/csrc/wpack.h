// monodetr_amd/csrc/wpack.h -- internal launcher declarations (see wpack.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <monodetr_amd.h>

namespace mdetr {

constexpr int kPackJobs = 48;                                    // job descriptors per launch (kernel arguments); longer lists: several launches
constexpr int kPosLevels = 8;                                    // level boundaries per launch (kernel arguments)

// message or nullptr: pointers aligned to their element, dtype MDETR_F32 / MDETR_BF16, elements >= 0
const char *pack_params_check(const mdetr_pack_job *jobs, int njobs);
// job i: dst[e] = src0[e] (src1 == NULL) or the once-rounded fp32 sum src0[e] + src1[e], e < elements.  `jobs` lives on the HOST.
hipError_t pack_params_launch(const mdetr_pack_job *jobs, int njobs, hipStream_t st);
// out[s][c] = sine[s][c] + embed[level of s][c] (fp32 sum; through bf16 where both operands are bf16; then out's type); counts[l]
// rows belong to level l.  C % 8 == 0, 16-byte aligned tensors, 0 < levels <= kPosLevels
hipError_t level_pos_launch(const void *sine, bool sine_bf16, const void *embed, bool embed_bf16, void *out, bool out_bf16, const int64_t *counts,
                            int levels, int C, hipStream_t st);

}  // namespace mdetr
