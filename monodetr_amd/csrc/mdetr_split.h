// monodetr_amd/csrc/mdetr_split.h -- the three-way bf16 split of an fp32 operand, shared by the fp32 forms of csrc/tgemm.hip and
// csrc/twgrad.hip:   hi = bf16(x),  mid = bf16(x - hi),  lo = bf16(x - hi - mid)
// Both subtractions are exact (attn.hip's split_bf16), so hi + mid + lo carries 24 significant bits of x; a product of two split
// operands is issued as the six terms lo.hi, hi.lo, mid.mid, mid.hi, hi.mid, hi.hi (small ones first) into one fp32 accumulator.
// x - bf16(x) is NaN for +-inf: an infinite operand yields NaN.
#pragma once
#include <mdetr_wave.h>

namespace mdetr {

// 4 fp32 values (the 16 bytes of a staged piece, or 4 gathered values) -> their hi / mid / lo bf16 parts, 8 bytes each
__device__ __forceinline__ void split4(const float (&x)[4], bf16x4 &h, bf16x4 &m, bf16x4 &l)
{
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const __bf16 hi = static_cast<__bf16>(x[i]);
        const float r1 = x[i] - static_cast<float>(hi);               // exact
        const __bf16 mi = static_cast<__bf16>(r1);
        h[i] = hi; m[i] = mi; l[i] = static_cast<__bf16>(r1 - static_cast<float>(mi));     // exact again; <= 8 significant bits are left
    }
}

}  // namespace mdetr
