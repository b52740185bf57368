// monodetr_amd/csrc/detect_math.h -- one selected (query, class) pair of the model's head outputs -> one KITTI detection: the
// arithmetic of helpers/decode_helper.py (the reference's lib/helpers/decode_helper.py:8-110), shared by the HIP kernel (detect.hip)
// and by its serial host form.
//
// Two results, in the two precisions the Python path computes them in:
//   the 37-float record of extract_dets_from_outputs, fp32, operation by operation as torch evaluates it:
//     [label, score, (x0 + x1) / 2, (y0 + y1) / 2, x1 - x0, y1 - y0, depth, 24 heading values, 3 sizes, cx, cy, sigma]
//     with (x0, y0, x1, y1) = (cx - l, cy - t, cx + r, cy + b), score = 1 / (1 + expf(-logit)), sigma = expf(-log variance);
//   the 14-value result row of decode_detections, fp64 from that record (numpy >= 2 promotes the fp32 record against the
//   int64 image size and the fp64 bin width to fp64; the calibration scalars are fp32 VALUES and arrive here as doubles):
//     [class, alpha, x1, y1, x2, y2, h, w, l, x, y, z, ry, score * sigma]          (the last product in fp32)
// and the keep flag score >= threshold, compared in fp32 as numpy compares an fp32 array with a Python float.
//
// Also here: the order in which (query, class) pairs are selected -- by LOGIT, which sorts as its sigmoid does wherever the
// sigmoid still tells two logits apart and decides where it does not.
#pragma once

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define MDETR_DT_HD __host__ __device__ __forceinline__
#else
#include <cmath>
#define MDETR_DT_HD inline
#endif

namespace mdetr {

constexpr int kDetectRecord = 37;                                // floats per record
constexpr int kDetectRow = 14;                                   // doubles per result row
constexpr int kDetectBins = 12;                                  // heading bins (datasets/utils.py: num_heading_bin)
constexpr double kDetectPi = 3.141592653589793;                  // numpy.pi

// Sort word of a logit: larger word = earlier rank.  NaN ranks first (as torch.topk / torch.sort place it), then +inf ... -inf
// by value; -0 and +0 get the same word.
MDETR_DT_HD uint32_t detect_order_word(float logit)
{
    uint32_t u;
    memcpy(&u, &logit, 4);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return 0xFFFFFFFFu;     // NaN, either sign
    if (u == 0x80000000u) u = 0u;                                // -0 == +0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);           // (below 0xFFFFFFFF: only the NaN 0x7FFFFFFF maps there)
}

// 64-bit sort key of flat index q * C + c: sort word high, complemented index low -- among equal words the smaller index has the
// larger key.  Distinct for distinct indices and never 0, the key of padding.
MDETR_DT_HD uint64_t detect_key(float logit, uint32_t flat)
{
    return (static_cast<uint64_t>(detect_order_word(logit)) << 32) | static_cast<uint64_t>(~flat);
}
MDETR_DT_HD uint32_t detect_key_index(uint64_t key) { return ~static_cast<uint32_t>(key); }

// box  [6] cx cy l r t b     angle [24] 12 bin logits + 12 residuals     dim [3]     depth [2] depth, log variance
// calib [6] cu cv fu fv tx ty     size [2] W H     mean [C][3]
// rec: 37 floats or NULL; row: 14 doubles.  -> keep
MDETR_DT_HD bool detect_decode_one(float logit, int label, const float *box, const float *angle, const float *dim, const float *depth,
                                   const double *calib, const double *size, const double *mean, float threshold, float *rec, double *row)
{
#pragma clang fp contract(off)
    // ---- extract_dets_from_outputs, fp32 ----
    const float score = 1.0f / (1.0f + expf(-logit));
    const float sigma = expf(-depth[1]);
    const float cx = box[0], cy = box[1];
    const float x0 = cx - box[2], y0 = cy - box[4], x1 = cx + box[3], y1 = cy + box[5];
    const float bx = (x0 + x1) / 2.0f, by = (y0 + y1) / 2.0f, bw = x1 - x0, bh = y1 - y0;
    const float z32 = depth[0];
    // np.argmax of the bin logits: the first maximum, a NaN counting as one
    int bin = 0;
    float best = angle[0], residual = angle[kDetectBins];
#pragma unroll
    for (int k = 1; k < kDetectBins; ++k) {
        const float v = angle[k];
        if (v > best || (v != v && best == best)) { best = v; bin = k; residual = angle[kDetectBins + k]; }
    }
    if (rec) {
        rec[0] = static_cast<float>(label); rec[1] = score; rec[2] = bx; rec[3] = by; rec[4] = bw; rec[5] = bh; rec[6] = z32;
#pragma unroll
        for (int k = 0; k < 2 * kDetectBins; ++k) rec[7 + k] = angle[k];
        rec[31] = dim[0]; rec[32] = dim[1]; rec[33] = dim[2]; rec[34] = cx; rec[35] = cy; rec[36] = sigma;
    }
    // ---- decode_detections, fp64 ----
    const double cu = calib[0], cv = calib[1], fu = calib[2], fv = calib[3], tx = calib[4], ty = calib[5];
    const double W = size[0], H = size[1];
    const double x = static_cast<double>(bx) * W, y = static_cast<double>(by) * H;
    const double w = static_cast<double>(bw) * W, h = static_cast<double>(bh) * H;
    const double z = static_cast<double>(z32);
    const double *m = mean + 3 * label;
    const double d0 = static_cast<double>(dim[0]) + m[0], d1 = static_cast<double>(dim[1]) + m[1], d2 = static_cast<double>(dim[2]) + m[2];
    const double u = static_cast<double>(cx) * W, v = static_cast<double>(cy) * H;
    const double lx = ((u - cu) * z) / fu + tx;                  // Calibration.img_to_rect
    double ly = ((v - cv) * z) / fv + ty;
    ly = ly + d0 / 2.0;                                          // box origin: bottom centre
    double alpha = static_cast<double>(bin) * (2.0 * kDetectPi / 12.0) + static_cast<double>(residual);      // class2angle, label format
    if (alpha > kDetectPi) alpha = alpha - 2.0 * kDetectPi;
    double ry = alpha + atan2(x - cu, fu);                       // Calibration.alpha2ry
    if (ry > kDetectPi) ry = ry - 2.0 * kDetectPi;
    if (ry < -kDetectPi) ry = ry + 2.0 * kDetectPi;
    row[0] = static_cast<double>(label); row[1] = alpha;
    row[2] = x - w / 2.0; row[3] = y - h / 2.0; row[4] = x + w / 2.0; row[5] = y + h / 2.0;
    row[6] = d0; row[7] = d1; row[8] = d2; row[9] = lx; row[10] = ly; row[11] = z; row[12] = ry;
    row[13] = static_cast<double>(score * sigma);
    return score >= threshold;
}

}  // namespace mdetr
