// decode_bbox of TransFusionHead (transfusion_head.py:636-645) for one query: the one statement of it for the inference decode
// (proposals.hip) and the cost kernel of the target assignment (tfassign.hip).  x = center * stride * voxel + range in f32, two
// multiplications and one addition, not contracted (-ffp-contract=off), which is the reference's sequence bit for bit; the
// sizes exp(dim) and the yaw atan2(sin, cos) are formed in f64 and rounded once.  Heads are (B, n, K) channel-major.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ void tf_decode_box(const float *__restrict__ center, const float *__restrict__ height,
                                              const float *__restrict__ dim, const float *__restrict__ rot,
                                              const float *__restrict__ vel, size_t b, int k, int K, float stride, float vx, float vy,
                                              float x0, float y0, float box[9]) {
    box[0] = center[(b * 2 + 0) * K + k] * stride * vx + x0;
    box[1] = center[(b * 2 + 1) * K + k] * stride * vy + y0;
    box[2] = height[b * K + k];
    for (int j = 0; j < 3; ++j) box[3 + j] = (float)exp((double)dim[(b * 3 + j) * K + k]);
    box[6] = (float)atan2((double)rot[(b * 2 + 0) * K + k], (double)rot[(b * 2 + 1) * K + k]);
    box[7] = box[8] = 0.f;
    if (vel) box[7] = vel[(b * 2 + 0) * K + k], box[8] = vel[(b * 2 + 1) * K + k];
}
