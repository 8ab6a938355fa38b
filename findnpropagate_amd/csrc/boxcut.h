// The point-in-box test of gt_sampling's cut (DataBaseSampler.add_sampled_boxes_to_scene -> box_utils.remove_points_in_boxes3d
// -> roiaware_pool3d.cpp points_in_boxes_cpu, the check_pt_in_box3d_cpu of its g++ build), defined once for the host entry
// fnp_host_points_outside_boxes and the device mark of fnp_prepare_points_cut.
//
// A record is 8 floats {cx, cy, cz, dx, dy, dz, cos(-h), sin(-h)}; fnp_host_cut_records writes the two trigonometric values with
// the C library's cosf / sinf, the calls the reference makes for every (point, box) pair, so the device evaluates no trigonometry
// and both sides test with the same bits.  The arithmetic is the reference's, rounding step by rounding step (the library builds
// with -ffp-contract=off):
//   z out        fabsf(z - cz) > dz / 2.0                            (f32 difference, compared in double, strict)
//   local x, y   lx = sx * c + sy * (-s),  ly = sx * s + sy * c       (sx = x - cx, sy = y - cy; f32, no contraction)
//   inside       |lx| < dx / 2.0 + MARGIN  and  |ly| < dy / 2.0 + MARGIN   (compared in double, MARGIN = 1e-2f)
// The double thresholds depend on the box alone and are prepared once per box.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

struct FnpCutBox {
    float cx, cy, cz, c, s;
    double hx, hy, hz;   // dx / 2.0 + MARGIN, dy / 2.0 + MARGIN, dz / 2.0
};

__host__ __device__ __forceinline__ FnpCutBox fnp_cut_box(const float *rec) {
    const float kMargin = 1e-2f;
    FnpCutBox b;
    b.cx = rec[0];
    b.cy = rec[1];
    b.cz = rec[2];
    b.c = rec[6];
    b.s = rec[7];
    b.hx = (double)rec[3] / 2.0 + (double)kMargin;
    b.hy = (double)rec[4] / 2.0 + (double)kMargin;
    b.hz = (double)rec[5] / 2.0;
    return b;
}

__host__ __device__ __forceinline__ bool fnp_cut_inside(const FnpCutBox &b, float x, float y, float z) {
    if ((double)fabsf(z - b.cz) > b.hz) return false;
    const float sx = x - b.cx, sy = y - b.cy;
    const float lx = sx * b.c + sy * (-b.s);
    const float ly = sx * b.s + sy * b.c;
    return (double)fabsf(lx) < b.hx && (double)fabsf(ly) < b.hy;
}
