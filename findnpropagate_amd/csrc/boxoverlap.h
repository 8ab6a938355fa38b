// Rotated-rectangle overlap in the BEV plane, the reference's arithmetic (pcdet/ops/iou3d_nms/src/iou3d_nms_kernel.cu:52-62,
// :201-224; see iou3d_nms.hip's head comment for how it is organised).  One statement of it for every kernel that needs the
// overlap of two boxes: the pairwise, aligned and NMS kernels of iou3d_nms.hip, the host twins there, and the cost kernel of
// tfassign.hip.  test_gpu_box_at_scale.py holds it to the reference's own kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace {

struct P2 {
    float x, y;
};

struct RBox {           // one rotated rectangle, prepared once
    float raw[7];
    P2 c[5];            // rotated corners, c[4] == c[0]
    float ncos, nsin;   // cos(-heading), sin(-heading) for the corner-inside test
    float hx, hy;       // dx/2 + 1e-2f, dy/2 + 1e-2f (f32, :61)
};

__host__ __device__ __forceinline__ float cross3(const P2 &p1, const P2 &p2, const P2 &p0) {
    return (p1.x - p0.x) * (p2.y - p0.y) - (p2.x - p0.x) * (p1.y - p0.y);
}

__host__ __device__ __forceinline__ void prep_box(const float *b, RBox &r) {
#pragma unroll
    for (int i = 0; i < 7; ++i) r.raw[i] = b[i];
    const float hx = b[3] / 2, hy = b[4] / 2;
    const float cx = b[0], cy = b[1];
    const float cs = cosf(b[6]), sn = sinf(b[6]);
    const float ox[4] = {cx - hx, cx + hx, cx + hx, cx - hx};
    const float oy[4] = {cy - hy, cy - hy, cy + hy, cy + hy};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        r.c[k].x = (ox[k] - cx) * cs + (oy[k] - cy) * (-sn) + cx;
        r.c[k].y = (ox[k] - cx) * sn + (oy[k] - cy) * cs + cy;
    }
    r.c[4] = r.c[0];
    r.ncos = cosf(-b[6]);
    r.nsin = sinf(-b[6]);
    r.hx = b[3] / 2 + 1e-2f;
    r.hy = b[4] / 2 + 1e-2f;
}

__host__ __device__ __forceinline__ bool corner_inside(const RBox &box, const P2 &p) {
    const float rx = (p.x - box.raw[0]) * box.ncos + (p.y - box.raw[1]) * (-box.nsin);
    const float ry = (p.x - box.raw[0]) * box.nsin + (p.y - box.raw[1]) * box.ncos;
    return fabsf(rx) < box.hx && fabsf(ry) < box.hy;
}

__host__ __device__ __forceinline__ bool seg_cross(const P2 &p1, const P2 &p0, const P2 &q1, const P2 &q0, P2 &ans) {
    const bool bb = fminf(p0.x, p1.x) <= fmaxf(q0.x, q1.x) && fminf(q0.x, q1.x) <= fmaxf(p0.x, p1.x) &&
                    fminf(p0.y, p1.y) <= fmaxf(q0.y, q1.y) && fminf(q0.y, q1.y) <= fmaxf(p0.y, p1.y);
    if (!bb) return false;
    const float s1 = cross3(q0, p1, p0);
    const float s2 = cross3(p1, q1, p0);
    const float s3 = cross3(p0, q1, q0);
    const float s4 = cross3(q1, p1, q0);
    if (!(s1 * s2 > 0 && s3 * s4 > 0)) return false;
    const float s5 = cross3(q1, p1, p0);
    if (fabsf(s5 - s1) > 1e-8f) {
        ans.x = (s5 * q0.x - s1 * q1.x) / (s5 - s1);
        ans.y = (s5 * q0.y - s1 * q1.y) / (s5 - s1);
    } else {
        const float a0 = p0.y - p1.y, b0 = p1.x - p0.x, c0 = p0.x * p1.y - p1.x * p0.y;
        const float a1 = q0.y - q1.y, b1 = q1.x - q0.x, c1 = q0.x * q1.y - q1.x * q0.y;
        const float D = a0 * b1 - a1 * b0;
        ans.x = (b0 * c1 - b1 * c0) / D;
        ans.y = (a1 * c0 - a0 * c1) / D;
    }
    return true;
}

// Where the polygon of an intersection lives while it is built, sorted and summed: at most 24 vertices (16 crossings, 8 corners)
// and their angular keys, indexed dynamically.  PolyLocal is a thread's own arrays (private memory on the device); PolyStrided
// is a slice of a caller's buffer, vertex i at [i * stride], which lets a kernel keep the polygons of a workgroup in LDS, one
// column per thread.  The arithmetic does not depend on the store.
struct PolyLocal {
    P2 v[24];
    float key[24];
    __host__ __device__ __forceinline__ P2 &p(int i) { return v[i]; }
    __host__ __device__ __forceinline__ float &k(int i) { return key[i]; }
};
struct PolyStrided {
    P2 *v;
    float *key;
    int stride;
    __host__ __device__ __forceinline__ P2 &p(int i) { return v[i * stride]; }
    __host__ __device__ __forceinline__ float &k(int i) { return key[i * stride]; }
};

template <class Poly>
__host__ __device__ __forceinline__ float overlap_area_in(const RBox &A, const RBox &B, Poly &st) {
    int cnt = 0;
    float sx = 0.f, sy = 0.f;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            P2 x;
            if (seg_cross(A.c[i + 1], A.c[i], B.c[j + 1], B.c[j], x)) {
                sx = sx + x.x;
                sy = sy + x.y;
                st.p(cnt++) = x;
            }
        }
    for (int k = 0; k < 4; ++k) {
        if (corner_inside(A, B.c[k])) {
            sx = sx + B.c[k].x;
            sy = sy + B.c[k].y;
            st.p(cnt++) = B.c[k];
        }
        if (corner_inside(B, A.c[k])) {
            sx = sx + A.c[k].x;
            sy = sy + A.c[k].y;
            st.p(cnt++) = A.c[k];
        }
    }
    if (cnt < 3) return 0.f;  // fan over < 3 vertices has zero area (reference: empty loop / zero cross)
    const float mx = sx / cnt, my = sy / cnt;
    for (int i = 0; i < cnt; ++i) st.k(i) = atan2f(st.p(i).y - my, st.p(i).x - mx);
    for (int i = 1; i < cnt; ++i) {  // stable insertion sort, ascending
        const P2 p = st.p(i);
        const float k = st.k(i);
        int j = i - 1;
        while (j >= 0 && st.k(j) > k) {
            st.p(j + 1) = st.p(j);
            st.k(j + 1) = st.k(j);
            --j;
        }
        st.p(j + 1) = p;
        st.k(j + 1) = k;
    }
    float area = 0.f;
    for (int k = 0; k < cnt - 1; ++k) {
        const P2 p0 = st.p(0), pk = st.p(k), pn = st.p(k + 1);
        const float ux = pk.x - p0.x, uy = pk.y - p0.y;
        const float vx = pn.x - p0.x, vy = pn.y - p0.y;
        area += ux * vy - uy * vx;
    }
    return fabsf(area) * 0.5f;  // == (float)(fabs(area) / 2.0)
}

__host__ __device__ float overlap_area(const RBox &A, const RBox &B) {
    PolyLocal st;
    return overlap_area_in(A, B, st);
}

}  // namespace
