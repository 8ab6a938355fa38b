// Point preparation in front of the voxeliser: the world augmentations of DataAugmentor (random_world_flip / _rotation /
// _scaling / _translation, pcdet/datasets/augmentor/data_augmentor.py:59-181), mask_points_and_boxes_outside_range (the points
// half, data_processor.py:80-94) and shuffle_points (data_processor.py:96-106), for a batch of concatenated scenes, in one pass
// over the rows the voxeliser reads next.  The reference runs these steps in numpy inside DataLoader workers.
//
//   1. mark : a thread per point applies the scene's op program to x, y, z (the reference's f32 arithmetic, see apply_program),
//             tests x and y against the range (both ends inclusive, z not tested); a wave ballot per 64 points, a kept count per
//             workgroup of 256 points                                                                         [prep_mark]
//   2. exclusive scan of the workgroup counts                                                                 [scan.hip]
//   3. per scene: the kept rows before its first point = its new offset; explicit permutation mode also
//      inverts the caller's permutation here                                                         [prep_offsets, prep_invert]
//   4. emit : every kept point recomputes its transform and writes its row to its slot; rows [kept, N) get the pad value
//             (outside every range: fnp_voxelize drops them, as behind fnp_stage_points)                       [prep_emit]
// Slot of the k-th kept point of scene b (m_b kept points, new offset o_b):
//   FNP_SHUFFLE_NONE     o_b + k                                  (stable compaction: the reference with shuffling disabled)
//   FNP_SHUFFLE_DEVICE   o_b + feistel_b(k)                       (a keyed bijection of [0, m_b); not numpy's permutation)
//   FNP_SHUFFLE_EXPLICIT j where perm[j] = k, j in [o_b, o_b + m_b)  (out[j] = kept[perm[j]]: the reference's order, bit for bit)
// No atomics, no host synchronisation; every row count is read from device memory.
//
// fnp_prepare_points_cut adds gt_sampling's cut (DataBaseSampler.add_sampled_boxes_to_scene, database_sampler.py:367-452) to
// the mark: row i of scene b is dropped when i >= off[b] + cut_from[b] (the pasted object rows lead the scene and are never cut)
// and the row, before its program moves it, lies inside one of the scene's records [cut_offsets[b], cut_offsets[b+1]) (boxcut.h).
// fnp_prepare_points_cut_window also bounds the test from above: only rows with cut_from[b] <= i - off[b] < cut_to[b] are tested
// (unknowns_copy_paste appends its pasted rows behind the scene rows, and the cut must not reach them).  The relative index is
// compared, so a "to the end" cut_to such as INT32_MAX cannot overflow.
// The entry points share every kernel; the cut is a compile-time flag of the mark, and the no-cut instantiation is the mark as
// it was.  The window is a pointer of the cut (NULL: no upper bound).
#include <vector>

#include "boxcut.h"
#include "rankgrid.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

enum { OP_NONE = 0, OP_FLIP_X = 1, OP_FLIP_Y = 2, OP_ROTATE = 3, OP_SCALE = 4, OP_TRANSLATE = 5 };

struct PrepWs {
    unsigned long long *mask;   // (G*4) ballot of kept points per wave
    int *cnt;                   // (G)   kept points per workgroup
    int *base;                  // (G)   exclusive scan of cnt
    int *total;                 // (1)
    int *inv;                   // (N)   explicit mode: kept rank -> output row
    void *scan_ws;
};

__host__ long long align_up(long long v) { return (v + 255) & ~255ll; }

__host__ long long carve(PrepWs &w, char *p, long long n) {
    const long long G = (n + kThreads - 1) / kThreads;
    long long off = 0;
    auto take = [&](long long bytes) {
        char *q = p ? p + off : nullptr;
        off += align_up(bytes);
        return q;
    };
    w.mask = (unsigned long long *)take(8 * G * kWaves);
    w.cnt = (int *)take(4 * G);
    w.base = (int *)take(4 * G);
    w.total = (int *)take(4);
    w.inv = (int *)take(4 * n);
    w.scan_ws = take(fnp_scan::workspace_bytes(G));
    return off;
}

__device__ __forceinline__ int scene_of(const int *__restrict__ off, int B, int i) {
    int lo = 0, hi = B;   // off[lo] <= i < off[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// The reference's arithmetic, rounding step by rounding step (the library builds with -ffp-contract=off; the one fused
// multiply-add is written out):
//   flip x      y = -y                       augmentor_utils.random_flip_along_x
//   flip y      x = -x                       augmentor_utils.random_flip_along_y
//   rotate      [x y z] @ [[c s 0] [-s c 0] [0 0 1]] in f32 (common_utils.rotate_points_along_z: torch's CPU matmul, whose
//               result is x' = fma(y, -s, x*c), y' = fma(y, c, x*s), z' = z); c, s = torch.cos / sin of the f32 angle, on the host
//   scale       xyz *= (float)noise_scale    (a Python float against an f32 array: an f32 multiply)
//   translate   xyz += noise_translate       (f32)
// prog: K rows of 4 floats {op, a, b, c}.
__device__ __forceinline__ void apply_program(const float *__restrict__ prog, int K, float &x, float &y, float &z) {
    for (int k = 0; k < K; ++k) {
        const float4 st = reinterpret_cast<const float4 *>(prog)[k];
        switch ((int)st.x) {
        case OP_FLIP_X: y = -y; break;
        case OP_FLIP_Y: x = -x; break;
        case OP_ROTATE: {
            const float c = st.y, s = st.z;
            const float xn = __fmaf_rn(y, -s, __fmul_rn(x, c));
            const float yn = __fmaf_rn(y, c, __fmul_rn(x, s));
            x = xn;
            y = yn;
            break;
        }
        case OP_SCALE:
            x = __fmul_rn(x, st.y);
            y = __fmul_rn(y, st.y);
            z = __fmul_rn(z, st.y);
            break;
        case OP_TRANSLATE:
            x = __fadd_rn(x, st.y);
            y = __fadd_rn(y, st.z);
            z = __fadd_rn(z, st.w);
            break;
        default: break;
        }
    }
}

struct XyRange { double x0, y0, x1, y1; };   // f32 point against the f64 range of the config: numpy compares in f64

__device__ __forceinline__ bool in_range(const XyRange &r, float x, float y) {
    const double dx = x, dy = y;
    return dx >= r.x0 && dx <= r.x1 && dy >= r.y0 && dy <= r.y1;
}

// scene of point i (searched once per wave for its first lane, per lane where the wave crosses a scene border)
__device__ __forceinline__ int scene_of_wave(const int *__restrict__ off, int B, int i) {
    const int i0 = __builtin_amdgcn_readfirstlane(i);
    int b = scene_of(off, B, i0);
    if (b + 1 < B && i >= off[b + 1]) b = scene_of(off, B, i);
    return b;
}

__device__ __forceinline__ bool kept_point(const float *__restrict__ pts, int C, int i, int b, const float *__restrict__ prog, int K,
                                           const XyRange &r) {
    const float *p = pts + (size_t)i * C;
    float x = p[0], y = p[1], z = p[2];
    if (prog) apply_program(prog + (size_t)b * K * 4, K, x, y, z);
    return in_range(r, x, y);
}

struct CutArgs {
    const float *rec;   // (M, 8) records, boxcut.h
    const int *off;     // (B+1) scene b owns records [off[b], off[b+1])
    const int *from;    // (B)   scene b's rows [0, from[b]) are never cut
    const int *to;      // (B)   or NULL: scene b's rows [to[b], end) are never cut either
};

// Is row i (raw x, y, z) of scene b cut?  A wave whose live lanes lie in one scene walks that scene's records with wave-uniform
// loads and leaves the walk once no lane needs another box; a wave that straddles two scenes walks each lane's own records.
__device__ __forceinline__ bool cut_row(const CutArgs &cut, const int *__restrict__ off, int b, int i, float x, float y, float z) {
    const int rel = i - off[b];
    const bool test = rel >= cut.from[b] && (!cut.to || rel < cut.to[b]);
    bool inside = false;
    const int b0 = __builtin_amdgcn_readfirstlane(b);
    if (__ballot(b != b0) == 0) {
        const int k1 = cut.off[b0 + 1];
        for (int k = cut.off[b0]; k < k1; ++k) {
            if (__ballot(test && !inside) == 0) break;
            const FnpCutBox bx = fnp_cut_box(cut.rec + (size_t)k * 8);
            if (test && !inside) inside = fnp_cut_inside(bx, x, y, z);
        }
    } else if (test) {
        const int k1 = cut.off[b + 1];
        for (int k = cut.off[b]; k < k1 && !inside; ++k) inside = fnp_cut_inside(fnp_cut_box(cut.rec + (size_t)k * 8), x, y, z);
    }
    return inside;
}

template <bool kCut>
__global__ __launch_bounds__(kThreads) void prep_mark_kernel(const float *__restrict__ pts, int n, int C, const int *__restrict__ off, int B,
                                                             const float *__restrict__ prog, int K, XyRange r, CutArgs cut,
                                                             unsigned long long *__restrict__ mask, int *__restrict__ cnt) {
    __shared__ int wcnt[kWaves];
    const int i = blockIdx.x * kThreads + threadIdx.x;
    const int lo = off[0], hi = off[B];
    bool keep = false;
    if (i < n && i >= lo && i < hi) {
        const int b = scene_of_wave(off, B, i);
        if constexpr (kCut) {
            const float *p = pts + (size_t)i * C;
            keep = !cut_row(cut, off, b, i, p[0], p[1], p[2]) && kept_point(pts, C, i, b, prog, K, r);
        } else {
            keep = kept_point(pts, C, i, b, prog, K, r);
        }
    }
    const unsigned long long bal = __ballot(keep);
    const int wave = threadIdx.x >> 6;
    if (fnp_lane() == 0) {
        mask[(size_t)blockIdx.x * kWaves + wave] = bal;
        wcnt[wave] = __popcll(bal);
    }
    __syncthreads();
    if (threadIdx.x == 0) cnt[blockIdx.x] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
}

// kept points in front of point i (i <= n): the workgroup base plus the ballots of the earlier waves and lanes
__device__ __forceinline__ int kept_before(const unsigned long long *__restrict__ mask, const int *__restrict__ base, int total, int n, int i) {
    if (i >= n) return total;
    const int blk = i / kThreads, w = (i % kThreads) >> 6, lane = i & 63;
    int k = base[blk];
    for (int j = 0; j < w; ++j) k += __popcll(mask[(size_t)blk * kWaves + j]);
    return k + __popcll(mask[(size_t)blk * kWaves + w] & ((1ull << lane) - 1ull));
}

// new offsets: o_b = kept points in front of off[b] (thread per entry; off[B] and beyond count every kept point)
__global__ __launch_bounds__(kThreads) void prep_offsets_kernel(const int *__restrict__ off, int B, int n,
                                                                const unsigned long long *__restrict__ mask, const int *__restrict__ base,
                                                                const int *__restrict__ total, int *__restrict__ out_off) {
    const int b = blockIdx.x * kThreads + threadIdx.x;
    if (b > B) return;
    const int t = *total;
    int i = off[b];
    i = i < 0 ? 0 : i;
    out_off[b] = b == B ? t : kept_before(mask, base, t, n, i);
}

// explicit permutation: inv[o_b + perm[j]] = j for every output row j < min(n_perm, kept) (perm[j] outside [0, m_b): ignored)
__global__ __launch_bounds__(kThreads) void prep_invert_kernel(const int *__restrict__ perm, long long n_perm, const int *__restrict__ out_off, int B,
                                                               int *__restrict__ inv) {
    const int total = out_off[B];
    const long long lim = n_perm < total ? n_perm : total;
    for (long long j = (long long)blockIdx.x * kThreads + threadIdx.x; j < lim; j += (long long)gridDim.x * kThreads) {
        const int b = scene_of(out_off, B, (int)j);
        const int o = out_off[b], m = out_off[b + 1] - o, k = perm[j];
        if (k >= 0 && k < m) inv[o + k] = (int)j;
    }
}

__device__ __forceinline__ unsigned mix32(unsigned x) {
    x ^= x >> 16; x *= 0x7feb352du;
    x ^= x >> 15; x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

constexpr int kFeistelRounds = 6;

// A keyed bijection of [0, m): a balanced Feistel network on the smallest even number of bits that holds m - 1, walked along
// its cycle until the value falls inside [0, m) (the cycle through k holds k itself, so the walk ends; it takes < 4 steps on
// average because 2^bits < 4m).
__device__ __forceinline__ unsigned feistel(unsigned k, unsigned m, const unsigned *key) {
    if (m <= 1) return 0;
    int bits = 32 - __clz(m - 1);
    bits += bits & 1;
    const int half = bits >> 1;
    const unsigned hm = (1u << half) - 1u;   // (half <= 16)
    unsigned x = k;
    do {
        unsigned L = x >> half, R = x & hm;
#pragma unroll
        for (int r = 0; r < kFeistelRounds; ++r) {
            const unsigned nl = R;
            R = L ^ (mix32(R ^ key[r]) & hm);
            L = nl;
        }
        x = (L << half) | R;
    } while (x >= m);
    return x;
}

__device__ __forceinline__ void feistel_keys(unsigned long long seed, int b, unsigned *key) {
    const unsigned s = mix32((unsigned)seed ^ mix32((unsigned)(seed >> 32) ^ mix32((unsigned)b * 0x9e3779b9u + 0x632be5abu)));
#pragma unroll
    for (int r = 0; r < kFeistelRounds; ++r) key[r] = mix32(s + (unsigned)(r + 1) * 0x85ebca6bu);
}

__global__ __launch_bounds__(kThreads) void prep_emit_kernel(const float *__restrict__ pts, int n, int C, const int *__restrict__ off, int B,
                                                             const float *__restrict__ prog, int K, int mode, unsigned long long seed,
                                                             const unsigned long long *__restrict__ mask, const int *__restrict__ base,
                                                             const int *__restrict__ inv, const int *__restrict__ out_off, float pad,
                                                             float *__restrict__ out) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int total = out_off[B];
    if (i >= total) {                                     // rows behind the kept points: pad in every column
        float *q = out + (size_t)i * C;
        for (int c = 0; c < C; ++c) q[c] = pad;
    }
    const unsigned long long bal = mask[(size_t)blockIdx.x * kWaves + (threadIdx.x >> 6)];
    const int lane = fnp_lane();
    if (!((bal >> lane) & 1ull)) return;
    const int b = scene_of_wave(off, B, i);
    const int pos = kept_before(mask, base, total, n, i);
    const int o = out_off[b], m = out_off[b + 1] - o, k = pos - o;
    if (k < 0 || k >= m) return;
    int slot;
    if (mode == FNP_SHUFFLE_DEVICE) {
        unsigned key[kFeistelRounds];
        feistel_keys(seed, b, key);
        slot = o + (int)feistel((unsigned)k, (unsigned)m, key);
    } else if (mode == FNP_SHUFFLE_EXPLICIT) {
        slot = inv[pos];
        if (slot < o || slot >= o + m) return;            // (not a permutation of the scene's kept rows: the row stays unwritten)
    } else {
        slot = pos;
    }
    const float *p = pts + (size_t)i * C;
    float x = p[0], y = p[1], z = p[2];
    if (prog) apply_program(prog + (size_t)b * K * 4, K, x, y, z);
    float *q = out + (size_t)slot * C;
    q[0] = x;
    q[1] = y;
    q[2] = z;
    for (int c = 3; c < C; ++c) q[c] = p[c];
}

}  // namespace

extern "C" int64_t fnp_prepare_points_workspace_bytes(int64_t n_points) {
    if (n_points < 0 || n_points > 0x7fffffffll) return FNP_ERR_ARG;
    PrepWs w;
    return carve(w, nullptr, n_points > 0 ? n_points : 1);
}

template <bool kCut>
static int prepare_points(const float *points, int64_t n_points, int num_features, const int *batch_offsets, int batch_size,
                          const float *program, int program_steps, CutArgs cut, double x_min, double y_min, double x_max, double y_max,
                          int shuffle_mode, const int *perm, int64_t n_perm, uint64_t seed, float pad,
                          void *workspace, int64_t workspace_bytes, float *out_points, int *out_offsets, fnp_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    if (n_points < 0 || n_points > 0x7fffffffll || num_features < 3 || batch_size <= 0 || !batch_offsets || !out_offsets) return FNP_ERR_ARG;
    if (program_steps < 0 || program_steps > FNP_PREP_MAX_STEPS || (program_steps > 0 && !program) || ((uintptr_t)program & 15)) return FNP_ERR_ARG;
    if (shuffle_mode != FNP_SHUFFLE_NONE && shuffle_mode != FNP_SHUFFLE_DEVICE && shuffle_mode != FNP_SHUFFLE_EXPLICIT) return FNP_ERR_ARG;
    if (shuffle_mode == FNP_SHUFFLE_EXPLICIT && (n_perm < 0 || (n_perm > 0 && !perm))) return FNP_ERR_ARG;
    if (kCut && (!cut.off || !cut.from || ((uintptr_t)cut.rec & 3))) return FNP_ERR_ARG;
    const int n = (int)n_points, B = batch_size, C = num_features;
    if (n == 0) {   // no rows: every scene keeps nothing
        return fnp_fill_words(out_offsets, (long long)B + 1, 0u, s);
    }
    if (!points || !workspace || !out_points) return FNP_ERR_ARG;
    PrepWs w;
    if (carve(w, (char *)workspace, n) > workspace_bytes) return FNP_ERR_WORKSPACE;
    const XyRange r{x_min, y_min, x_max, y_max};
    const float *prog = program_steps > 0 ? program : nullptr;
    const int G = fnp_divup(n, kThreads);

    hipLaunchKernelGGL(prep_mark_kernel<kCut>, dim3(G), dim3(kThreads), 0, s, points, n, C, batch_offsets, B, prog, program_steps, r, cut,
                       w.mask, w.cnt);
    FNP_LAUNCH_CHECK();
    int rc = fnp_scan::int32(w.cnt, G, w.base, w.total, w.scan_ws, s);
    if (rc) return rc;
    hipLaunchKernelGGL(prep_offsets_kernel, dim3(fnp_divup(B + 1, kThreads)), dim3(kThreads), 0, s, batch_offsets, B, n,
                       (const unsigned long long *)w.mask, (const int *)w.base, (const int *)w.total, out_offsets);
    FNP_LAUNCH_CHECK();
    if (shuffle_mode == FNP_SHUFFLE_EXPLICIT && n_perm > 0) {
        hipLaunchKernelGGL(prep_invert_kernel, dim3(fnp_grid_for(n_perm < n ? n_perm : n, kThreads)), dim3(kThreads), 0, s, perm, n_perm,
                           (const int *)out_offsets, B, w.inv);
        FNP_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(prep_emit_kernel, dim3(G), dim3(kThreads), 0, s, points, n, C, batch_offsets, B, prog, program_steps, shuffle_mode,
                       (unsigned long long)seed, (const unsigned long long *)w.mask, (const int *)w.base, (const int *)w.inv,
                       (const int *)out_offsets, pad, out_points);
    FNP_LAUNCH_CHECK();
    return FNP_OK;
}

extern "C" int fnp_prepare_points(const float *points, int64_t n_points, int num_features, const int *batch_offsets, int batch_size,
                                  const float *program, int program_steps, double x_min, double y_min, double x_max, double y_max,
                                  int shuffle_mode, const int *perm, int64_t n_perm, uint64_t seed, float pad,
                                  void *workspace, int64_t workspace_bytes, float *out_points, int *out_offsets, fnp_stream_t stream) {
    return prepare_points<false>(points, n_points, num_features, batch_offsets, batch_size, program, program_steps, CutArgs{},
                                 x_min, y_min, x_max, y_max, shuffle_mode, perm, n_perm, seed, pad, workspace, workspace_bytes,
                                 out_points, out_offsets, stream);
}

extern "C" int fnp_prepare_points_cut(const float *points, int64_t n_points, int num_features, const int *batch_offsets, int batch_size,
                                      const float *program, int program_steps, const float *cut_records, const int *cut_offsets,
                                      const int *cut_from, double x_min, double y_min, double x_max, double y_max,
                                      int shuffle_mode, const int *perm, int64_t n_perm, uint64_t seed, float pad,
                                      void *workspace, int64_t workspace_bytes, float *out_points, int *out_offsets, fnp_stream_t stream) {
    return prepare_points<true>(points, n_points, num_features, batch_offsets, batch_size, program, program_steps,
                                CutArgs{cut_records, cut_offsets, cut_from, nullptr}, x_min, y_min, x_max, y_max, shuffle_mode, perm,
                                n_perm, seed, pad, workspace, workspace_bytes, out_points, out_offsets, stream);
}

extern "C" int fnp_prepare_points_cut_window(const float *points, int64_t n_points, int num_features, const int *batch_offsets,
                                             int batch_size, const float *program, int program_steps, const float *cut_records,
                                             const int *cut_offsets, const int *cut_from, const int *cut_to, double x_min,
                                             double y_min, double x_max, double y_max, int shuffle_mode, const int *perm,
                                             int64_t n_perm, uint64_t seed, float pad, void *workspace, int64_t workspace_bytes,
                                             float *out_points, int *out_offsets, fnp_stream_t stream) {
    if (!cut_to) return FNP_ERR_ARG;
    return prepare_points<true>(points, n_points, num_features, batch_offsets, batch_size, program, program_steps,
                                CutArgs{cut_records, cut_offsets, cut_from, cut_to}, x_min, y_min, x_max, y_max, shuffle_mode, perm,
                                n_perm, seed, pad, workspace, workspace_bytes, out_points, out_offsets, stream);
}

// ---- host entry points of the cut (DataLoader workers: no device, no stream) ----
extern "C" int fnp_host_cut_records(const float *boxes, int m, float *records) {
    if (m < 0 || (m > 0 && (!boxes || !records))) return FNP_ERR_ARG;
    for (int j = 0; j < m; ++j) {
        const float *b = boxes + (size_t)j * 7;
        float *q = records + (size_t)j * 8;
        for (int c = 0; c < 6; ++c) q[c] = b[c];
        q[6] = cosf(-b[6]);
        q[7] = sinf(-b[6]);
    }
    return FNP_OK;
}

// remove_points_in_boxes3d's keep mask (points_in_boxes_cpu(...).sum(0) == 0) without the (M, N) matrix: a point leaves the box
// loop at its first box.  The prefilter |sx| > R or |sy| > R, R = 1.001 * (hx + hy) + 1e-3, drops no point the test keeps: for
// a point inside, the f32 rotation (l, two products and a sum, relative error < 2^-22 of |sx| + |sy|; c^2 + s^2 within 2^-22 of
// 1) bounds max(|sx|, |sy|) <= |(sx, sy)| < (hx + hy) * (1 + 1e-6).  A NaN passes the prefilter and fails the test.
extern "C" int fnp_host_points_outside_boxes(const float *points, int64_t n, int num_features, const float *records, int m,
                                             unsigned char *keep) {
    if (n < 0 || m < 0 || num_features < 3 || (n > 0 && (!points || !keep)) || (n > 0 && m > 0 && !records)) return FNP_ERR_ARG;
    std::vector<FnpCutBox> bx((size_t)m);
    std::vector<float> reach((size_t)m);
    for (int j = 0; j < m; ++j) {
        bx[j] = fnp_cut_box(records + (size_t)j * 8);
        reach[j] = (float)(1.001 * (bx[j].hx + bx[j].hy) + 1e-3);
    }
    for (int64_t i = 0; i < n; ++i) {
        const float *p = points + (size_t)i * num_features;
        const float x = p[0], y = p[1], z = p[2];
        bool inside = false;
        for (int j = 0; j < m && !inside; ++j) {
            const FnpCutBox &b = bx[j];
            if (fabsf(x - b.cx) > reach[j] || fabsf(y - b.cy) > reach[j]) continue;
            inside = fnp_cut_inside(b, x, y, z);
        }
        keep[i] = inside ? 0 : 1;
    }
    return FNP_OK;
}
