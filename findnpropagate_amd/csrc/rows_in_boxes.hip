// The rows of a batch that lie inside boxes, compact, on the device: fnp_host_points_in_boxes_compact (points_in_boxes.hip) for
// the scenes that fnp_assemble_sweeps leaves on the card, where unknowns_copy_paste feeds its queue from the rows inside the
// copy boxes of every scene (PseudoSampler.__call__, pcdet/datasets/augmentor/pseudo_loader.py:356-418).
//
// Box t of scene b (box_offsets) is tested against the rows [off[b], off[b+1]) of that scene only; a row inside it that the
// scene's pending cut would drop (boxcut.h, rows cut_from[b] <= i - off[b] < cut_to[b]) is left out.  Output order is the host's:
// box after box, rows in row order inside a box.  No atomics, so the order is fixed:
//   1. count : a workgroup per 256 rows reads them as 5120 contiguous bytes into LDS (the load_tile of sweeps.hip), then tests
//              its rows against the boxes of the scenes it touches, staged in LDS 64 at a time; a wave ballot per (box, wave),
//              one count per (box, workgroup) into cnt[t * G + g], box-major                              [rows_in_boxes<false>]
//   2. exclusive scan of cnt over all T * G entries                                                         [scan.hip]
//   3. counts[t] = base[(t + 1) * G] - base[t * G]                                                          [rib_counts]
//   4. emit  : the same tests where cnt[t * G + g] > 0 (most pairs are empty); a row's slot is base[t * G + g] plus the rows
//              inside in front of it in its workgroup (ballots of the earlier waves, popc of the earlier lanes); slots below
//              `capacity` receive the scene-relative row index and the raw row                              [rows_in_boxes<true>]
// The membership test is fnp_host_points_in_boxes_frame's, expression by expression (faces inclusive, half extents through
// fminf / fmaxf, the f32 rotation uncontracted), behind the host's conservative reach prefilter |x - cx| <= R, |y - cy| <= R,
// R = 1.001 * (|hx| + |hy|) + 1e-3, which drops no row that the test keeps (points_in_boxes.hip has the bound).
#include "boxcut.h"
#include "rankgrid.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kCols = 5;
constexpr int kTileWords = kThreads * kCols;   // 1280
constexpr int kTileChunks = kTileWords / 4;    // 320
constexpr int kBoxTile = 64;

struct RibBox {
    float cx, cy, cz, ca, sa;
    float x1, x2, y1, y2, z1, z2, reach;
    int scene;
};

struct RibCut {
    const float *records;   // (M, 8) or null
    const int *offsets;     // (B+1)
    const int *from, *to;   // (B)
    int m;
};

struct RibWs {
    int *cnt;    // (T * G) rows inside box t in workgroup g, box-major
    int *base;   // (T * G) exclusive scan
    void *scan_ws;
};

__host__ long long rib_align(long long v) { return (v + 255) & ~255ll; }

__host__ long long rib_carve(RibWs &w, char *p, long long n, long long t) {
    const long long G = (n + kThreads - 1) / kThreads, E = (t > 0 ? t : 1) * G;
    long long off = 0;
    auto take = [&](long long bytes) {
        char *q = p ? p + off : nullptr;
        off += rib_align(bytes);
        return q;
    };
    w.cnt = (int *)take(4 * E);
    w.base = (int *)take(4 * E);
    w.scan_ws = take(fnp_scan::workspace_bytes(E));
    return off;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the workgroup's rows [blk * 256, blk * 256 + 256) of points (n, 5), cut at row n, into tile; the caller synchronises
__device__ __forceinline__ void rib_load_tile(const float *__restrict__ pts, long long n, float *tile) {
    const long long w0 = (long long)blockIdx.x * kTileWords, wend = n * kCols;
    for (int c = threadIdx.x; c < kTileChunks; c += kThreads) {
        const long long w = w0 + 4 * c;
        if (w + 4 <= wend) {
            *reinterpret_cast<float4 *>(tile + 4 * c) = *reinterpret_cast<const float4 *>(pts + w);
        } else {
            for (int j = 0; j < 4; ++j)
                if (w + j < wend) tile[4 * c + j] = pts[w + j];
        }
    }
}

// the entry e of an offsets array (B+1 values, taken as non-decreasing) with off[e] <= i < off[e+1]; B where i lies in none
__device__ __forceinline__ int range_of(const int *__restrict__ off, int B, int i) {
    if (i >= off[B] || i < off[0]) return B;
    int lo = 0, hi = B;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ void stage_box(const float *__restrict__ rec, int scene, RibBox &o) {
    o.cx = rec[0];
    o.cy = rec[1];
    o.cz = rec[2];
    o.ca = rec[6];
    o.sa = rec[7];
    const float hx = rec[3] * 0.5f, hy = rec[4] * 0.5f, hz = rec[5] * 0.5f;
    o.x1 = fminf(hx, -hx);
    o.x2 = fmaxf(hx, -hx);
    o.y1 = fminf(hy, -hy);
    o.y2 = fmaxf(hy, -hy);
    o.z1 = fminf(hz, -hz);
    o.z2 = fmaxf(hz, -hz);
    o.reach = (float)(1.001 * ((double)fabsf(hx) + (double)fabsf(hy)) + 1e-3);
    o.scene = scene;
}

__device__ __forceinline__ bool row_in_box(const RibBox &b, float x, float y, float z) {
    if (!((fabsf(x - b.cx) <= b.reach) & (fabsf(y - b.cy) <= b.reach))) return false;
    const float px = x - b.cx, py = y - b.cy, pz = z - b.cz;
    const float rx = px * b.ca + py * (-b.sa), ry = px * b.sa + py * b.ca;
    return rx >= b.x1 && rx <= b.x2 && ry >= b.y1 && ry <= b.y2 && pz >= b.z1 && pz <= b.z2;
}

// is row `rel` of scene b, at (x, y, z), dropped by the scene's pending cut
__device__ bool row_is_cut(const RibCut &cut, int b, int rel, float x, float y, float z) {
    if (!cut.records) return false;
    int lo = cut.from[b];
    lo = lo < 0 ? 0 : lo;
    if (rel < lo || rel >= cut.to[b]) return false;
    const int j0 = clampi(cut.offsets[b], 0, cut.m), j1 = clampi(cut.offsets[b + 1], j0, cut.m);
    for (int j = j0; j < j1; ++j)
        if (fnp_cut_inside(fnp_cut_box(cut.records + (size_t)j * 8), x, y, z)) return true;
    return false;
}

template <bool kEmit>
__global__ __launch_bounds__(kThreads) void rows_in_boxes_kernel(const float *__restrict__ pts, int n, const int *__restrict__ off, int B,
                                                                 const float *__restrict__ records, const int *__restrict__ box_off, int T,
                                                                 RibCut cut, int G, int *__restrict__ cnt, const int *__restrict__ base,
                                                                 long long capacity, int *__restrict__ indices, float *__restrict__ rows) {
    __shared__ __attribute__((aligned(16))) float tile[kTileWords];
    __shared__ RibBox boxes[kBoxTile];
    __shared__ int wcnt[kWaves][kBoxTile];   // count pass: rows inside per (wave, staged box)
    __shared__ int wsum[2][kWaves];          // emit pass: the waves' ballot counts of one box, double-buffered
    const int g = blockIdx.x;
    const int i0 = g * kThreads, i = i0 + threadIdx.x;
    const int last = min(i0 + kThreads, n) - 1;
    // the scenes this workgroup's rows belong to, and their boxes [t_lo, t_hi)
    const int b_lo = range_of(off, B, i0), b_hi = range_of(off, B, last);
    const int t_lo = b_lo >= B ? T : clampi(box_off[b_lo], 0, T);
    const int t_hi = b_lo >= B ? T : clampi(box_off[b_hi >= B ? B : b_hi + 1], t_lo, T);
    if (!kEmit) {   // every other box holds none of these rows
        for (int t = threadIdx.x; t < T; t += kThreads)
            if (t < t_lo || t >= t_hi) cnt[(size_t)t * G + g] = 0;
    }
    if (t_lo >= t_hi) return;
    rib_load_tile(pts, n, tile);
    const int b = i < n ? range_of(off, B, i) : B;
    const int rel = b < B ? i - off[b] : 0;
    const int wave = threadIdx.x >> 6, lane = fnp_lane();
    int cut_state = 0;   // 0 untested, 1 kept, 2 cut
    int par = 0;
    for (int t0 = t_lo; t0 < t_hi; t0 += kBoxTile) {
        const int nt = min(kBoxTile, t_hi - t0);
        __syncthreads();   // (the tile on the first round; the staged boxes and wcnt of the round before)
        if (threadIdx.x < nt) stage_box(records + (size_t)(t0 + threadIdx.x) * 8, range_of(box_off, B, t0 + threadIdx.x), boxes[threadIdx.x]);
        __syncthreads();
        const float x = tile[threadIdx.x * kCols], y = tile[threadIdx.x * kCols + 1], z = tile[threadIdx.x * kCols + 2];
        for (int k = 0; k < nt; ++k) {
            int slot0 = 0;
            if (kEmit) {
                if (cnt[(size_t)(t0 + k) * G + g] == 0) continue;   // (the whole workgroup)
                slot0 = base[(size_t)(t0 + k) * G + g];
            }
            bool in = b < B && boxes[k].scene == b && row_in_box(boxes[k], x, y, z);
            if (in) {
                if (!cut_state) cut_state = row_is_cut(cut, b, rel, x, y, z) ? 2 : 1;
                in = cut_state == 1;
            }
            const unsigned long long bal = __ballot(in);
            if (!kEmit) {
                if (lane == 0) wcnt[wave][k] = __popcll(bal);
            } else {
                if (lane == 0) wsum[par][wave] = __popcll(bal);
                __syncthreads();
                int slot = slot0 + __popcll(bal & ((1ull << lane) - 1ull));
                for (int w = 0; w < wave; ++w) slot += wsum[par][w];
                par ^= 1;
                if (in && slot >= 0 && slot < capacity) {
                    indices[slot] = rel;
                    float *q = rows + (size_t)slot * kCols;
                    const float *p = tile + threadIdx.x * kCols;
                    for (int c = 0; c < kCols; ++c) q[c] = p[c];
                }
            }
        }
        if (!kEmit) {
            __syncthreads();
            if (threadIdx.x < nt)
                cnt[(size_t)(t0 + threadIdx.x) * G + g] = wcnt[0][threadIdx.x] + wcnt[1][threadIdx.x] + wcnt[2][threadIdx.x] + wcnt[3][threadIdx.x];
        }
    }
}

__global__ __launch_bounds__(kThreads) void rib_counts_kernel(const int *__restrict__ base, const int *__restrict__ total, int T, int G,
                                                              int *__restrict__ counts) {
    const int t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= T) return;
    const int hi = t + 1 < T ? base[(size_t)(t + 1) * G] : *total;
    counts[t] = hi - base[(size_t)t * G];
}

}  // namespace

extern "C" int64_t fnp_rows_in_boxes_workspace_bytes(int64_t n_points, int num_boxes) {
    if (n_points < 0 || n_points > 0x7fffffffll || num_boxes < 0) return FNP_ERR_ARG;
    const long long n = n_points > 0 ? n_points : 1, G = (n + kThreads - 1) / kThreads;
    if ((long long)(num_boxes > 0 ? num_boxes : 1) * G > 0x7fffffffll) return FNP_ERR_ARG;
    RibWs w;
    return rib_carve(w, nullptr, n, num_boxes);
}

extern "C" int fnp_rows_in_boxes(const float *points, int64_t n_points, int num_features, const int *batch_offsets, int batch_size,
                                 const float *box_records, int num_boxes, const int *box_offsets, const float *cut_records,
                                 int num_cut_records, const int *cut_offsets, const int *cut_from, const int *cut_to, int64_t capacity,
                                 void *workspace, int64_t workspace_bytes, int *counts, int *total, int *indices, float *rows,
                                 fnp_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    if (n_points < 0 || n_points > 0x7fffffffll || num_features != kCols || batch_size <= 0 || num_boxes < 0 || num_cut_records < 0 ||
        capacity < 0 || !total)
        return FNP_ERR_ARG;
    if ((num_boxes > 0 && !counts) || (capacity > 0 && (!indices || !rows))) return FNP_ERR_ARG;
    if (num_cut_records > 0 && (!cut_records || !cut_offsets || !cut_from || !cut_to)) return FNP_ERR_ARG;
    const int n = (int)n_points, T = num_boxes, B = batch_size;
    if (n == 0 || T == 0) {   // nothing inside anything
        if (T > 0) {
            const int rc = fnp_fill_words(counts, T, 0u, s);
            if (rc) return rc;
        }
        return fnp_fill_words(total, 1, 0u, s);
    }
    if (!points || !batch_offsets || !box_records || !box_offsets || !workspace) return FNP_ERR_ARG;
    if ((uintptr_t)points & 15) return FNP_ERR_ARG;   // (the tile load reads 16 bytes per lane)
    const int G = fnp_divup(n, kThreads);
    if ((long long)T * G > 0x7fffffffll) return FNP_ERR_ARG;
    RibWs w;
    if (rib_carve(w, (char *)workspace, n, T) > workspace_bytes) return FNP_ERR_WORKSPACE;
    const RibCut cut{num_cut_records > 0 ? cut_records : nullptr, cut_offsets, cut_from, cut_to, num_cut_records};

    hipLaunchKernelGGL(rows_in_boxes_kernel<false>, dim3(G), dim3(kThreads), 0, s, points, n, batch_offsets, B, box_records, box_offsets, T,
                       cut, G, w.cnt, (const int *)nullptr, (long long)0, (int *)nullptr, (float *)nullptr);
    FNP_LAUNCH_CHECK();
    const int rc = fnp_scan::int32(w.cnt, (long long)T * G, w.base, total, w.scan_ws, s);
    if (rc) return rc;
    hipLaunchKernelGGL(rib_counts_kernel, dim3(fnp_divup(T, kThreads)), dim3(kThreads), 0, s, (const int *)w.base, (const int *)total, T, G,
                       counts);
    FNP_LAUNCH_CHECK();
    if (capacity > 0) {
        hipLaunchKernelGGL(rows_in_boxes_kernel<true>, dim3(G), dim3(kThreads), 0, s, points, n, batch_offsets, B, box_records, box_offsets,
                           T, cut, G, w.cnt, (const int *)w.base, (long long)capacity, indices, rows);
        FNP_LAUNCH_CHECK();
    }
    return FNP_OK;
}
