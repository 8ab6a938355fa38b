// Multi-sweep assembly in front of fnp_prepare_points: NuScenesDataset.get_lidar_with_sweeps / get_sweep
// (pcdet/datasets/nuscenes/nuscenes_dataset.py:88-121) for a batch of scenes, from the rows of the sweep files as they lie on
// disk to the (x, y, z, intensity, time lag) rows the rest of the device chain reads.  The reference runs these steps in numpy
// inside DataLoader workers: drop a sweep's ego returns, move the sweep into the key frame by a 4x4 matrix in f64, append the
// time-lag column, concatenate.
//
//   1. mark : a thread per raw row finds its sweep (a search over sweep_offsets, once per wave where the wave lies in one
//             sweep) and tests the ego square on the raw f32 x, y; a wave ballot per 64 rows, a kept count per workgroup of
//             256 rows                                                                                      [sweeps_mark]
//   2. exclusive scan of the workgroup counts                                                               [scan.hip]
//   3. per scene: the kept rows in front of its first sweep's first row = its offset                        [sweeps_offsets]
//   4. emit : every kept row recomputes its transform and writes its row to its slot (the kept rows in front of it: a
//             stable compaction over the whole batch is one per scene, scene after scene); rows [kept, R) get the pad value
//                                                                                                           [sweeps_emit]
// No atomics, no host synchronisation; every row count is read from device memory.
//
// fnp_assemble_sweeps_window runs the same four launches on the <true> instantiations of the three kernels: a sweep flagged
// SWEEP_FINISHED (gt_sampling's object rows in front of a scene, unknowns_copy_paste's pasted rows behind it) keeps every row and
// leaves as it came, five columns bit for bit; sweeps_offsets also counts, per scene, the kept rows in front of the first and the
// end row of the scene's cut window — the cut_from / cut_to of fnp_prepare_points_cut_window, which the host cannot know once the
// ego returns are dropped here.  fnp_assemble_sweeps keeps the <false> instantiations: the code it had.
//
// ROWS OF 20 BYTES.  A thread that loads its own row issues dword loads 20 bytes apart: five instructions that each touch ten
// 128-byte lines.  Both passes instead read the workgroup's 256 rows as what they are, 5120 contiguous bytes, 16 bytes per lane
// (320 chunks, 16-byte aligned because the base is and 5120 is a multiple of 16), into LDS; a thread then reads its row at a
// stride of five words, odd, so the 32 lanes of a half-wave fall on 32 different banks.  The mark needs x and y only (8 of the
// row's 20 bytes: the algorithmic count is R x 28 B read over both passes) but requests the whole row like the emit (R x 40 B):
// the lines that hold x and y hold the rest of the row too, so memory moves the same either way.  The kept rows leave as five dword stores per lane to consecutive rows.
//
// The mask / count / kept_before helpers restate those of prep.hip (which stays as it is: its kernels are the measured ones).
#include "rankgrid.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kCols = 5;                          // a raw row: x, y, z, intensity, ring index
constexpr int kTileWords = kThreads * kCols;      // 1280
constexpr int kTileChunks = kTileWords / 4;       // 320

enum { SWEEP_DROP_EGO = 1, SWEEP_TRANSFORM = 2, SWEEP_FINISHED = 4 };

struct SweepWs {
    unsigned long long *mask;   // (G*4) ballot of kept rows per wave
    int *cnt;                   // (G)   kept rows per workgroup
    int *base;                  // (G)   exclusive scan of cnt
    int *total;                 // (1)
    void *scan_ws;
};

__host__ long long align_up(long long v) { return (v + 255) & ~255ll; }

__host__ long long carve(SweepWs &w, char *p, long long n) {
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
    w.scan_ws = take(fnp_scan::workspace_bytes(G));
    return off;
}

// the workgroup's rows [blk * 256, blk * 256 + 256) of raw (n, 5), cut at row n, into tile (1280 words); the caller synchronises
__device__ __forceinline__ void load_tile(const float *__restrict__ raw, long long n, float *tile) {
    const long long w0 = (long long)blockIdx.x * kTileWords, wend = n * kCols;
    for (int c = threadIdx.x; c < kTileChunks; c += kThreads) {
        const long long w = w0 + 4 * c;
        if (w + 4 <= wend) {
            *reinterpret_cast<float4 *>(tile + 4 * c) = *reinterpret_cast<const float4 *>(raw + w);
        } else {
            for (int j = 0; j < 4; ++j)
                if (w + j < wend) tile[4 * c + j] = raw[w + j];
        }
    }
}

__device__ __forceinline__ int sweep_of(const int *__restrict__ off, int T, int i) {
    int lo = 0, hi = T;   // off[lo] <= i < off[hi]; an empty sweep is never the answer
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// sweep of row i (searched once per wave for its first live lane, per lane where the wave crosses a sweep border)
__device__ __forceinline__ int sweep_of_wave(const int *__restrict__ off, int T, int i) {
    const int i0 = __builtin_amdgcn_readfirstlane(i);
    int t = sweep_of(off, T, i0);
    if (t + 1 < T && i >= off[t + 1]) t = sweep_of(off, T, i);
    return t;
}

// remove_ego_points: both comparisons strict, on the raw f32 values against the f64 radius
__device__ __forceinline__ bool ego_return(float x, float y, double r) { return fabs((double)x) < r && fabs((double)y) < r; }

// kFinished (fnp_assemble_sweeps_window): a sweep with SWEEP_FINISHED holds finished rows, which are never ego returns
template <bool kFinished>
__global__ __launch_bounds__(kThreads) void sweeps_mark_kernel(const float *__restrict__ raw, int n, const int *__restrict__ off, int T,
                                                               const int *__restrict__ flags, double radius,
                                                               unsigned long long *__restrict__ mask, int *__restrict__ cnt) {
    __shared__ __attribute__((aligned(16))) float tile[kTileWords];
    __shared__ int wcnt[kWaves];
    load_tile(raw, n, tile);
    __syncthreads();
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    bool keep = false;
    if (i < n && i >= off[0] && i < off[T]) {
        const int t = sweep_of_wave(off, T, (int)i);
        const int f = flags[t];
        const bool drop = (f & SWEEP_DROP_EGO) && !(kFinished && (f & SWEEP_FINISHED));
        keep = !(drop && ego_return(tile[threadIdx.x * kCols], tile[threadIdx.x * kCols + 1], radius));
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

// kept rows in front of row i (i <= n): the workgroup base plus the ballots of the earlier waves and lanes
__device__ __forceinline__ int kept_before(const unsigned long long *__restrict__ mask, const int *__restrict__ base, int total, int n, int i) {
    if (i >= n) return total;
    const int blk = i / kThreads, w = (i % kThreads) >> 6, lane = i & 63;
    int k = base[blk];
    for (int j = 0; j < w; ++j) k += __popcll(mask[(size_t)blk * kWaves + j]);
    return k + __popcll(mask[(size_t)blk * kWaves + w] & ((1ull << lane) - 1ull));
}

// scene offsets: o_b = kept rows in front of the first row of scene b's first sweep (thread per entry; o_B = every kept row).
// kWindow: also out_window[b] = {kept rows of scene b in front of the first row of sweep window_sweeps[b][0], in front of the first
// row of sweep window_sweeps[b][1]}, both sweep indices clamped into the scene's own sweep range, both counts relative to o_b.
template <bool kWindow>
__global__ __launch_bounds__(kThreads) void sweeps_offsets_kernel(const int *__restrict__ off, int T, const int *__restrict__ scene_sweeps, int B,
                                                                  int n, const unsigned long long *__restrict__ mask,
                                                                  const int *__restrict__ base, const int *__restrict__ total,
                                                                  int *__restrict__ out_off, const int *__restrict__ window_sweeps,
                                                                  int *__restrict__ out_window) {
    const int b = blockIdx.x * kThreads + threadIdx.x;
    if (b > B) return;
    const int tot = *total;
    int t = scene_sweeps[b];
    t = t < 0 ? 0 : (t > T ? T : t);
    int i = off[t];
    i = i < 0 ? 0 : i;
    const int o = b == B ? tot : kept_before(mask, base, tot, n, i);
    out_off[b] = o;
    if (kWindow && b < B) {
        int t1 = scene_sweeps[b + 1];
        t1 = t1 < t ? t : (t1 > T ? T : t1);
        for (int k = 0; k < 2; ++k) {
            int w = window_sweeps[2 * b + k];
            w = w < t ? t : (w > t1 ? t1 : w);
            int j = off[w];
            j = j < i ? i : j;
            out_window[2 * b + k] = kept_before(mask, base, tot, n, j) - o;
        }
    }
}

// One output coordinate of get_sweep's transform_matrix.dot(vstack((xyz, ones))), stored into the f32 array: x, y, z widened to
// f64, the row's four terms accumulated in order as BLAS's dgemm does it on an FMA machine (numpy hands the (4, 4) x (4, n)
// product to OpenBLAS, whose kernels keep one accumulator per output element and fuse every step):
//   fma(m3, 1, fma(m2, z, fma(m1, y, m0 * x)))  =  fma(m2, z, fma(m1, y, m0 * x)) + m3,    rounded to f32 once.
// Checked against numpy on 692 k coordinates of synthetic.make_raw_sweeps: every f64 value equal bit for bit.  The unfused
// chain ((m0*x + m1*y) + m2*z) + m3 differs from it in the last f64 bit of one value in six, which the rounding to f32 hides
// except where the sum cancels (a return brought back to x = 1e-9 of the key frame: 10 f32 values of those 692 k).
__device__ __forceinline__ float xform_row(const double *__restrict__ m, double x, double y, double z) {
    const double s = __dadd_rn(__fma_rn(m[2], z, __fma_rn(m[1], y, __dmul_rn(m[0], x))), m[3]);
    return __double2float_rn(s);
}

// kFinished: a sweep with SWEEP_FINISHED leaves as it came, all five columns bit for bit (no transform, its own column 4)
template <bool kFinished>
__global__ __launch_bounds__(kThreads) void sweeps_emit_kernel(const float *__restrict__ raw, int n, const int *__restrict__ off, int T,
                                                               const double *__restrict__ xform, const int *__restrict__ flags,
                                                               const float *__restrict__ time_lag, const unsigned long long *__restrict__ mask,
                                                               const int *__restrict__ cnt, const int *__restrict__ base,
                                                               const int *__restrict__ total_p, float pad, float *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) float tile[kTileWords];
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    const int total = *total_p;
    if (i < n && i >= total) {                            // rows behind the kept rows: pad in every column
        float *q = out + (size_t)i * kCols;
        for (int c = 0; c < kCols; ++c) q[c] = pad;
    }
    if (cnt[blockIdx.x] == 0) return;                     // (the whole workgroup: nothing kept here, nothing to read)
    load_tile(raw, n, tile);
    __syncthreads();
    const unsigned long long bal = mask[(size_t)blockIdx.x * kWaves + (threadIdx.x >> 6)];
    if (!((bal >> fnp_lane()) & 1ull)) return;            // (a kept row has i < n and lies in a sweep)
    const int t = sweep_of_wave(off, T, (int)i);
    const int slot = kept_before(mask, base, total, n, (int)i);
    if (slot < 0 || slot >= total) return;
    const float *p = tile + threadIdx.x * kCols;
    float *q = out + (size_t)slot * kCols;
    if (kFinished && (flags[t] & SWEEP_FINISHED)) {
        for (int c = 0; c < kCols; ++c) q[c] = p[c];
        return;
    }
    float x = p[0], y = p[1], z = p[2];
    if (flags[t] & SWEEP_TRANSFORM) {                     // (never an identity for "no matrix": 1*x + 0 + 0 + 0 loses the sign of -0.0)
        const double *m = xform + (size_t)t * 12;
        const double dx = x, dy = y, dz = z;
        x = xform_row(m, dx, dy, dz);
        y = xform_row(m + 4, dx, dy, dz);
        z = xform_row(m + 8, dx, dy, dz);
    }
    q[0] = x;
    q[1] = y;
    q[2] = z;
    q[3] = p[3];
    q[4] = time_lag[t];
}

}  // namespace

extern "C" int64_t fnp_assemble_sweeps_workspace_bytes(int64_t n_rows) {
    if (n_rows < 0 || n_rows > 0x7fffffffll) return FNP_ERR_ARG;
    SweepWs w;
    return carve(w, nullptr, n_rows > 0 ? n_rows : 1);
}

namespace {

template <bool kWindow>
int assemble(const float *raw, int64_t n_rows, const int *sweep_offsets, int num_sweeps, const int *scene_sweeps, int batch_size,
             const double *xform, const int *flags, const float *time_lag, double center_radius, float pad, void *workspace,
             int64_t workspace_bytes, float *out_points, int *out_offsets, const int *window_sweeps, int *out_window, hipStream_t s) {
    if (n_rows < 0 || n_rows > 0x7fffffffll || num_sweeps < 0 || batch_size <= 0 || !scene_sweeps || !out_offsets) return FNP_ERR_ARG;
    if (kWindow && (!window_sweeps || !out_window)) return FNP_ERR_ARG;
    const int n = (int)n_rows, B = batch_size, T = num_sweeps;
    if (n == 0) {   // no rows: every scene keeps nothing
        if (kWindow) {
            const int rc = fnp_fill_words(out_window, 2ll * B, 0u, s);
            if (rc) return rc;
        }
        return fnp_fill_words(out_offsets, (long long)B + 1, 0u, s);
    }
    if (!raw || !sweep_offsets || !workspace || !out_points) return FNP_ERR_ARG;
    if (T > 0 && (!xform || !flags || !time_lag)) return FNP_ERR_ARG;
    if (((uintptr_t)raw & 15) || ((uintptr_t)xform & 7)) return FNP_ERR_ARG;   // (load_tile reads 16 bytes per lane)
    SweepWs w;
    if (carve(w, (char *)workspace, n) > workspace_bytes) return FNP_ERR_WORKSPACE;
    const int G = fnp_divup(n, kThreads);

    hipLaunchKernelGGL(sweeps_mark_kernel<kWindow>, dim3(G), dim3(kThreads), 0, s, raw, n, sweep_offsets, T, flags, center_radius, w.mask,
                       w.cnt);
    FNP_LAUNCH_CHECK();
    int rc = fnp_scan::int32(w.cnt, G, w.base, w.total, w.scan_ws, s);
    if (rc) return rc;
    hipLaunchKernelGGL(sweeps_offsets_kernel<kWindow>, dim3(fnp_divup(B + 1, kThreads)), dim3(kThreads), 0, s, sweep_offsets, T, scene_sweeps,
                       B, n, (const unsigned long long *)w.mask, (const int *)w.base, (const int *)w.total, out_offsets, window_sweeps,
                       out_window);
    FNP_LAUNCH_CHECK();
    hipLaunchKernelGGL(sweeps_emit_kernel<kWindow>, dim3(G), dim3(kThreads), 0, s, raw, n, sweep_offsets, T, xform, flags, time_lag,
                       (const unsigned long long *)w.mask, (const int *)w.cnt, (const int *)w.base, (const int *)w.total, pad, out_points);
    FNP_LAUNCH_CHECK();
    return FNP_OK;
}

}  // namespace

extern "C" int fnp_assemble_sweeps(const float *raw, int64_t n_rows, const int *sweep_offsets, int num_sweeps, const int *scene_sweeps,
                                   int batch_size, const double *xform, const int *flags, const float *time_lag, double center_radius,
                                   float pad, void *workspace, int64_t workspace_bytes, float *out_points, int *out_offsets,
                                   fnp_stream_t stream) {
    return assemble<false>(raw, n_rows, sweep_offsets, num_sweeps, scene_sweeps, batch_size, xform, flags, time_lag, center_radius, pad,
                           workspace, workspace_bytes, out_points, out_offsets, nullptr, nullptr, (hipStream_t)stream);
}

// fnp_assemble_sweeps with finished-row sweeps (FNP_SWEEP_FINISHED) and a cut window per scene: the same four launches
extern "C" int fnp_assemble_sweeps_window(const float *raw, int64_t n_rows, const int *sweep_offsets, int num_sweeps,
                                          const int *scene_sweeps, int batch_size, const double *xform, const int *flags,
                                          const float *time_lag, double center_radius, float pad, void *workspace,
                                          int64_t workspace_bytes, float *out_points, int *out_offsets, const int *window_sweeps,
                                          int *out_window, fnp_stream_t stream) {
    return assemble<true>(raw, n_rows, sweep_offsets, num_sweeps, scene_sweeps, batch_size, xform, flags, time_lag, center_radius, pad,
                          workspace, workspace_bytes, out_points, out_offsets, window_sweeps, out_window, (hipStream_t)stream);
}
