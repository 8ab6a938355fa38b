// BatchNorm2d in TRAINING mode + ReLU on rows that stand for a dense map: the tail of the first BaseBEVBackbone block
// (pcdet/models/backbones_2d/base_bev_backbone.py:31-40: ZeroPad2d, Conv2d(256 -> 128, 3x3, no bias), BatchNorm2d, ReLU) when the
// convolution ran on the sparse rows.  x (cap, C) holds the convolution's output on its n output sites coords [b, 0, y, x]; every
// other of the N = B * H * W cells holds the exact zero of a bias-free convolution with nothing in reach.  The batch statistics
// run over all N cells, so the zeros count:
//
//   forward :  mean = sum_r x / N,  var = sum_r x^2 / N - mean^2 (biased, f64),  invstd = 1 / sqrt(var + eps),
//              running_mean / running_var updated like torch (momentum, var * N / (N - 1)),
//              fill_c = relu((0 - mean) * invstd * gamma + beta)                     the value of a cell without a row,
//              y (B, C, H, W) = relu((x - mean) * invstd * gamma + beta) at the row cells, fill_c elsewhere, written ONCE
//   backward:  g = G * [y > 0] at the row cells (y recomputed from x by the forward's own f32 sequence and rounded to the map's
//              dtype: the bits the forward stored), [fill_c > 0] at the others;  T = sum_cells G,  R = sum_row cells G,
//              dbeta = sum_rows g + [fill > 0] (T - R),  dgamma = sum_rows g xhat + [fill > 0] xhat_bg (T - R),
//              xhat_bg = (0 - mean) * invstd,  dx_r = gamma * invstd * (g_r - dbeta / N - xhat_r * dgamma / N),  0 for r >= n
//
// Launches.  Forward, 5: clear of the cell -> row map, the map, row statistics, finish, apply-and-write (dense_tile.h's tiling:
// the rows of a tile's occupied cells go to LDS raw, every wave then normalises and writes channel plane by channel plane; the
// normalised rows are never stored on their own).  Backward, 6: clear, map, plane sums of G (one workgroup per (b, c) plane,
// coalesced), row-cell pass (the tiles' G values gathered through LDS as fnp_sparse_to_dense_backward does; it adds the three row
// sums and parks the gathered G rows in dx), finish, apply (dx in place).  G is read twice (plane pass; the gather touches only
// the sectors of occupied cells), x twice per direction.
// The house rules of bnorm.hip: every sum in f64 through per-workgroup partials that a finishing launch adds in a fixed order,
// no atomics, bit-identical from run to run; the row count is read on the device; no allocation, no host synchronisation.
// coords must lie in the grid and be unique per site (what a rulebook's output sites are); anything else is memory-safe only.
#include "common.h"
#include "dense_tile.h"
#include "rowvec.h"

namespace {

constexpr int kThreads = kDenseThreads;
constexpr int kStatParts = 256;   // workgroups of the row statistics pass (as bnorm.hip)
constexpr int kCellParts = 512;   // workgroups of the backward's row-cell pass (each walks tiles wg, wg + grid, ...)
constexpr int kFinC = 16;         // channels per finishing workgroup
constexpr int kSlots = kDenseSlots;

// THE f32 sequence of a map element; fill is this with x = 0, the backward's mask this rounded to the map's dtype
__device__ __forceinline__ float bev_apply(float x, float mean, float invstd, float gamma, float beta) {
    float v = (x - mean) * invstd * gamma + beta;
    if (v < 0.f) v = 0.f;
    return v;
}

// ---------------------------------------------------------------------------------------------------------------- forward
// part[(wg * C + c) * 2 + {0, 1}] = sum x, sum x^2 over the workgroup's contiguous row range
template <typename T>
__global__ __launch_bounds__(kThreads) void bev_stats_kernel(const T *__restrict__ x, const int *__restrict__ n_rows, int cap, int C,
                                                             double *__restrict__ part) {
    __shared__ double red[kThreads][16];
    const int n = min(*n_rows, cap);
    const int tpr = C / 8, rows_per_iter = kThreads / tpr;      // (tpr a power of two <= 32)
    const int cg = threadIdx.x % tpr, rl = threadIdx.x / tpr;
    double sa[8], sb[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) sa[j] = sb[j] = 0.0;
    const long long per = ((long long)n + gridDim.x - 1) / gridDim.x;
    const long long r0 = per * blockIdx.x, r1 = min((long long)n, r0 + per);
    constexpr int U = 4;
    for (long long r = r0 + rl; r < r1; r += (long long)U * rows_per_iter) {
        float xv[U][8];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long long ru = r + (long long)u * rows_per_iter;
            if (ru < r1) load8(x + (size_t)ru * C + cg * 8, xv[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long long ru = r + (long long)u * rows_per_iter;
            if (ru >= r1) break;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                sa[j] += (double)xv[u][j];
                sb[j] += (double)xv[u][j] * (double)xv[u][j];
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        red[threadIdx.x][j] = sa[j];
        red[threadIdx.x][8 + j] = sb[j];
    }
    __syncthreads();
    for (int slot = threadIdx.x; slot < tpr * 16; slot += kThreads) {   // thread lines in thread order: a fixed order
        const int g = slot >> 4, j = slot & 15;
        double v = 0.0;
        for (int q = 0; q < rows_per_iter; ++q) v += red[q * tpr + g][j];
        part[((size_t)blockIdx.x * C + g * 8 + (j & 7)) * 2 + (j >> 3)] = v;
    }
}

// NS sums per channel, `parts` partials laid out [p][c][NS]: thread (slice, c) adds p = slice, slice + S, ..., the slices meet
// in an LDS tree.  The result is valid in the threads of slice 0.
template <int NS>
__device__ __forceinline__ void finish_sums(const double *__restrict__ part, int parts, int C, int c, int CW, double (&v)[NS],
                                            double (*red)[kThreads]) {
    const int S = kThreads / CW, slice = threadIdx.x / CW;
#pragma unroll
    for (int j = 0; j < NS; ++j) v[j] = 0.0;
    for (int p = slice; p < parts; p += S) {
#pragma unroll
        for (int j = 0; j < NS; ++j) v[j] += part[((size_t)p * C + c) * NS + j];
    }
#pragma unroll
    for (int j = 0; j < NS; ++j) red[j][threadIdx.x] = v[j];
    __syncthreads();
    for (int s = S / 2; s > 0; s >>= 1) {
        if (slice < s) {
#pragma unroll
            for (int j = 0; j < NS; ++j) red[j][threadIdx.x] += red[j][threadIdx.x + s * CW];
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < NS; ++j) v[j] = red[j][threadIdx.x];
}

__global__ __launch_bounds__(kThreads) void bev_finish_forward_kernel(const double *__restrict__ part, int parts, int C, long long N,
                                                                      float eps, float momentum, const float *__restrict__ gamma,
                                                                      const float *__restrict__ beta, float *__restrict__ save_mean,
                                                                      float *__restrict__ save_invstd, float *__restrict__ fill,
                                                                      float *__restrict__ running_mean, float *__restrict__ running_var,
                                                                      long long *__restrict__ batches_tracked) {
    if (batches_tracked && blockIdx.x == 0 && threadIdx.x == 0) *batches_tracked += 1;
    __shared__ double red[2][kThreads];
    const int CW = C < kFinC ? C : kFinC;
    const int c = blockIdx.x * CW + threadIdx.x % CW;
    double v[2];
    finish_sums<2>(part, parts, C, c, CW, v, red);
    if (threadIdx.x < CW) {
        const double m = v[0] / (double)N;
        double var = v[1] / (double)N - m * m;
        if (var < 0.0) var = 0.0;
        const float mf = (float)m, isf = (float)(1.0 / sqrt(var + (double)eps));
        save_mean[c] = mf;
        save_invstd[c] = isf;
        fill[c] = bev_apply(0.f, mf, isf, gamma[c], beta[c]);
        if (running_mean) {
            const double unb = N > 1 ? var * ((double)N / (double)(N - 1)) : var;
            running_mean[c] = (float)((1.0 - (double)momentum) * (double)running_mean[c] + (double)momentum * m);
            running_var[c] = (float)((1.0 - (double)momentum) * (double)running_var[c] + (double)momentum * unb);
        }
    }
}

// dense_write_kernel of dense.hip with D = 1 and the normalisation between the LDS slot and the store
template <typename T, int VEC>
__global__ __launch_bounds__(kThreads) void bev_write_kernel(const T *__restrict__ x, const int *__restrict__ index, int C,
                                                             long long plane, int tiles_per_plane, const float *__restrict__ mean,
                                                             const float *__restrict__ invstd, const float *__restrict__ gamma,
                                                             const float *__restrict__ beta, const float *__restrict__ fill,
                                                             T *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char fnp_bev_smem[];
    typedef T TVec __attribute__((ext_vector_type(VEC)));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long tile = blockIdx.x;
    const long long b = tile / tiles_per_plane;
    const long long l0 = (tile % tiles_per_plane) * (64 * VEC);
    const bool in = l0 + (long long)VEC * lane < plane;          // (plane % VEC == 0: all of the lane's cells or none)
    int r[VEC];
    fnp_dense_tile_rows<VEC>(index, b * plane + l0 + (long long)VEC * lane, in, r);
    unsigned long long occ[VEC];                                  // same in all four waves
    int total = 0;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        occ[j] = __ballot(r[j] >= 0);
        total += __popcll(occ[j]);
    }
    const int row_bytes = C * (int)sizeof(T), stride = row_bytes + 4;
    T *o = out + b * C * plane + l0 + (long long)VEC * lane;      // channel c adds c * plane
    const unsigned long long below = (1ull << lane) - 1ull;

    if (total == 0) {
        if (!in) return;
        for (int c = wave; c < C; c += 4) {
            const T bg = (T)fill[c];
            TVec v;
#pragma unroll
            for (int j = 0; j < VEC; ++j) v[j] = bg;
            *reinterpret_cast<TVec *>(o + c * plane) = v;
        }
    } else if (total <= kSlots) {
        int first = 0, myslot[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            myslot[j] = first + __popcll(occ[j] & below);
            first = fnp_dense_stage_rows(fnp_bev_smem, x, row_bytes, stride, occ[j], r[j], first, lane, wave);
        }
        __syncthreads();
        if (!in) return;
        for (int c = wave; c < C; c += 4) {
            const float mu = mean[c], is = invstd[c], ga = gamma[c], be = beta[c];
            const T bg = (T)fill[c];
            TVec v;
#pragma unroll
            for (int j = 0; j < VEC; ++j)
                v[j] = ((occ[j] >> lane) & 1ull)
                           ? (T)bev_apply((float)reinterpret_cast<const T *>(fnp_bev_smem + myslot[j] * stride)[c], mu, is, ga, be)
                           : bg;
            *reinterpret_cast<TVec *>(o + c * plane) = v;
        }
    } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j) {   // (workgroup-uniform path: the barriers match)
            fnp_dense_stage_rows(fnp_bev_smem, x, row_bytes, stride, occ[j], r[j], 0, lane, wave);
            __syncthreads();
            if (in) {
                const bool has = (occ[j] >> lane) & 1ull;
                const T *mine = reinterpret_cast<const T *>(fnp_bev_smem + __popcll(occ[j] & below) * stride);
                for (int c = wave; c < C; c += 4)
                    o[c * plane + j] = has ? (T)bev_apply((float)mine[c], mean[c], invstd[c], gamma[c], beta[c]) : (T)fill[c];
            }
            __syncthreads();
        }
    }
}

// --------------------------------------------------------------------------------------------------------------- backward
// plane_sum[b * C + c] = sum of the (b, c) plane of G in f64: thread t adds elements (or 16-byte chunks) t, t + 256, ... in
// order, the threads meet in an LDS tree
template <typename T>
__global__ __launch_bounds__(kThreads) void bev_plane_kernel(const T *__restrict__ G, long long plane, int vec,
                                                             double *__restrict__ plane_sum) {
    __shared__ double red[kThreads];
    const T *p = G + (long long)blockIdx.x * plane;
    double s = 0.0;
    if (vec) {   // plane * sizeof(T) a multiple of 16 and G 16-byte aligned: every plane starts aligned
        constexpr int E = 16 / (int)sizeof(T);
        const long long chunks = plane / E;
        for (long long i = threadIdx.x; i < chunks; i += kThreads) {
            const uint4 raw = reinterpret_cast<const uint4 *>(p)[i];
            const T *e = reinterpret_cast<const T *>(&raw);
#pragma unroll
            for (int j = 0; j < E; ++j) s += (double)(float)e[j];
        }
    } else {
        for (long long i = threadIdx.x; i < plane; i += kThreads) s += (double)(float)p[i];
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int k = kThreads / 2; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) plane_sum[blockIdx.x] = red[0];
}

// rows r >= n of dx: 0 (rows r < n are written by the row-cell pass, all of them: their sites lie in the grid)
template <typename T>
__global__ __launch_bounds__(kThreads) void bev_index_kernel(const int *__restrict__ coords, const int *__restrict__ n_rows, int cap,
                                                             int C, int B, int H, int W, int *__restrict__ index, T *__restrict__ dx) {
    const int n = min(*n_rows, cap);
    for (int r = blockIdx.x * kThreads + threadIdx.x; r < n; r += gridDim.x * kThreads) {
        const int4 c = reinterpret_cast<const int4 *>(coords)[r];
        if (c.x < 0 || c.x >= B || c.y != 0 || c.z < 0 || c.z >= H || c.w < 0 || c.w >= W) continue;
        index[((long long)c.x * H + c.z) * W + c.w] = r;
    }
    const long long end = (long long)cap * C;
    for (long long t = (long long)n * C + (long long)blockIdx.x * kThreads + threadIdx.x; t < end; t += (long long)gridDim.x * kThreads)
        dx[t] = (T)0;
}

// Workgroup wg walks tiles wg, wg + grid, ...  Per tile with rows: the G values of its row cells through LDS slots
// (fnp_dense_gather_tile), then thread (group, c) takes slots group, group + 256 / C, ...: reads x of the slot's row, adds
// R += G, A += g, Bs += g * xhat in f64, and parks G in dx[row, c].  part[(wg * C + c) * 3 + {0, 1, 2}] = R, A, Bs.
template <typename T, int VEC>
__global__ __launch_bounds__(kThreads) void bev_cells_kernel(const T *__restrict__ G, const T *__restrict__ x,
                                                             const int *__restrict__ index, int C, long long plane, int tiles_per_plane,
                                                             long long tiles, const float *__restrict__ mean,
                                                             const float *__restrict__ invstd, const float *__restrict__ gamma,
                                                             const float *__restrict__ beta, T *__restrict__ dx,
                                                             double *__restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) unsigned char fnp_bev_smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row_bytes = C * (int)sizeof(T), stride = row_bytes + 4;
    int *slot_row = reinterpret_cast<int *>(fnp_bev_smem + kSlots * stride);
    const int c = threadIdx.x % C, group = threadIdx.x / C, groups = kThreads / C;   // (C <= 256 a power of two)
    const float mu = mean[c], is = invstd[c], ga = gamma[c], be = beta[c];
    double sR = 0.0, sA = 0.0, sB = 0.0;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long b = tile / tiles_per_plane;
        const long long l0 = (tile % tiles_per_plane) * (64 * VEC);
        const bool in = l0 + (long long)VEC * lane < plane;
        int r[VEC];
        fnp_dense_tile_rows<VEC>(index, b * plane + l0 + (long long)VEC * lane, in, r);
        int total = 0, slot[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const unsigned long long occ = __ballot(r[j] >= 0);    // (same in all four waves: they own the same cells)
            slot[j] = total + __popcll(occ & below);
            total += __popcll(occ);
        }
        if (total == 0) continue;                                    // (workgroup-uniform)
        const T *g = G + b * C * plane + l0 + (long long)VEC * lane;   // channel c adds c * plane
        for (int p0 = 0; p0 < total; p0 += kSlots) {
            bool mine[VEC], any = false;
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                mine[j] = r[j] >= 0 && slot[j] >= p0 && slot[j] < p0 + kSlots;
                any |= mine[j];
                if (mine[j] && wave == 0) slot_row[slot[j] - p0] = r[j];
            }
            if (any) fnp_dense_gather_tile<T, VEC>(fnp_bev_smem, g, plane, C, stride, wave, mine, slot, p0);
            __syncthreads();
            const int cnt = min(total - p0, kSlots);
            for (int k = group; k < cnt; k += groups) {
                const size_t at = (size_t)slot_row[k] * C + c;
                const T Gt = reinterpret_cast<const T *>(fnp_bev_smem + k * stride)[c];
                const float Gv = (float)Gt, xv = ldf(x, at);
                const float gv = (float)(T)bev_apply(xv, mu, is, ga, be) > 0.f ? Gv : 0.f;
                const float xh = (xv - mu) * is;
                sR += (double)Gv;
                sA += (double)gv;
                sB += (double)gv * (double)xh;
                dx[at] = Gt;
            }
            __syncthreads();                                         // (before the next pass or tile overwrites the slots)
        }
    }
    // the groups of a channel meet in group order
    double *red = reinterpret_cast<double *>(fnp_bev_smem);
    red[threadIdx.x * 3 + 0] = sR;
    red[threadIdx.x * 3 + 1] = sA;
    red[threadIdx.x * 3 + 2] = sB;
    __syncthreads();
    for (int i = threadIdx.x; i < C * 3; i += kThreads) {
        const int cc = i / 3, j = i - cc * 3;
        double v = 0.0;
        for (int q = 0; q < groups; ++q) v += red[(q * C + cc) * 3 + j];
        part[((size_t)blockIdx.x * C + cc) * 3 + j] = v;
    }
}

__global__ __launch_bounds__(kThreads) void bev_finish_backward_kernel(const double *__restrict__ part, int parts,
                                                                       const double *__restrict__ plane_sum, int B, int C,
                                                                       const float *__restrict__ mean, const float *__restrict__ invstd,
                                                                       const float *__restrict__ fill, float *__restrict__ dbeta,
                                                                       float *__restrict__ dgamma) {
    __shared__ double red[3][kThreads];
    const int CW = C < kFinC ? C : kFinC;
    const int c = blockIdx.x * CW + threadIdx.x % CW;
    double v[3];
    finish_sums<3>(part, parts, C, c, CW, v, red);
    if (threadIdx.x < CW) {
        double db = v[1], dg = v[2];
        if (fill[c] > 0.f) {
            double T = 0.0;
            for (int b = 0; b < B; ++b) T += plane_sum[(size_t)b * C + c];
            const float xhat_bg = (0.f - mean[c]) * invstd[c];
            db += T - v[0];
            dg += (double)xhat_bg * (T - v[0]);
        }
        dbeta[c] = (float)db;
        dgamma[c] = (float)dg;
    }
}

// dx[r] holds G at row r's cell (row-cell pass): dx = gamma * invstd * (g - dbeta / N - xhat * dgamma / N) in place
template <typename T>
__global__ __launch_bounds__(kThreads) void bev_backward_apply_kernel(const T *__restrict__ x, const int *__restrict__ n_rows, int cap,
                                                                      int C, float inv_n, const float *__restrict__ mean,
                                                                      const float *__restrict__ invstd, const float *__restrict__ gamma,
                                                                      const float *__restrict__ beta, const float *__restrict__ dbeta,
                                                                      const float *__restrict__ dgamma, T *__restrict__ dx) {
    const int n = min(*n_rows, cap);
    const long long chunks = (long long)n * (C / 8);
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < chunks; i += (long long)gridDim.x * kThreads) {
        const int c0 = (int)(i % (C / 8)) * 8;
        float gv[8], xv[8], o[8];
        load8(dx + i * 8, gv);
        load8(x + i * 8, xv);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float mu = mean[c0 + j], is = invstd[c0 + j];
            const float g = (float)(T)bev_apply(xv[j], mu, is, gamma[c0 + j], beta[c0 + j]) > 0.f ? gv[j] : 0.f;
            const float xh = (xv[j] - mu) * is;
            o[j] = gamma[c0 + j] * is * (g - dbeta[c0 + j] * inv_n - xh * dgamma[c0 + j] * inv_n);
        }
        store8(dx + i * 8, o);
    }
}

// ------------------------------------------------------------------------------------------------------------------- host
bool shape_ok(int cap, int C, int B, int H, int W, size_t esize) {
    if (cap <= 0 || B <= 0 || H <= 0 || W <= 0 || C < 8 || C > 256 || (C & (C - 1)) != 0) return false;   // 8 | C, C | 256
    if ((long long)B * H * W > 0x7fffffffll) return false;
    return (size_t)kSlots * (C * esize + 4) + kSlots * 4 <= 64 * 1024;   // the LDS slots of a tile (C = 256 in f32 does not fit)
}
size_t lds_bytes(int C, size_t esize) {
    const size_t slots = (size_t)kSlots * (C * esize + 4) + kSlots * 4, red = (size_t)kThreads * 3 * sizeof(double);
    return slots > red ? slots : red;
}
int64_t index_bytes(int B, int H, int W) { return (((int64_t)B * H * W * 4) + 15) / 16 * 16; }
int stats_grid(int cap, int C) {
    int g = fnp_divup(cap, (kThreads / (C / 8)) * 8);
    return g > kStatParts ? kStatParts : (g < 1 ? 1 : g);
}
int vec_of(long long plane, const void *map, const void *ws, size_t esize) {   // cells per lane (dense.hip's choice)
    const bool al = ((uintptr_t)map % 16 == 0) && ((uintptr_t)ws % 16 == 0);
    const int max_vec = 16 / (int)esize < kDenseVec ? 16 / (int)esize : kDenseVec;
    return (max_vec >= 2 && al && plane % 2 == 0) ? 2 : 1;
}
static_assert(kDenseVec == 2, "vec_of and the launches below know cells per lane 1 and 2");

template <typename T>
int run_forward(const void *x, const int *coords, const int *n_rows, int cap, int C, int B, int H, int W, const float *gamma,
                const float *beta, float *rm, float *rv, float momentum, float eps, void *y, float *save_mean, float *save_invstd,
                float *fill, long long *nbt, void *ws, hipStream_t s) {
    const long long plane = (long long)H * W, cells = (long long)B * plane;
    int *index = (int *)ws;
    double *part = (double *)((unsigned char *)ws + index_bytes(B, H, W));
    {
        const int frc = fnp_fill_words(index, cells, 0xffffffffu, s);
        if (frc) return frc;
    }
    hipLaunchKernelGGL(fnp_dense_index_kernel, dim3(fnp_grid_for(cap, kThreads)), dim3(kThreads), 0, s, coords, n_rows, cap, B, 1, H, W,
                       index);
    FNP_LAUNCH_CHECK();
    const int g = stats_grid(cap, C);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(bev_stats_kernel<T>), dim3(g), dim3(kThreads), 0, s, (const T *)x, n_rows, cap, C, part);
    FNP_LAUNCH_CHECK();
    hipLaunchKernelGGL(bev_finish_forward_kernel, dim3(C <= kFinC ? 1 : C / kFinC), dim3(kThreads), 0, s, (const double *)part, g, C,
                       cells, eps, momentum, gamma, beta, save_mean, save_invstd, fill, rm, rv, nbt);
    FNP_LAUNCH_CHECK();
    const int vec = vec_of(plane, y, ws, sizeof(T));
    const int tiles_per_plane = (int)((plane + 64 * vec - 1) / (64 * vec));
    const long long tiles = (long long)B * tiles_per_plane;
    if (tiles > 0x7fffffffll) return FNP_ERR_ARG;
    const size_t lds = (size_t)kSlots * (C * sizeof(T) + 4);
    if (vec == 2)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(bev_write_kernel<T, 2>), dim3((unsigned)tiles), dim3(kThreads), lds, s, (const T *)x, index, C,
                           plane, tiles_per_plane, save_mean, save_invstd, gamma, beta, fill, (T *)y);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(bev_write_kernel<T, 1>), dim3((unsigned)tiles), dim3(kThreads), lds, s, (const T *)x, index, C,
                           plane, tiles_per_plane, save_mean, save_invstd, gamma, beta, fill, (T *)y);
    FNP_LAUNCH_CHECK();
    return FNP_OK;
}

template <typename T>
int run_backward(const void *G, const void *x, const int *coords, const int *n_rows, int cap, int C, int B, int H, int W,
                 const float *gamma, const float *beta, const float *save_mean, const float *save_invstd, const float *fill, void *dx,
                 float *dgamma, float *dbeta, void *ws, hipStream_t s) {
    const long long plane = (long long)H * W, cells = (long long)B * plane;
    int *index = (int *)ws;
    double *part = (double *)((unsigned char *)ws + index_bytes(B, H, W));
    {
        const int frc = fnp_fill_words(index, cells, 0xffffffffu, s);
        if (frc) return frc;
    }
    hipLaunchKernelGGL(HIP_KERNEL_NAME(bev_index_kernel<T>), dim3(fnp_grid_for(cap, kThreads)), dim3(kThreads), 0, s, coords, n_rows, cap,
                       C, B, H, W, index, (T *)dx);
    FNP_LAUNCH_CHECK();
    const int vec = vec_of(plane, G, ws, sizeof(T));
    const int tiles_per_plane = (int)((plane + 64 * vec - 1) / (64 * vec));
    const long long tiles = (long long)B * tiles_per_plane;
    const int parts = (int)(tiles < kCellParts ? tiles : kCellParts);
    double *plane_sum = part + (size_t)kCellParts * C * 3;
    const int pvec = (plane * (long long)sizeof(T)) % 16 == 0 && (uintptr_t)G % 16 == 0;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(bev_plane_kernel<T>), dim3((unsigned)(B * C)), dim3(kThreads), 0, s, (const T *)G, plane, pvec,
                       plane_sum);
    FNP_LAUNCH_CHECK();
    const size_t lds = lds_bytes(C, sizeof(T));
    if (vec == 2)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(bev_cells_kernel<T, 2>), dim3(parts), dim3(kThreads), lds, s, (const T *)G, (const T *)x, index, C,
                           plane, tiles_per_plane, tiles, save_mean, save_invstd, gamma, beta, (T *)dx, part);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(bev_cells_kernel<T, 1>), dim3(parts), dim3(kThreads), lds, s, (const T *)G, (const T *)x, index, C,
                           plane, tiles_per_plane, tiles, save_mean, save_invstd, gamma, beta, (T *)dx, part);
    FNP_LAUNCH_CHECK();
    hipLaunchKernelGGL(bev_finish_backward_kernel, dim3(C <= kFinC ? 1 : C / kFinC), dim3(kThreads), 0, s, (const double *)part, parts,
                       (const double *)plane_sum, B, C, save_mean, save_invstd, fill, dbeta, dgamma);
    FNP_LAUNCH_CHECK();
    hipLaunchKernelGGL(HIP_KERNEL_NAME(bev_backward_apply_kernel<T>), dim3(fnp_grid_for((long long)cap * (C / 8), kThreads, 2048)),
                       dim3(kThreads), 0, s, (const T *)x, n_rows, cap, C, 1.0f / (float)cells, save_mean, save_invstd, gamma, beta, dbeta,
                       dgamma, (T *)dx);
    FNP_LAUNCH_CHECK();
    return FNP_OK;
}

size_t esize_of(int dtype) { return dtype == FNP_F32 ? 4 : (dtype == FNP_BF16 || dtype == FNP_F16) ? 2 : 0; }

}  // namespace

extern "C" int64_t fnp_bev_bn_workspace_bytes(int C, int B, int H, int W) {
    if (C <= 0 || B <= 0 || H <= 0 || W <= 0) return 0;
    const int64_t fwd = (int64_t)kStatParts * C * 2, bwd = (int64_t)kCellParts * C * 3 + (int64_t)B * C;
    return index_bytes(B, H, W) + (fwd > bwd ? fwd : bwd) * (int64_t)sizeof(double);
}

extern "C" int fnp_bev_bn_train_forward(const void *x, int dtype, const int *coords, const int *n_rows, int cap, int C, int B, int H,
                                        int W, const float *gamma, const float *beta, float *running_mean, float *running_var,
                                        float momentum, float eps, void *y, float *save_mean, float *save_invstd, float *fill,
                                        long long *num_batches_tracked, void *workspace, int64_t workspace_bytes, fnp_stream_t stream) {
    const size_t es = esize_of(dtype);
    if (!x || !coords || !n_rows || !gamma || !beta || !y || !save_mean || !save_invstd || !fill || !workspace || !es ||
        !shape_ok(cap, C, B, H, W, es))
        return FNP_ERR_ARG;
    if ((running_mean == nullptr) != (running_var == nullptr)) return FNP_ERR_ARG;
    if ((uintptr_t)workspace % 8 != 0 || (uintptr_t)x % 16 != 0) return FNP_ERR_ARG;
    if (workspace_bytes < fnp_bev_bn_workspace_bytes(C, B, H, W)) return FNP_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == FNP_F32)
        return run_forward<float>(x, coords, n_rows, cap, C, B, H, W, gamma, beta, running_mean, running_var, momentum, eps, y, save_mean,
                                  save_invstd, fill, num_batches_tracked, workspace, s);
    if (dtype == FNP_BF16)
        return run_forward<__bf16>(x, coords, n_rows, cap, C, B, H, W, gamma, beta, running_mean, running_var, momentum, eps, y, save_mean,
                                   save_invstd, fill, num_batches_tracked, workspace, s);
    return run_forward<_Float16>(x, coords, n_rows, cap, C, B, H, W, gamma, beta, running_mean, running_var, momentum, eps, y, save_mean,
                                 save_invstd, fill, num_batches_tracked, workspace, s);
}

extern "C" int fnp_bev_bn_train_backward(const void *grad_out, const void *x, int dtype, const int *coords, const int *n_rows, int cap,
                                         int C, int B, int H, int W, const float *gamma, const float *beta, const float *save_mean,
                                         const float *save_invstd, const float *fill, void *grad_x, float *grad_gamma, float *grad_beta,
                                         void *workspace, int64_t workspace_bytes, fnp_stream_t stream) {
    const size_t es = esize_of(dtype);
    if (!grad_out || !x || !coords || !n_rows || !gamma || !beta || !save_mean || !save_invstd || !fill || !grad_x || !grad_gamma ||
        !grad_beta || !workspace || !es || !shape_ok(cap, C, B, H, W, es))
        return FNP_ERR_ARG;
    if ((uintptr_t)workspace % 8 != 0 || (uintptr_t)x % 16 != 0 || (uintptr_t)grad_x % 16 != 0) return FNP_ERR_ARG;
    if (workspace_bytes < fnp_bev_bn_workspace_bytes(C, B, H, W)) return FNP_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == FNP_F32)
        return run_backward<float>(grad_out, x, coords, n_rows, cap, C, B, H, W, gamma, beta, save_mean, save_invstd, fill, grad_x,
                                   grad_gamma, grad_beta, workspace, s);
    if (dtype == FNP_BF16)
        return run_backward<__bf16>(grad_out, x, coords, n_rows, cap, C, B, H, W, gamma, beta, save_mean, save_invstd, fill, grad_x,
                                    grad_gamma, grad_beta, workspace, s);
    return run_backward<_Float16>(grad_out, x, coords, n_rows, cap, C, B, H, W, gamma, beta, save_mean, save_invstd, fill, grad_x,
                                  grad_gamma, grad_beta, workspace, s);
}
