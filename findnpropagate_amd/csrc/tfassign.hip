// Hungarian assignment and per-query targets of TransFusionHead (pcdet/models/dense_heads/transfusion_head.py:352-444 and
// target_assigner/hungarian_assigner.py:61-132).  Per scene the reference tests every ground-truth row from Python, decodes the
// predictions, builds three K x M cost matrices in some thirty launches, copies their sum to the host for scipy's
// linear_sum_assignment, copies the match back and loops over the positives in Python.  Here the batch is four launches and
// nothing is read back:
//
//   valid : a workgroup per scene compacts the valid rows of gt_boxes in ascending order -> valid_map, num_valid [valid_kernel]
//   cost  : a workgroup per 8 queries x 16 valid boxes; the first 24 threads decode the queries (tfdecode.h) and prepare
//           both sides' rectangles (boxoverlap.h) into LDS, then a thread per pair forms cls + reg + iou_cost in f32 in the
//           reference's order.  The intersection polygon of a pair (24 vertices and keys, indexed dynamically) lives in an LDS
//           column per thread, 36 KB per workgroup, not in private memory: the kernel uses no scratch.  Every element of
//           cost and iou is written once; columns behind num_valid are 0                                          [cost_kernel]
//   match : one wave per scene walks scipy's shortest-augmenting-path solver (lsap.h states it and what fixes its result).
//           The solver is serial in its rows and in the steps of a path; what is parallel is the scan of the remaining
//           columns inside a step, which the 64 lanes share by POSITION in `remaining`, so the array's order (start nc-1 .. 0,
//           removal by a swap with the last entry) is kept as it is.  Per step every lane relaxes its columns, then the wave
//           takes the minimum of the path costs and, among the positions that attain it, the last whose column is unassigned
//           or else the first: the position the sequential scan ends on.  All state lives in LDS (f64 duals and path costs,
//           16-bit indices: 54 KB at the contract's largest shape); the cost is read from global memory (L2) as it is, also
//           when the solver runs on the transpose.  A workgroup IS one wave, so its barriers order the LDS traffic and cost no
//           wait.  Every value that steers control flow is broadcast from lane 0 after a reduction, so the lanes cannot part
//           ways whatever the costs hold; each inner step removes a column, which bounds every loop.               [match_kernel]
//   target: a thread per (scene, query) writes labels, weights, the encoded box of its match (encode_bbox, :604-614) and the
//           unknown mask; workgroup 0 also counts the matches of the batch into num_pos (integers: any order)     [target_kernel]
//
// Nothing here allocates or synchronises, there are no atomics, and a scene's result depends on its own rows alone.
//
// ARITHMETIC.  Parity is with the reference run on the CPU, as for the heatmap slice.  Every f32 division is formed in f64 and
// rounded once (the correctly rounded f32 quotient); exp, atan2, log, sin and cos of the decode and the encode are formed in f64
// and rounded once; the sigmoid and the logarithms of the classification cost are f32 (expf, logf) and held by a bound, not
// bit for bit.  A Python scalar meets a tensor as its f32 rounding: the host entry points round alpha, 1 - alpha, eps and the
// weights that way.  pow(gamma) is a product for gamma = 2, as torch makes it, and powf otherwise.
// VALID ROWS: dx > 0 and dy > 0 (the reference's "filter empty boxes"), a label inside 1..C and finite x, y, dx, dy; the
// reference wraps on a label below 1 and raises on one above C or a non-finite box, all out of contract here and skipped, the
// rule of fnp_heatmap_box_params.  A label with a fraction is truncated, as the reference's .long() does (10.5 is class 10).
#include "common.h"
#include "boxoverlap.h"
#include "lsap.h"
#include "tfdecode.h"

namespace {

constexpr int kWave = 64;
constexpr int kThreads = 256;
constexpr int kMaxQueries = 2048, kMaxBoxes = 1024;

__device__ __forceinline__ float div_rn(float a, float b) { return (float)((double)a / (double)b); }
__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= 3.402823466e38f; }   // false for NaN

__global__ __launch_bounds__(kThreads) void valid_kernel(const float *__restrict__ gt, int Mcap, int ncol, int C,
                                                         int *__restrict__ valid_map, int *__restrict__ num_valid) {
    __shared__ int wcnt[kThreads / kWave];
    const int b = blockIdx.x;
    int kept = 0;
    for (int base = 0; base < Mcap; base += kThreads) {
        const int m = base + threadIdx.x;
        bool ok = false;
        if (m < Mcap) {
            const float *r = gt + ((size_t)b * Mcap + m) * ncol;
            const float lab = r[ncol - 1];
            ok = r[3] > 0.f && r[4] > 0.f && finite_f(r[0]) && finite_f(r[1]) && finite_f(r[3]) && finite_f(r[4]) && lab >= 1.f &&
                 lab < (float)(C + 1);
        }
        const unsigned long long bal = __ballot(ok);
        const int wave = threadIdx.x >> 6;
        if (fnp_lane() == 0) wcnt[wave] = __popcll(bal);
        __syncthreads();
        int pos = kept + __popcll(bal & ((1ull << fnp_lane()) - 1ull));
        for (int j = 0; j < kThreads / kWave; ++j) {
            if (j < wave) pos += wcnt[j];
            kept += wcnt[j];
        }
        __syncthreads();
        if (ok) valid_map[(size_t)b * Mcap + pos] = m;
    }
    for (int m = kept + threadIdx.x; m < Mcap; m += kThreads) valid_map[(size_t)b * Mcap + m] = -1;
    if (threadIdx.x == 0) num_valid[b] = kept;
}

struct CostCfg {
    float stride, vx, vy, x0, y0, rx, ry;       // rx, ry: f32(range[3:5]) - f32(range[0:2]), in f32
    float alpha, one_m_alpha, gamma, eps, w_cls, w_reg, w_iou;
    int C, K, Mcap, ncol, has_vel;
};

__device__ __forceinline__ float pow_gamma(float x, float gamma) { return gamma == 2.f ? x * x : powf(x, gamma); }

constexpr int kCostQ = 8, kCostG = 16, kCostThreads = kCostQ * kCostG;   // the tile: 8 queries x 16 boxes

__global__ __launch_bounds__(kCostThreads) void cost_kernel(const float *__restrict__ heatmap, const float *__restrict__ center,
                                                        const float *__restrict__ height, const float *__restrict__ dim,
                                                        const float *__restrict__ rot, const float *__restrict__ vel,
                                                        const float *__restrict__ gt, const int *__restrict__ valid_map,
                                                        const int *__restrict__ num_valid, CostCfg cfg, float *__restrict__ cost,
                                                        float *__restrict__ iou, float *__restrict__ boxes) {
    __shared__ RBox sq[kCostQ], sg[kCostG];
    __shared__ int slabel[kCostG];
    __shared__ P2 poly_v[24 * kCostThreads];        // vertex i of thread t at [i * kCostThreads + t]: conflict-free columns
    __shared__ float poly_k[24 * kCostThreads];
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
    const int b = blockIdx.z, k0 = blockIdx.y * kCostQ, m0 = blockIdx.x * kCostG;
    const int K = cfg.K, Mcap = cfg.Mcap;
    int nv = num_valid[b];
    nv = nv < 0 ? 0 : (nv > Mcap ? Mcap : nv);
    const int k = k0 + ty, m = m0 + tx;
    if (m0 >= nv) {                               // (whole workgroup) a tile behind the valid columns: zeros, nothing decoded
        if (k < K && m < Mcap) {
            const size_t at = ((size_t)b * K + k) * Mcap + m;
            cost[at] = 0.f, iou[at] = 0.f;
        }
        if (!(boxes && blockIdx.x == 0)) return;
    }
    if (threadIdx.x < kCostQ) {
        const int q = k0 + threadIdx.x;
        if (q < K) {
            float box[9];
            tf_decode_box(center, height, dim, rot, cfg.has_vel ? vel : nullptr, (size_t)b, q, K, cfg.stride, cfg.vx, cfg.vy, cfg.x0,
                          cfg.y0, box);
            prep_box(box, sq[threadIdx.x]);
            if (boxes && blockIdx.x == 0) {
                const int nb = cfg.has_vel ? 9 : 7;
                for (int j = 0; j < nb; ++j) boxes[((size_t)b * K + q) * nb + j] = box[j];
            }
        }
    } else if (threadIdx.x < kCostQ + kCostG) {
        const int t = threadIdx.x - kCostQ;
        if (m0 + t < nv) {
            const int row = valid_map[(size_t)b * Mcap + m0 + t];
            const float *r = gt + ((size_t)b * Mcap + (row < 0 ? 0 : (row >= Mcap ? Mcap - 1 : row))) * cfg.ncol;
            prep_box(r, sg[t]);
            const int lab = (int)r[cfg.ncol - 1] - 1;
            slabel[t] = lab < 0 ? 0 : (lab >= cfg.C ? cfg.C - 1 : lab);      // valid rows hold 1..C; the clamp guards the read below
        }
    }
    __syncthreads();
    if (m0 >= nv || k >= K || m >= Mcap) return;
    const size_t at = ((size_t)b * K + k) * Mcap + m;
    if (m >= nv) {
        cost[at] = 0.f, iou[at] = 0.f;
        return;
    }
    const RBox &Q = sq[ty];
    const RBox &G = sg[tx];
    // focal_loss_cost: (pos - neg)[k, label] * weight
    const float x = heatmap[((size_t)b * cfg.C + slabel[tx]) * K + k];
    const float p = __fdiv_rn(1.f, 1.f + expf(-x));
    const float neg = ((-logf((1.f - p) + cfg.eps)) * cfg.one_m_alpha) * pow_gamma(p, cfg.gamma);
    const float pos = ((-logf(p + cfg.eps)) * cfg.alpha) * pow_gamma(1.f - p, cfg.gamma);
    const float cls = (pos - neg) * cfg.w_cls;
    // bevbox_cost: L1 distance of the xy normalised by the range
    const float qx = div_rn(Q.raw[0] - cfg.x0, cfg.rx), qy = div_rn(Q.raw[1] - cfg.y0, cfg.ry);
    const float gx = div_rn(G.raw[0] - cfg.x0, cfg.rx), gy = div_rn(G.raw[1] - cfg.y0, cfg.ry);
    const float reg = (fabsf(qx - gx) + fabsf(qy - gy)) * cfg.w_reg;
    // iou3d_cost: overlaps(), z is the bottom of a box there
    const float q_top = Q.raw[2] + Q.raw[5], g_top = G.raw[2] + G.raw[5];
    const float bottom = Q.raw[2] > G.raw[2] ? Q.raw[2] : G.raw[2];
    const float top = q_top < g_top ? q_top : g_top;
    float oh = top - bottom;
    oh = oh < 0.f ? 0.f : oh;
    PolyStrided st{poly_v + threadIdx.x, poly_k + threadIdx.x, kCostThreads};
    const float o3 = overlap_area_in(Q, G, st) * oh;
    const float vq = Q.raw[3] * Q.raw[4] * Q.raw[5], vg = G.raw[3] * G.raw[4] * G.raw[5];
    float den = vq + vg - o3;
    den = den < 1e-8f ? 1e-8f : den;
    const float u = div_rn(o3, den);
    iou[at] = u;
    cost[at] = (cls + reg) + (-u) * cfg.w_iou;
}

struct TargetCfg {
    float x0, y0, div_x, div_y;                  // f32(range[0:2]); f32(stride * voxel) formed in f64
    int C, K, Mcap, ncol, code;
    unsigned long long unk_mask;
};

__global__ __launch_bounds__(kThreads) void target_kernel(const int *__restrict__ assigned, const float *__restrict__ gt,
                                                          long long n, TargetCfg cfg, long long *__restrict__ labels,
                                                          float *__restrict__ label_weights, float *__restrict__ bbox_targets,
                                                          float *__restrict__ bbox_weights, unsigned char *__restrict__ unknown,
                                                          int *__restrict__ num_pos) {
    __shared__ int part[kThreads];
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) {
        const int b = (int)(i / cfg.K), a = assigned[i];
        float t[10];
        for (int j = 0; j < 10; ++j) t[j] = 0.f;
        long long label = cfg.C;
        bool unk = false;
        const bool hit = a >= 0 && a < cfg.Mcap;
        if (hit) {
            const float *r = gt + ((size_t)b * cfg.Mcap + a) * cfg.ncol;
            t[0] = div_rn(r[0] - cfg.x0, cfg.div_x);
            t[1] = div_rn(r[1] - cfg.y0, cfg.div_y);
            t[2] = r[2];
            for (int j = 3; j < 6; ++j) t[j] = (float)log((double)r[j]);
            t[6] = (float)sin((double)r[6]);
            t[7] = (float)cos((double)r[6]);
            if (cfg.code == 10) t[8] = r[7], t[9] = r[8];
            const int l0 = (int)r[cfg.ncol - 1] - 1;
            label = l0;
            unk = l0 >= 0 && l0 < 64 && ((cfg.unk_mask >> l0) & 1ull);
        }
        labels[i] = label;
        label_weights[i] = 1.f;               // positives and negatives alike (:432, :444)
        unknown[i] = unk ? 1 : 0;
        for (int j = 0; j < cfg.code; ++j) {
            bbox_targets[i * cfg.code + j] = t[j];
            bbox_weights[i * cfg.code + j] = hit ? 1.f : 0.f;
        }
    }
    if (blockIdx.x == 0) {
        int s = 0;
        for (long long j = threadIdx.x; j < n; j += kThreads) {
            const int a = assigned[j];
            s += a >= 0 && a < cfg.Mcap;
        }
        part[threadIdx.x] = s;
        __syncthreads();
        for (int h = kThreads / 2; h > 0; h >>= 1) {
            if ((int)threadIdx.x < h) part[threadIdx.x] += part[threadIdx.x + h];
            __syncthreads();
        }
        if (threadIdx.x == 0) *num_pos = part[0];
    }
}

struct MatchLds {   // carve of the dynamic LDS for solver shapes up to nr_cap x nc_cap
    double *spc, *v, *u;
    short *path, *row4col, *remaining, *col4row;
};
__host__ __device__ inline size_t match_lds_bytes(int nr_cap, int nc_cap) {
    return (size_t)8 * (2 * nc_cap + nr_cap) + (size_t)2 * (3 * nc_cap + nr_cap);
}

__device__ __forceinline__ double bcast0(double x) { return __shfl(x, 0, kWave); }
__device__ __forceinline__ int bcast0(int x) { return __shfl(x, 0, kWave); }

__global__ __launch_bounds__(kWave) void match_kernel(const float *__restrict__ cost, const float *__restrict__ iou,
                                                      const int *__restrict__ num_valid, const int *__restrict__ valid_map, int K,
                                                      int Mcap, int nr_cap, int nc_cap, int *__restrict__ assigned,
                                                      float *__restrict__ matched_iou) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    MatchLds s;
    s.spc = (double *)lds_raw, s.v = s.spc + nc_cap, s.u = s.v + nc_cap;
    s.path = (short *)(s.u + nr_cap), s.row4col = s.path + nc_cap, s.remaining = s.row4col + nc_cap, s.col4row = s.remaining + nc_cap;
    const int b = blockIdx.x, lane = threadIdx.x;
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    int M = num_valid[b];
    M = M < 0 ? 0 : (M > Mcap ? Mcap : M);
    cost += (size_t)b * K * Mcap;
    int *out = assigned + (size_t)b * K;
    float *out_iou = matched_iou ? matched_iou + (size_t)b * K : nullptr;
    for (int k = lane; k < K; k += kWave) {
        out[k] = -1;
        if (out_iou) out_iou[k] = 0.f;
    }
    if (M == 0) return;
    // scipy transposes a matrix with fewer columns than rows: the solver's rows are then the boxes, its columns the queries
    const bool transposed = M < K;
    const int nr = transposed ? M : K, nc = transposed ? K : M;
    const size_t row_stride = transposed ? 1 : (size_t)Mcap, col_stride = transposed ? (size_t)Mcap : 1;
    for (int j = lane; j < nc; j += kWave) s.v[j] = 0.0, s.row4col[j] = -1;
    for (int i = lane; i < nr; i += kWave) s.u[i] = 0.0, s.col4row[i] = -1;
    bool ok = true;
    for (int cur = 0; cur < nr && ok; ++cur) {
        for (int it = lane; it < nc; it += kWave) s.remaining[it] = (short)(nc - 1 - it), s.spc[it] = inf;
        __syncthreads();
        double min_val = 0.0;
        int nrem = nc, sink = -1, i = cur;
        while (sink == -1) {
            const double ui = s.u[i];
            const float *crow = cost + (size_t)i * row_stride;
            double lowest = inf;
            int last_free = -1, first = 0x7fffffff;   // among this lane's positions that attain `lowest`
            for (int it = lane; it < nrem; it += kWave) {
                const int j = s.remaining[it];
                const double r = ((min_val + (double)crow[(size_t)j * col_stride]) - ui) - s.v[j];
                double sp = s.spc[j];
                if (r < sp) s.path[j] = (short)i, s.spc[j] = sp = r;
                const bool free_col = s.row4col[j] == -1;
                if (sp < lowest) lowest = sp, first = it, last_free = free_col ? it : -1;
                else if (sp == lowest && free_col) last_free = it;
            }
            double wave_low = lowest;
            for (int k = 32; k > 0; k >>= 1) {
                const double o = __shfl_xor(wave_low, k, kWave);
                wave_low = o < wave_low ? o : wave_low;
            }
            wave_low = bcast0(wave_low);
            const bool attains = lowest == wave_low && first != 0x7fffffff;
            int wl = attains ? last_free : -1, wf = attains ? first : 0x7fffffff;
            for (int k = 32; k > 0; k >>= 1) {
                wl = max(wl, __shfl_xor(wl, k, kWave));
                wf = min(wf, __shfl_xor(wf, k, kWave));
            }
            const int index = bcast0(wl >= 0 ? wl : wf);
            min_val = wave_low;
            if (index < 0 || index >= nrem || !(min_val < inf)) {   // no finite path: a NaN or an infinite cost, out of contract
                ok = false;
                break;
            }
            const int j = s.remaining[index];
            const int r4c = s.row4col[j];
            if (r4c == -1) sink = j;
            else i = r4c;
            __syncthreads();                                         // every lane has read remaining[index] and remaining[nrem - 1]
            --nrem;
            if (lane == 0) {                                         // the scanned columns collect behind the live ones, at [nrem, nc)
                s.remaining[index] = s.remaining[nrem];
                s.remaining[nrem] = (short)j;
            }
            __syncthreads();
        }
        if (!ok) break;
        // duals: the scanned columns are remaining[nrem .. nc); the scanned rows besides `cur` are those columns' rows
        for (int t = nrem + lane; t < nc; t += kWave) {
            const int j = s.remaining[t];
            const double d = min_val - s.spc[j];
            const int r = s.row4col[j];
            if (r >= 0) s.u[r] += d;
            s.v[j] -= d;
        }
        if (lane == 0) s.u[cur] += min_val;
        __syncthreads();
        if (lane == 0) {
            for (int j = sink;;) {
                const int r = s.path[j];
                s.row4col[j] = (short)r;
                const int next = s.col4row[r];
                s.col4row[r] = (short)j;
                j = next;
                if (r == cur) break;
            }
        }
        __syncthreads();
    }
    if (!ok) return;
    for (int i = lane; i < nr; i += kWave) {
        const int j = s.col4row[i];
        const int k = transposed ? j : i, m = transposed ? i : j;   // query, compact box
        if (k < 0 || m < 0) continue;
        out[k] = valid_map ? valid_map[(size_t)b * Mcap + m] : m;
        if (out_iou) {
            const float x = iou[((size_t)b * K + k) * Mcap + m];
            out_iou[k] = x < 0.f ? 0.f : (x > 1.f ? 1.f : x);       // (keeps a NaN, as torch.clamp does)
        }
    }
}

}  // namespace

extern "C" int fnp_host_lsap(const float *cost, int nr, int nc, int *rows, int *cols) {
    if (nr < 0 || nc < 0) return FNP_ERR_ARG;
    if (nr == 0 || nc == 0) return FNP_OK;
    if (!cost || !rows || !cols) return FNP_ERR_ARG;
    return fnp_lsap(cost, nr, nc, rows, cols) ? FNP_OK : FNP_ERR_ARG;
}

extern "C" int fnp_tf_assign_match(const float *cost, const float *iou, const int *num_valid, const int *valid_map, int batch_size,
                                   int num_queries, int max_boxes, int *assigned, float *matched_iou, fnp_stream_t stream) {
    if (batch_size < 0 || num_queries < 0 || max_boxes < 0 || num_queries > kMaxQueries || max_boxes > kMaxBoxes) return FNP_ERR_ARG;
    if (batch_size == 0 || num_queries == 0) return FNP_OK;
    if (!assigned || !num_valid || (max_boxes > 0 && !cost) || (matched_iou && max_boxes > 0 && !iou)) return FNP_ERR_ARG;
    const int nr_cap = num_queries < max_boxes ? num_queries : max_boxes, nc_cap = num_queries > max_boxes ? num_queries : max_boxes;
    const size_t lds = match_lds_bytes(nr_cap > 0 ? nr_cap : 1, nc_cap);   // <= 54 KB: within the default dynamic LDS limit
    hipLaunchKernelGGL(match_kernel, dim3(batch_size), dim3(kWave), lds, (hipStream_t)stream, cost, iou, num_valid, valid_map,
                       num_queries, max_boxes, nr_cap > 0 ? nr_cap : 1, nc_cap, assigned, matched_iou);
    FNP_LAUNCH_CHECK();
    return FNP_OK;
}

extern "C" int fnp_tf_assign_cost(const float *heatmap, const float *center, const float *height, const float *dim, const float *rot,
                                  const float *vel, const float *gt_boxes, int batch_size, int num_classes, int num_queries,
                                  int max_boxes, int ncol, int feature_map_stride, float voxel_x, float voxel_y,
                                  const float *point_cloud_range, double cls_weight, double alpha, double gamma, double eps,
                                  double reg_weight, double iou_weight, int *num_valid, int *valid_map, float *cost, float *iou,
                                  float *boxes, fnp_stream_t stream) {
    if (batch_size < 0 || batch_size > 65535 || num_classes < 1 || num_classes > 64 || num_queries < 0 || num_queries > kMaxQueries ||
        max_boxes < 0 || max_boxes > kMaxBoxes || (ncol != 8 && ncol != 10) || feature_map_stride < 1 || !point_cloud_range)
        return FNP_ERR_ARG;
    if (batch_size == 0) return FNP_OK;
    if (!num_valid || (max_boxes > 0 && (!gt_boxes || !valid_map))) return FNP_ERR_ARG;
    if (num_queries > 0 && (!heatmap || !center || !height || !dim || !rot || (ncol == 10 && !vel) || (max_boxes > 0 && (!cost || !iou))))
        return FNP_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(valid_kernel, dim3(batch_size), dim3(kThreads), 0, s, gt_boxes, max_boxes, ncol, num_classes, valid_map, num_valid);
    FNP_LAUNCH_CHECK();
    if (num_queries == 0) return FNP_OK;
    CostCfg cfg;
    const float *r = point_cloud_range;          // HOST array of 6 floats: x0 y0 z0 x1 y1 z1
    cfg.stride = (float)feature_map_stride, cfg.vx = voxel_x, cfg.vy = voxel_y, cfg.x0 = r[0], cfg.y0 = r[1];
    cfg.rx = r[3] - r[0], cfg.ry = r[4] - r[1];
    cfg.alpha = (float)alpha, cfg.one_m_alpha = (float)(1 - alpha), cfg.gamma = (float)gamma, cfg.eps = (float)eps;
    cfg.w_cls = (float)cls_weight, cfg.w_reg = (float)reg_weight, cfg.w_iou = (float)iou_weight;
    cfg.C = num_classes, cfg.K = num_queries, cfg.Mcap = max_boxes, cfg.ncol = ncol, cfg.has_vel = ncol == 10;
    const int gx = max_boxes > 0 ? fnp_divup(max_boxes, kCostG) : 1;
    hipLaunchKernelGGL(cost_kernel, dim3(gx, fnp_divup(num_queries, kCostQ), batch_size), dim3(kCostThreads), 0, s, heatmap, center, height, dim,
                       rot, vel, gt_boxes, (const int *)valid_map, (const int *)num_valid, cfg, cost, iou, boxes);
    FNP_LAUNCH_CHECK();
    return FNP_OK;
}

extern "C" int fnp_tf_assign_targets(const int *assigned, const float *gt_boxes, int batch_size, int num_classes, int num_queries,
                                     int max_boxes, int ncol, int feature_map_stride, double voxel_x, double voxel_y, float range_x,
                                     float range_y, uint64_t unknown_mask, int64_t *labels, float *label_weights, float *bbox_targets,
                                     float *bbox_weights, unsigned char *unknown, int *num_pos, fnp_stream_t stream) {
    if (batch_size < 0 || num_classes < 1 || num_classes > 64 || num_queries < 0 || num_queries > kMaxQueries || max_boxes < 0 ||
        max_boxes > kMaxBoxes || (ncol != 8 && ncol != 10) || feature_map_stride < 1 || !num_pos)
        return FNP_ERR_ARG;
    const long long n = (long long)batch_size * num_queries;
    if (n > 0 && (!assigned || !labels || !label_weights || !bbox_targets || !bbox_weights || !unknown || (max_boxes > 0 && !gt_boxes)))
        return FNP_ERR_ARG;
    TargetCfg cfg;
    cfg.x0 = range_x, cfg.y0 = range_y;
    cfg.div_x = (float)(feature_map_stride * voxel_x), cfg.div_y = (float)(feature_map_stride * voxel_y);   // Python's f64 product
    cfg.C = num_classes, cfg.K = num_queries > 0 ? num_queries : 1, cfg.Mcap = max_boxes, cfg.ncol = ncol, cfg.code = ncol;
    cfg.unk_mask = unknown_mask;
    hipLaunchKernelGGL(target_kernel, dim3(n > 0 ? fnp_divup(n, kThreads) : 1), dim3(kThreads), 0, (hipStream_t)stream, assigned,
                       gt_boxes, n, cfg, (long long *)labels, label_weights, bbox_targets, bbox_weights, unknown, num_pos);
    FNP_LAUNCH_CHECK();
    return FNP_OK;
}

// ---- the two query losses (transfusion_head.py:500-504, :561-597; loss_utils.py SigmoidFocalClassificationLoss, L1Loss) -----------
//   loss    : one pass over the queries, a thread per (scene, query) walking its C logits and its code channels, both read from the
//             heads' own (B, n, K) arrays (no cat, no permute): f32 per element, an f64 sum per thread, then per workgroup in a
//             fixed order                                                                                       [qloss_kernel]
//   finish  : one workgroup adds the partial sums in order and divides both by max(num_pos, 1), read from the device [qloss_finish_kernel]
//   backward: one elementwise launch recomputes the derivatives and writes the gradients in the heads' layouts and dtype; the
//             focal weight is differentiated through; the L1 gradient is sign(pred - target), 0 at equality     [qloss_bwd_kernel]
// Per element, in the reference's order: t = 1 at column `label`, else 0; p = sigmoid(x); focal = (t a + (1 - t)(1 - a)) * pt^gamma
// with pt = t (1 - p) + (1 - t) p; bce = max(x, 0) - x t + log1p(exp(-|x|)); cls = (focal * bce) * w, w = label_weight, times
// unknown_cls_weight on the unknown mask.  bbox = |pred - target| * ((bbox_weight * code_weight) * unknown_code_weight on the mask).
#include "f32io.h"

namespace {

constexpr int kLossBlocks = 256;
constexpr int kMaxHeads = 8, kMaxCode = 16;

struct QLossCfg {
    const void *head[kMaxHeads];        // regression heads in HEAD_ORDER, (B, ch[h], K)
    void *grad[kMaxHeads];              // backward only
    int ch[kMaxHeads];
    int n_heads, C, K, code;
    float alpha, one_m_alpha, gamma, unk_cls_w;
    float code_w[kMaxCode], unk_code_w[kMaxCode];
};

struct FocalTerm { float loss, dloss; };   // focal * bce and its derivative in the logit

template <bool GRAD>
__device__ __forceinline__ FocalTerm focal_bce(float x, bool hit, const QLossCfg &cfg) {
    const float p = __fdiv_rn(1.f, 1.f + expf(-x));
    const float aw = hit ? cfg.alpha : cfg.one_m_alpha;
    const float pt = hit ? 1.f - p : p;
    const float ptg = cfg.gamma == 2.f ? pt * pt : powf(pt, cfg.gamma);
    const float focal = aw * ptg;
    const float bce = (fmaxf(x, 0.f) - (hit ? x : 0.f)) + log1pf(expf(-fabsf(x)));
    FocalTerm r;
    r.loss = focal * bce;
    r.dloss = 0.f;
    if (GRAD) {
        const float dpt = hit ? -(p * (1.f - p)) : p * (1.f - p);
        const float dptg = cfg.gamma == 2.f ? 2.f * pt : cfg.gamma * powf(pt, cfg.gamma - 1.f);
        r.dloss = aw * ((dptg * dpt) * bce + ptg * (p - (hit ? 1.f : 0.f)));
    }
    return r;
}

__device__ __forceinline__ double wg_sum(double v, double *part) {   // wave then workgroup, fixed order; valid in thread 0
    for (int k = 32; k > 0; k >>= 1) v += __shfl_down(v, k, 64);
    if (fnp_lane() == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int j = 0; j < kThreads / kWave; ++j) s += part[j];
    __syncthreads();
    return s;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void qloss_kernel(const T *__restrict__ logits, QLossCfg cfg, const long long *__restrict__ labels,
                                                         const float *__restrict__ label_w, const float *__restrict__ targets,
                                                         const float *__restrict__ bbox_w, const unsigned char *__restrict__ unknown,
                                                         long long n, double *__restrict__ partial) {
    __shared__ double part[kThreads / kWave];
    double acc_cls = 0.0, acc_box = 0.0;
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
        const long long b = i / cfg.K;
        const int k = (int)(i - b * cfg.K);
        const bool unk = unknown[i] != 0;
        const long long label = labels[i];
        const float w = unk ? label_w[i] * cfg.unk_cls_w : label_w[i];
        for (int c = 0; c < cfg.C; ++c) {
            const float x = load_f32<T>(logits, (b * cfg.C + c) * cfg.K + k);
            acc_cls += (double)(focal_bce<false>(x, label == c, cfg).loss * w);
        }
        int j = 0;
        for (int h = 0; h < cfg.n_heads; ++h)
            for (int c = 0; c < cfg.ch[h]; ++c, ++j) {
                const float pred = load_f32<T>((const T *)cfg.head[h], (b * cfg.ch[h] + c) * cfg.K + k);
                float rw = bbox_w[i * cfg.code + j] * cfg.code_w[j];
                if (unk) rw *= cfg.unk_code_w[j];
                acc_box += (double)(fabsf(pred - targets[i * cfg.code + j]) * rw);
            }
    }
    const double s_cls = wg_sum(acc_cls, part);
    const double s_box = wg_sum(acc_box, part);
    if (threadIdx.x == 0) partial[2 * blockIdx.x] = s_cls, partial[2 * blockIdx.x + 1] = s_box;
}

__global__ __launch_bounds__(kThreads) void qloss_finish_kernel(const double *__restrict__ partial, int n_partial,
                                                                const int *__restrict__ num_pos, float *__restrict__ loss) {
    __shared__ double part[kThreads / kWave];
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < n_partial; i += kThreads) a += partial[2 * i], b += partial[2 * i + 1];
    const double s_cls = wg_sum(a, part);
    const double s_box = wg_sum(b, part);
    if (threadIdx.x == 0) {
        const int np = *num_pos;
        const double d = (double)(np > 1 ? np : 1);
        loss[0] = (float)(s_cls / d);
        loss[1] = (float)(s_box / d);
    }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void qloss_bwd_kernel(const T *__restrict__ logits, QLossCfg cfg, const long long *__restrict__ labels,
                                                             const float *__restrict__ label_w, const float *__restrict__ targets,
                                                             const float *__restrict__ bbox_w, const unsigned char *__restrict__ unknown,
                                                             long long n, const int *__restrict__ num_pos,
                                                             const float *__restrict__ grad_out, T *__restrict__ grad_logits) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int np = *num_pos;
    const float den = (float)(np > 1 ? np : 1);
    const float s_cls = __fdiv_rn(grad_out[0], den), s_box = __fdiv_rn(grad_out[1], den);
    const long long b = i / cfg.K;
    const int k = (int)(i - b * cfg.K);
    const bool unk = unknown[i] != 0;
    const long long label = labels[i];
    const float w = unk ? label_w[i] * cfg.unk_cls_w : label_w[i];
    for (int c = 0; c < cfg.C; ++c) {
        const long long at = (b * cfg.C + c) * cfg.K + k;
        const float x = load_f32<T>(logits, at);
        store_f32<T>(grad_logits, at, (focal_bce<true>(x, label == c, cfg).dloss * w) * s_cls);
    }
    int j = 0;
    for (int h = 0; h < cfg.n_heads; ++h)
        for (int c = 0; c < cfg.ch[h]; ++c, ++j) {
            const long long at = (b * cfg.ch[h] + c) * cfg.K + k;
            const float d = load_f32<T>((const T *)cfg.head[h], at) - targets[i * cfg.code + j];
            float rw = bbox_w[i * cfg.code + j] * cfg.code_w[j];
            if (unk) rw *= cfg.unk_code_w[j];
            const float sign = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
            store_f32<T>((T *)cfg.grad[h], at, (sign * rw) * s_box);
        }
}

int qloss_cfg(QLossCfg &cfg, const void *const *heads, void *const *grads, const int *head_channels, int n_heads, int C, int K, int code,
              double alpha, double gamma, const float *code_weights, const float *unknown_code_weights, double unknown_cls_weight) {
    if (n_heads < 1 || n_heads > kMaxHeads || C < 1 || K < 1 || K > kMaxQueries || code < 1 || code > kMaxCode || !heads || !head_channels ||
        !code_weights)
        return FNP_ERR_ARG;
    int sum = 0;
    for (int h = 0; h < kMaxHeads; ++h) {
        cfg.head[h] = h < n_heads ? heads[h] : nullptr;
        cfg.grad[h] = (grads && h < n_heads) ? grads[h] : nullptr;
        cfg.ch[h] = h < n_heads ? head_channels[h] : 0;
        if (h < n_heads && (!heads[h] || head_channels[h] < 1 || (grads && !grads[h]))) return FNP_ERR_ARG;
        sum += cfg.ch[h];
    }
    if (sum != code) return FNP_ERR_ARG;
    cfg.n_heads = n_heads, cfg.C = C, cfg.K = K, cfg.code = code;
    cfg.alpha = (float)alpha, cfg.one_m_alpha = (float)(1 - alpha), cfg.gamma = (float)gamma, cfg.unk_cls_w = (float)unknown_cls_weight;
    for (int j = 0; j < kMaxCode; ++j) {
        cfg.code_w[j] = j < code ? code_weights[j] : 0.f;
        cfg.unk_code_w[j] = (j < code && unknown_code_weights) ? unknown_code_weights[j] : 1.f;
    }
    return FNP_OK;
}

}  // namespace

extern "C" int64_t fnp_tf_query_loss_workspace_bytes(void) { return 16ll * kLossBlocks; }

extern "C" int fnp_tf_query_loss_forward(const void *heatmap, const void *const *heads, const int *head_channels, int n_heads, int dtype,
                                         int batch_size, int num_classes, int num_queries, int code_size, const int64_t *labels,
                                         const float *label_weights, const float *bbox_targets, const float *bbox_weights,
                                         const unsigned char *unknown, const int *num_pos, double alpha, double gamma,
                                         const float *code_weights, const float *unknown_code_weights, double unknown_cls_weight,
                                         void *workspace, int64_t workspace_bytes, float *loss, fnp_stream_t stream) {
    QLossCfg cfg;
    if (batch_size < 1 || !heatmap || !labels || !label_weights || !bbox_targets || !bbox_weights || !unknown || !num_pos || !loss ||
        !workspace || ((uintptr_t)workspace & 7))
        return FNP_ERR_ARG;
    if (qloss_cfg(cfg, heads, nullptr, head_channels, n_heads, num_classes, num_queries, code_size, alpha, gamma, code_weights,
                  unknown_code_weights, unknown_cls_weight) != FNP_OK || (dtype != FNP_F32 && dtype != FNP_F16 && dtype != FNP_BF16))
        return FNP_ERR_ARG;
    if (workspace_bytes < 16ll * kLossBlocks) return FNP_ERR_WORKSPACE;
    const long long n = (long long)batch_size * num_queries;
    const int G = fnp_grid_for(n, kThreads, kLossBlocks);
    double *partial = (double *)workspace;
    hipStream_t s = (hipStream_t)stream;
#define FNP_QLOSS(T)                                                                                                              \
    hipLaunchKernelGGL(qloss_kernel<T>, dim3(G), dim3(kThreads), 0, s, (const T *)heatmap, cfg, (const long long *)labels, label_weights, \
                       bbox_targets, bbox_weights, unknown, n, partial)
    if (dtype == FNP_F32) FNP_QLOSS(float);
    else if (dtype == FNP_F16) FNP_QLOSS(__half);
    else FNP_QLOSS(unsigned short);
#undef FNP_QLOSS
    FNP_LAUNCH_CHECK();
    hipLaunchKernelGGL(qloss_finish_kernel, dim3(1), dim3(kThreads), 0, s, (const double *)partial, G, num_pos, loss);
    FNP_LAUNCH_CHECK();
    return FNP_OK;
}

extern "C" int fnp_tf_query_loss_backward(const void *heatmap, const void *const *heads, const int *head_channels, int n_heads, int dtype,
                                          int batch_size, int num_classes, int num_queries, int code_size, const int64_t *labels,
                                          const float *label_weights, const float *bbox_targets, const float *bbox_weights,
                                          const unsigned char *unknown, const int *num_pos, double alpha, double gamma,
                                          const float *code_weights, const float *unknown_code_weights, double unknown_cls_weight,
                                          const float *grad_out, void *grad_heatmap, void *const *grad_heads, fnp_stream_t stream) {
    QLossCfg cfg;
    if (batch_size < 1 || !heatmap || !labels || !label_weights || !bbox_targets || !bbox_weights || !unknown || !num_pos || !grad_out ||
        !grad_heatmap || !grad_heads)
        return FNP_ERR_ARG;
    if (qloss_cfg(cfg, heads, grad_heads, head_channels, n_heads, num_classes, num_queries, code_size, alpha, gamma, code_weights,
                  unknown_code_weights, unknown_cls_weight) != FNP_OK || (dtype != FNP_F32 && dtype != FNP_F16 && dtype != FNP_BF16))
        return FNP_ERR_ARG;
    const long long n = (long long)batch_size * num_queries;
    const int G = fnp_divup(n, kThreads);
    hipStream_t s = (hipStream_t)stream;
#define FNP_QLOSS_BWD(T)                                                                                                              \
    hipLaunchKernelGGL(qloss_bwd_kernel<T>, dim3(G), dim3(kThreads), 0, s, (const T *)heatmap, cfg, (const long long *)labels, label_weights, \
                       bbox_targets, bbox_weights, unknown, n, num_pos, grad_out, (T *)grad_heatmap)
    if (dtype == FNP_F32) FNP_QLOSS_BWD(float);
    else if (dtype == FNP_F16) FNP_QLOSS_BWD(__half);
    else FNP_QLOSS_BWD(unsigned short);
#undef FNP_QLOSS_BWD
    FNP_LAUNCH_CHECK();
    return FNP_OK;
}
