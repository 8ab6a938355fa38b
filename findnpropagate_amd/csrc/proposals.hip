// Inference side of TransFusionHead around its decoder (pcdet/models/dense_heads/transfusion_head.py): the heatmap proposals
// of predict (:201-294, :321-324), the query initialisation (:295-313) and get_bboxes + decode_bbox(filter=True) (:616-728).
// The reference runs a full-map sigmoid, a max_pool2d with three elementwise passes, a full argsort of C*H*W values per
// scene to keep K of them, three gathers, a one-hot Conv1d, some twenty small launches in the decode and a Python loop with
// an .item() per query.  Here:
//
//   1. proposals : fill (the per-scene key count), then
//        prop_mask_kernel   a workgroup per 32 x 8 tile of one (scene, class) plane reads every value once through an LDS
//                           tile with a one-cell halo, and appends the 64-bit keys of its POSITIVE survivors to the scene's
//                           key list (compacted in the workgroup, one atomic per workgroup);
//        prop_select_kernel one workgroup per scene: a radix select over the keys finds the prefix at which the count
//                           reaches K (a 4096-bin LDS histogram of the top 12 bits, then 10 bits per further pass over the
//                           key list, only while the candidates do not fit LDS), gathers the <= 4096 candidates, sorts
//                           them in LDS (bitonic), writes the K results and the zero fill, and then query_heatmap_score
//                           for all C classes at the chosen cells.  Every pass over the key list loads eight keys per
//                           thread before it uses one (a one-key loop is a chain of ~90 dependent memory latencies).
//      A first version merged a per-workgroup histogram into a per-scene one in pass 1 and took one atomic per wave: some
//      200,000 global atomics per scene on a few cache lines made pass 1 cost 40 us per scene (122 us for the three launches
//      at one scene).
//      Three launches, no host read, nothing allocated.
//   2. query init: one elementwise launch [query_init_kernel]
//   3. box decode: one workgroup per scene, a thread per query, compacted in query order [tf_decode_kernel]
//
// KEY: (value bits << 32) | (0xFFFFFFFF - flat), flat = c*H*W + h*W + w.  Positive f32 values order as their bits, so the
// descending key order is: value descending, then flat index ascending — a total order on unique keys.  The append order of
// pass 1 (atomics) therefore cannot reach the results: they are bit-identical from run to run.
//
// DECODE ARITHMETIC: centres are the reference's f32 sequence (two multiplications, one addition, not contracted) and are
// bit-exact.  The score sigmoid(x) * q, the sizes exp(d) and the yaw atan2(s, c) are formed in f64 and rounded once to f32
// (K threads per scene: the cost is nothing): within 0.5 ulp and a hair of the true value, which is inside twice the error
// of the reference's own f32 run (0.5 ulp for sizes and yaw, about 1 ulp for scores) whatever the inputs; the f32 functions
// expf and atan2f carry 1 ulp and more and would meet that only by luck.
//
// MASKED VALUE: prop_prob() and prop_masked() below are the only definition of it; the selecting pass and the
// query_heatmap_score pass both call them, so the two cannot disagree.
#include "common.h"
#include "tfdecode.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTileW = 32, kTileH = 8;            // kTileW * kTileH == kThreads
constexpr int kLdsW = kTileW + 2, kLdsH = kTileH + 2;
constexpr int kBins0 = 4096;                      // top 12 bits of the key = sign, exponent and 3 mantissa bits of the value
constexpr int kShift0 = 52;
constexpr int kDigit = 10;                        // bits per further radix pass: 1024 bins, one per thread
constexpr int kSelThreads = 1024;
constexpr int kCap = 4096;                        // candidate keys sorted in LDS
constexpr int kMaxK = 2048;
constexpr int kHeaderWords = 64;                  // per scene: the key count (word 0), one 256-byte line
constexpr int kUnroll = 8;                        // keys in flight per thread in a pass over the key list

typedef unsigned long long u64;

// the probability of a heatmap value: the fused sigmoid is exactly this expression (no contraction: -ffp-contract=off)
__device__ __forceinline__ float prop_prob(float x, int from_logits) { return from_logits ? 1.0f / (1.0f + expf(-x)) : x; }

// s: the cell's probability, m: the maximum of its 3 x 3 neighbourhood (itself included), interior: not on the map's border
__device__ __forceinline__ float prop_masked(float s, float m, bool interior, bool point_class) {
    if (point_class) return s;
    return (interior && s == m) ? s : 0.f;
}

// the masked value of one cell straight from global memory (the query_heatmap_score pass)
__device__ float prop_masked_at(const float *__restrict__ plane, int h, int w, int H, int W, int from_logits, bool point_class) {
    const float s = prop_prob(plane[(size_t)h * W + w], from_logits);
    const bool interior = h > 0 && h < H - 1 && w > 0 && w < W - 1;
    float m = s;
    if (!point_class && interior) {
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) m = fmaxf(m, prop_prob(plane[(size_t)(h + dy) * W + (w + dx)], from_logits));
    }
    return prop_masked(s, m, interior, point_class);
}

__global__ __launch_bounds__(kThreads) void prop_mask_kernel(const float *__restrict__ heat, int C, int H, int W, int from_logits,
                                                             u64 point_mask, unsigned *__restrict__ header, u64 *__restrict__ keys,
                                                             long long cap) {
    __shared__ float tile[kLdsH][kLdsW + 1];
    __shared__ int wcnt[kWaves];
    __shared__ unsigned wg_base;
    const int tiles_x = (W + kTileW - 1) / kTileW;
    const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x, c = blockIdx.y, b = blockIdx.z;
    const int x_lo = tx * kTileW, y_lo = ty * kTileH;
    const float *plane = heat + ((size_t)b * C + c) * H * W;
    for (int i = threadIdx.x; i < kLdsH * kLdsW; i += kThreads) {
        const int ly = i / kLdsW, lx = i - ly * kLdsW;
        const int y = y_lo + ly - 1, x = x_lo + lx - 1;
        float v = 0.f;                             // outside the map: never read (a border cell is no interior cell)
        if (y >= 0 && y < H && x >= 0 && x < W) v = prop_prob(plane[(size_t)y * W + x], from_logits);
        tile[ly][lx] = v;
    }
    __syncthreads();
    const int lx = threadIdx.x & (kTileW - 1), ly = threadIdx.x / kTileW;
    const int x = x_lo + lx, y = y_lo + ly;
    const bool point_class = (point_mask >> c) & 1ull;
    float v = 0.f;
    if (x < W && y < H) {
        const float s = tile[ly + 1][lx + 1];
        const bool interior = y > 0 && y < H - 1 && x > 0 && x < W - 1;
        float m = s;
        if (!point_class && interior) {
            for (int dy = 0; dy < 3; ++dy)
                for (int dx = 0; dx < 3; ++dx) m = fmaxf(m, tile[ly + dy][lx + dx]);
        }
        v = prop_masked(s, m, interior, point_class);
    }
    const bool keep = v > 0.f;                     // (false for a NaN, which is out of contract)
    const u64 bal = __ballot(keep);
    const int wave = threadIdx.x >> 6;
    if (fnp_lane() == 0) wcnt[wave] = __popcll(bal);
    __syncthreads();
    int pos = __popcll(bal & ((1ull << fnp_lane()) - 1ull)), total = 0;
    for (int j = 0; j < kWaves; ++j) {
        if (j < wave) pos += wcnt[j];
        total += wcnt[j];
    }
    if (total == 0) return;                        // (the same in every thread)
    if (threadIdx.x == 0) wg_base = atomicAdd(header + (size_t)b * kHeaderWords, (unsigned)total);
    __syncthreads();
    if (keep) {
        const long long at = (long long)wg_base + pos;
        const unsigned flat = (unsigned)(((size_t)c * H + y) * W + x);
        if (at < cap) keys[(size_t)b * cap + at] = ((u64)__float_as_uint(v) << 32) | (u64)(0xFFFFFFFFu - flat);
    }
}

// One pass of the workgroup over keys[0, n): every thread loads kUnroll keys, then hands them to f.
template <class F>
__device__ __forceinline__ void prop_for_keys(const u64 *__restrict__ keys, int n, F f) {
    for (long long base = 0; base < n; base += kUnroll * kSelThreads) {
        u64 k[kUnroll];
#pragma unroll
        for (int j = 0; j < kUnroll; ++j) {
            const long long i = base + j * kSelThreads + (int)threadIdx.x;
            k[j] = i < n ? keys[i] : 0ull;         // 0 is no key: a key's value bits are > 0
        }
#pragma unroll
        for (int j = 0; j < kUnroll; ++j)
            if (k[j]) f(k[j]);
    }
}

// Finds the bin T of hist[0, nb) with (sum of the bins above T) < r <= (sum of the bins from T up), for 1 <= r <= the total.
// -> ctl[0] = T, ctl[1] = the sum above T, ctl[2] = hist[T].  Every thread of the workgroup calls it.
__device__ void prop_find_bin(const int *hist, int nb, int r, int *scan, int *ctl) {
    const int t = threadIdx.x;
    const int per = nb >= kSelThreads ? nb / kSelThreads : 1;
    int local = 0;
    for (int j = 0; j < per; ++j) {
        const int i = t * per + j;
        if (i < nb) local += hist[i];
    }
    scan[t] = local;
    __syncthreads();
    for (int off = 1; off < kSelThreads; off <<= 1) {   // inclusive suffix sum
        const int v = scan[t] + (t + off < kSelThreads ? scan[t + off] : 0);
        __syncthreads();
        scan[t] = v;
        __syncthreads();
    }
    const int incl = scan[t], excl = incl - local;
    if (excl < r && r <= incl) {                         // exactly one thread
        int acc = excl;
        for (int j = per - 1; j >= 0; --j) {
            const int i = t * per + j;
            const int n = i < nb ? hist[i] : 0;
            if (acc + n >= r) {
                ctl[0] = i, ctl[1] = acc, ctl[2] = n;
                break;
            }
            acc += n;
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(kSelThreads) void prop_select_kernel(const float *__restrict__ heat, int C, int H, int W, int K,
                                                                  int from_logits, u64 point_mask,
                                                                  const unsigned *__restrict__ header, const u64 *__restrict__ keys,
                                                                  long long cap, long long *__restrict__ top_class,
                                                                  long long *__restrict__ top_index, float *__restrict__ top_score,
                                                                  float *__restrict__ qhs) {
    __shared__ u64 skey[kCap];
    __shared__ int shist[kBins0];
    __shared__ int sscan[kSelThreads];
    __shared__ int sflat[kMaxK];
    __shared__ int ctl[4];
    const int t = threadIdx.x, b = blockIdx.x;
    const unsigned *scene_hdr = header + (size_t)b * kHeaderWords;
    const u64 *scene_keys = keys + (size_t)b * cap;
    const long long HW = (long long)H * W;
    long long n_ll = scene_hdr[0];
    const int n = (int)(n_ll < cap ? n_ll : cap);       // positive survivors of the scene
    const int need = n < K ? n : K;
    // radix select: the keys with (key >> shift) >= prefix are `above` + `at` <= kCap candidates that hold the top `need`
    int shift = 0;
    u64 prefix = 0;
    if (n > kCap) {
        for (int i = t; i < kBins0; i += kSelThreads) shist[i] = 0;
        if (t == 0) ctl[0] = 0, ctl[1] = 0, ctl[2] = 0;
        __syncthreads();
        prop_for_keys(scene_keys, n, [&](u64 k) { atomicAdd(&shist[(int)(k >> kShift0)], 1); });   // (v > 0: below 2048)
        __syncthreads();
        int above = 0, nb = kBins0;
        shift = kShift0;
        for (;;) {
            prop_find_bin(shist, nb, need - above, sscan, ctl);
            const int T = ctl[0];
            above += ctl[1];
            const int at = ctl[2];
            prefix = (prefix << (nb == kBins0 ? 12 : (nb == 4 ? 2 : kDigit))) | (u64)T;
            __syncthreads();
            if (above + at <= kCap || shift == 0) break;
            const int bits = shift >= kDigit ? kDigit : shift;   // 52 = 5 * 10 + 2
            const int nshift = shift - bits;
            nb = 1 << bits;
            for (int i = t; i < kSelThreads; i += kSelThreads) shist[i] = 0;
            if (t == 0) ctl[0] = 0, ctl[1] = 0, ctl[2] = 0;
            __syncthreads();
            prop_for_keys(scene_keys, n, [&](u64 k) {
                if ((k >> shift) == prefix) atomicAdd(&shist[(int)((k >> nshift) & (u64)(nb - 1))], 1);
            });
            __syncthreads();
            shift = nshift;
        }
    }
    if (t == 0) ctl[3] = 0;
    __syncthreads();
    prop_for_keys(scene_keys, n, [&](u64 k) {
        if ((k >> shift) >= prefix) {
            const int p = atomicAdd(&ctl[3], 1);
            if (p < kCap) skey[p] = k;
        }
    });
    __syncthreads();
    const int cnt = ctl[3] < kCap ? ctl[3] : kCap;
    int m = 1;
    while (m < cnt) m <<= 1;
    for (int i = cnt + t; i < m; i += kSelThreads) skey[i] = 0;       // below every key (a key's value bits are > 0)
    __syncthreads();
    for (int k2 = 2; k2 <= m; k2 <<= 1) {                              // bitonic, descending
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            for (int i = t; i < (m >> 1); i += kSelThreads) {
                const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo | j;
                const bool desc = (lo & k2) == 0;
                const u64 a = skey[lo], c = skey[hi];
                if ((a < c) == desc) skey[lo] = c, skey[hi] = a;
            }
            __syncthreads();
        }
    }
    long long *o_class = top_class + (size_t)b * K, *o_index = top_index + (size_t)b * K;
    float *o_score = top_score + (size_t)b * K;
    for (int k = t; k < need; k += kSelThreads) {
        const u64 key = skey[k];
        const unsigned flat = 0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull);
        sflat[k] = (int)flat;
        o_class[k] = (long long)flat / HW;
        o_index[k] = (long long)flat % HW;
        o_score[k] = __uint_as_float((unsigned)(key >> 32));
    }
    if (need < K) {
        // zero fill: the lowest flat indices that are no positive survivor; K - need of them lie in [0, K).  Here n < K: every
        // survivor is in skey.
        for (int i = t; i < K; i += kSelThreads) shist[i] = 0;
        __syncthreads();
        for (int i = t; i < n; i += kSelThreads) {
            const unsigned flat = 0xFFFFFFFFu - (unsigned)(skey[i] & 0xFFFFFFFFull);
            if (flat < (unsigned)K) shist[flat] = 1;
        }
        __syncthreads();
        const int i0 = 2 * t, i1 = 2 * t + 1;                          // K <= kMaxK = 2 * kSelThreads
        const int f0 = (i0 < K && !shist[i0]) ? 1 : 0, f1 = (i1 < K && !shist[i1]) ? 1 : 0;
        sscan[t] = f0 + f1;
        __syncthreads();
        for (int off = 1; off < kSelThreads; off <<= 1) {              // inclusive prefix sum
            const int v = sscan[t] + (t >= off ? sscan[t - off] : 0);
            __syncthreads();
            sscan[t] = v;
            __syncthreads();
        }
        const int excl = sscan[t] - f0 - f1;
        if (f0) {
            const int k = need + excl;
            if (k < K) sflat[k] = i0, o_class[k] = i0 / HW, o_index[k] = i0 % HW, o_score[k] = 0.f;
        }
        if (f1) {
            const int k = need + excl + f0;
            if (k < K) sflat[k] = i1, o_class[k] = i1 / HW, o_index[k] = i1 % HW, o_score[k] = 0.f;
        }
    }
    __syncthreads();
    // query_heatmap_score[b, c, k]: the masked value of class c at top_index[b, k]
    const float *scene_heat = heat + (size_t)b * C * HW;
    float *o_qhs = qhs + (size_t)b * C * K;
    for (int i = t; i < C * K; i += kSelThreads) {
        const int c = i / K, k = i - c * K;
        const int cell = (int)((long long)sflat[k] % HW);
        const int h = cell / W, w = cell - h * W;
        o_qhs[i] = prop_masked_at(scene_heat + (size_t)c * HW, h, w, H, W, from_logits, (point_mask >> c) & 1ull);
    }
}

__global__ __launch_bounds__(kThreads) void query_init_kernel(const float *__restrict__ feat, const float *__restrict__ bev_pos,
                                                              long long bev_scene_stride, const float *__restrict__ enc_w,
                                                              const float *__restrict__ enc_b, const long long *__restrict__ top_class,
                                                              const long long *__restrict__ top_index, int F, long long HW, int C,
                                                              int K, long long total, long long total_pos,
                                                              float *__restrict__ query_feat, float *__restrict__ query_pos) {
    const float nan = __uint_as_float(0x7fc00000u);
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < total; i += (long long)gridDim.x * kThreads) {
        const int k = (int)(i % K);
        const long long bf = i / K;
        const int f = (int)(bf % F);
        const long long b = bf / F;
        const long long idx = top_index[b * K + k], cls = top_class[b * K + k];
        float v = nan;                                                  // an index outside the map is never followed
        if (idx >= 0 && idx < HW && cls >= 0 && cls < C) v = feat[(size_t)bf * HW + idx] + (enc_w[(size_t)f * C + cls] + enc_b[f]);
        query_feat[i] = v;
        if (i < total_pos) {                                            // (B, K, 2): element i is (b', k', j)
            const int j = (int)(i & 1);
            const long long bk = i >> 1, bb = bk / K;
            const long long id2 = top_index[bk];
            query_pos[i] = (id2 >= 0 && id2 < HW) ? bev_pos[bb * bev_scene_stride + id2 * 2 + (1 - j)] : nan;
        }
    }
}

struct DecodeCfg {
    float stride, vx, vy, x0, y0;
    float thresh, thresh_unk;
    float rmin[3], rmax[3];
    u64 unk_mask;
    int C, K, has_vel;
};

__global__ __launch_bounds__(kThreads) void tf_decode_kernel(const float *__restrict__ heatmap, const float *__restrict__ qhs,
                                                             const float *__restrict__ center, const float *__restrict__ height,
                                                             const float *__restrict__ dim, const float *__restrict__ rot,
                                                             const float *__restrict__ vel, const long long *__restrict__ labels_in,
                                                             const int *__restrict__ relabel, DecodeCfg cfg, float *__restrict__ boxes,
                                                             float *__restrict__ scores, int *__restrict__ labels, int *__restrict__ counts) {
    __shared__ int wcnt[kWaves];
    const int b = blockIdx.x, K = cfg.K, C = cfg.C, ncol = cfg.has_vel ? 9 : 7;
    float *o_box = boxes + (size_t)b * K * ncol, *o_score = scores + (size_t)b * K;
    int *o_label = labels + (size_t)b * K;
    int kept = 0;
    for (int base = 0; base < K; base += kThreads) {
        const int k = base + threadIdx.x;
        bool keep = false;
        float box[9], score = 0.f;
        int label = 0;
        if (k < K) {
            const long long q = labels_in[(size_t)b * K + k];
            float v = 0.f;
            if (q >= 0 && q < C) {
                const size_t at = ((size_t)b * C + q) * K + k;
                v = (float)((1.0 / (1.0 + exp(-(double)heatmap[at]))) * (double)qhs[at]);
            }
            label = v > 0.f ? (int)q : 0;      // the maximum over an all-zero column is at index 0
            score = v > 0.f ? v : 0.f;
            tf_decode_box(center, height, dim, rot, cfg.has_vel ? vel : nullptr, (size_t)b, k, K, cfg.stride, cfg.vx, cfg.vy, cfg.x0,
                          cfg.y0, box);
            const float thresh = ((cfg.unk_mask >> label) & 1ull) ? cfg.thresh_unk : cfg.thresh;   // bit (1-based label - 1)
            keep = score > thresh;
            for (int j = 0; j < 3; ++j) keep = keep && box[j] >= cfg.rmin[j] && box[j] <= cfg.rmax[j];
            label += 1;
            if (relabel) label = relabel[label];
        }
        const u64 bal = __ballot(keep);
        const int wave = threadIdx.x >> 6;
        if (fnp_lane() == 0) wcnt[wave] = __popcll(bal);
        __syncthreads();
        int pos = kept + __popcll(bal & ((1ull << fnp_lane()) - 1ull));
        for (int j = 0; j < kWaves; ++j) {
            if (j < wave) pos += wcnt[j];
            kept += wcnt[j];
        }
        __syncthreads();
        if (keep) {
            float *row = o_box + (size_t)pos * ncol;
#pragma unroll
            for (int j = 0; j < 7; ++j) row[j] = box[j];
            if (cfg.has_vel) row[7] = box[7], row[8] = box[8];
            o_score[pos] = score;
            o_label[pos] = label;
        }
    }
    for (int k = kept + threadIdx.x; k < K; k += kThreads) {           // the padding rows: every element is written
        for (int j = 0; j < ncol; ++j) o_box[(size_t)k * ncol + j] = 0.f;
        o_score[k] = 0.f;
        o_label[k] = 0;
    }
    if (threadIdx.x == 0) counts[b] = kept;
}

long long prop_tiles(int H, int W) { return (long long)((W + kTileW - 1) / kTileW) * ((H + kTileH - 1) / kTileH); }

bool prop_shape_ok(int B, int C, int H, int W, int K) {
    if (B < 0 || B > 65535 || C < 1 || C > 64 || H < 1 || W < 1 || K < 1 || K > kMaxK) return false;
    const long long cells = (long long)C * H * W;
    return cells < 0x7fffffffll && K <= cells && prop_tiles(H, W) <= 0x7fffffffll;
}

}  // namespace

extern "C" int64_t fnp_proposals_workspace_bytes(int batch_size, int num_classes, int height, int width, int num_proposals) {
    if (!prop_shape_ok(batch_size, num_classes, height, width, num_proposals)) return FNP_ERR_ARG;
    const long long B = batch_size > 0 ? batch_size : 1;
    return B * kHeaderWords * 4ll + B * (long long)num_classes * height * width * 8ll;
}

extern "C" int fnp_proposals(const float *heatmap, int batch_size, int num_classes, int height, int width, int num_proposals,
                             int from_logits, uint64_t point_class_mask, void *workspace, int64_t workspace_bytes,
                             int64_t *top_class, int64_t *top_index, float *top_score, float *query_heatmap_score,
                             fnp_stream_t stream) {
    if (!prop_shape_ok(batch_size, num_classes, height, width, num_proposals)) return FNP_ERR_ARG;
    if (batch_size == 0) return FNP_OK;
    if (!heatmap || !workspace || ((uintptr_t)workspace & 7) || !top_class || !top_index || !top_score || !query_heatmap_score)
        return FNP_ERR_ARG;
    if (workspace_bytes < fnp_proposals_workspace_bytes(batch_size, num_classes, height, width, num_proposals)) return FNP_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const long long cap = (long long)num_classes * height * width;
    unsigned *header = (unsigned *)workspace;
    u64 *keys = (u64 *)(header + (size_t)batch_size * kHeaderWords);   // kHeaderWords * 4 is a multiple of 8
    const int rc = fnp_fill_words(header, (long long)batch_size * kHeaderWords, 0u, s);
    if (rc != FNP_OK) return rc;
    hipLaunchKernelGGL(prop_mask_kernel, dim3((unsigned)prop_tiles(height, width), num_classes, batch_size), dim3(kThreads), 0, s,
                       heatmap, num_classes, height, width, from_logits ? 1 : 0, (u64)point_class_mask, header, keys, cap);
    FNP_LAUNCH_CHECK();
    hipLaunchKernelGGL(prop_select_kernel, dim3(batch_size), dim3(kSelThreads), 0, s, heatmap, num_classes, height, width,
                       num_proposals, from_logits ? 1 : 0, (u64)point_class_mask, (const unsigned *)header, (const u64 *)keys, cap,
                       (long long *)top_class, (long long *)top_index, top_score, query_heatmap_score);
    FNP_LAUNCH_CHECK();
    return FNP_OK;
}

extern "C" int fnp_query_init(const float *lidar_feat, const float *bev_pos, int bev_pos_batched, const float *enc_weight,
                              const float *enc_bias, const int64_t *top_class, const int64_t *top_index, int batch_size,
                              int num_features, int64_t num_cells, int num_classes, int num_proposals, float *query_feat,
                              float *query_pos, fnp_stream_t stream) {
    if (batch_size < 0 || num_features < 1 || num_cells < 1 || num_classes < 1 || num_proposals < 1) return FNP_ERR_ARG;
    if (batch_size == 0) return FNP_OK;
    if (!lidar_feat || !bev_pos || !enc_weight || !enc_bias || !top_class || !top_index || !query_feat || !query_pos) return FNP_ERR_ARG;
    const long long total = (long long)batch_size * num_features * num_proposals, total_pos = (long long)batch_size * num_proposals * 2;
    if (total_pos > total && num_features < 2) return FNP_ERR_ARG;     // (F >= 2 makes the feature grid cover the positions)
    hipLaunchKernelGGL(query_init_kernel, dim3(fnp_grid_for(total, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, lidar_feat, bev_pos,
                       bev_pos_batched ? (long long)num_cells * 2 : 0ll, enc_weight, enc_bias, (const long long *)top_class,
                       (const long long *)top_index, num_features, (long long)num_cells, num_classes, num_proposals, total, total_pos,
                       query_feat, query_pos);
    FNP_LAUNCH_CHECK();
    return FNP_OK;
}

extern "C" int fnp_tf_decode(const float *heatmap, const float *query_heatmap_score, const float *center, const float *height,
                             const float *dim, const float *rot, const float *vel, const int64_t *query_labels, int batch_size,
                             int num_classes, int num_proposals, int feature_map_stride, float voxel_x, float voxel_y, float range_x,
                             float range_y, float score_thresh, float score_thresh_unk, uint64_t unknown_mask,
                             const float *post_center_range, const int *relabel, float *boxes, float *scores, int *labels,
                             int *counts, fnp_stream_t stream) {
    if (batch_size < 0 || batch_size > 0x7fffffff / 2 || num_classes < 1 || num_classes > 64 || num_proposals < 1 || !post_center_range)
        return FNP_ERR_ARG;
    if (batch_size == 0) return FNP_OK;
    if (!heatmap || !query_heatmap_score || !center || !height || !dim || !rot || !query_labels || !boxes || !scores || !labels || !counts)
        return FNP_ERR_ARG;
    DecodeCfg cfg;
    cfg.stride = (float)feature_map_stride, cfg.vx = voxel_x, cfg.vy = voxel_y, cfg.x0 = range_x, cfg.y0 = range_y;
    cfg.thresh = score_thresh, cfg.thresh_unk = score_thresh_unk, cfg.unk_mask = unknown_mask;
    for (int j = 0; j < 3; ++j) cfg.rmin[j] = post_center_range[j], cfg.rmax[j] = post_center_range[3 + j];
    cfg.C = num_classes, cfg.K = num_proposals, cfg.has_vel = vel ? 1 : 0;
    hipLaunchKernelGGL(tf_decode_kernel, dim3(batch_size), dim3(kThreads), 0, (hipStream_t)stream, heatmap, query_heatmap_score, center,
                       height, dim, rot, vel, (const long long *)query_labels, relabel, cfg, boxes, scores, labels, counts);
    FNP_LAUNCH_CHECK();
    return FNP_OK;
}
