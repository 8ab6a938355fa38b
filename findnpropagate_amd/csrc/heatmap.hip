// Dense heatmap targets and the heatmap loss of TransFusionHead (pcdet/models/dense_heads/transfusion_head.py:446-470 and
// :492-498, with centernet_utils.gaussian_radius / draw_gaussian_to_heatmap, loss_utils.GaussianFocalLoss and
// transfusion_utils.clip_sigmoid).  The reference draws one ground-truth box at a time from Python, about twenty tensor
// operations, several device-to-host reads and one numpy Gaussian per box; the loss behind it is some fifteen elementwise
// launches forward, as many backward, and an .item().  Here:
//
//   1. params : a thread per (scene, box) -> {class, cx, cy, r}; class -1 = skipped                    [hm_params_kernel]
//   2. draw   : a workgroup per 32 x 8 tile of one (scene, class) plane gathers: it compacts the scene's boxes of its class
//               whose window meets the tile into LDS, 256 boxes at a time (no cap on M), and every thread takes the maximum
//               over the boxes that cover its pixel.  Every element of (B, C, H, W) is written exactly once: no clear pass,
//               no atomics, and (a maximum) no dependence on box order.  The elements equal to 1 are counted per workgroup
//               and summed by one workgroup into num_pos                                [hm_draw_kernel, hm_count_kernel]
//   3. loss   : GaussianFocalLoss(clip_sigmoid(x), t).sum() / max(num_pos, 1) in one pass, f32 per element, f64 partial sums
//               per thread and per workgroup in a fixed order, finished by one workgroup that reads num_pos from device
//               memory                                                              [hm_loss_kernel, hm_loss_finish_kernel]
//               backward: one elementwise kernel that recomputes dT/dx from the logits and the targets and scales it by
//               grad_out / max(num_pos, 1), both read from device memory                              [hm_loss_bwd_kernel]
// Nothing here allocates or synchronises.
//
// PARAMETER ARITHMETIC: parity is with the reference run on the CPU (on a GPU torch divides by a host scalar as a
// multiplication by its reciprocal, a last-bit difference the fixtures cannot pin; MeanVFE is held the same way).  Every
// f32 division and square root is formed in f64 and rounded once to f32: for f32 operands that IS the correctly rounded f32
// result (53 >= 2 * 24 + 2), whatever the compiler's f32 division and sqrt lower to.
//
// GAUSSIAN WEIGHTS: float32(exp_f64(-(dx^2 + dy^2) / (2 sigma^2))), sigma = (2r + 1) / 6 in f64, numpy's operation order.
// exp and the rounding to f32 are monotone, so the maximum over boxes is taken over the f64 ARGUMENTS and exp runs once per
// pixel.  For every radius 0..128 and every offset the f64 weight lies >= 209 f64 ulps from an f32 rounding midpoint, so an
// exp within a few ulps rounds to numpy's f32; above 128 the arithmetic is the same, the proof is not made.
// gaussian2D's `h[h < eps * h.max()] = 0` is left out: it never fires (the smallest weight of any radius is the corner's,
// about exp(-9), against eps = 2.2e-16).
#include "common.h"
#include "f32io.h"

#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTileW = 32, kTileH = 8;          // kTileW * kTileH == kThreads; a tile row is one 128-byte line
constexpr int kMaxRadius = 1 << 20;             // out-of-contract sizes are clamped so that no integer below can overflow
constexpr int kMaxCentre = 1 << 30;
constexpr int kLossBlocks = 1024;               // upper bound of the loss grid = partial sums the finishing workgroup reads

struct HmCfg {
    float vx, vy, stride, x0, y0;
    float k1n, k1d, k2, kb3, kc3, k4a3;         // f32(1-o), f32(1+o), f32(1-o), f32(-2o), f32(o-1), f32(4*(4o)), formed in f64
    int min_radius, num_classes;
    unsigned long long unk_mask;                // bit (label - 1) set: the 1-based label is an unknown class
    double unk_mult;
};

__device__ __forceinline__ float div_rn(float a, float b) { return (float)((double)a / (double)b); }
__device__ __forceinline__ float sqrt_rn(float a) { return (float)sqrt((double)a); }
__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= 3.402823466e38f; }   // false for NaN

__global__ __launch_bounds__(kThreads) void hm_params_kernel(const float *__restrict__ boxes, long long n, int ncol, HmCfg cfg,
                                                             int4 *__restrict__ out) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const float *b = boxes + (size_t)i * ncol;
    const float x = b[0], y = b[1], lab = b[ncol - 1];
    int4 r = make_int4(-1, 0, 0, 0);
    const float w = div_rn(div_rn(b[3], cfg.vx), cfg.stride);
    const float h = div_rn(div_rn(b[4], cfg.vy), cfg.stride);   // gaussian_radius(height = length, width = width)
    // the reference raises on a label above C and wraps on one below 1: both out of contract here, skipped like padding
    if (b[3] > 0.f && b[4] > 0.f && w > 0.f && h > 0.f && finite_f(w) && finite_f(h) && finite_f(x) && finite_f(y) && lab >= 1.f &&
        lab < (float)(cfg.num_classes + 1)) {
        const int label = (int)lab;   // (.long() truncates)
        const float hw = h + w;
        const float b1 = hw;
        const float c1 = div_rn((w * h) * cfg.k1n, cfg.k1d);
        const float r1 = (b1 + sqrt_rn(b1 * b1 - 4.f * c1)) * 0.5f;
        const float b2 = 2.f * hw;
        const float c2 = (cfg.k2 * w) * h;
        const float r2 = (b2 + sqrt_rn(b2 * b2 - 16.f * c2)) * 0.5f;
        const float b3 = cfg.kb3 * hw;
        const float c3 = (cfg.kc3 * w) * h;
        const float r3 = (b3 + sqrt_rn(b3 * b3 - cfg.k4a3 * c3)) * 0.5f;
        float rf = fminf(fminf(r1, r2), r3);
        rf = rf < (float)kMaxRadius ? rf : (float)kMaxRadius;   // (also takes a NaN to the clamp)
        int rad = rf > 0.f ? (int)rf : 0;
        rad = rad > cfg.min_radius ? rad : cfg.min_radius;
        if ((cfg.unk_mask >> (label - 1)) & 1ull) {             // int(radius * UNK_RADIUS_MULT) in f64
            const double m = (double)rad * cfg.unk_mult;
            rad = m < (double)kMaxRadius ? (int)m : kMaxRadius;
        }
        rad = rad < 0 ? 0 : (rad > kMaxRadius ? kMaxRadius : rad);
        float fx = div_rn(div_rn(x - cfg.x0, cfg.vx), cfg.stride);
        float fy = div_rn(div_rn(y - cfg.y0, cfg.vy), cfg.stride);
        fx = fminf(fmaxf(fx, -(float)kMaxCentre), (float)kMaxCentre);
        fy = fminf(fmaxf(fy, -(float)kMaxCentre), (float)kMaxCentre);
        r = make_int4(label - 1, (int)fx, (int)fy, rad);        // (the conversion truncates toward zero)
    }
    out[i] = r;
}

// exclusive position of this thread among the threads of the workgroup with `flag`, and their number; two barriers
__device__ __forceinline__ int block_compact(bool flag, int *wcnt, int &total) {
    const unsigned long long bal = __ballot(flag);
    const int wave = threadIdx.x >> 6;
    if (fnp_lane() == 0) wcnt[wave] = __popcll(bal);
    __syncthreads();
    int pos = __popcll(bal & ((1ull << fnp_lane()) - 1ull));
    total = 0;
    for (int j = 0; j < kWaves; ++j) {
        if (j < wave) pos += wcnt[j];
        total += wcnt[j];
    }
    __syncthreads();
    return pos;
}

__global__ __launch_bounds__(kThreads) void hm_draw_kernel(const int4 *__restrict__ params, int M, int C, int H, int W,
                                                           float *__restrict__ out, int *__restrict__ wg_count) {
    __shared__ int4 sbox[kThreads];
    __shared__ double sden[kThreads];
    __shared__ int wcnt[kWaves];
    const int tiles_x = (W + kTileW - 1) / kTileW;
    const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x, c = blockIdx.y, b = blockIdx.z;
    const int x_lo = tx * kTileW, y_lo = ty * kTileH;
    const int x_hi = min(W, x_lo + kTileW) - 1, y_hi = min(H, y_lo + kTileH) - 1;
    const int px = x_lo + (threadIdx.x & (kTileW - 1)), py = y_lo + threadIdx.x / kTileW;
    const int4 *scene = params + (size_t)b * M;
    double best = 0.0;
    bool covered = false;
    for (int base = 0; base < M; base += kThreads) {
        const int i = base + threadIdx.x;
        int4 p = make_int4(-1, 0, 0, 0);
        if (i < M) p = scene[i];
        const bool take = p.x == c && p.y + p.w >= x_lo && p.y - p.w <= x_hi && p.z + p.w >= y_lo && p.z - p.w <= y_hi;
        int total;
        const int pos = block_compact(take, wcnt, total);
        if (take) {
            const double sigma = (double)(2 * p.w + 1) / 6.0;
            sbox[pos] = p;
            sden[pos] = (2.0 * sigma) * sigma;
        }
        __syncthreads();
        for (int j = 0; j < total; ++j) {
            const int4 q = sbox[j];
            const int dx = px - q.y, dy = py - q.z;
            if (dx >= -q.w && dx <= q.w && dy >= -q.w && dy <= q.w) {
                const double d2 = (double)dx * (double)dx + (double)dy * (double)dy;
                const double arg = -d2 / sden[j];
                best = covered ? fmax(best, arg) : arg;
                covered = true;
            }
        }
        __syncthreads();
    }
    const bool live = px < W && py < H;
    const float v = covered ? (float)exp(best) : 0.f;
    if (live) out[(((size_t)b * C + c) * H + py) * W + px] = v;
    int total;
    block_compact(live && v == 1.0f, wcnt, total);
    if (threadIdx.x == 0) wg_count[((size_t)b * C + c) * gridDim.x + blockIdx.x] = total;
}

// num_pos = sum of the per-workgroup counts (one workgroup; integers: any order gives the same sum)
__global__ __launch_bounds__(kThreads) void hm_count_kernel(const int *__restrict__ wg_count, long long n, int *__restrict__ num_pos) {
    __shared__ int part[kThreads];
    int s = 0;
    for (long long i = threadIdx.x; i < n; i += kThreads) s += wg_count[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int k = kThreads / 2; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) part[threadIdx.x] += part[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) *num_pos = part[0];
}

// ---- loss ----------------------------------------------------------------------------------------------------------

// clip_sigmoid: p = clamp(1 / (1 + exp(-x)), f32(1e-4), f32(1 - 1e-4)); `inside` = the clamp passes the gradient.
// GaussianFocalLoss adds eps = 1e-12 to p and to 1 - p before the logarithm: both are >= 1e-4, whose f32 spacing is 7e-12, so
// the sum rounds back to the operand and is left out.
struct Sig { float p, q; bool inside; };
__device__ __forceinline__ Sig clip_sigmoid(float x) {
    const float lo = 1e-4f, hi = (float)(1.0 - 1e-4);
    const float s = __fdiv_rn(1.f, 1.f + expf(-x));
    Sig r;
    r.inside = s >= lo && s <= hi;
    r.p = s < lo ? lo : (s > hi ? hi : s);       // (keeps a NaN, as torch.clamp does)
    r.q = 1.f - r.p;
    return r;
}

__device__ __forceinline__ float pow4(float w) { const float w2 = w * w; return w2 * w2; }

// wave then workgroup sum in a fixed order; the result is valid in thread 0
__device__ __forceinline__ double block_sum(double v, double *part) {
    for (int k = 32; k > 0; k >>= 1) v += __shfl_down(v, k, 64);
    if (fnp_lane() == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int j = 0; j < kWaves; ++j) s += part[j];
    return s;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void hm_loss_kernel(const T *__restrict__ x, const float *__restrict__ t, long long n,
                                                           double *__restrict__ partial) {
    __shared__ double part[kWaves];
    double acc = 0.0;
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
        const Sig s = clip_sigmoid(load_f32<T>(x, i));
        const float tt = t[i];
        float term;
        if (tt == 1.f) term = (-logf(s.p)) * (s.q * s.q);
        else term = ((-logf(s.q)) * (s.p * s.p)) * pow4(1.f - tt);
        acc += (double)term;
    }
    const double sum = block_sum(acc, part);
    if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}

__global__ __launch_bounds__(kThreads) void hm_loss_finish_kernel(const double *__restrict__ partial, int n_partial,
                                                                  const int *__restrict__ num_pos, float *__restrict__ loss) {
    __shared__ double part[kWaves];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n_partial; i += kThreads) acc += partial[i];
    const double sum = block_sum(acc, part);
    if (threadIdx.x == 0) {
        const int np = *num_pos;
        *loss = (float)(sum / (double)(np > 1 ? np : 1));
    }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void hm_loss_bwd_kernel(const T *__restrict__ x, const float *__restrict__ t, long long n,
                                                               const int *__restrict__ num_pos, const float *__restrict__ grad_out,
                                                               T *__restrict__ grad) {
    const int np = *num_pos;
    const float scale = __fdiv_rn(*grad_out, (float)(np > 1 ? np : 1));
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
        const Sig s = clip_sigmoid(load_f32<T>(x, i));
        const float tt = t[i];
        float g = 0.f;
        if (s.inside) {                                    // dT/dp * p * q
            const float p = s.p, q = s.q;
            if (tt == 1.f) {
                const float q2 = q * q;
                g = 2.f * ((p * q2) * logf(p)) - q2 * q;   // -q^3 + 2 p q^2 log p
            } else {
                const float p2 = p * p;
                g = pow4(1.f - tt) * (p2 * p - 2.f * ((p2 * q) * logf(q)));   // w (p^3 - 2 p^2 q log q)
            }
            g *= scale;
        }
        store_f32<T>(grad, i, g);
    }
}

int loss_grid(long long n) {
    const long long need = (n + kThreads - 1) / kThreads;
    return (int)(need < 1 ? 1 : (need > kLossBlocks ? kLossBlocks : need));
}

}  // namespace

extern "C" int fnp_heatmap_box_params(const float *gt_boxes, int batch_size, int max_boxes, int ncol, int num_classes, float voxel_x,
                                      float voxel_y, int stride, float range_x, float range_y, double overlap, int min_radius,
                                      uint64_t unknown_mask, double unknown_mult, int *out_params, fnp_stream_t stream) {
    if (batch_size < 0 || max_boxes < 0 || ncol < 6 || num_classes < 1 || num_classes > 64 || stride < 1) return FNP_ERR_ARG;
    const long long n = (long long)batch_size * max_boxes;
    if (n == 0) return FNP_OK;
    if (!gt_boxes || !out_params || ((uintptr_t)out_params & 15) || n > 0x7fffffffll) return FNP_ERR_ARG;
    HmCfg cfg;
    cfg.vx = voxel_x, cfg.vy = voxel_y, cfg.stride = (float)stride, cfg.x0 = range_x, cfg.y0 = range_y;
    const double a3 = 4 * overlap;   // Python's scalars: formed in f64, rounded to f32 where they meet the tensor
    cfg.k1n = (float)(1 - overlap), cfg.k1d = (float)(1 + overlap), cfg.k2 = (float)(1 - overlap);
    cfg.kb3 = (float)(-2 * overlap), cfg.kc3 = (float)(overlap - 1), cfg.k4a3 = (float)(4 * a3);
    cfg.min_radius = min_radius, cfg.num_classes = num_classes, cfg.unk_mask = unknown_mask, cfg.unk_mult = unknown_mult;
    hipLaunchKernelGGL(hm_params_kernel, dim3(fnp_divup(n, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, gt_boxes, n, ncol, cfg,
                       (int4 *)out_params);
    FNP_LAUNCH_CHECK();
    return FNP_OK;
}

static long long hm_tiles(int H, int W) { return (long long)((W + kTileW - 1) / kTileW) * ((H + kTileH - 1) / kTileH); }

extern "C" int64_t fnp_heatmap_draw_workspace_bytes(int batch_size, int num_classes, int height, int width) {
    if (batch_size < 0 || num_classes < 1 || height < 1 || width < 1) return FNP_ERR_ARG;
    const long long g = hm_tiles(height, width) * num_classes * batch_size;
    return 4 * (g > 0 ? g : 1);
}

extern "C" int fnp_heatmap_draw(const int *params, int batch_size, int max_boxes, int num_classes, int height, int width,
                                void *workspace, int64_t workspace_bytes, float *heatmap, int *num_pos, fnp_stream_t stream) {
    if (batch_size < 0 || max_boxes < 0 || num_classes < 1 || num_classes > 65535 || batch_size > 65535 || height < 1 || width < 1 ||
        !num_pos)
        return FNP_ERR_ARG;
    const long long tiles = hm_tiles(height, width), g = tiles * num_classes * batch_size;
    if (tiles > 0x7fffffffll || g > 0x7fffffffll) return FNP_ERR_ARG;
    if (batch_size > 0) {
        if (!heatmap || !workspace || ((uintptr_t)workspace & 3) || (max_boxes > 0 && (!params || ((uintptr_t)params & 15))))
            return FNP_ERR_ARG;
        if (4 * g > workspace_bytes) return FNP_ERR_WORKSPACE;
        hipLaunchKernelGGL(hm_draw_kernel, dim3((unsigned)tiles, num_classes, batch_size), dim3(kThreads), 0, (hipStream_t)stream,
                           (const int4 *)params, max_boxes, num_classes, height, width, heatmap, (int *)workspace);
        FNP_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(hm_count_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, (const int *)workspace, g, num_pos);
    FNP_LAUNCH_CHECK();
    return FNP_OK;
}

extern "C" int64_t fnp_heatmap_loss_workspace_bytes(int64_t n) {
    if (n < 0) return FNP_ERR_ARG;
    return 8ll * kLossBlocks;
}

extern "C" int fnp_heatmap_loss_forward(const void *logits, int dtype, const float *target, int64_t n, const int *num_pos,
                                        void *workspace, int64_t workspace_bytes, float *loss, fnp_stream_t stream) {
    if (n < 0 || !num_pos || !loss || !workspace || ((uintptr_t)workspace & 7) || (n > 0 && (!logits || !target))) return FNP_ERR_ARG;
    if (workspace_bytes < 8ll * kLossBlocks) return FNP_ERR_WORKSPACE;
    const int G = loss_grid(n);
    double *partial = (double *)workspace;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == FNP_F32)
        hipLaunchKernelGGL(hm_loss_kernel<float>, dim3(G), dim3(kThreads), 0, s, (const float *)logits, target, (long long)n, partial);
    else if (dtype == FNP_F16)
        hipLaunchKernelGGL(hm_loss_kernel<__half>, dim3(G), dim3(kThreads), 0, s, (const __half *)logits, target, (long long)n, partial);
    else if (dtype == FNP_BF16)
        hipLaunchKernelGGL(hm_loss_kernel<unsigned short>, dim3(G), dim3(kThreads), 0, s, (const unsigned short *)logits, target,
                           (long long)n, partial);
    else
        return FNP_ERR_ARG;
    FNP_LAUNCH_CHECK();
    hipLaunchKernelGGL(hm_loss_finish_kernel, dim3(1), dim3(kThreads), 0, s, (const double *)partial, G, num_pos, loss);
    FNP_LAUNCH_CHECK();
    return FNP_OK;
}

extern "C" int fnp_heatmap_loss_backward(const void *logits, int dtype, const float *target, int64_t n, const int *num_pos,
                                         const float *grad_out, void *grad_logits, fnp_stream_t stream) {
    if (n < 0 || !num_pos || !grad_out) return FNP_ERR_ARG;
    if (n == 0) return FNP_OK;
    if (!logits || !target || !grad_logits) return FNP_ERR_ARG;
    const int G = fnp_grid_for(n, kThreads, 4096);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == FNP_F32)
        hipLaunchKernelGGL(hm_loss_bwd_kernel<float>, dim3(G), dim3(kThreads), 0, s, (const float *)logits, target, (long long)n, num_pos,
                           grad_out, (float *)grad_logits);
    else if (dtype == FNP_F16)
        hipLaunchKernelGGL(hm_loss_bwd_kernel<__half>, dim3(G), dim3(kThreads), 0, s, (const __half *)logits, target, (long long)n,
                           num_pos, grad_out, (__half *)grad_logits);
    else if (dtype == FNP_BF16)
        hipLaunchKernelGGL(hm_loss_bwd_kernel<unsigned short>, dim3(G), dim3(kThreads), 0, s, (const unsigned short *)logits, target,
                           (long long)n, num_pos, grad_out, (unsigned short *)grad_logits);
    else
        return FNP_ERR_ARG;
    FNP_LAUNCH_CHECK();
    return FNP_OK;
}
