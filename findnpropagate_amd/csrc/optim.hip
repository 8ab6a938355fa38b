// The adam_onecycle optimizer step (include/fnp.h: fnp_adam_onecycle_step): three launches over a chunk table.
//   (a) optim_norm_kernel:   per chunk, the f64 sum of squares of the unscaled gradient and a non-finite flag
//   (b) optim_update_kernel: per chunk, decay + Adam; every workgroup reduces (a)'s partials in the same fixed order
//   (c) optim_finish_kernel: one workgroup: the per-tensor step counts, the loss scale, grad_norm and found_inf
// (b) reads steps[], (c) writes it: the two cannot be one launch.  No atomics anywhere; a streaming kernel: 16-byte accesses
// wherever an array is 16-byte aligned at the chunk's body, dword accesses for the head, the tail and a misaligned array.
#include <math.h>

#include "common.h"

namespace {

constexpr int kThreads = 256;

// fixed tree over the workgroup: lanes by shuffles, the four waves through LDS; every thread gets the sum
__device__ __forceinline__ double block_sum(double x, int &flag, double *lds_sum, int *lds_flag) {
    for (int d = 32; d > 0; d >>= 1) {
        x += __shfl_down(x, d, 64);
        flag |= __shfl_down(flag, d, 64);
    }
    const int wave = threadIdx.x >> 6;
    if (fnp_lane() == 0) {
        lds_sum[wave] = x;
        lds_flag[wave] = flag;
    }
    __syncthreads();
    double s = lds_sum[0];
    int f = lds_flag[0];
    for (int w = 1; w < kThreads / 64; ++w) {
        s += lds_sum[w];
        f |= lds_flag[w];
    }
    __syncthreads();
    flag = f;
    return s;
}

// the chunks' partials in a fixed order: thread i takes i, i + 256, ... in turn, then the tree.  Every workgroup that calls
// this gets the same bits.
__device__ __forceinline__ double reduce_partials(const double *partial, const int *flags, long long num_chunks, int &found,
                                                  double *lds_sum, int *lds_flag) {
    double s = 0.0;
    int f = 0;
    for (long long i = threadIdx.x; i < num_chunks; i += kThreads) {
        s += partial[i];
        f |= flags[i];
    }
    s = block_sum(s, f, lds_sum, lds_flag);
    found = f;
    return s;
}

__device__ __forceinline__ float inv_scale(const float *scale) {
    return scale ? (float)(1.0 / (double)*scale) : 1.0f;
}

__device__ __forceinline__ int head_of(const void *p, int length) {   // elements in front of the first 16-byte boundary
    const int h = (int)(((16 - ((uintptr_t)p & 15)) & 15) >> 2);
    return h < length ? h : length;
}

__device__ __forceinline__ float4 load4(const float *p, bool aligned) {
    if (aligned) return *reinterpret_cast<const float4 *>(p);
    return make_float4(p[0], p[1], p[2], p[3]);
}

__device__ __forceinline__ void store4(float *p, bool aligned, float4 x) {
    if (aligned) {
        *reinterpret_cast<float4 *>(p) = x;
    } else {
        p[0] = x.x; p[1] = x.y; p[2] = x.z; p[3] = x.w;
    }
}

__device__ __forceinline__ void square_in(float g, float inv, double &sum, int &bad) {
    const float u = g * inv;
    bad |= !isfinite(u);
    sum += (double)u * (double)u;
}

__global__ __launch_bounds__(kThreads) void optim_norm_kernel(const fnp_optim_chunk *__restrict__ chunks,
                                                               const float *const *__restrict__ grads,
                                                               const float *__restrict__ scale, double *__restrict__ partial,
                                                               int *__restrict__ flags) {
    __shared__ double lds_sum[kThreads / 64];
    __shared__ int lds_flag[kThreads / 64];
    const fnp_optim_chunk ch = chunks[blockIdx.x];
    const float *gbase = grads[ch.tensor];
    double sum = 0.0;
    int bad = 0;
    if (gbase) {      // (uniform over the workgroup)
        const float *g = gbase + ch.offset;
        const float inv = inv_scale(scale);
        const int head = head_of(g, ch.length);
        const int n4 = (ch.length - head) >> 2, tail0 = head + (n4 << 2);
        for (int i = threadIdx.x; i < n4; i += kThreads) {
            const float4 x = *reinterpret_cast<const float4 *>(g + head + 4 * i);
            square_in(x.x, inv, sum, bad);
            square_in(x.y, inv, sum, bad);
            square_in(x.z, inv, sum, bad);
            square_in(x.w, inv, sum, bad);
        }
        if ((int)threadIdx.x < head) square_in(g[threadIdx.x], inv, sum, bad);
        if ((int)threadIdx.x < ch.length - tail0) square_in(g[tail0 + threadIdx.x], inv, sum, bad);
    }
    sum = block_sum(sum, bad, lds_sum, lds_flag);
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = sum;
        flags[blockIdx.x] = bad;
    }
}

struct StepScalars {      // one tensor's f32 constants of the step
    float decay, inv, clip, omb1, b2, omb2, step_size, bc2_sqrt, eps;
};

__device__ __forceinline__ void adam_one(float &p, float g, float &m, float &v, const StepScalars &k) {
    const float gp = (g * k.inv) * k.clip;
    m = m + (gp - m) * k.omb1;
    v = k.b2 * v + (k.omb2 * gp) * gp;
    const float den = sqrtf(v) / k.bc2_sqrt + k.eps;
    p = p * k.decay - k.step_size * (m / den);
}

__global__ __launch_bounds__(kThreads) void optim_update_kernel(const fnp_optim_chunk *__restrict__ chunks, long long num_chunks,
                                                                 float *const *__restrict__ params,
                                                                 const float *const *__restrict__ grads,
                                                                 float *const *__restrict__ exp_avg,
                                                                 float *const *__restrict__ exp_avg_sq,
                                                                 const int *__restrict__ steps, const float *__restrict__ scale,
                                                                 const double *__restrict__ partial, const int *__restrict__ flags,
                                                                 double lr, double beta1, double beta2, double eps, double wd,
                                                                 double max_norm) {
    __shared__ double lds_sum[kThreads / 64];
    __shared__ int lds_flag[kThreads / 64];
    __shared__ StepScalars lds_k;
    int found;
    const double total = reduce_partials(partial, flags, num_chunks, found, lds_sum, lds_flag);
    if (found) return;      // (uniform over the whole launch: nothing is written)
    const fnp_optim_chunk ch = chunks[blockIdx.x];
    const float *gbase = grads[ch.tensor];
    if (threadIdx.x == 0) {
        StepScalars k;
        k.decay = (float)(1.0 - wd * lr);
        k.inv = inv_scale(scale);
        const double clip = max_norm / (sqrt(total) + 1e-6);
        k.clip = (float)(clip < 1.0 ? clip : 1.0);
        k.omb1 = (float)(1.0 - beta1);
        k.b2 = (float)beta2;
        k.omb2 = (float)(1.0 - beta2);
        k.eps = (float)eps;
        const double t = (double)(steps[ch.tensor] + 1);
        k.step_size = (float)(lr / (1.0 - pow(beta1, t)));
        k.bc2_sqrt = (float)sqrt(1.0 - pow(beta2, t));
        lds_k = k;
    }
    __syncthreads();
    const StepScalars k = lds_k;
    float *p = params[ch.tensor] + ch.offset;
    const int head = head_of(p, ch.length);
    const int n4 = (ch.length - head) >> 2, tail0 = head + (n4 << 2);
    if (!gbase) {           // no gradient this step: the decay alone
        for (int i = threadIdx.x; i < n4; i += kThreads) {
            float4 x = *reinterpret_cast<float4 *>(p + head + 4 * i);
            x.x *= k.decay; x.y *= k.decay; x.z *= k.decay; x.w *= k.decay;
            *reinterpret_cast<float4 *>(p + head + 4 * i) = x;
        }
        if ((int)threadIdx.x < head) p[threadIdx.x] *= k.decay;
        if ((int)threadIdx.x < ch.length - tail0) p[tail0 + threadIdx.x] *= k.decay;
        return;
    }
    const float *g = gbase + ch.offset;
    float *m = exp_avg[ch.tensor] + ch.offset, *v = exp_avg_sq[ch.tensor] + ch.offset;
    // p is 16-byte aligned behind the head by construction; g, m, v each may or may not be (a parameter that is a view)
    const bool ga = (((uintptr_t)(g + head)) & 15) == 0, ma = (((uintptr_t)(m + head)) & 15) == 0, va = (((uintptr_t)(v + head)) & 15) == 0;
    for (int i = threadIdx.x; i < n4; i += kThreads) {
        const int e = head + 4 * i;
        float4 pp = *reinterpret_cast<float4 *>(p + e);
        const float4 gg = load4(g + e, ga);
        float4 mm = load4(m + e, ma), vv = load4(v + e, va);
        adam_one(pp.x, gg.x, mm.x, vv.x, k);
        adam_one(pp.y, gg.y, mm.y, vv.y, k);
        adam_one(pp.z, gg.z, mm.z, vv.z, k);
        adam_one(pp.w, gg.w, mm.w, vv.w, k);
        *reinterpret_cast<float4 *>(p + e) = pp;
        store4(m + e, ma, mm);
        store4(v + e, va, vv);
    }
    int e = -1;
    if ((int)threadIdx.x < head) e = threadIdx.x;
    else if ((int)threadIdx.x - head < ch.length - tail0) e = tail0 + (int)threadIdx.x - head;      // (head + tail <= 6 < 256)
    if (e >= 0) {
        float pp = p[e], mm = m[e], vv = v[e];
        adam_one(pp, g[e], mm, vv, k);
        p[e] = pp; m[e] = mm; v[e] = vv;
    }
}

__global__ __launch_bounds__(kThreads) void optim_finish_kernel(int num_tensors, long long num_chunks,
                                                                 const float *const *__restrict__ grads, int *__restrict__ steps,
                                                                 float *__restrict__ scale, int *__restrict__ growth_tracker,
                                                                 const double *__restrict__ partial, const int *__restrict__ flags,
                                                                 double growth_factor, double backoff_factor, int growth_interval,
                                                                 float *__restrict__ grad_norm, int *__restrict__ found_inf) {
    __shared__ double lds_sum[kThreads / 64];
    __shared__ int lds_flag[kThreads / 64];
    int found;
    const double total = reduce_partials(partial, flags, num_chunks, found, lds_sum, lds_flag);
    if (!found)
        for (int i = threadIdx.x; i < num_tensors; i += kThreads)
            if (grads[i]) steps[i] += 1;
    if (threadIdx.x == 0) {
        *grad_norm = (float)sqrt(total);
        *found_inf = found ? 1 : 0;
        if (scale) {
            if (found) {
                *scale = *scale * (float)backoff_factor;
                *growth_tracker = 0;
            } else {
                const int ok = *growth_tracker + 1;
                if (ok == growth_interval) {
                    const float grown = *scale * (float)growth_factor;
                    if (isfinite(grown)) *scale = grown;
                    *growth_tracker = 0;
                } else {
                    *growth_tracker = ok;
                }
            }
        }
    }
}

inline int64_t flags_offset(int64_t num_chunks) { return ((num_chunks > 0 ? num_chunks : 1) * 8 + 15) & ~(int64_t)15; }

}  // namespace

extern "C" int64_t fnp_adam_onecycle_workspace_bytes(int64_t num_chunks) {
    if (num_chunks < 0) return FNP_ERR_ARG;
    return flags_offset(num_chunks) + (num_chunks > 0 ? num_chunks : 1) * 4;
}

extern "C" int fnp_adam_onecycle_step(int num_tensors, int64_t num_chunks, const struct fnp_optim_chunk *chunks, float *const *params,
                                      const float *const *grads, float *const *exp_avg, float *const *exp_avg_sq, int32_t *steps,
                                      float *scale, int32_t *growth_tracker, double lr, double beta1, double beta2, double eps,
                                      double wd, double max_norm, double growth_factor, double backoff_factor, int growth_interval,
                                      void *workspace, int64_t workspace_bytes, float *grad_norm, int32_t *found_inf,
                                      fnp_stream_t stream) {
    if (num_tensors < 0 || num_chunks < 0 || num_chunks > 0x7fffffffLL || !grad_norm || !found_inf) return FNP_ERR_ARG;
    if (num_tensors > 0 && (!params || !grads || !exp_avg || !exp_avg_sq || !steps)) return FNP_ERR_ARG;
    if (num_chunks > 0 && (!chunks || num_tensors == 0)) return FNP_ERR_ARG;
    if ((scale == nullptr) != (growth_tracker == nullptr)) return FNP_ERR_ARG;
    // lr, eps, wd finite; the betas in [0, 1); max_norm >= 0, +infinity allowed (no clipping); NaN fails every comparison
    if (!isfinite(lr) || !isfinite(wd) || !(eps >= 0.0) || !isfinite(eps) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) ||
        !(max_norm >= 0.0))
        return FNP_ERR_ARG;
    if (scale && (!(growth_factor > 0.0) || !isfinite(growth_factor) || !(backoff_factor > 0.0) || !isfinite(backoff_factor) || growth_interval < 1))
        return FNP_ERR_ARG;
    if (!workspace || ((uintptr_t)workspace & 7)) return FNP_ERR_ARG;
    if (workspace_bytes < fnp_adam_onecycle_workspace_bytes(num_chunks)) return FNP_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    double *partial = (double *)workspace;
    int *flags = (int *)((char *)workspace + flags_offset(num_chunks));
    if (num_chunks > 0) {
        hipLaunchKernelGGL(optim_norm_kernel, dim3((unsigned)num_chunks), dim3(kThreads), 0, s, chunks, grads, (const float *)scale,
                           partial, flags);
        FNP_LAUNCH_CHECK();
        hipLaunchKernelGGL(optim_update_kernel, dim3((unsigned)num_chunks), dim3(kThreads), 0, s, chunks, (long long)num_chunks, params,
                           grads, exp_avg, exp_avg_sq, (const int *)steps, (const float *)scale, (const double *)partial,
                           (const int *)flags, lr, beta1, beta2, eps, wd, max_norm);
        FNP_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(optim_finish_kernel, dim3(1), dim3(kThreads), 0, s, num_tensors, (long long)num_chunks, grads, steps, scale,
                       growth_tracker, (const double *)partial, (const int *)flags, growth_factor, backoff_factor, growth_interval,
                       grad_norm, found_inf);
    FNP_LAUNCH_CHECK();
    return FNP_OK;
}
