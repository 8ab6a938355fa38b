// Row-vector helpers of the BatchNorm kernels (csrc/bnorm.hip on (cap, C) rows, csrc/bev_bn.hip on rows that stand for a dense
// map): one element or 8 consecutive channels of a row of f32 / bf16 / fp16 as floats, and an f64 lane exchange.
#pragma once
#include "common.h"

__device__ __forceinline__ float ldf(const float *p, size_t i) { return p[i]; }
__device__ __forceinline__ float ldf(const __bf16 *p, size_t i) { return (float)p[i]; }
__device__ __forceinline__ float ldf(const _Float16 *p, size_t i) { return (float)p[i]; }
__device__ __forceinline__ void stf(float *p, size_t i, float v) { p[i] = v; }
__device__ __forceinline__ void stf(__bf16 *p, size_t i, float v) { p[i] = (__bf16)v; }
__device__ __forceinline__ void stf(_Float16 *p, size_t i, float v) { p[i] = (_Float16)v; }

// 8 consecutive channels of one row as floats
template <typename T> __device__ __forceinline__ void load8(const T *p, float (&v)[8]) {
    if constexpr (sizeof(T) == 2) {
        const uint4 raw = *reinterpret_cast<const uint4 *>(p);
        const T *e = reinterpret_cast<const T *>(&raw);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (float)e[j];
    } else {
        const float4 a = reinterpret_cast<const float4 *>(p)[0], b = reinterpret_cast<const float4 *>(p)[1];
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    }
}
template <typename T> __device__ __forceinline__ void store8(T *p, const float (&v)[8]) {
    if constexpr (sizeof(T) == 2) {
        uint4 raw;
        T *e = reinterpret_cast<T *>(&raw);
#pragma unroll
        for (int j = 0; j < 8; ++j) e[j] = (T)v[j];
        *reinterpret_cast<uint4 *>(p) = raw;
    } else {
        reinterpret_cast<float4 *>(p)[0] = make_float4(v[0], v[1], v[2], v[3]);
        reinterpret_cast<float4 *>(p)[1] = make_float4(v[4], v[5], v[6], v[7]);
    }
}

__device__ __forceinline__ double shfl_xor_f64(double v, int m) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __shfl_xor(lo, m);
    hi = __shfl_xor(hi, m);
    return __hiloint2double(hi, lo);
}
