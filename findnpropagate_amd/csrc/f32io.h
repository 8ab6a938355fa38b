// Element access for the kernels that take f32, f16 or bf16 arrays (FNP_F32 / FNP_F16 / FNP_BF16): an exact upcast on load, round to
// nearest even on store.  bf16 crosses as its 16 bits (unsigned short); a NaN stays a NaN.  Shared by heatmap.hip and tfassign.hip.
#pragma once
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

template <typename T> __device__ __forceinline__ float load_f32(const T *p, long long i);
template <> __device__ __forceinline__ float load_f32<float>(const float *p, long long i) { return p[i]; }
template <> __device__ __forceinline__ float load_f32<__half>(const __half *p, long long i) { return __half2float(p[i]); }
template <> __device__ __forceinline__ float load_f32<unsigned short>(const unsigned short *p, long long i) {   // bf16 bits
    return __uint_as_float((unsigned)p[i] << 16);
}
template <typename T> __device__ __forceinline__ void store_f32(T *p, long long i, float v);
template <> __device__ __forceinline__ void store_f32<float>(float *p, long long i, float v) { p[i] = v; }
template <> __device__ __forceinline__ void store_f32<__half>(__half *p, long long i, float v) { p[i] = __float2half_rn(v); }
template <> __device__ __forceinline__ void store_f32<unsigned short>(unsigned short *p, long long i, float v) {
    const unsigned u = __float_as_uint(v);
    unsigned short r;
    if ((u & 0x7fffffffu) > 0x7f800000u) r = (unsigned short)((u >> 16) | 0x40u);          // NaN stays a NaN
    else r = (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);                     // round to nearest even
    p[i] = r;
}
