// The attention dropout mask keep(seed, scene, head, query, key) of the fnp_tf_attention_dropout_* block of include/fnp.h: a pure
// function of its five values in integer arithmetic, the one statement of it that the forward (csrc/tfdecoder.hip), both
// backward kernels and the mask writer (csrc/tfattn_grad.hip) call.  Plain C++: a host program compiles it as it stands.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FNP_DROPOUT_FN __host__ __device__ __forceinline__
#else
#define FNP_DROPOUT_FN static inline
#endif

// what a dropout launch gets on top of the plain one's arguments
struct fnp_dropout_args {
    const unsigned long long *seed;    // device pointer: the kernels read it, the host never does
    uint32_t threshold;                // T = (uint32)((double)p * 2^32): keep iff word >= T
    float scale;                       // 1 / (1 - T / 2^32)
};

#if defined(__HIPCC__)
// a kernel template takes `DROP... drop`: empty (the plain instantiation, no argument added) or one fnp_dropout_args
__device__ __forceinline__ fnp_dropout_args fnp_dropout_of() { return fnp_dropout_args{nullptr, 0u, 1.f}; }
__device__ __forceinline__ fnp_dropout_args fnp_dropout_of(fnp_dropout_args d) { return d; }
#endif

static inline uint32_t fnp_dropout_threshold(float p) { return (uint32_t)((double)p * 4294967296.0); }
static inline float fnp_dropout_scale(uint32_t threshold) { return (float)(1.0 / (1.0 - (double)threshold / 4294967296.0)); }

// Philox4x32-10 (Salmon et al., SC'11): counter c[4], key (k0, k1) -> c[4]
FNP_DROPOUT_FN void fnp_philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint64_t a = (uint64_t)0xD2511F53u * c[0], b = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(b >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(a >> 32) ^ c[3] ^ k1;
        c[0] = n0, c[1] = (uint32_t)b, c[2] = n2, c[3] = (uint32_t)a;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
}

// the four words of keys 4 * key_group .. 4 * key_group + 3 against one query: word r belongs to key 4 * key_group + r
FNP_DROPOUT_FN void fnp_dropout_words(unsigned long long seed, int scene, int head, int query, int key_group, uint32_t w[4]) {
    w[0] = (uint32_t)key_group, w[1] = (uint32_t)query, w[2] = (uint32_t)(scene * 8 + head), w[3] = 0u;
    fnp_philox4x32_10(w, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// bit r: key 4 * key_group + r is kept
FNP_DROPOUT_FN uint32_t fnp_dropout_keep4(unsigned long long seed, uint32_t threshold, int scene, int head, int query, int key_group) {
    uint32_t w[4];
    fnp_dropout_words(seed, scene, head, query, key_group, w);
    return (uint32_t)(w[0] >= threshold) | (uint32_t)(w[1] >= threshold) << 1 | (uint32_t)(w[2] >= threshold) << 2 |
           (uint32_t)(w[3] >= threshold) << 3;
}
