// The backward of the attention core softmax(0.25 q k^T) v (fnp_tf_attention_stats is its forward, csrc/tfdecoder.hip); the
// contract is the fnp_tf_attention_backward block of include/fnp.h.
//
// All arithmetic is f32 on v_mfma_f32_16x16x4_f32, no atomics, no LDS, no barrier: every result is bit-identical from run to
// run and a scene's result does not depend on the batch it runs in.  The scores are never stored: both kernels recompute them
// from q and k with the forward's arithmetic (q scaled by 0.25 first, the same four-step chain per score), so s - M <= 0 holds
// exactly as it did in the forward, and P = exp(s - M) * (1 / L) with the forward's (M, L).
//
// The operand trick of tfdecoder.hip carries both kernels: a lane (i = lane & 15, g = lane >> 4) holds C[row 4g + r][col i] of
// a product, which is the B operand (k = g) of a next product whose step r contracts rows {4g + r}.
//
//   key-stationary    S = Q K^T and dP = dO V^T (A = 16 queries, B = 16 keys): a lane holds query 4g + r against key i.  That
//   (dK, dV)          is the B operand of dV^T += dO^T P and dK^T += Q^T dS contracted over the queries, with A = one scalar of
//                     dO or q per step: (query 4g + r, dim i).  A wave owns 64 keys (four column blocks: their k and v rows and
//                     eight accumulators stay in registers) and walks all queries; a dK or dV row has one owner.
//   query-stationary  S^T = K Q^T and dP^T = V dO^T (A = 16 keys, B = 16 queries) in the forward's orientation and on the
//   (dQ)              forward's splits; dS^T is the B operand of dQ^T += K^T dS^T contracted over the keys.  Per split, then the
//                     splits in split order.
#include <math.h>

#include "common.h"
#include "tfattn_dropout.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kD = 128;            // d_model
constexpr int kHeads = 8;          // heads of 16
constexpr int kTile = 64;          // keys per tile of the query-stationary kernel (the forward's tile_len)
constexpr int kThreads = 256;
constexpr int kWaveKeys = 64;      // keys a wave of the key-stationary kernel owns
constexpr int kKeyBlock = 256;     // keys per workgroup of the key-stationary kernel: four waves

#define MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

// x of lane `from` (0..3) of this lane's quad: a DPP quad permute, every lane of the wave active
__device__ __forceinline__ uint32_t quad_lane(uint32_t x, int from) {
    switch (from) {
        case 0: return (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0x00, 0xf, 0xf, false);
        case 1: return (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0x55, 0xf, 0xf, false);
        case 2: return (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0xaa, 0xf, 0xf, false);
        default: return (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0xff, 0xf, 0xf, false);
    }
}

// ---- D_i = dO_i . O_i per head: the diagonal of dO O^T, one wave per (16 queries, head, scene) -------------------------------

__global__ __launch_bounds__(64) void tf_attn_bwd_d_kernel(const float *__restrict__ out, const float *__restrict__ d_out, int Kq,
                                                           float *__restrict__ dsum) {
    const int blk = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int lane = threadIdx.x, i = lane & 15, g = lane >> 4;
    const int row = min(blk * 16 + i, Kq - 1);
    const size_t at = ((size_t)b * Kq + row) * kD + 16 * h + 4 * g;
    const float4 a = *reinterpret_cast<const float4 *>(d_out + at);
    const float4 o = *reinterpret_cast<const float4 *>(out + at);
    f32x4 c = {0.f, 0.f, 0.f, 0.f};
    c = MFMA(a.x, o.x, c);
    c = MFMA(a.y, o.y, c);
    c = MFMA(a.z, o.z, c);
    c = MFMA(a.w, o.w, c);                                 // c[r] = dO (query 4g + r) . O (query i)
    const int r = i & 3;
    const float d = r == 0 ? c[0] : (r == 1 ? c[1] : (r == 2 ? c[2] : c[3]));
    if ((i >> 2) == g && blk * 16 + i < Kq) dsum[((size_t)b * kHeads + h) * Kq + blk * 16 + i] = d;
}

// ---- dK and dV, key-stationary ------------------------------------------------------------------------------------------------

// DROP is empty (fnp_tf_attention_backward: the kernel and its arguments as they always were) or one fnp_dropout_args: then
// dV sums dO (P Z) and dS = P (Z dP - D), Z = keep / (1 - p_eff) (tfattn_dropout.h).  A lane holds four QUERIES 4g + r against one
// key, but a generator call serves four KEYS of one query: lane i calls for (query 4g + (i & 3), the aligned key group of key i)
// and keeps the four bits; the lanes of a quad share that key group, so the bit of (query 4g + r, key i) is bit i & 3 of quad
// lane r's word, fetched by a quad broadcast.  (Four calls per lane instead: 184 us against 130 us for dK and dV at one scene)
template <bool WANT_DK, bool WANT_DV, typename... DROP>
__global__ __launch_bounds__(kThreads) void tf_attn_bwd_kv_kernel(const float *__restrict__ q, const float *__restrict__ k,
                                                                  const float *__restrict__ v, const float *__restrict__ d_out,
                                                                  const float *__restrict__ stats, const float *__restrict__ dsum,
                                                                  int Kq, int N, float *__restrict__ dk, float *__restrict__ dv,
                                                                  DROP... drop) {
    const int h = blockIdx.y, b = blockIdx.z;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, g = lane >> 4;
    const int key0 = blockIdx.x * kKeyBlock + wave * kWaveKeys;
    if (key0 >= N) return;                                 // wave-uniform; the kernel has no barrier
    constexpr bool kDrop = sizeof...(DROP) != 0;
    const fnp_dropout_args da = fnp_dropout_of(drop...);
    const unsigned long long seed = kDrop ? *da.seed : 0ull;
    const float *qs = q + (size_t)b * Kq * kD + 16 * h;
    const float *dos = d_out + (size_t)b * Kq * kD + 16 * h;
    const float *st = stats + ((size_t)b * kHeads + h) * Kq * 2;
    const float *ds_ = dsum + ((size_t)b * kHeads + h) * Kq;
    float4 kf[4], vf[4];
    f32x4 acck[4], accv[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const size_t at = ((size_t)b * N + min(key0 + 16 * c + i, N - 1)) * kD + 16 * h + 4 * g;
        kf[c] = *reinterpret_cast<const float4 *>(k + at);
        vf[c] = *reinterpret_cast<const float4 *>(v + at);
        acck[c] = f32x4{0.f, 0.f, 0.f, 0.f};
        accv[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const int nblk = (Kq + 15) >> 4;
    for (int blk = 0; blk < nblk; ++blk) {
        const int rowa = min(blk * 16 + i, Kq - 1);
        const float4 x = *reinterpret_cast<const float4 *>(qs + (size_t)rowa * kD + 4 * g);
        const float4 qf = make_float4(0.25f * x.x, 0.25f * x.y, 0.25f * x.z, 0.25f * x.w);   // as the forward scales it: exact
        const float4 dof = *reinterpret_cast<const float4 *>(dos + (size_t)rowa * kD + 4 * g);
        float qcol[4], docol[4], m[4], inv_l[4], dd[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = blk * 16 + 4 * g + r, rc = min(row, Kq - 1);
            qcol[r] = qs[(size_t)rc * kD + i];
            docol[r] = dos[(size_t)rc * kD + i];
            const float2 ml = *reinterpret_cast<const float2 *>(st + (size_t)rc * 2);
            m[r] = ml.x;
            inv_l[r] = row < Kq ? 1.0f / ml.y : 0.f;       // a row past Kq enters with P = 0
            dd[r] = ds_[rc];
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
            s = MFMA(qf.x, kf[c].x, s);
            s = MFMA(qf.y, kf[c].y, s);
            s = MFMA(qf.z, kf[c].z, s);
            s = MFMA(qf.w, kf[c].w, s);                    // s[r]: query 4g + r against key i
            dp = MFMA(dof.x, vf[c].x, dp);
            dp = MFMA(dof.y, vf[c].y, dp);
            dp = MFMA(dof.z, vf[c].z, dp);
            dp = MFMA(dof.w, vf[c].w, dp);
            uint32_t mine = 0;                             // the mask indexes nothing: a row past Kq or a key past N is a value like any
            if (kDrop) mine = fnp_dropout_keep4(seed, da.threshold, b, h, blk * 16 + 4 * g + (i & 3), (key0 + 16 * c + i) >> 2);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = expf(s[r] - m[r]) * inv_l[r];
                if (kDrop) {
                    const float z = (quad_lane(mine, r) >> (i & 3)) & 1 ? da.scale : 0.f;
                    if (WANT_DV) accv[c] = MFMA(docol[r], p * z, accv[c]);
                    if (WANT_DK) acck[c] = MFMA(qcol[r], p * (z * dp[r] - dd[r]), acck[c]);
                } else {
                    if (WANT_DV) accv[c] = MFMA(docol[r], p, accv[c]);
                    if (WANT_DK) acck[c] = MFMA(qcol[r], p * (dp[r] - dd[r]), acck[c]);
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {                          // acc[r]: dim 4g + r of key i
        const int key = key0 + 16 * c + i;
        if (key >= N) continue;
        const size_t at = ((size_t)b * N + key) * kD + 16 * h + 4 * g;
        if (WANT_DK) *reinterpret_cast<float4 *>(dk + at) = make_float4(0.25f * acck[c][0], 0.25f * acck[c][1], 0.25f * acck[c][2], 0.25f * acck[c][3]);
        if (WANT_DV) *reinterpret_cast<float4 *>(dv + at) = make_float4(accv[c][0], accv[c][1], accv[c][2], accv[c][3]);
    }
}

// ---- dQ, query-stationary on the forward's splits ------------------------------------------------------------------------------

// DROP as in the key-stationary kernel: dS = P (Z dP - D).  In the forward's orientation a lane's four keys of a query are one
// aligned group of four, one generator call, as in tf_attn_kernel.
template <int QB, typename... DROP>
__global__ __launch_bounds__(kThreads) void tf_attn_bwd_q_kernel(const float *__restrict__ q, const float *__restrict__ k,
                                                                 const float *__restrict__ v, const float *__restrict__ d_out,
                                                                 const float *__restrict__ stats, const float *__restrict__ dsum,
                                                                 int Kq, int N, int split_len, int nsplit, int nchunk,
                                                                 float *__restrict__ part, float *__restrict__ dq, DROP... drop) {
    const int split = blockIdx.x, h = blockIdx.y, b = blockIdx.z / nchunk, chunk = blockIdx.z % nchunk;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, g = lane >> 4;
    const int nblk = (Kq + 15) >> 4;
    constexpr bool kDrop = sizeof...(DROP) != 0;
    const fnp_dropout_args da = fnp_dropout_of(drop...);
    const unsigned long long seed = kDrop ? *da.seed : 0ull;
    const float *qs = q + (size_t)b * Kq * kD + 16 * h;
    const float *dos = d_out + (size_t)b * Kq * kD + 16 * h;
    const float *ks = k + (size_t)b * N * kD + 16 * h;
    const float *vs = v + (size_t)b * N * kD + 16 * h;

    float4 qf[QB], dof[QB];
    f32x4 acc[QB];
    float m[QB], inv_l[QB], dd[QB];
    bool valid[QB];
    bool any = false;
#pragma unroll
    for (int t = 0; t < QB; ++t) {
        const int blk = chunk * (4 * QB) + t * 4 + wave;
        valid[t] = blk < nblk;
        any |= valid[t];
        const int row = min(blk * 16 + i, Kq - 1);
        const float4 x = *reinterpret_cast<const float4 *>(qs + (size_t)row * kD + 4 * g);
        qf[t] = make_float4(0.25f * x.x, 0.25f * x.y, 0.25f * x.z, 0.25f * x.w);
        dof[t] = *reinterpret_cast<const float4 *>(dos + (size_t)row * kD + 4 * g);
        const size_t sr = ((size_t)b * kHeads + h) * Kq + row;
        const float2 ml = *reinterpret_cast<const float2 *>(stats + sr * 2);
        m[t] = ml.x;
        inv_l[t] = 1.0f / ml.y;
        dd[t] = dsum[sr];
        acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (!any) return;                                      // wave-uniform; the kernel has no barrier
    const int n_begin = split * split_len, n_end = min(N, n_begin + split_len);
    for (int n0 = n_begin; n0 < n_end; n0 += kTile) {
        float4 kf[4], vf[4];
        float kcol[4][4];
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            const int key = min(n0 + 16 * kb + i, N - 1);
            kf[kb] = *reinterpret_cast<const float4 *>(ks + (size_t)key * kD + 4 * g);
            vf[kb] = *reinterpret_cast<const float4 *>(vs + (size_t)key * kD + 4 * g);
        }
#pragma unroll
        for (int kb = 0; kb < 4; ++kb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = min(n0 + 16 * kb + 4 * g + r, N - 1);
                kcol[kb][r] = ks[(size_t)key * kD + i];
            }
#pragma unroll
        for (int t = 0; t < QB; ++t) {
            if (!valid[t]) continue;
            f32x4 o = acc[t];
#pragma unroll
            for (int kb = 0; kb < 4; ++kb) {
                f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
                s = MFMA(kf[kb].x, qf[t].x, s);
                s = MFMA(kf[kb].y, qf[t].y, s);
                s = MFMA(kf[kb].z, qf[t].z, s);
                s = MFMA(kf[kb].w, qf[t].w, s);            // s[r]: key 4g + r against query i
                dp = MFMA(vf[kb].x, dof[t].x, dp);
                dp = MFMA(vf[kb].y, dof[t].y, dp);
                dp = MFMA(vf[kb].z, dof[t].z, dp);
                dp = MFMA(vf[kb].w, dof[t].w, dp);
                uint32_t keep = 0;                         // the mask indexes nothing: a row past Kq or a key past N is a value like any
                if (kDrop) keep = fnp_dropout_keep4(seed, da.threshold, b, h, (chunk * (4 * QB) + t * 4 + wave) * 16 + i, (n0 + 16 * kb + 4 * g) >> 2);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float p = expf(s[r] - m[t]) * inv_l[t];
                    if (n0 + 16 * kb + 4 * g + r >= n_end) p = 0.f;
                    if (kDrop) o = MFMA(kcol[kb][r], p * (((keep >> r) & 1 ? da.scale : 0.f) * dp[r] - dd[t]), o);
                    else o = MFMA(kcol[kb][r], p * (dp[r] - dd[t]), o);
                }
            }
            acc[t] = o;
        }
    }
#pragma unroll
    for (int t = 0; t < QB; ++t) {
        if (!valid[t]) continue;
        const int row = (chunk * (4 * QB) + t * 4 + wave) * 16 + i;
        if (row >= Kq) continue;
        if (nsplit == 1) {
            *reinterpret_cast<float4 *>(dq + ((size_t)b * Kq + row) * kD + 16 * h + 4 * g) =
                make_float4(0.25f * acc[t][0], 0.25f * acc[t][1], 0.25f * acc[t][2], 0.25f * acc[t][3]);
        } else {
            const size_t slot = (((size_t)b * nsplit + split) * kHeads + h) * Kq + row;
            *reinterpret_cast<float4 *>(part + slot * 16 + 4 * g) = make_float4(acc[t][0], acc[t][1], acc[t][2], acc[t][3]);
        }
    }
}

// one thread per (scene, query, head, 4 dims): the parts of the splits in split order
__global__ __launch_bounds__(256) void tf_attn_bwd_q_merge_kernel(const float *__restrict__ part, int Kq, int nsplit, long long total,
                                                                  float *__restrict__ dq) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int quad = (int)(e & 3), h = (int)((e >> 2) & 7);
    const long long br = e >> 5;                           // b * Kq + row
    const long long b = br / Kq;
    const int row = (int)(br - b * Kq);
    float o0 = 0.f, o1 = 0.f, o2 = 0.f, o3 = 0.f;
    for (int s = 0; s < nsplit; ++s) {
        const size_t slot = (((size_t)b * nsplit + s) * kHeads + h) * Kq + row;
        const float4 a = *reinterpret_cast<const float4 *>(part + slot * 16 + 4 * quad);
        o0 += a.x, o1 += a.y, o2 += a.z, o3 += a.w;
    }
    *reinterpret_cast<float4 *>(dq + (size_t)br * kD + 16 * h + 4 * quad) = make_float4(0.25f * o0, 0.25f * o1, 0.25f * o2, 0.25f * o3);
}

// ---- the mask written out: one thread per (scene x head, query, aligned group of four keys) -------------------------------------

__global__ __launch_bounds__(256) void tf_attn_dropout_mask_kernel(const unsigned long long *__restrict__ seed, uint32_t threshold, int Kq,
                                                                   int N, uint8_t *__restrict__ keep) {
    const int group = blockIdx.x * 256 + threadIdx.x, query = blockIdx.y, b = blockIdx.z >> 3, h = blockIdx.z & 7;
    if (4ll * group >= N) return;
    const uint32_t bits = fnp_dropout_keep4(*seed, threshold, b, h, query, group);
    uint8_t *row = keep + ((size_t)blockIdx.z * Kq + query) * N;
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (4 * group + r < N) row[4 * group + r] = (bits >> r) & 1;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------

bool shape_ok(long long B, long long Kq, long long N) {      // fnp_tf_attention's
    if (B < 0 || Kq < 1 || Kq > 2048 || N < 1 || N >= (1ll << 31) / kD) return false;
    return B * ((Kq + 63) / 64) <= 65535;
}

long long d_floats(long long B, long long Kq) { return (B * kHeads * Kq + 3) / 4 * 4; }    // the parts behind it stay 16-byte aligned

long long ws_floats(long long B, long long Kq, long long N) {
    int sl, tl;
    if (fnp_tf_attention_geometry(N, &sl, &tl) != FNP_OK) return -1;
    const long long nsplit = (N + sl - 1) / sl, b = B > 0 ? B : 1;
    return d_floats(b, Kq) + (nsplit > 1 ? b * nsplit * kHeads * Kq * 16 : 0);
}

}  // namespace

extern "C" int fnp_tf_attention_backward_geometry(int64_t n_keys, int *key_block, int *wave_keys) {
    if (n_keys < 1 || n_keys >= (1ll << 31) / kD || !key_block || !wave_keys) return FNP_ERR_ARG;
    *key_block = kKeyBlock;
    *wave_keys = kWaveKeys;
    return FNP_OK;
}

extern "C" int64_t fnp_tf_attention_backward_workspace_bytes(int batch_size, int num_queries, int64_t num_keys) {
    if (!shape_ok(batch_size, num_queries, num_keys)) return FNP_ERR_ARG;
    return ws_floats(batch_size, num_queries, num_keys) * 4;
}

namespace {

// DROP: empty, or the one fnp_dropout_args every gradient kernel of the call gets
template <typename... DROP>
int launch_backward(const float *q, const float *k, const float *v, const float *out, const float *stats, const float *d_out,
                    int batch_size, int num_queries, int64_t num_keys, void *workspace, int64_t workspace_bytes, float *dq, float *dk,
                    float *dv, fnp_stream_t stream, DROP... drop) {
    if (!shape_ok(batch_size, num_queries, num_keys)) return FNP_ERR_ARG;
    if (batch_size == 0) return FNP_OK;
    if (!q || !k || !v || !out || !stats || !d_out) return FNP_ERR_ARG;
    if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out | (uintptr_t)stats | (uintptr_t)d_out | (uintptr_t)workspace |
         (uintptr_t)dq | (uintptr_t)dk | (uintptr_t)dv) & 15)
        return FNP_ERR_ARG;
    if (!dq && !dk && !dv) return FNP_OK;
    const int B = batch_size, Kq = num_queries, N = (int)num_keys;
    if (!workspace || workspace_bytes < ws_floats(B, Kq, N) * 4) return FNP_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    float *dsum = (float *)workspace, *part = dsum + d_floats(B, Kq);
    const int nblk = (Kq + 15) / 16;
    hipLaunchKernelGGL(tf_attn_bwd_d_kernel, dim3(nblk, kHeads, B), dim3(64), 0, s, out, d_out, Kq, dsum);
    FNP_LAUNCH_CHECK();
    if (dk || dv) {
        const dim3 grid((N + kKeyBlock - 1) / kKeyBlock, kHeads, B);
#define FNP_KV(WK, WV)                                                                                                            \
    hipLaunchKernelGGL(HIP_KERNEL_NAME(tf_attn_bwd_kv_kernel<WK, WV, DROP...>), grid, dim3(kThreads), 0, s, q, k, v, d_out, stats, \
                       (const float *)dsum, Kq, N, dk, dv, drop...)
        if (dk && dv) FNP_KV(true, true);
        else if (dk) FNP_KV(true, false);
        else FNP_KV(false, true);
#undef FNP_KV
        FNP_LAUNCH_CHECK();
    }
    if (dq) {
        int sl, tl;
        if (fnp_tf_attention_geometry(N, &sl, &tl) != FNP_OK) return FNP_ERR_ARG;
        // the forward's query chunks (launch_attention of tfdecoder.hip): up to four blocks of 16 queries per wave with several
        // splits, one with a single split; a block's arithmetic does not depend on the workgroup it runs in
        const int nsplit = (N + sl - 1) / sl;
        const int qb = nsplit == 1 ? 1 : (nblk >= 16 ? 4 : (nblk + 3) / 4);
        const int nchunk = (nblk + 4 * qb - 1) / (4 * qb);
        const dim3 grid(nsplit, kHeads, B * nchunk);
#define FNP_Q(QB)                                                                                                                 \
    hipLaunchKernelGGL(HIP_KERNEL_NAME(tf_attn_bwd_q_kernel<QB, DROP...>), grid, dim3(kThreads), 0, s, q, k, v, d_out, stats,     \
                       (const float *)dsum, Kq, N, sl, nsplit, nchunk, part, dq, drop...)
        if (qb == 1) FNP_Q(1);
        else if (qb == 2) FNP_Q(2);
        else if (qb == 3) FNP_Q(3);
        else FNP_Q(4);
#undef FNP_Q
        FNP_LAUNCH_CHECK();
        if (nsplit > 1) {
            const long long total = (long long)B * Kq * 32;
            hipLaunchKernelGGL(tf_attn_bwd_q_merge_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const float *)part, Kq,
                               nsplit, total, dq);
            FNP_LAUNCH_CHECK();
        }
    }
    return FNP_OK;
}

}  // namespace

extern "C" int fnp_tf_attention_backward(const float *q, const float *k, const float *v, const float *out, const float *stats,
                                         const float *d_out, int batch_size, int num_queries, int64_t num_keys, void *workspace,
                                         int64_t workspace_bytes, float *dq, float *dk, float *dv, fnp_stream_t stream) {
    return launch_backward(q, k, v, out, stats, d_out, batch_size, num_queries, num_keys, workspace, workspace_bytes, dq, dk, dv, stream);
}

// the same launches on the dropout instantiations of the two gradient kernels; out is the dropped output, so the prologue's D holds
extern "C" int fnp_tf_attention_dropout_backward(const float *q, const float *k, const float *v, const float *out, const float *stats,
                                                 const float *d_out, int batch_size, int num_queries, int64_t num_keys, void *workspace,
                                                 int64_t workspace_bytes, float *dq, float *dk, float *dv, float p, const uint64_t *seed,
                                                 fnp_stream_t stream) {
    if (!(p >= 0.f && p < 1.f)) return FNP_ERR_ARG;
    if (batch_size > 0 && (!seed || ((uintptr_t)seed & 7))) return FNP_ERR_ARG;
    const uint32_t threshold = fnp_dropout_threshold(p);
    return launch_backward(q, k, v, out, stats, d_out, batch_size, num_queries, num_keys, workspace, workspace_bytes, dq, dk, dv, stream,
                           fnp_dropout_args{(const unsigned long long *)seed, threshold, fnp_dropout_scale(threshold)});
}

// keep (B, 8, Kq, N), one byte per element: what the three kernels derive, written out for the tests; no training path launches it
extern "C" int fnp_tf_attention_dropout_mask(const uint64_t *seed, float p, int batch_size, int num_queries, int64_t num_keys,
                                             uint8_t *keep, fnp_stream_t stream) {
    if (!shape_ok(batch_size, num_queries, num_keys) || !(p >= 0.f && p < 1.f)) return FNP_ERR_ARG;
    if (batch_size == 0) return FNP_OK;
    if (!seed || ((uintptr_t)seed & 7) || !keep || (long long)batch_size * kHeads > 65535) return FNP_ERR_ARG;
    const int N = (int)num_keys, groups = (N + 3) / 4;
    hipLaunchKernelGGL(tf_attn_dropout_mask_kernel, dim3((groups + 255) / 256, num_queries, batch_size * kHeads), dim3(256), 0,
                       (hipStream_t)stream, (const unsigned long long *)seed, fnp_dropout_threshold(p), num_queries, N, keep);
    FNP_LAUNCH_CHECK();
    return FNP_OK;
}
