// TransFusionHead's decoder layer and prediction heads (pcdet/models/model_utils/transfusion_utils.py:29-101 and
// transfusion_head.py:20-54, eval mode) as seven launches (eight with more than 256 queries: the self-attention then has splits to merge); the contract is the fnp_tf_decoder block of include/fnp.h.
//
// All arithmetic is f32 on v_mfma_f32_16x16x4_f32 (a k-ordered fmaf chain per output element), no atomics: every result is
// bit-identical from run to run, and a scene's result does not depend on the batch it runs in.
//
// Operand trick used throughout: the contraction index of an MFMA step is a sum index, so it may be permuted as long as both
// operands agree.  A lane (i = lane & 15, g = lane >> 4) loads ONE float4 at column 4g of a 16-wide chunk and feeds element s
// to step s: step s then contracts columns {4g + s}, and the four steps cover the chunk.  No operand needs a transpose in LDS.
//
//   attention   S^T = K Q^T (A = keys, B = queries): a lane holds the scores of query i against keys 4g + r, which is exactly
//               the B operand (k = g) of O^T = V^T P^T when step r contracts keys {4g + r}.  The softmax statistics of query i
//               live in lane column i, the same column the O^T accumulators of that query live in.
//   kv_proj     eight waves; wave w keeps the 16 output columns 16w.. of Wk AND Wv in registers (64 VGPRs) and the workgroup
//               walks 64-key tiles of the channel-major feature map staged (with the position embedding added) in LDS.
//   row kernels 16 queries per workgroup, the activations in LDS, the weights straight from L2 as B operands.
#include <math.h>

#include "common.h"
#include "tfattn_dropout.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kD = 128;            // d_model
constexpr int kHeads = 8;          // heads of 16
constexpr int kTile = 64;          // keys per tile (tile_len)
constexpr int kMinSplit = 256;     // a split is never shorter: N <= 256 is one split (the self-attention)
constexpr int kSplits = 64;        // target number of splits of a scene: 8 heads x 64 = 512 workgroups, two per CU
constexpr int kAttThreads = 256;
constexpr int kRS = 132;           // LDS row stride of a 16 x 128 activation tile (floats; rows stay 16-byte aligned)
constexpr int kHS = 516;           // LDS row stride of the 16 x 512 hidden tile
constexpr int kHidChunk = 512;     // FFN hidden columns per pass
constexpr int kMaxHeads = 8;       // prediction heads (64 hidden columns each fill the hidden tile)
constexpr int kHeadMid = 64;
constexpr int kRowThreads = 256;
constexpr int kKvThreads = 512;
constexpr int kXS = 68;            // LDS row stride of the 128 x 64 feature tile of kv_proj

#define MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

inline void att_geometry(long long n, int *split_len, int *tile_len) {
    long long per = (n + kSplits - 1) / kSplits;
    long long len = (per + kTile - 1) / kTile * kTile;
    if (len < kMinSplit) len = kMinSplit;
    *split_len = (int)len;
    *tile_len = kTile;
}

// ---- (a) attention ---------------------------------------------------------------------------------------------------------

// stats (NULL in fnp_tf_attention and in the decoder): the softmax statistics (M, L) per (scene, head, query) for the backward of
// tfattn_grad.hip, written by whichever launch writes out; the arithmetic of out does not depend on it.
// DROP is empty (every launch but fnp_tf_attention_dropout_stats': the kernel and its arguments as they always were) or one
// fnp_dropout_args: then p feeds the V product as p * Z, Z = keep / (1 - p_eff) (tfattn_dropout.h), and l still sums every p.  A
// lane's four keys n0 + 16 kb + 4 g + r of a query are one aligned group of four: one generator call.
template <int QB, typename... DROP>
__global__ __launch_bounds__(kAttThreads) void tf_attn_kernel(const float *__restrict__ q, const float *__restrict__ k,
                                                              const float *__restrict__ v, int Kq, int N, int split_len, int nsplit,
                                                              int nchunk, float *__restrict__ pacc, float *__restrict__ pml,
                                                              float *__restrict__ out, float *__restrict__ stats, DROP... drop) {
    const int split = blockIdx.x, h = blockIdx.y, b = blockIdx.z / nchunk, chunk = blockIdx.z % nchunk;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, g = lane >> 4;
    const int nblk = (Kq + 15) >> 4;
    const float *qs = q + (size_t)b * Kq * kD + 16 * h;
    const float *ks = k + (size_t)b * N * kD + 16 * h;
    const float *vs = v + (size_t)b * N * kD + 16 * h;
    constexpr bool kDrop = sizeof...(DROP) != 0;
    const fnp_dropout_args da = fnp_dropout_of(drop...);
    const unsigned long long seed = kDrop ? *da.seed : 0ull;

    float4 qf[QB];
    f32x4 acc[QB];
    float m[QB], l[QB];
    bool valid[QB];
    bool any = false;
#pragma unroll
    for (int t = 0; t < QB; ++t) {
        const int blk = chunk * (4 * QB) + t * 4 + wave;
        valid[t] = blk < nblk;
        any |= valid[t];
        const int row = min(blk * 16 + i, Kq - 1);
        const float4 x = *reinterpret_cast<const float4 *>(qs + (size_t)row * kD + 4 * g);
        qf[t] = make_float4(0.25f * x.x, 0.25f * x.y, 0.25f * x.z, 0.25f * x.w);   // 1 / sqrt(16): exact
        acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        m[t] = -INFINITY;
        l[t] = 0.f;
    }
    if (!any) return;                                      // wave-uniform; the kernel has no barrier
    const int n_begin = split * split_len, n_end = min(N, n_begin + split_len);
    for (int n0 = n_begin; n0 < n_end; n0 += kTile) {
        float4 kf[4];
        float vf[4][4];
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            const int key = min(n0 + 16 * kb + i, N - 1);
            kf[kb] = *reinterpret_cast<const float4 *>(ks + (size_t)key * kD + 4 * g);
        }
#pragma unroll
        for (int kb = 0; kb < 4; ++kb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = min(n0 + 16 * kb + 4 * g + r, N - 1);
                vf[kb][r] = vs[(size_t)key * kD + i];
            }
#pragma unroll
        for (int t = 0; t < QB; ++t) {
            if (!valid[t]) continue;
            f32x4 s[4];
            float tmax = -INFINITY;
#pragma unroll
            for (int kb = 0; kb < 4; ++kb) {
                f32x4 c = {0.f, 0.f, 0.f, 0.f};
                c = MFMA(kf[kb].x, qf[t].x, c);
                c = MFMA(kf[kb].y, qf[t].y, c);
                c = MFMA(kf[kb].z, qf[t].z, c);
                c = MFMA(kf[kb].w, qf[t].w, c);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (n0 + 16 * kb + 4 * g + r >= n_end) c[r] = -INFINITY;
                    tmax = fmaxf(tmax, c[r]);
                }
                s[kb] = c;
            }
            tmax = fmaxf(tmax, __shfl_xor(tmax, 16));
            tmax = fmaxf(tmax, __shfl_xor(tmax, 32));      // finite: a tile holds at least one key of the split
            const float m_new = fmaxf(m[t], tmax);
            const float sc = expf(m[t] - m_new);           // first tile: exp(-inf) = 0
            m[t] = m_new;
            float psum = 0.f;
            f32x4 o = acc[t];
#pragma unroll
            for (int r = 0; r < 4; ++r) o[r] *= sc;
#pragma unroll
            for (int kb = 0; kb < 4; ++kb) {
                uint32_t keep = 0;                         // the mask indexes nothing: a row past Kq or a key past N is a value like any
                if (kDrop) keep = fnp_dropout_keep4(seed, da.threshold, b, h, (chunk * (4 * QB) + t * 4 + wave) * 16 + i, (n0 + 16 * kb + 4 * g) >> 2);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p = expf(s[kb][r] - m_new);
                    psum += p;
                    o = MFMA(vf[kb][r], kDrop ? ((keep >> r) & 1 ? p * da.scale : 0.f) : p, o);
                }
            }
            acc[t] = o;
            l[t] = l[t] * sc + psum;
        }
    }
#pragma unroll
    for (int t = 0; t < QB; ++t) {
        if (!valid[t]) continue;
        float lt = l[t];
        lt += __shfl_xor(lt, 16);
        lt += __shfl_xor(lt, 32);
        const int row = (chunk * (4 * QB) + t * 4 + wave) * 16 + i;
        if (row >= Kq) continue;
        if (nsplit == 1) {
            float4 o = make_float4(acc[t][0] / lt, acc[t][1] / lt, acc[t][2] / lt, acc[t][3] / lt);
            *reinterpret_cast<float4 *>(out + ((size_t)b * Kq + row) * kD + 16 * h + 4 * g) = o;
            if (stats && g == 0) *reinterpret_cast<float2 *>(stats + (((size_t)b * kHeads + h) * Kq + row) * 2) = make_float2(m[t], lt);
        } else {
            const size_t slot = (((size_t)b * nsplit + split) * kHeads + h) * Kq + row;
            *reinterpret_cast<float4 *>(pacc + slot * 16 + 4 * g) = make_float4(acc[t][0], acc[t][1], acc[t][2], acc[t][3]);
            if (g == 0) pml[slot * 2] = m[t], pml[slot * 2 + 1] = lt;
        }
    }
}

// one thread per (scene, query, head, 4 dims): the partials of the splits in split order; stats (or NULL) gets (M, L)
__global__ __launch_bounds__(256) void tf_attn_merge_kernel(const float *__restrict__ pacc, const float *__restrict__ pml, int Kq,
                                                            int nsplit, long long total, float *__restrict__ out,
                                                            float *__restrict__ stats) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int quad = (int)(e & 3), h = (int)((e >> 2) & 7);
    const long long br = e >> 5;                           // b * Kq + row
    const long long b = br / Kq;
    const int row = (int)(br - b * Kq);
    float M = -INFINITY;
    for (int s = 0; s < nsplit; ++s) M = fmaxf(M, pml[((((size_t)b * nsplit + s) * kHeads + h) * Kq + row) * 2]);
    float L = 0.f, o0 = 0.f, o1 = 0.f, o2 = 0.f, o3 = 0.f;
    for (int s = 0; s < nsplit; ++s) {
        const size_t slot = (((size_t)b * nsplit + s) * kHeads + h) * Kq + row;
        const float w = expf(pml[slot * 2] - M);
        const float4 a = *reinterpret_cast<const float4 *>(pacc + slot * 16 + 4 * quad);
        L = fmaf(pml[slot * 2 + 1], w, L);
        o0 = fmaf(a.x, w, o0), o1 = fmaf(a.y, w, o1), o2 = fmaf(a.z, w, o2), o3 = fmaf(a.w, w, o3);
    }
    *reinterpret_cast<float4 *>(out + (size_t)br * kD + 16 * h + 4 * quad) = make_float4(o0 / L, o1 / L, o2 / L, o3 / L);
    if (stats && quad == 0) *reinterpret_cast<float2 *>(stats + (((size_t)b * kHeads + h) * Kq + row) * 2) = make_float2(M, L);
}

// ---- (b) key / value projection ----------------------------------------------------------------------------------------------

// K = (x + pe) Wk^T + bk, V = (x + pe) Wv^T + bv.  x (B, 128, N) and pe (128, N), or (B, 128, N) with pe_stride = 128 N, channel-major, wkv = [Wk; Wv] (256, 128),
// bkv (256); K, V (B, N, 128).  Tiles of 64 keys, grid-strided.
__global__ __launch_bounds__(kKvThreads) void tf_kv_proj_kernel(const float *__restrict__ x, const float *__restrict__ pe_all,
                                                                long long pe_stride, const float *__restrict__ wkv, const float *__restrict__ bkv, int N,
                                                                int tiles_per_scene, int total_tiles, float *__restrict__ Ko,
                                                                float *__restrict__ Vo) {
    __shared__ __attribute__((aligned(16))) float xs[kD * kXS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, g = lane >> 4;
    float4 wk[8], wv[8];
#pragma unroll
    for (int cc = 0; cc < 8; ++cc) {
        wk[cc] = *reinterpret_cast<const float4 *>(wkv + (size_t)(16 * wave + i) * kD + 16 * cc + 4 * g);
        wv[cc] = *reinterpret_cast<const float4 *>(wkv + (size_t)(kD + 16 * wave + i) * kD + 16 * cc + 4 * g);
    }
    const float bk = bkv[16 * wave + i], bv = bkv[kD + 16 * wave + i];
    for (int tile = blockIdx.x; tile < total_tiles; tile += gridDim.x) {
        const int b = tile / tiles_per_scene, n0 = (tile - b * tiles_per_scene) * kTile;
        const float *xb = x + (size_t)b * kD * N;
        const float *pe = pe_all + (size_t)b * pe_stride;
        __syncthreads();                                   // the previous tile's readers are done
        for (int e = tid; e < kD * kTile; e += kKvThreads) {
            const int c = e >> 6, j = e & 63;
            const int n = n0 + j;
            float val = 0.f;
            if (n < N) val = xb[(size_t)c * N + n] + pe[(size_t)c * N + n];
            xs[c * kXS + j] = val;
        }
        __syncthreads();
#pragma unroll 1
        for (int mb = 0; mb < 4; ++mb) {
            if (n0 + 16 * mb >= N) break;
            f32x4 ak = {0.f, 0.f, 0.f, 0.f}, av = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int cc = 0; cc < 8; ++cc) {
                const float *xr = xs + (16 * cc + 4 * g) * kXS + 16 * mb + i;
                const float a0 = xr[0], a1 = xr[kXS], a2 = xr[2 * kXS], a3 = xr[3 * kXS];
                ak = MFMA(a0, wk[cc].x, ak), av = MFMA(a0, wv[cc].x, av);
                ak = MFMA(a1, wk[cc].y, ak), av = MFMA(a1, wv[cc].y, av);
                ak = MFMA(a2, wk[cc].z, ak), av = MFMA(a2, wv[cc].z, av);
                ak = MFMA(a3, wk[cc].w, ak), av = MFMA(a3, wv[cc].w, av);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = n0 + 16 * mb + 4 * g + r;
                if (n < N) {
                    const size_t o = ((size_t)b * N + n) * kD + 16 * wave + i;
                    Ko[o] = ak[r] + bk;
                    Vo[o] = av[r] + bv;
                }
            }
        }
    }
}

// ---- (c) query-side row kernels -----------------------------------------------------------------------------------------------

struct TfOff {      // offsets into the packed parameter block, in floats (the layout is documented in include/fnp.h)
    int eps, qpe_w1, qpe_b1, qpe_w2, qpe_b2, sa_w, sa_b, sa_ow, sa_ob, ln1_g, ln1_b, ca_w, ca_b, ca_ow, ca_ob, ln2_g, ln2_b;
    int f_w1, f_b1, f_w2, f_b2, ln3_g, ln3_b, h_w1, h_b1, h_w2, h_b2, total;
};

struct TfHeads {
    int n, center;
    int n_out[kMaxHeads], row_off[kMaxHeads], out_off[kMaxHeads];   // padded row offset into h_w2; channel offset of the outputs
    int blocks;                                                       // sum of ceil(n_out / 16)
};

bool tf_layout(int ffn, int n_heads, const int *head_out, int center_head, TfOff *o, TfHeads *hd) {
    if (ffn < 16 || ffn > 1024 || (ffn & 15) || n_heads < 0 || n_heads > kMaxHeads || (n_heads && !head_out)) return false;
    if (center_head >= n_heads) return false;
    hd->n = n_heads, hd->center = center_head, hd->blocks = 0;
    int rows = 0, chans = 0;
    for (int h = 0; h < n_heads; ++h) {
        if (head_out[h] < 1 || head_out[h] > 64) return false;
        hd->n_out[h] = head_out[h], hd->row_off[h] = rows, hd->out_off[h] = chans;
        rows += (head_out[h] + 15) / 16 * 16, chans += head_out[h];
        hd->blocks += (head_out[h] + 15) / 16;
    }
    if (center_head >= 0 && head_out[center_head] != 2) return false;
    for (int h = n_heads; h < kMaxHeads; ++h) hd->n_out[h] = hd->row_off[h] = hd->out_off[h] = 0;
    int p = 0;
    auto take = [&p](int n) { const int at = p; p += n; return at; };
    o->eps = take(4);
    o->qpe_w1 = take(kD * 2), o->qpe_b1 = take(kD), o->qpe_w2 = take(kD * kD), o->qpe_b2 = take(kD);
    o->sa_w = take(3 * kD * kD), o->sa_b = take(3 * kD), o->sa_ow = take(kD * kD), o->sa_ob = take(kD);
    o->ln1_g = take(kD), o->ln1_b = take(kD);
    o->ca_w = take(3 * kD * kD), o->ca_b = take(3 * kD), o->ca_ow = take(kD * kD), o->ca_ob = take(kD);
    o->ln2_g = take(kD), o->ln2_b = take(kD);
    o->f_w1 = take(ffn * kD), o->f_b1 = take(ffn), o->f_w2 = take(kD * ffn), o->f_b2 = take(kD);
    o->ln3_g = take(kD), o->ln3_b = take(kD);
    o->h_w1 = take(n_heads * kHeadMid * kD), o->h_b1 = take(n_heads * kHeadMid);
    o->h_w2 = take(rows * kHeadMid), o->h_b2 = take(rows);
    o->total = p;
    return true;
}

// NB blocks of 16 output columns from o0: acc[nb] (row 4g + r, column o0 + 16 nb + i) += X (LDS, 16 rows of stride xstride,
// CIN columns, CIN a multiple of 16) . W^T, W rows of leading dimension ldw in global memory.  CIN is a compile-time constant
// so that every weight load of the call is issued before the first product: the row kernels run a handful of workgroups and
// are bound by the latency of these loads, not by their number.
template <int NB, int CIN>
__device__ __forceinline__ void row_gemm(const float *Xs, int xstride, const float *__restrict__ W, int ldw, int o0, f32x4 *acc) {
    const int lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
    const float *xr = Xs + i * xstride + 4 * g;
    const float *wr = W + (size_t)(o0 + i) * ldw + 4 * g;
    float4 w[NB][CIN / 16];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int c = 0; c < CIN / 16; ++c) w[nb][c] = *reinterpret_cast<const float4 *>(wr + (size_t)nb * 16 * ldw + 16 * c);
#pragma unroll
    for (int c = 0; c < CIN / 16; ++c) {
        const float4 a = *reinterpret_cast<const float4 *>(xr + 16 * c);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            acc[nb] = MFMA(a.x, w[nb][c].x, acc[nb]);
            acc[nb] = MFMA(a.y, w[nb][c].y, acc[nb]);
            acc[nb] = MFMA(a.z, w[nb][c].z, acc[nb]);
            acc[nb] = MFMA(a.w, w[nb][c].w, acc[nb]);
        }
    }
}

// the same over a run-time number of columns (a multiple of 16): 128 at a time, then 16 at a time, in ascending order
template <int NB>
__device__ __forceinline__ void row_gemm_n(const float *Xs, int xstride, const float *__restrict__ W, int ldw, int cin, int o0, f32x4 *acc) {
    int c = 0;
    for (; c + 128 <= cin; c += 128) row_gemm<NB, 128>(Xs + c, xstride, W + c, ldw, o0, acc);
    for (; c < cin; c += 16) row_gemm<NB, 16>(Xs + c, xstride, W + c, ldw, o0, acc);
}

// LayerNorm of the 16 rows of S (stride kRS) in place: biased variance, two passes; 16 threads per row, fixed reduction order
__device__ __forceinline__ void row_layernorm(float *S, const float *__restrict__ gamma, const float *__restrict__ beta, float eps) {
    const int row = threadIdx.x >> 4, sub = threadIdx.x & 15;
    float *s = S + row * kRS;
    float x[8], sum = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = s[sub + 16 * j], sum += x[j];
#pragma unroll
    for (int d = 1; d < 16; d <<= 1) sum += __shfl_xor(sum, d);
    const float mean = sum / (float)kD;
    float sq = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] -= mean, sq = fmaf(x[j], x[j], sq);
#pragma unroll
    for (int d = 1; d < 16; d <<= 1) sq += __shfl_xor(sq, d);
    const float rstd = 1.0f / sqrtf(sq / (float)kD + eps);
#pragma unroll
    for (int j = 0; j < 8; ++j) s[sub + 16 * j] = fmaf(x[j] * rstd, gamma[sub + 16 * j], beta[sub + 16 * j]);
}

// 16 rows of a (B*K, 128) row-major array into an LDS tile, rows past `rows` as zeros
__device__ __forceinline__ void load_rows(float *S, const float *__restrict__ src, int rows) {
    for (int e = threadIdx.x; e < 16 * 32; e += kRowThreads) {
        const int j = e >> 5, c4 = e & 31;
        float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
        if (j < rows) val = *reinterpret_cast<const float4 *>(src + (size_t)j * kD + 4 * c4);
        *reinterpret_cast<float4 *>(S + j * kRS + 4 * c4) = val;
    }
}

// front: rows x = query_feat^T, qpe = self_posembed(query_pos), self-attention in-projection of x + qpe
__global__ __launch_bounds__(kRowThreads) void tf_front_kernel(const float *__restrict__ query_feat, const float *__restrict__ query_pos,
                                                               const float *__restrict__ P, TfOff off, int K, float *__restrict__ xrow,
                                                               float *__restrict__ qpe, float *__restrict__ qs, float *__restrict__ ks,
                                                               float *__restrict__ vs) {
    __shared__ __attribute__((aligned(16))) float Xs[16 * kRS], Ps[16 * kRS], Hs[16 * kRS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, g = lane >> 4;
    const int b = blockIdx.y, k0 = blockIdx.x * 16, rows = min(16, K - k0);
    const size_t base = ((size_t)b * K + k0) * kD;
    for (int e = tid; e < 16 * kD; e += kRowThreads) {
        const int c = e >> 4, j = e & 15;
        Xs[j * kRS + c] = j < rows ? query_feat[((size_t)b * kD + c) * K + k0 + j] : 0.f;
    }
    for (int e = tid; e < 16 * kD; e += kRowThreads) {
        const int j = e >> 7, c = e & 127;
        float hval = 0.f;
        if (j < rows) {
            const float px = query_pos[((size_t)b * K + k0 + j) * 2], py = query_pos[((size_t)b * K + k0 + j) * 2 + 1];
            hval = fmaxf(fmaf(P[off.qpe_w1 + 2 * c + 1], py, fmaf(P[off.qpe_w1 + 2 * c], px, P[off.qpe_b1 + c])), 0.f);
        }
        Hs[j * kRS + c] = hval;
    }
    __syncthreads();
    {
        f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        row_gemm<2, kD>(Hs, kRS, P + off.qpe_w2, kD, 32 * wave, acc);
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int col = 32 * wave + 16 * nb + i, j = 4 * g + r;
                const float val = acc[nb][r] + P[off.qpe_b2 + col];
                Ps[j * kRS + col] = val;
                if (j < rows) qpe[base + (size_t)j * kD + col] = val;
            }
    }
    __syncthreads();
    for (int e = tid; e < 16 * kD; e += kRowThreads) {
        const int j = e >> 7, c = e & 127;
        const float xv = Xs[j * kRS + c];
        if (j < rows) xrow[base + (size_t)j * kD + c] = xv;
        Hs[j * kRS + c] = xv + Ps[j * kRS + c];
    }
    __syncthreads();
#pragma unroll 1
    for (int pass = 0; pass < 3; ++pass) {                 // 24 column blocks: wave w takes 6w .. 6w + 5
        f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        const int o0 = 96 * wave + 32 * pass;
        row_gemm<2, kD>(Hs, kRS, P + off.sa_w, kD, o0, acc);
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            const int col = o0 + 16 * nb + i;
            float *dst = col < kD ? qs : (col < 2 * kD ? ks : vs);
            const float bias = P[off.sa_b + col];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = 4 * g + r;
                if (j < rows) dst[base + (size_t)j * kD + (col & 127)] = acc[nb][r] + bias;
            }
        }
    }
}

// mid: x1 = LayerNorm1(x + attn . Wo^T + bo), cross-attention query projection of x1 + qpe
__global__ __launch_bounds__(kRowThreads) void tf_mid_kernel(const float *__restrict__ attn, const float *__restrict__ xrow,
                                                             const float *__restrict__ qpe, const float *__restrict__ P, TfOff off, int K,
                                                             float *__restrict__ x1, float *__restrict__ qc) {
    __shared__ __attribute__((aligned(16))) float As[16 * kRS], Xs[16 * kRS], Ys[16 * kRS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, g = lane >> 4;
    const int b = blockIdx.y, k0 = blockIdx.x * 16, rows = min(16, K - k0);
    const size_t base = ((size_t)b * K + k0) * kD;
    load_rows(As, attn + base, rows);
    load_rows(Xs, xrow + base, rows);
    __syncthreads();
    {
        f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        row_gemm<2, kD>(As, kRS, P + off.sa_ow, kD, 32 * wave, acc);
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int col = 32 * wave + 16 * nb + i, j = 4 * g + r;
                Ys[j * kRS + col] = Xs[j * kRS + col] + (acc[nb][r] + P[off.sa_ob + col]);
            }
    }
    __syncthreads();
    row_layernorm(Ys, P + off.ln1_g, P + off.ln1_b, P[off.eps]);
    __syncthreads();
    for (int e = tid; e < 16 * 32; e += kRowThreads) {
        const int j = e >> 5, c4 = e & 31;
        const float4 y = *reinterpret_cast<const float4 *>(Ys + j * kRS + 4 * c4);
        float4 pe = make_float4(0.f, 0.f, 0.f, 0.f);
        if (j < rows) {
            *reinterpret_cast<float4 *>(x1 + base + (size_t)j * kD + 4 * c4) = y;
            pe = *reinterpret_cast<const float4 *>(qpe + base + (size_t)j * kD + 4 * c4);
        }
        *reinterpret_cast<float4 *>(As + j * kRS + 4 * c4) = make_float4(y.x + pe.x, y.y + pe.y, y.z + pe.z, y.w + pe.w);
    }
    __syncthreads();
    {
        f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        row_gemm<2, kD>(As, kRS, P + off.ca_w, kD, 32 * wave, acc);
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int col = 32 * wave + 16 * nb + i, j = 4 * g + r;
                if (j < rows) qc[base + (size_t)j * kD + col] = acc[nb][r] + P[off.ca_b + col];
            }
    }
}

// tail: x2 = LayerNorm2(x1 + attn . Wo^T + bo), x3 = LayerNorm3(x2 + FFN(x2)) -> query_feat (B, 128, K); the prediction heads
__global__ __launch_bounds__(kRowThreads) void tf_tail_kernel(const float *__restrict__ attn, const float *__restrict__ x1,
                                                              const float *__restrict__ query_pos, const float *__restrict__ P, TfOff off,
                                                              TfHeads hd, int B, int K, int ffn, float *__restrict__ out_feat,
                                                              float *__restrict__ out_heads) {
    __shared__ __attribute__((aligned(16))) float As[16 * kRS], Ys[16 * kRS], Hid[16 * kHS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, g = lane >> 4;
    const int b = blockIdx.y, k0 = blockIdx.x * 16, rows = min(16, K - k0);
    const size_t base = ((size_t)b * K + k0) * kD;
    load_rows(As, attn + base, rows);
    load_rows(Ys, x1 + base, rows);
    __syncthreads();
    {
        f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        row_gemm<2, kD>(As, kRS, P + off.ca_ow, kD, 32 * wave, acc);
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {          // each (row, column) of Ys is read and written by this lane alone
                const int col = 32 * wave + 16 * nb + i, j = 4 * g + r;
                Ys[j * kRS + col] = Ys[j * kRS + col] + (acc[nb][r] + P[off.ca_ob + col]);
            }
    }
    __syncthreads();
    row_layernorm(Ys, P + off.ln2_g, P + off.ln2_b, P[off.eps + 1]);
    __syncthreads();
    f32x4 ffn_acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    for (int c0 = 0; c0 < ffn; c0 += kHidChunk) {
        const int width = min(kHidChunk, ffn - c0);        // a multiple of 16
        for (int cb = 2 * wave; cb < width / 16; cb += 8) {        // column blocks in pairs; an odd count ends in a single one
            f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
            const int nb_here = cb + 1 < width / 16 ? 2 : 1;
            if (nb_here == 2) row_gemm<2, kD>(Ys, kRS, P + off.f_w1 + (size_t)c0 * kD, kD, 16 * cb, acc);
            else row_gemm<1, kD>(Ys, kRS, P + off.f_w1 + (size_t)c0 * kD, kD, 16 * cb, acc);
            for (int nb = 0; nb < nb_here; ++nb) {
                const float bias = P[off.f_b1 + c0 + 16 * (cb + nb) + i];
#pragma unroll
                for (int r = 0; r < 4; ++r) Hid[(4 * g + r) * kHS + 16 * (cb + nb) + i] = fmaxf(acc[nb][r] + bias, 0.f);
            }
        }
        __syncthreads();
        row_gemm_n<2>(Hid, kHS, P + off.f_w2 + c0, ffn, width, 32 * wave, ffn_acc);
        __syncthreads();
    }
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int col = 32 * wave + 16 * nb + i, j = 4 * g + r;
            As[j * kRS + col] = Ys[j * kRS + col] + (ffn_acc[nb][r] + P[off.f_b2 + col]);
        }
    __syncthreads();
    row_layernorm(As, P + off.ln3_g, P + off.ln3_b, P[off.eps + 2]);
    __syncthreads();
    for (int e = tid; e < 16 * kD; e += kRowThreads) {
        const int c = e >> 4, j = e & 15;
        if (j < rows) out_feat[((size_t)b * kD + c) * K + k0 + j] = As[j * kRS + c];
    }
    if (hd.n == 0) return;
    for (int cb = 2 * wave; cb < hd.n * kHeadMid / 16; cb += 8) {  // 4 blocks per head: an even count
        f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        row_gemm<2, kD>(As, kRS, P + off.h_w1, kD, 16 * cb, acc);
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            const float bias = P[off.h_b1 + 16 * (cb + nb) + i];
#pragma unroll
            for (int r = 0; r < 4; ++r) Hid[(4 * g + r) * kHS + 16 * (cb + nb) + i] = fmaxf(acc[nb][r] + bias, 0.f);
        }
    }
    __syncthreads();
    for (int blk = wave; blk < hd.blocks; blk += 4) {
        int h = 0, rem = blk;
        while (rem >= (hd.n_out[h] + 15) / 16) rem -= (hd.n_out[h] + 15) / 16, ++h;
        f32x4 acc[1] = {{0.f, 0.f, 0.f, 0.f}};
        row_gemm<1, kHeadMid>(Hid + h * kHeadMid, kHS, P + off.h_w2 + (size_t)hd.row_off[h] * kHeadMid, kHeadMid, 16 * rem, acc);
        const int o = 16 * rem + i;
        if (o >= hd.n_out[h]) continue;
        const float bias = P[off.h_b2 + hd.row_off[h] + o];
        float *dst = out_heads + (size_t)B * K * hd.out_off[h] + ((size_t)b * hd.n_out[h] + o) * K + k0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = 4 * g + r;
            if (j >= rows) continue;
            float val = acc[0][r] + bias;
            if (h == hd.center) val = val + query_pos[((size_t)b * K + k0 + j) * 2 + o];
            dst[j] = val;
        }
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------

bool att_shape_ok(long long B, long long Kq, long long N) {
    if (B < 0 || Kq < 1 || Kq > 2048 || N < 1 || N >= (1ll << 31) / kD) return false;
    return B * ((Kq + 63) / 64) <= 65535;          // grid.z: scenes x chunks of at least 64 queries
}

long long att_ws_floats(long long B, long long Kq, long long N) {
    int sl, tl;
    att_geometry(N, &sl, &tl);
    const long long nsplit = (N + sl - 1) / sl;
    if (nsplit == 1) return 0;
    return (B > 0 ? B : 1) * nsplit * kHeads * Kq * 18;
}

template <typename... DROP>
int launch_attention(const float *q, const float *k, const float *v, int B, int Kq, int N, float *ws, float *out, hipStream_t s,
                     float *stats, DROP... drop) {
    int sl, tl;
    att_geometry(N, &sl, &tl);
    // A workgroup takes 4 * QB blocks of 16 queries (wave w the blocks w, w + 4, ...).  Many keys: up to four blocks per wave, so
    // that the K and V a wave has loaded serve four query blocks.  One split (N <= 256, the self-attention): one block per wave,
    // i.e. a workgroup per 64 queries and head -- with four blocks per wave the 8 x B workgroups of the launch each ran 16
    // dependent tile passes, 25 us for 20 MFLOP (profiles/r10_bench_decoder.json).  Both choices depend on N and Kq only, and
    // a query block's arithmetic does not depend on the workgroup it runs in.
    const int nsplit = (N + sl - 1) / sl, nblk = (Kq + 15) / 16;
    const int qb = nsplit == 1 ? 1 : (nblk >= 16 ? 4 : (nblk + 3) / 4);
    const int nchunk = (nblk + 4 * qb - 1) / (4 * qb);
    float *pacc = ws, *pml = ws ? ws + (size_t)B * nsplit * kHeads * Kq * 16 : nullptr;
    const dim3 grid(nsplit, kHeads, B * nchunk);
#define FNP_ATT(QB)                                                                                                              \
    hipLaunchKernelGGL(HIP_KERNEL_NAME(tf_attn_kernel<QB, DROP...>), grid, dim3(kAttThreads), 0, s, q, k, v, Kq, N, sl, nsplit, nchunk, \
                       pacc, pml, out, stats, drop...)
    if (qb == 1) FNP_ATT(1);
    else if (qb == 2) FNP_ATT(2);
    else if (qb == 3) FNP_ATT(3);
    else FNP_ATT(4);
#undef FNP_ATT
    FNP_LAUNCH_CHECK();
    if (nsplit > 1) {
        const long long total = (long long)B * Kq * 32;
        hipLaunchKernelGGL(tf_attn_merge_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const float *)pacc,
                           (const float *)pml, Kq, nsplit, total, out, stats);
        FNP_LAUNCH_CHECK();
    }
    return FNP_OK;
}

int launch_attention(const float *q, const float *k, const float *v, int B, int Kq, int N, float *ws, float *out, hipStream_t s) {
    return launch_attention(q, k, v, B, Kq, N, ws, out, s, nullptr);
}

int launch_kv_proj(const float *x, const float *pe, int pe_batched, const float *wkv, const float *bkv, int B, int N, float *Ko, float *Vo,
                   hipStream_t s) {
    const int tiles = (N + kTile - 1) / kTile;
    const long long total_tiles = (long long)B * tiles;
    if (total_tiles > 0x7fffffffll) return FNP_ERR_ARG;
    hipLaunchKernelGGL(tf_kv_proj_kernel, dim3((unsigned)(total_tiles < 512 ? total_tiles : 512)), dim3(kKvThreads), 0, s, x, pe,
                       pe_batched ? (long long)kD * N : 0ll, wkv, bkv, N, tiles, (int)total_tiles, Ko, Vo);
    FNP_LAUNCH_CHECK();
    return FNP_OK;
}

}  // namespace

extern "C" int fnp_tf_attention_geometry(int64_t n_keys, int *split_len, int *tile_len) {
    if (n_keys < 1 || n_keys >= (1ll << 31) / kD || !split_len || !tile_len) return FNP_ERR_ARG;
    att_geometry(n_keys, split_len, tile_len);
    return FNP_OK;
}

extern "C" int64_t fnp_tf_attention_workspace_bytes(int batch_size, int num_queries, int64_t num_keys) {
    if (!att_shape_ok(batch_size, num_queries, num_keys)) return FNP_ERR_ARG;
    return att_ws_floats(batch_size, num_queries, num_keys) * 4;
}

extern "C" int fnp_tf_attention(const float *q, const float *k, const float *v, int batch_size, int num_queries, int64_t num_keys,
                                void *workspace, int64_t workspace_bytes, float *out, fnp_stream_t stream) {
    if (!att_shape_ok(batch_size, num_queries, num_keys)) return FNP_ERR_ARG;
    if (batch_size == 0) return FNP_OK;
    if (!q || !k || !v || !out || (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out | (uintptr_t)workspace) & 15)) return FNP_ERR_ARG;
    const long long need = att_ws_floats(batch_size, num_queries, num_keys) * 4;
    if (need && (!workspace || workspace_bytes < need)) return FNP_ERR_WORKSPACE;
    return launch_attention(q, k, v, batch_size, num_queries, (int)num_keys, (float *)workspace, out, (hipStream_t)stream);
}

// the same launches with the softmax statistics (M, L) per (scene, head, query) written as well: what fnp_tf_attention_backward reads
extern "C" int fnp_tf_attention_stats(const float *q, const float *k, const float *v, int batch_size, int num_queries, int64_t num_keys,
                                      void *workspace, int64_t workspace_bytes, float *out, float *stats, fnp_stream_t stream) {
    if (!att_shape_ok(batch_size, num_queries, num_keys)) return FNP_ERR_ARG;
    if (batch_size == 0) return FNP_OK;
    if (!q || !k || !v || !out || !stats) return FNP_ERR_ARG;
    if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out | (uintptr_t)stats | (uintptr_t)workspace) & 15) return FNP_ERR_ARG;
    const long long need = att_ws_floats(batch_size, num_queries, num_keys) * 4;
    if (need && (!workspace || workspace_bytes < need)) return FNP_ERR_WORKSPACE;
    return launch_attention(q, k, v, batch_size, num_queries, (int)num_keys, (float *)workspace, out, (hipStream_t)stream, stats);
}

// fnp_tf_attention_stats with the dropout instantiation of the attention kernel: out is the dropped output, stats are the plain ones
extern "C" int fnp_tf_attention_dropout_stats(const float *q, const float *k, const float *v, int batch_size, int num_queries,
                                              int64_t num_keys, void *workspace, int64_t workspace_bytes, float *out, float *stats,
                                              float p, const uint64_t *seed, fnp_stream_t stream) {
    if (!att_shape_ok(batch_size, num_queries, num_keys) || !(p >= 0.f && p < 1.f)) return FNP_ERR_ARG;
    if (batch_size == 0) return FNP_OK;
    if (!q || !k || !v || !out || !stats || !seed || ((uintptr_t)seed & 7)) return FNP_ERR_ARG;
    if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out | (uintptr_t)stats | (uintptr_t)workspace) & 15) return FNP_ERR_ARG;
    const long long need = att_ws_floats(batch_size, num_queries, num_keys) * 4;
    if (need && (!workspace || workspace_bytes < need)) return FNP_ERR_WORKSPACE;
    const uint32_t threshold = fnp_dropout_threshold(p);
    return launch_attention(q, k, v, batch_size, num_queries, (int)num_keys, (float *)workspace, out, (hipStream_t)stream, stats,
                            fnp_dropout_args{(const unsigned long long *)seed, threshold, fnp_dropout_scale(threshold)});
}

extern "C" int64_t fnp_tf_decoder_workspace_bytes(int batch_size, int num_queries, int64_t num_keys, int ffn, int n_head_out) {
    if (!att_shape_ok(batch_size, num_queries, num_keys) || ffn < 16 || ffn > 1024 || (ffn & 15) || n_head_out < 0) return FNP_ERR_ARG;
    const long long B = batch_size > 0 ? batch_size : 1;
    const long long rows = B * num_queries * kD, keys = B * num_keys * kD;
    long long att = att_ws_floats(B, num_queries, num_keys);
    const long long self = att_ws_floats(B, num_queries, num_queries);
    if (self > att) att = self;
    return (8 * rows + 2 * keys + att) * 4;
}

// stages: bit 0 front, 1 self-attention, 2 mid, 3 kv_proj, 4 cross-attention (+ merge), 5 tail
extern "C" int fnp_tf_decoder_stages(const float *query_feat, const float *lidar_feat, const float *query_pos, const float *key_pe,
                                     int key_pe_batched, const float *params, int64_t params_floats, int batch_size, int num_queries,
                                     int64_t num_keys, int ffn, int n_heads, const int *head_out, int center_head, void *workspace,
                                     int64_t workspace_bytes, float *out_query_feat, float *out_heads, int stages, fnp_stream_t stream) {
    TfOff off;
    TfHeads hd;
    if (!att_shape_ok(batch_size, num_queries, num_keys) || batch_size > 65535 || !tf_layout(ffn, n_heads, head_out, center_head, &off, &hd))
        return FNP_ERR_ARG;
    if (params_floats != off.total) return FNP_ERR_ARG;
    if (batch_size == 0) return FNP_OK;
    if (!query_feat || !lidar_feat || !query_pos || !key_pe || !params || !out_query_feat || (n_heads && !out_heads)) return FNP_ERR_ARG;
    if (((uintptr_t)params | (uintptr_t)workspace) & 15) return FNP_ERR_ARG;
    int n_head_out = 0;
    for (int h = 0; h < n_heads; ++h) n_head_out += head_out[h];
    if (!workspace || workspace_bytes < fnp_tf_decoder_workspace_bytes(batch_size, num_queries, num_keys, ffn, n_head_out)) return FNP_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int B = batch_size, K = num_queries, N = (int)num_keys;
    const size_t rows = (size_t)B * K * kD, keys = (size_t)B * N * kD;
    float *w = (float *)workspace;
    float *xrow = w, *qpe = w + rows, *qs = w + 2 * rows, *ks = w + 3 * rows, *vs = w + 4 * rows, *ao = w + 5 * rows, *x1 = w + 6 * rows,
          *qc = w + 7 * rows, *Kc = w + 8 * rows, *Vc = Kc + keys, *att = Vc + keys;
    const dim3 rgrid((K + 15) / 16, B);
    int rc = FNP_OK;
    if (stages & 1) {
        hipLaunchKernelGGL(tf_front_kernel, rgrid, dim3(kRowThreads), 0, s, query_feat, query_pos, params, off, K, xrow, qpe, qs, ks, vs);
        FNP_LAUNCH_CHECK();
    }
    if (stages & 2) rc = launch_attention(qs, ks, vs, B, K, K, att, ao, s);     // (K > 256: several splits, so a merge launch of its own)
    if (rc != FNP_OK) return rc;
    if (stages & 4) {
        hipLaunchKernelGGL(tf_mid_kernel, rgrid, dim3(kRowThreads), 0, s, (const float *)ao, (const float *)xrow, (const float *)qpe, params,
                           off, K, x1, qc);
        FNP_LAUNCH_CHECK();
    }
    if (stages & 8) rc = launch_kv_proj(lidar_feat, key_pe, key_pe_batched, params + off.ca_w + kD * kD, params + off.ca_b + kD, B, N, Kc, Vc, s);
    if (rc != FNP_OK) return rc;
    if (stages & 16) rc = launch_attention(qc, Kc, Vc, B, K, N, att, ao, s);
    if (rc != FNP_OK) return rc;
    if (stages & 32) {
        hipLaunchKernelGGL(tf_tail_kernel, rgrid, dim3(kRowThreads), 0, s, (const float *)ao, (const float *)x1, query_pos, params, off, hd, B,
                           K, ffn, out_query_feat, out_heads);
        FNP_LAUNCH_CHECK();
    }
    return FNP_OK;
}

extern "C" int fnp_tf_decoder(const float *query_feat, const float *lidar_feat, const float *query_pos, const float *key_pe,
                              int key_pe_batched, const float *params, int64_t params_floats, int batch_size, int num_queries, int64_t num_keys, int ffn,
                              int n_heads, const int *head_out, int center_head, void *workspace, int64_t workspace_bytes,
                              float *out_query_feat, float *out_heads, fnp_stream_t stream) {
    return fnp_tf_decoder_stages(query_feat, lidar_feat, query_pos, key_pe, key_pe_batched, params, params_floats, batch_size, num_queries,
                                 num_keys, ffn, n_heads, head_out, center_head, workspace, workspace_bytes, out_query_feat, out_heads, 63,
                                 stream);
}
