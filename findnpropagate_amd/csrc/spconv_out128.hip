// conv_out of the backbone — 128 -> 128 channels, kernel (3,1,1), stride (2,1,1), 16-bit in, 16-bit or f32 out, no residual — with
// the three weight slabs RESIDENT in LDS and no workgroup barrier in the row loop.
//
// spconv_mfma_kernel<128, 128, ..., KVOL = 0> (spconv.hip) runs this layer as a 27-offset sweep that happens to have three offsets:
// per 384-row tile it restages every 32 KB slab through LDS behind a workgroup barrier, and index -> gather -> first MFMA at the top
// of a tile and the epilogue at its end are paid with all eight waves in the same phase.  That fixed cost is sized for 27 offsets of
// work; here it buys three.  Three slabs are 96 KB:
//   * one workgroup per CU (persistent grid of 256) stages them once, in the swizzle of spconv.hip; ONE barrier follows;
//   * after it the waves are independent.  Wave v of workgroup range g owns the contiguous rows of wave range 8 g + v of 8 G (cut at
//     16-row blocks, fnp_range_rows; g runs XCD-contiguous, fnp_xcd_map) and walks them in tiles of two 16-row blocks;
//   * the rows of tile t + 1 are requested offset by offset into the registers that tile t's matrix steps free, both 64-byte halves of
//     a 128-byte line back to back, so a whole tile (24 KB per wave) is in flight under the matrix work and the epilogue of tile t;
//     the table entries run one more tile ahead.  Nothing synchronises the waves, so they drift apart and cover each other's waits;
//   * the epilogue transposes through a wave-private LDS strip and stores whole rows (16 bytes per lane).
// Same matrix instructions on the same operands in the same order as the generic kernel — offsets 0, 1, 2, the four 32-wide K steps
// inside each, absent neighbours as zero fragments — and the same epilogue arithmetic: the outputs are the same bits.
// Library-internal; reached from dispatch_16 (spconv.hip), which states when.
#include "sortedsweep.h"   // Vec16, mfma16, fnp_range_rows
#include <type_traits>

namespace {

constexpr int kO128C = 128;                      // channels in and out
constexpr int kO128K = 3;                        // kernel offsets
constexpr int kO128NW = 8, kO128NT = kO128NW * 64;
constexpr int kO128MB = 2;                       // 16-row blocks of a wave tile
constexpr int kO128CH = kO128C / 8;              // 16-byte chunks of a weight row
constexpr int kO128Slab = kO128C * kO128CH;      // chunks of a slab
constexpr int kO128SlabBytes = kO128K * kO128Slab * 16;
// transposing strip of a wave: 16 rows of 16-bit outputs or 8 rows of f32 outputs, 16 bytes of padding per row
constexpr int kO128StripBytes = 16 * (kO128C * 2 + 16);
static_assert(8 * (kO128C * 4 + 16) <= kO128StripBytes, "f32 pass of eight rows fits the strip");
constexpr int kO128Lds = kO128SlabBytes + kO128NW * kO128StripBytes + 2 * kO128C * 4;   // (+ BatchNorm scale / shift)
static_assert(kO128Lds <= 160 * 1024, "LDS of a CU");

template <typename TAct, typename TOut>
__global__ __launch_bounds__(kO128NT, 2) void spconv_out128_kernel(const TAct *__restrict__ x, int x_bytes, const TAct *__restrict__ w,
                                                                   const int *__restrict__ nbr, int nbr_stride, const int *__restrict__ n_out, int cap,
                                                                   TOut *__restrict__ y, const float *__restrict__ scale, const float *__restrict__ shift,
                                                                   int relu) {
    using bf16x8 = typename Vec16<TAct>::v8;   // (named after the default activation type)
    using bf16x4 = typename Vec16<TAct>::v4;
    static_assert(sizeof(TOut) == 4 || std::is_same<TOut, TAct>::value, "16-bit outputs have the activation type");
    constexpr int C = kO128C, K = kO128K, CH = kO128CH, SLAB = kO128Slab, MB = kO128MB;
    constexpr int KS = C / 32;   // 32-wide K steps of the MFMA
    constexpr int NB = C / 16;   // 16-channel output blocks
    constexpr int NBH = 4;       // A fragments held at once

    extern __shared__ __attribute__((aligned(16))) unsigned char o128_smem[];
    uint4 *const wl = reinterpret_cast<uint4 *>(o128_smem);
    float *const ss_lds = reinterpret_cast<float *>(o128_smem + kO128SlabBytes + kO128NW * kO128StripBytes);

    const int n = min(*n_out, cap);
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, q = lane >> 4;

    // slab image of spconv.hip: weight row `row` (an output channel) stores logical chunk c at physical chunk c ^ (row & 15)
#define FNP_O128_POS(row, chunk) ((row) * CH + ((chunk) ^ ((row) & (CH - 1))))
    for (int p = tid; p < K * SLAB; p += kO128NT) {
        const int kk = p / SLAB, r = p % SLAB;
        wl[kk * SLAB + FNP_O128_POS(r / CH, r % CH)] = reinterpret_cast<const uint4 *>(w)[p];
    }
    for (int c = tid; c < 2 * C; c += kO128NT) ss_lds[c] = scale ? (c < C ? scale[c] : shift[c - C]) : (c < C ? 1.f : 0.f);
    __syncthreads();   // the only barrier: every wave of the workgroup reaches it, whatever rows it owns

    // rows of this wave (see the head of the file); placement only affects speed, never results
    int row_begin, row_end;
    fnp_range_rows(n, (int)fnp_xcd_block() * kO128NW + wave, (int)gridDim.x * kO128NW, row_begin, row_end);
    if (row_begin >= row_end) return;

    int aoff[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) aoff[ks] = FNP_O128_POS(l15, ks * 4 + q);
#undef FNP_O128_POS

    const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc((void *)x, 0, x_bytes, 0x00020000);
    // byte offset of (row id, this lane's 16-byte chunk of MFMA step 0); absent rows get an offset that stays out of range after the
    // + ks * 64 of the later steps and read zeros
    auto row_off = [&](int id, int r) -> unsigned {
        return (id < 0 || r >= row_end) ? 0x80000000u : (unsigned)id * (unsigned)(C * 2) + (unsigned)q * 16u;
    };
    auto gather = [&](unsigned roff, int ks) -> bf16x8 {
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(xrsrc, roff + (unsigned)ks * 64u, 0, 0);
        return *reinterpret_cast<const bf16x8 *>(&v);
    };
    // table entry of row r for offset k, untouched (validity is decided where it is consumed, a tile later); rows past the range read a
    // valid address
    auto ent_raw = [&](int k, int r) -> int { return nbr[(size_t)k * nbr_stride + (r < row_end ? r : row_end - 1)]; };

    unsigned char *const eb = o128_smem + kO128SlabBytes + wave * kO128StripBytes;
    constexpr int ES = C * (int)sizeof(TOut) + 16;        // bytes of a strip row
    constexpr int EH = sizeof(TOut) == 2 ? 16 : 8;        // rows of a strip pass
    constexpr int LPR = C * (int)sizeof(TOut) / 16;       // 16-byte chunks (lanes) of an output row
    constexpr int SPI = 64 / LPR;                         // rows of a wave-wide 16-byte access
    constexpr int NRD = EH / SPI;                         // accesses of a pass
    const int wsite = lane / LPR, wchunk = lane % LPR;

    // prologue: rows of the first tile, entries of the second
    bf16x8 xb[K][KS][MB];
    int eq[K][MB];   // raw entries of the NEXT tile
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) eq[k][mb] = ent_raw(k, row_begin + MB * 16 + mb * 16 + l15);
    // (requested in the order the loop requests and consumes them: the loop's first wait then leaves the younger ones in flight)
    unsigned ro0[K][MB];
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) {
            const int r = row_begin + mb * 16 + l15;
            ro0[k][mb] = row_off(ent_raw(k, r), r);
        }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int ks = 1; ks < KS; ks += 2) {
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) {
                xb[k][ks - 1][mb] = gather(ro0[k][mb], ks - 1);
                xb[k][ks][mb] = gather(ro0[k][mb], ks);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }

    for (int row0 = row_begin; row0 < row_end; row0 += MB * 16) {
        // entries of the tile after the next: requested first, so that they are older than the gathers issued below
        int en[K][MB];
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) en[k][mb] = ent_raw(k, row0 + 2 * MB * 16 + mb * 16 + l15);
        f32x4 acc[NB][MB];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) acc[nb][mb] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const uint4 *wk = wl + k * SLAB;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
                for (int h = 0; h < NB; h += NBH) {
                    bf16x8 wa[NBH];
#pragma unroll
                    for (int j = 0; j < NBH; ++j) {
                        const uint4 t = wk[aoff[ks] + (h + j) * 16 * CH];
                        wa[j] = *reinterpret_cast<const bf16x8 *>(&t);
                    }
#pragma unroll
                    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                        for (int j = 0; j < NBH; ++j) acc[h + j][mb] = mfma16(wa[j], xb[k][ks][mb], acc[h + j][mb]);
                }
                // the registers of two steps are free: the next tile's rows of this offset, both halves of a 128-byte line together
                if (ks & 1) {
#pragma unroll
                    for (int mb = 0; mb < MB; ++mb) {
                        const int r = row0 + MB * 16 + mb * 16 + l15;
                        const unsigned ro = row_off(eq[k][mb], r);
                        xb[k][ks - 1][mb] = gather(ro, ks - 1);
                        xb[k][ks][mb] = gather(ro, ks);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);   // keep the steps in program order
            }
        }
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) eq[k][mb] = en[k][mb];

        // epilogue: lane holds out[row0 + mb*16 + l15][c0 .. c0+3], c0 = nb*16 + q*4; EH rows at a time go through the wave's strip
        // (written by the lanes that hold them, read back as whole rows: LDS accesses of one wave complete in order)
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) {
            if (row0 + mb * 16 >= row_end) break;   // (wave-uniform: the last tile of a range may hold one block)
#pragma unroll
            for (int h = 0; h < 16 / EH; ++h) {
                const int rb = row0 + mb * 16 + h * EH;
                const bool mine = EH == 16 || (l15 / EH) == h;   // this lane's row is in the pass
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) {
                    const int c0 = nb * 16 + q * 4;
                    float v[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = acc[nb][mb][j];
                    if (scale) {
                        const float4 s4 = *reinterpret_cast<const float4 *>(ss_lds + c0);
                        const float4 h4 = *reinterpret_cast<const float4 *>(ss_lds + C + c0);
                        v[0] = v[0] * s4.x + h4.x; v[1] = v[1] * s4.y + h4.y; v[2] = v[2] * s4.z + h4.z; v[3] = v[3] * s4.w + h4.w;
                    }
                    if (relu) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) v[j] = v[j] < 0.f ? 0.f : v[j];
                    }
                    if (mine) {
                        unsigned char *slot = eb + (l15 % EH) * ES + c0 * (int)sizeof(TOut);
                        if constexpr (sizeof(TOut) == 2) *reinterpret_cast<bf16x4 *>(slot) = bf16x4{(TAct)v[0], (TAct)v[1], (TAct)v[2], (TAct)v[3]};
                        else *reinterpret_cast<f32x4 *>(slot) = (f32x4){v[0], v[1], v[2], v[3]};
                    }
                }
#pragma unroll
                for (int i = 0; i < NRD; ++i) {
                    const int r = rb + i * SPI + wsite;
                    const u32x4 t = *reinterpret_cast<const u32x4 *>(eb + (i * SPI + wsite) * ES + wchunk * 16);
                    if (r < row_end) *reinterpret_cast<u32x4 *>(reinterpret_cast<unsigned char *>(y) + (size_t)r * (C * sizeof(TOut)) + wchunk * 16) = t;
                }
            }
        }
    }
}

template <typename TAct, typename TOut>
int launch_out128(const ConvArgs &a) {
    auto kern = spconv_out128_kernel<TAct, TOut>;
    static bool raised = false;
    if (const int rc = fnp_raise_lds(reinterpret_cast<const void *>(kern), kO128Lds, raised)) return rc;
    // persistent grid, one workgroup per CU (its LDS admits no second one); the kernel cuts the rows evenly over the grid's waves
    hipLaunchKernelGGL(kern, dim3(256), dim3(kO128NT), kO128Lds, a.stream, (const TAct *)a.x, (int)a.x_bytes, (const TAct *)a.w, a.nbr, a.nbr_stride, a.n_out,
                       a.cap, (TOut *)a.y, a.scale, a.shift, a.relu);
    FNP_LAUNCH_CHECK();
    return FNP_OK;
}

}  // namespace

int fnp_launch_out128(int in_dtype, int out_f32, const ConvArgs &a) {
    return fnp_dispatch16(in_dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        return out_f32 ? launch_out128<T, float>(a) : launch_out128<T, T>(a);
    });
}
