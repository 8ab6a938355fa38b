// Class-sorted 128 -> 128 sweep (3x3x3 SubM layers of stage 4, 16-bit features in and out) as a DOUBLE-BUFFERED LDS-DMA ROW PIPELINE.
//
// Why rows go through LDS at all (tools/gather_probe.py): the gathers of spconv_mfma_kernel are fragment shaped
// — a wave instruction = 16 rows x 64 bytes — and the address path is paced by the cache lines an instruction touches, not by its
// bytes: the same rows fetched in whole 128-byte lines run 1.4x faster.  An MFMA B fragment is 16 rows x 64 bytes whatever the
// load shape, so whole lines have to be landed in LDS and the fragments read from there.  The whole-row form of round 6 did that
// with ONE buffer of everything (64 KB of slabs + 96 KB of row strips = the CU's 160 KB) and a __syncthreads() per offset, which
// drains every LDS-DMA in flight: its memory side and its matrix side added up instead of overlapping, and it lost.
//
// This form cuts the sweep into STEPS of (kernel offset, 64-channel half of Cin).  A half row is 128 bytes = one cache line, so a
// global_load_lds_dwordx4 still touches 8 whole lines (8 lanes per line); per wave and step 48 half rows = 6 KB, and a half slab
// (128 Cout x 64 Cin) is 16 KB.  LDS: a ring of three half slabs (48 KB), two row buffers per wave (96 KB), two 256-byte entry slots per
// wave (4 KB): 148 KB, one workgroup per CU as before.  With that, rows AND weights are requested TWO steps ahead:
//
//   step s = 2 k + h (offset k of the tile's live offsets, half h), row buffer h, slab ring slot s mod 3; on entry the step's six B
//   fragments are on their way from row buffer h to registers (issued behind the wait of the step before)
//     1. A fragments of the first matrix group, s_waitcnt lgkmcnt(0): the B fragments are in registers, the row buffer is free again
//     2. 48 MFMAs in four groups (A fragments from ring slot s mod 3, read one group ahead), and BETWEEN them, one piece behind
//        every four or five MFMAs, batch(s): the rows of step s + 2 into the same row buffer (6 pieces), the half slab of step s + 2 into
//        ring slot (s + 2) mod 3 (2 pieces per wave; last read in step s - 1, a barrier ago), and in even steps the rulebook entries
//        of offset k + 2 into entry slot k & 1 (one global_load_lds_dword per wave: lane l fetches the entry of "its" position).
//        Issued as one block ahead of the MFMAs the pieces cost their whole issue time: the barrier keeps the eight waves in step, so
//        all of them sat in the address path together and then in the matrix pipe together (measured: 0.78 ms against 0.71)
//     3. s_waitcnt vmcnt(|batch(s)|): batch(s - 1) — rows, slab and entries of step s + 1 — has landed, batch(s) stays in flight
//     4. the B fragments of step s + 1 are requested (the rows are the wave's own: its vmcnt orders them, no barrier needed)
//     5. s_barrier: every wave's slab pieces of step s + 1 are in; every wave is done reading ring slot s mod 3
//   The count in 3 is exact because a wave issues NOTHING else on the vector-memory queue inside the sweep: rulebook entries come by
//   LDS-DMA too and are read back with ds_read (an ordinary load beside LDS-DMA in flight makes the compiler wait vmcnt(0) at its
//   use).  The wait is vmcnt(0) only in the two steps of a tile's last offset, where no piece is issued: those two steps are peeled off
//   the loop, and ahead of them go the ordinary loads of what the epilogue starts with — the rows behind the wave's positions (perm) and
//   the next tile's block masks and entry row — so that they land under the 48 MFMAs of the first of the two steps (its vmcnt(0)
//   retires them; their first use is the epilogue, another 48 MFMAs on) instead of standing at the epilogue's top (a load there
//   breaks no count: nothing has to stay in flight across these waits).  Slabs are read one phase
//   after the wait that retires them (the barrier of 5 lies between); a buffer is restaged only after an lgkmcnt(0) (rows: the wave's
//   own reads) or a barrier (slabs: every wave's reads).  No __syncthreads() in the sweep: its fence would drain the prefetch.
//   What a tile needs before its first piece (live offsets, perm rows, the entries of its first two offsets: three dependent trips to
//   HBM) is fetched by the tile before: the first two in its last offset, the entries at the top of its epilogue (TileSt below).
//
// LDS images are lane-linear per piece (the DMA writes base + lane * 16), so the XOR swizzle that makes the fragment reads
// conflict-free is applied to the SOURCE address: slot r (128 bytes: row r of a row buffer, output channel r of a half slab) holds
// logical 16-byte chunk c at position c ^ ((r >> 1) & 7); the 16 lanes of a fragment read that share a chunk then hit 16 different
// 16-byte positions of the 256-byte bank row.  Absent neighbours fetch a line of zeros.
//
// Same sums as spconv_mfma_kernel<128, 128, 3, 27, ..., SORTED>: a row adds its neighbours in ascending offset order, inside an offset
// the four 32-wide K steps in order (half 0 = K steps 0-1, half 1 = K steps 2-3), same operands per matrix instruction, same
// epilogue arithmetic: bit-identical.  Tiles, rounds, slot rotation and skipped (tile, offset) pairs are that kernel's (sortedsweep.h).
#include "sortedsweep.h"
#include <type_traits>

// Instrument (development builds only; the shipped library has 0):
//   FNP_R128_ABLATE  timing probes, a bit mask (results are wrong): 1 = no MFMA, 2 = no slab DMA, 4 = no row DMA, 8 = every row
//                    piece fetches the line of zeros (same issue, one line per piece), 16 = no vmcnt wait inside the sweep
#ifndef FNP_R128_ABLATE
#define FNP_R128_ABLATE 0
#endif

namespace {

__device__ uint4 g_rows128_zero[8];   // 128 bytes of zeros: the half row an absent neighbour fetches

template <int I> __device__ __forceinline__ int fnp_row_share(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x150 + I, 0xf, 0xf, false); }
template <int I, int N, typename F> __device__ __forceinline__ void fnp_static_for(F &&f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        fnp_static_for<I + 1, N>(f);
    }
}
typedef __attribute__((address_space(1))) const void *fnp_gptr;
typedef __attribute__((address_space(3))) void *fnp_lptr;

#define FNP_VMCNT(N) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory")
#define FNP_LGKMCNT0() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")

constexpr int kR128NW = kSortedNW, kR128MB = kSortedMB, kR128NT = kR128NW * 64;
constexpr int kR128Slab = 128 * 128, kR128Ring = 3;                 // half slab: 128 output channels x 64 input channels x 2 bytes
constexpr int kR128RowBuf = kR128MB * 16 * 128;                     // one wave's half rows of a step
constexpr int kR128RowsOff = kR128Ring * kR128Slab, kR128EntOff = kR128RowsOff + 2 * kR128NW * kR128RowBuf;
constexpr int kR128Lds = kR128EntOff + kR128NW * 2 * 256;
static_assert(kR128Lds == 148 * 1024 && kR128Lds <= 160 * 1024, "slab ring + two row buffers + entry slots");
static_assert(kR128RowBuf >= 16 * (128 * 2 + 16), "the epilogue's transpose strip aliases the wave's first row buffer");

template <typename TAct>
__global__ __launch_bounds__(kR128NT, 2) void spconv_rows128_kernel(const TAct *__restrict__ x, const TAct *__restrict__ w, const int *__restrict__ nbr,
                                                                    int nbr_stride, const int *__restrict__ n_out, int cap, TAct *__restrict__ y,
                                                                    const float *__restrict__ scale, const float *__restrict__ shift,
                                                                    const TAct *__restrict__ residual, int relu, SortedRb srb) {
    using bf16x8 = typename Vec16<TAct>::v8;   // (named after the default activation type)
    using bf16x4 = typename Vec16<TAct>::v4;
    constexpr int C = 128, NB = 8, NBH = 4, NW = kR128NW, MB = kR128MB, ROWS_PER_WG = NW * MB * 16;
    constexpr int NSLAB = (FNP_R128_ABLATE & 2) ? 0 : 2;   // slab pieces per wave and step
    extern __shared__ __attribute__((aligned(16))) unsigned char fnp_smem[];   // (ALL of the kernel's LDS: one array)
    const int n = min(*n_out, cap);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, q = lane >> 4;   // fragment roles: column (site / output channel) l15, k-chunk q
    const int r8 = lane >> 3, c8 = lane & 7;    // fetch roles: 16-byte chunk c8 of the line this 8-lane group fetches
    unsigned char *const rowbuf = fnp_smem + kR128RowsOff + wave * kR128RowBuf;   // buffer h at + h * NW * kR128RowBuf
    unsigned char *const entbuf = fnp_smem + kR128EntOff + wave * 512;            // slot i at + i * 256

    const int G = gridDim.x, xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const XcdRows xr = fnp_xcd_rows(n, G, xcd);
    const int row_begin = xr.X0, row_end = xr.X1, xslots = xr.S;
    if (row_begin >= row_end) return;

    // fragment byte offsets inside a slot group of 16 (A: output channels nb * 16 + l15 of a half slab, B: positions mb * 16 + l15 of a
    // row buffer): slot l15, logical chunk 4 ksl + q at position chunk ^ ((l15 >> 1) & 7); + nb (mb) * 2048
    unsigned foff[2];
#pragma unroll
    for (int ksl = 0; ksl < 2; ++ksl) foff[ksl] = (unsigned)l15 * 128u + ((unsigned)((ksl * 4 + q) ^ ((l15 >> 1) & 7)) << 4);
    // half slab by LDS-DMA: piece j * 8 + wave (j = 0, 1) = slab rows 8 piece + r8; the swizzle goes on the SOURCE
    unsigned wsrc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int wr = (j * 8 + wave) * 8 + r8;
        wsrc[j] = (unsigned)wr * 256u + ((unsigned)(c8 ^ ((wr >> 1) & 7)) << 4);
    }
    auto dma_slab_piece = [&](int koffset, int half, int ring, int j) {
        const unsigned char *wk = reinterpret_cast<const unsigned char *>(w) + (size_t)koffset * (C * C * 2) + half * 128;
        __builtin_amdgcn_global_load_lds((fnp_gptr)(wk + wsrc[j]), (fnp_lptr)(fnp_smem + ring * kR128Slab + (j * 8 + wave) * 1024), 16, 0, 0);
    };

    // What a tile's sweep needs before its first piece can go out — the live offsets (Kt of them; lane l of kl holds the l-th) and the row
    // behind the position whose rulebook ENTRY this lane fetches — comes from two cold lines (blockmask, perm), and the entries of the first
    // two offsets from a third: three dependent round trips to HBM.  They are made for tile t + 1 by tile t: tile_loads at the
    // top of its last offset, beside its own perm loads; tile_state + the two entry DMAs at the top of its epilogue, beside its residual
    // loads — so that a tile's prologue waits for its first rows only.  `mbt`: 16-position blocks per wave of the tile (MB; fewer in the partial round).
    // Piece ii of a step fetches positions 8 ii + r8; the entry of position 8 ii + r8 is held by lane 2 ii + (r8 & 1) of the 16-lane row
    // r8 >> 1: lane (r4, c16), c16 < 4 mbt, holds position 8 (c16 >> 1) + 2 r4 + (c16 & 1).
    struct TileSt {
        int Kt, kl, erow;
    };
    const int c16 = lane & 15, r4 = lane >> 4;
    auto tile_epos = [&](int tile_base, int mbt) -> int { return tile_base + wave * (mbt * 16) + 8 * (c16 >> 1) + 2 * r4 + (c16 & 1); };
    auto tile_loads = [&](int tile_base, int mbt, unsigned &m, int &erow) {
        const int nbt = min(NW * mbt, (row_end - tile_base + 15) >> 4);
        m = lane < nbt ? srb.blockmask[(tile_base >> 4) + lane] : 0u;
        erow = srb.perm[min(tile_epos(tile_base, mbt), row_end - 1)];
    };
    // (as spconv_mfma_kernel's SORTED form: the union of the tile's block masks, in every wave)
    auto tile_state = [&](unsigned m, int erow) -> TileSt {
        TileSt st;
        st.erow = erow;
        st.kl = 0;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) m |= (unsigned)__shfl_xor((int)m, d);
        m = (unsigned)__builtin_amdgcn_readfirstlane((int)m) & 0x7ffffffu;
        if (m == 0u) m = 1u << 13;   // (cannot happen for a tile with rows: a row is its own neighbour at offset 13)
        st.Kt = __popc(m);
        int cnt = 0;
#pragma unroll
        for (int pbit = 0; pbit < 27; ++pbit) {
            if ((m >> pbit) & 1u) {   // (uniform)
                if (lane >= cnt) st.kl = pbit;
                ++cnt;
            }
        }
        return st;
    };
    // entries of sweep offset i of a tile -> entry slot es: each lane fetches its own word, the DMA puts it at slot + lane * 4
    auto dma_ent_of = [&](const TileSt &st, int i, int es) {
        const int ko = __builtin_amdgcn_readlane(st.kl, i < st.Kt ? i : st.Kt - 1);
        __builtin_amdgcn_global_load_lds((fnp_gptr)(nbr + (size_t)ko * nbr_stride + st.erow), (fnp_lptr)(entbuf + es * 256), 4, 0, 0);
    };

    // one tile; its entries of offsets 0 and 1 are in flight (or in); returns the state of the next tile (next_mbt blocks per wave, 0 = none)
    auto run_tile = [&](auto mbt_tag, const int tile_base, const TileSt st, const int next_base, const int next_mbt) __attribute__((always_inline)) -> TileSt {
        constexpr int MBT = decltype(mbt_tag)::value, NI = MBT * 2;   // NI pieces of 8 half rows fetch the wave's MBT * 16 rows of a step
        constexpr int NROW = (FNP_R128_ABLATE & 4) ? 0 : NI;
        const int row0 = tile_base + wave * (MBT * 16);
        const int Kt = st.Kt, kl = st.kl;
        auto koff = [&](int i) -> int { return __builtin_amdgcn_readlane(kl, i < Kt ? i : Kt - 1); };
        const bool ehas = c16 < 2 * NI && tile_epos(tile_base, MBT) < row_end;
        auto dma_ent = [&](int i, int es) { dma_ent_of(st, i, es); };
        auto read_ent = [&](int es) -> int { return *reinterpret_cast<const int *>(entbuf + es * 256 + lane * 4); };
        // row piece ii of a step (entries e, already masked): 8 half rows -> slots 8 ii .. 8 ii + 7 of row buffer `half`
        auto dma_row_piece = [&](int ev, auto half_tag, auto ic) {
            constexpr int half = decltype(half_tag)::value, ii = decltype(ic)::value;
            const int e0 = fnp_row_share<2 * ii>(ev), e1 = fnp_row_share<2 * ii + 1>(ev);
            const int er = (FNP_R128_ABLATE & 8) ? -1 : (lane & 8) ? e1 : e0;
            const int sw = ((ii & 1) << 2) | (r8 >> 1);   // ((8 ii + r8) >> 1) & 7
            const unsigned char *src = er >= 0 ? reinterpret_cast<const unsigned char *>(x) + (size_t)er * 256 + (half * 128 + ((c8 ^ sw) << 4))
                                               : reinterpret_cast<const unsigned char *>(g_rows128_zero) + (c8 << 4);
            __builtin_amdgcn_global_load_lds((fnp_gptr)src, (fnp_lptr)(rowbuf + half * (NW * kR128RowBuf) + ii * 1024), 16, 0, 0);
        };
        // piece p of batch(s): p < NROW a row piece, then the NSLAB slab pieces, then (even steps) the entries
        auto dma_piece = [&](auto pc, auto half_tag, const int k, const int ev, const int ring_s2) {
            constexpr int p = decltype(pc)::value, half = decltype(half_tag)::value;
            if constexpr (p < NROW) dma_row_piece(ev, half_tag, pc);
            else if constexpr (p < NROW + NSLAB) dma_slab_piece(koff(k + 1), half, ring_s2, p - NROW);
            else if constexpr (p == NROW + NSLAB && half == 0) dma_ent(k + 2, k & 1);
        };
        // B fragments of a step: the wave's own half rows, row buffer `half` -> registers
        bf16x8 xb[2][MBT];
        auto read_xb = [&](int half, int k) {
            const unsigned char *rb = rowbuf + half * (NW * kR128RowBuf);
#pragma unroll
            for (int ksl = 0; ksl < 2; ++ksl)
#pragma unroll
                for (int mb = 0; mb < MBT; ++mb) {
                    u32x4 t = u32x4{(unsigned)k, 0u, 0u, 0u};
                    if (!(FNP_R128_ABLATE & 4)) t = *reinterpret_cast<const u32x4 *>(rb + mb * 2048 + foff[ksl]);
                    xb[ksl][mb] = *reinterpret_cast<const bf16x8 *>(&t);
                }
        };

        f32x4 acc[NB][MBT];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int mb = 0; mb < MBT; ++mb) acc[nb][mb] = (f32x4){0.f, 0.f, 0.f, 0.f};

        // one step: see the head of the file.  `more`: the tile has another offset behind this one (a constant: the sweep's last offset is
        // peeled off the loop).  On entry the step's B
        // fragments are on their way to xb (read behind the wait of the step before: the rows are the wave's own).
        auto step = [&](auto half_tag, auto more_tag, const int k, const int e_next, const int ring_s, const int ring_s2) __attribute__((always_inline)) {
            constexpr int half = decltype(half_tag)::value;
            constexpr bool more = decltype(more_tag)::value;
            constexpr int NG = 4, SLOTS = NG * MBT, NP = NROW + NSLAB + 1;   // a slot = 4 MFMAs; the NP pieces are spread evenly over the slots
            const unsigned char *wk = fnp_smem + ring_s * kR128Slab;
            const int ev = ehas ? e_next : -1;
            bf16x8 wa[2][NBH];   // A fragments of matrix group g (K step ksl = g >> 1, output channels 64 (g & 1) ..): two sets, read a group ahead
            auto read_wa = [&](auto gc) {
                constexpr int g = decltype(gc)::value;
#pragma unroll
                for (int j = 0; j < NBH; ++j) {
                    u32x4 t = u32x4{(unsigned)k, 1u, 0u, 0u};
                    if (!(FNP_R128_ABLATE & 2)) t = *reinterpret_cast<const u32x4 *>(wk + ((g & 1) * NBH + j) * 2048 + foff[g >> 1]);
                    wa[g & 1][j] = *reinterpret_cast<const bf16x8 *>(&t);
                }
            };
            read_wa(std::integral_constant<int, 0>{});
            FNP_LGKMCNT0();   // xb (and, in even steps, e_next) are in registers: the row buffer may be refilled
            __builtin_amdgcn_sched_barrier(0);
            // batch(s) goes out piece by piece BETWEEN the matrix instructions (a piece = a dozen address VALU + one VMEM issue in the
            // shadow of four MFMAs): issued in one block, all eight waves would sit in the address path together and then in the
            // matrix pipe together (the barrier keeps them in step), and the two sides add up
            fnp_static_for<0, NG>([&](auto gc) {
                constexpr int g = decltype(gc)::value;
                if constexpr (g + 1 < NG) read_wa(std::integral_constant<int, g + 1>{});
                fnp_static_for<0, MBT>([&](auto mc) {
                    constexpr int mb = decltype(mc)::value, sl = g * MBT + mb;
#pragma unroll
                    for (int j = 0; j < NBH; ++j) {
                        if (FNP_R128_ABLATE & 1) asm volatile("" ::"v"(wa[g & 1][j]), "v"(xb[g >> 1][mb]));
                        else acc[(g & 1) * NBH + j][mb] = mfma16(wa[g & 1][j], xb[g >> 1][mb], acc[(g & 1) * NBH + j][mb]);
                    }
                    if (more) {   // (uniform)
                        fnp_static_for<sl * NP / SLOTS, (sl + 1) * NP / SLOTS>([&](auto pc) { dma_piece(pc, half_tag, k, ev, ring_s2); });
                    }
                    __builtin_amdgcn_sched_barrier(0);
                });
            });
            if (FNP_R128_ABLATE & 16) {
            } else if (more) FNP_VMCNT(NROW + NSLAB + (half == 0 ? 1 : 0));   // batch(s - 1) has landed, batch(s) stays in flight
            else FNP_VMCNT(0);                                                // (last offset of the tile: nothing younger was issued)
            if (half == 0 || more) read_xb(half ^ 1, k);               // the next step's rows are the wave's own: no barrier needed
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();   // (slab reads of this step: consumed by its MFMAs, long retired)
            __builtin_amdgcn_sched_barrier(0);
        };

        // prologue: the entries of offsets 0 and 1 were requested by the tile before; batch(-2) = step 0 and batch(-1) = step 1 (both
        // halves of offset 0)
        FNP_LGKMCNT0();   // the epilogue of the previous tile is done with the row buffer
        FNP_VMCNT(0);
        __builtin_amdgcn_sched_barrier(0);
        {
            const int e0 = read_ent(0);
            FNP_LGKMCNT0();
            __builtin_amdgcn_sched_barrier(0);
            const int ev0 = ehas ? e0 : -1;
            fnp_static_for<0, NROW>([&](auto ic) { dma_row_piece(ev0, std::integral_constant<int, 0>{}, ic); });
            fnp_static_for<0, NSLAB>([&](auto jc) { dma_slab_piece(koff(0), 0, 0, decltype(jc)::value); });
            fnp_static_for<0, NROW>([&](auto ic) { dma_row_piece(ev0, std::integral_constant<int, 1>{}, ic); });
            fnp_static_for<0, NSLAB>([&](auto jc) { dma_slab_piece(koff(0), 1, 1, decltype(jc)::value); });
        }
        __builtin_amdgcn_sched_barrier(0);
        FNP_VMCNT(NROW + NSLAB);   // step 0's rows and slab pieces are in, step 1's in flight
        read_xb(0, 0);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        // What the epilogue needs from two cold lines — the rows behind the positions this lane stores (orow) and the next tile's block
        // masks and entry row (tile_loads) — is requested at the top of the tile's LAST offset: its two steps issue no piece and wait
        // vmcnt(0) anyway, so an ordinary load there breaks no count, and the epilogue starts with its addresses in registers.
        // (one register across the sweep's last steps, not twelve: lane l fetches the row behind position row0 + l, and the epilogue
        //  hands the rows to the lanes that store them with a lane exchange)
        int prow = 0;
        unsigned nm = 0u;
        int nerow = 0;
        int ring = 0;   // ring slot of step 2 k
        for (int k = 0; k + 1 < Kt; ++k) {
            const int r1 = ring == 2 ? 0 : ring + 1, r2 = r1 == 2 ? 0 : r1 + 1;
            const int e_next = read_ent((k + 1) & 1);   // entries of offset k + 1 (landed a step ago)
            step(std::integral_constant<int, 0>{}, std::true_type{}, k, e_next, ring, r2);
            step(std::integral_constant<int, 1>{}, std::true_type{}, k, e_next, r1, ring);
            ring = r2;
        }
        {   // the last offset (Kt >= 1)
            const int r1 = ring == 2 ? 0 : ring + 1, r2 = r1 == 2 ? 0 : r1 + 1;
            if (next_mbt) tile_loads(next_base, next_mbt, nm, nerow);   // (uniform)
            prow = srb.perm[min(row0 + lane, row_end - 1)];
            step(std::integral_constant<int, 0>{}, std::false_type{}, Kt - 1, 0, ring, r2);
            step(std::integral_constant<int, 1>{}, std::false_type{}, Kt - 1, 0, r1, ring);
        }

        // epilogue (spconv_mfma_kernel's wide form: a 16-site block transposed through a wave-private strip, 16 bytes per lane over whole
        // rows); the strip is the wave's first row buffer: every DMA into it has landed and its fragments are in registers
        constexpr int EH = 16, LPR = C / 8, SPI = 64 / LPR, NRD = EH / SPI, ES = C * 2 + 16;
        unsigned char *const eb = rowbuf;
        const int wsite = lane / LPR, wchunk = lane % LPR;
        u32x4 rs_all[MBT][NRD];
        int orow[MBT][NRD];
#pragma unroll
        for (int mb = 0; mb < MBT; ++mb)
#pragma unroll
            for (int i = 0; i < NRD; ++i) orow[mb][i] = __shfl(prow, mb * 16 + i * SPI + wsite);   // (positions past the range: the last row's)
        TileSt nst{1, 13, 0};
        if (next_mbt) {   // the next tile's first entries fly while this one's outputs are made (the entry slots are free: the sweep is over)
            nst = tile_state(nm, nerow);
            dma_ent_of(nst, 0, 0);
            dma_ent_of(nst, 1, 1);
        }
        if (residual) {
#pragma unroll
            for (int mb = 0; mb < MBT; ++mb)
#pragma unroll
                for (int i = 0; i < NRD; ++i)   // (positions past the range read the last row's: never stored; no branch, no wait per load)
                    rs_all[mb][i] = *reinterpret_cast<const u32x4 *>(residual + (size_t)orow[mb][i] * C + wchunk * 8);
        }
#pragma unroll
        for (int mb = 0; mb < MBT; ++mb) {
            const int rb = row0 + mb * 16;
            if (residual) {
#pragma unroll
                for (int i = 0; i < NRD; ++i) *reinterpret_cast<u32x4 *>(eb + (i * SPI + wsite) * ES + wchunk * 16) = rs_all[mb][i];
            }
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const int c0 = nb * 16 + q * 4;
                float v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = acc[nb][mb][j];
                if (scale) {
                    const float4 s4 = *reinterpret_cast<const float4 *>(scale + c0);
                    const float4 h4 = *reinterpret_cast<const float4 *>(shift + c0);
                    v[0] = v[0] * s4.x + h4.x; v[1] = v[1] * s4.y + h4.y; v[2] = v[2] * s4.z + h4.z; v[3] = v[3] * s4.w + h4.w;
                }
                bf16x4 *slotp = reinterpret_cast<bf16x4 *>(eb + l15 * ES + c0 * 2);
                if (residual) {
                    const bf16x4 t = *slotp;
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = v[j] + (float)t[j];
                }
                if (relu) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = v[j] < 0.f ? 0.f : v[j];
                }
                *slotp = bf16x4{(TAct)v[0], (TAct)v[1], (TAct)v[2], (TAct)v[3]};
            }
#pragma unroll
            for (int i = 0; i < NRD; ++i) {
                const int r = rb + i * SPI + wsite;
                const u32x4 t = *reinterpret_cast<const u32x4 *>(eb + (i * SPI + wsite) * ES + wchunk * 16);
                if (r < row_end) *reinterpret_cast<u32x4 *>(y + (size_t)orow[mb][i] * C + wchunk * 8) = t;
            }
        }
        return nst;
    };

    // tiles of this slot: its tile of every full round of the XCD group (rotated, see spconv_mfma_kernel), then its share of the partial round
    const int round_rows = xslots * ROWS_PER_WG;
    const int full = (row_end - row_begin) / round_rows;
    const int left0 = row_begin + full * round_rows;
    int tper = fnp_tail_blocks(row_end - left0, xslots, NW);
    const int tail_base = left0 + slot * (NW * tper * 16);
    if (tail_base >= row_end) tper = 0;
    const int rot = (xslots * 3 + 4) >> 3;
    auto full_base = [&](int t) -> int { return row_begin + t * round_rows + ((slot + t * rot) % xslots) * ROWS_PER_WG; };
    if (full == 0 && tper == 0) return;
    TileSt st;
    {
        unsigned m0;
        int erow0;
        tile_loads(full ? full_base(0) : tail_base, full ? MB : tper, m0, erow0);
        st = tile_state(m0, erow0);
        dma_ent_of(st, 0, 0);
        dma_ent_of(st, 1, 1);
    }
    for (int t = 0; t < full; ++t) {
        const bool last = t + 1 == full;
        st = run_tile(std::integral_constant<int, MB>{}, full_base(t), st, last ? tail_base : full_base(t + 1), last ? tper : MB);
    }
    if (tper == 3) run_tile(std::integral_constant<int, 3>{}, tail_base, st, 0, 0);
    if (tper == 2) run_tile(std::integral_constant<int, 2>{}, tail_base, st, 0, 0);
    if (tper == 1) run_tile(std::integral_constant<int, 1>{}, tail_base, st, 0, 0);
}

template <typename TAct>
int launch_rows128(const ConvArgs &a, const SortedRb &srb, int grid) {
    auto kern = spconv_rows128_kernel<TAct>;
    static bool raised = false;
    if (const int rc = fnp_raise_lds(reinterpret_cast<const void *>(kern), kR128Lds, raised)) return rc;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kR128NT), kR128Lds, a.stream, (const TAct *)a.x, (const TAct *)a.w, a.nbr, a.nbr_stride, a.n_out, a.cap,
                       (TAct *)a.y, a.scale, a.shift, (const TAct *)a.residual, a.relu, srb);
    FNP_LAUNCH_CHECK();
    return FNP_OK;
}

}  // namespace

int fnp_launch_rows128(int dtype, const ConvArgs &a, const int *perm, const unsigned *blockmask, int grid) {
    const SortedRb srb{perm, blockmask};
    return fnp_dispatch16(dtype, [&](auto t) { return launch_rows128<typename decltype(t)::type>(a, srb, grid); });
}
