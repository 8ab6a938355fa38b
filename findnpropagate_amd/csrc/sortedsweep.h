// What the class-sorted 128 -> 128 sweeps share: the activation vector types and matrix instruction, the processing order
// (SortedRb) and the work split every kernel that runs on that order must cut identically (the class sort made perm and
// blockmask for it): spconv_mfma_kernel<..., SORTED> in spconv.hip, its f32-out form, and the LDS-DMA row pipeline of
// spconv_rows128.hip.
#pragma once
#include "conv_launch.h"   // ConvArgs

namespace {

// 16-bit activation types of the MFMA path: bf16 (default) and fp16 (the reference's AMP mode, train_utils.py:172:
// autocast makes spconv run fp16 features with fp32 accumulation).  Same kernel, same fragment layouts
// (v_mfma_f32_16x16x32_bf16 / _f16 take the same cycles); only the matrix instruction and the conversions differ.
template <typename T> struct Vec16 {
    typedef T v8 __attribute__((ext_vector_type(8)));
    typedef T v4 __attribute__((ext_vector_type(4)));
};
typedef float f32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f32x4_t mfma16(Vec16<__bf16>::v8 a, Vec16<__bf16>::v8 b, f32x4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4_t mfma16(Vec16<_Float16>::v8 a, Vec16<_Float16>::v8 b, f32x4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// SORTED (the 128 -> 128 SubM layers of stage 4): the rows a workgroup owns are processed in an order sorted by
// neighbourhood class (fnp_rulebook_classsort: no neighbour below / above / both / neither in z), so that most tiles hold
// rows of one class and the tile sweeps only the kernel offsets at least one of its rows has a neighbour at — the
// offset's slab load, barrier, gathers and matrix work all go (20 % of the (tile, offset) pairs on lidar scenes;
// unsorted, every tile needs every offset).  `perm` maps a processing position to its row (rulebook entries, residual
// and output rows are addressed through it), `blockmask` holds the union of the 27-bit neighbour masks of each 16
// positions.  Every row still sums its own neighbours in ascending offset order: same values as the unsorted sweep.
struct SortedRb {
    const int *perm;
    const unsigned *blockmask;
};

// rows [row_begin, row_end) of workgroup range `range` of `G` when n rows are cut at 16-row blocks: the split of
// spconv_mfma_kernel, shared with the class-sort pass (which must sort exactly the rows a workgroup will own)
__device__ __forceinline__ void fnp_range_rows(int n, int range, int G, int &row_begin, int &row_end) {
    const long long nblk16 = (n + 15) >> 4;
    row_begin = (int)((nblk16 * range) / G) << 4;
    row_end = min(n, (int)((nblk16 * (range + 1)) / G) << 4);
}

// neighbourhood class of a row's 27-bit mask, in sort order: no neighbour in either adjacent z plane, above only (offsets 18..26), both,
// below only (offsets 0..8)
__device__ __forceinline__ int fnp_zclass(unsigned m) {
    const bool lo = (m & 0x1ffu) != 0u, hi = (m & (0x1ffu << 18)) != 0u;
    return lo ? (hi ? 2 : 3) : (hi ? 1 : 0);
}

// SORTED work split.  Blocks b and b + 8 share an XCD (and its L2); the slots of one such group own ONE contiguous run of rows
// [X0, X1) together and take its tiles round-robin: round j = positions [X0 + j S T, X0 + (j + 1) S T), slot s its s-th
// tile of T rows.  At any time the S workgroups of a group sweep S consecutive tiles — one contiguous region of the
// feature map, about the XCD's L2 in size — and the class sort orders the rows of each ROUND: of its S tiles all but the
// two or three at the class boundaries hold rows of one class.  (Sorting the rows of a private per-workgroup range
// instead made every tile gather from the whole range: L2 misses + 31 %, and most of the skipped offsets' time went back
// into gather latency.)  The last, partial round is cut into S tiles of fewer blocks per wave, so that the matrix work of
// the tail stays proportional to its rows.  Placement only affects speed, never results.
struct XcdRows {
    int X0, X1, S;   // rows of the group, number of slots
};
__device__ __forceinline__ XcdRows fnp_xcd_rows(int n, int G, int xcd) {
    const int per = G >> 3, rem = G & 7;
    XcdRows x;
    x.S = per + (xcd < rem ? 1 : 0);
    x.X0 = x.X1 = 0;
    if (x.S > 0) {
        const int first = xcd < rem ? xcd * (per + 1) : rem * (per + 1) + (xcd - rem) * per;
        int t;
        fnp_range_rows(n, first, G, x.X0, t);
        fnp_range_rows(n, first + x.S - 1, G, t, x.X1);
    }
    return x;
}
// blocks per wave (0 = no tile) of the partial last round of `rows_left` rows cut into S tiles of NW waves
__device__ __forceinline__ int fnp_tail_blocks(int rows_left, int S, int NW) {
    const int nb = (rows_left + 15) >> 4;
    return ((nb + S - 1) / S + NW - 1) / NW;
}

// tile of the class-sorted 16-bit sweep: 8 waves x 3 blocks x 16 positions (MfmaWg<128, 128>::NW and ::MB of spconv.hip)
constexpr int kSortedNW = 8, kSortedMB = 3;

}  // namespace

// spconv_rows128.hip: the class-sorted 128 -> 128 sweep, 16-bit in and out, as a double-buffered LDS-DMA row pipeline.  `grid` is the
// workgroup count perm / blockmask were made for.  Library-internal (not part of the C ABI).
__attribute__((visibility("hidden"))) int fnp_launch_rows128(int dtype, const ConvArgs &a, const int *perm, const unsigned *blockmask, int grid);

// spconv_out128.hip: a 128 -> 128 convolution of three kernel offsets (conv_out), 16-bit in, 16-bit (out_f32 == 0: the input's type) or f32
// out, no residual, with the three weight slabs resident in LDS.  Library-internal (not part of the C ABI).
__attribute__((visibility("hidden"))) int fnp_launch_out128(int in_dtype, int out_f32, const ConvArgs &a);
