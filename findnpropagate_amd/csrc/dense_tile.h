// The plane tiling shared by the dense writer / its adjoint (csrc/dense.hip) and the BatchNorm2d-on-rows operator
// (csrc/bev_bn.hip): the cell -> row map, which rows a tile's lanes own, and the two LDS stagings (rows -> slots for a write,
// channel planes -> slots for a gather).  One tile = 64 * VEC consecutive cells of a (b, z) plane; lane l owns cells
// VEC * l .. VEC * l + VEC - 1; the four waves of a workgroup own the same cells and split the channels.
#pragma once
#include "common.h"

constexpr int kDenseThreads = 256;
// LDS: kDenseSlots rows of C*sizeof(T) + 4 bytes (the + 4 spreads the rows over the banks): the occupied cells of a tile
// (~10 %) get consecutive slots
constexpr int kDenseSlots = 64;
// Cells per lane.  Measured on MI355X (16 scenes, 265 MB bf16): 2 -> 101 us (2.6 TB/s), 4 -> 120 us,
// 8 -> 296 us (tiles of 256+ cells overflow the 64 LDS slots near the ego vehicle and take the element-
// store path), 1 -> 134 us; memset + row scatter 264 us.
constexpr int kDenseVec = 2;

static __global__ __launch_bounds__(kDenseThreads) void fnp_dense_index_kernel(const int *__restrict__ coords,
                                                                               const int *__restrict__ n_rows, int cap, int B, int D,
                                                                               int H, int W, int *__restrict__ index) {
    const int n = min(*n_rows, cap);
    for (int r = blockIdx.x * kDenseThreads + threadIdx.x; r < n; r += gridDim.x * kDenseThreads) {
        const int4 c = reinterpret_cast<const int4 *>(coords)[r];
        if (c.x < 0 || c.x >= B || c.y < 0 || c.y >= D || c.z < 0 || c.z >= H || c.w < 0 || c.w >= W) continue;
        index[(((long long)c.x * D + c.y) * H + c.z) * W + c.w] = r;
    }
}

// rows of the lane's VEC cells (-1: no row, or the lane lies behind the plane's end); cell0 = the lane's first cell in `index`
template <int VEC> __device__ __forceinline__ void fnp_dense_tile_rows(const int *__restrict__ index, long long cell0, bool in, int (&r)[VEC]) {
    typedef int IVec __attribute__((ext_vector_type(VEC)));
    if (in) {
        if constexpr (VEC == 1) {
            r[0] = index[cell0];
        } else {
            const IVec v = *reinterpret_cast<const IVec *>(index + cell0);
#pragma unroll
            for (int j = 0; j < VEC; ++j) r[j] = v[j];
        }
    } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j) r[j] = -1;
    }
}

// rows of the cells in mask m (taken from rj) -> slots first, first + 1, ...; wave w copies every 4th.  -> the next free slot
__device__ __forceinline__ int fnp_dense_stage_rows(unsigned char *smem, const void *feats, int row_bytes, int stride,
                                                    unsigned long long m, const int rj, int first, int lane, int wave) {
    int k = first;
    while (m) {
        const int x = __ffsll((long long)m) - 1;
        m &= m - 1;
        const int rr = __shfl(rj, x);
        const int slot = k++;
        if ((slot & 3) != wave) continue;
        const unsigned *src = reinterpret_cast<const unsigned *>(reinterpret_cast<const unsigned char *>(feats) + (size_t)rr * row_bytes);
        unsigned *dst = reinterpret_cast<unsigned *>(smem + slot * stride);
        for (int q = lane; q * 4 < row_bytes; q += 64) dst[q] = src[q];
    }
    return k;
}

// the adjoint's staging: the lanes that own a cell of this pass (mine[j]) read their VEC cells of every channel plane the wave
// handles (coalesced, VEC*sizeof(T) bytes per lane, U planes in flight) and park the occupied ones in slot[j] - p0.
// g: the lane's first cell in channel plane 0; channel c adds c * cstep.
template <typename T, int VEC>
__device__ __forceinline__ void fnp_dense_gather_tile(unsigned char *smem, const T *__restrict__ g, long long cstep, int C, int stride,
                                                      int wave, const bool (&mine)[VEC], const int (&slot)[VEC], int p0) {
    typedef T TVec __attribute__((ext_vector_type(VEC)));
    constexpr int U = 8;                                         // channel planes in flight per wave
    for (int c0 = wave; c0 < C; c0 += 4 * U) {
        TVec v[U];
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (c0 + 4 * u < C) {
                if constexpr (VEC == 1) v[u][0] = g[(c0 + 4 * u) * cstep];
                else v[u] = *reinterpret_cast<const TVec *>(g + (c0 + 4 * u) * cstep);
            }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (c0 + 4 * u < C) {
#pragma unroll
                for (int j = 0; j < VEC; ++j)
                    if (mine[j]) reinterpret_cast<T *>(smem + (slot[j] - p0) * stride)[c0 + 4 * u] = v[u][j];
            }
    }
}
