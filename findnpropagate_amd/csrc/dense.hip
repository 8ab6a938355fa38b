// SparseConvTensor.dense() as consumed by HeightCompression (pcdet/models/backbones_2d/map_to_bev/
// height_compression.py:20-24: dense (B,C,D,H,W) then viewed as (B, C*D, H, W)): the largest single
// HBM write after the backbone (265 MB bf16 for 16 scenes of (128, 2, 180, 180)).
//
// A row-driven scatter writes C separate 2-byte elements per site, each into a different channel
// plane: 13.9 M sector-sized partial writes on top of the memset of the whole tensor.  Here the
// tensor is written ONCE, zeros included, in plane order:
//   1. index map: cell (b,z,y,x) -> row or -1 (4 bytes per cell, memset + one 4-byte scatter per row);
//   2. one workgroup per 64 consecutive cells of a (b,z) plane: the feature rows of the occupied
//      cells (~10 %) are copied whole (coalesced) into a padded LDS tile, then every wave writes,
//      channel plane by channel plane, 64 consecutive elements (one 128-byte bf16 segment per store);
//      a tile without sites only writes zeros.
// Without a workspace the scatter path is used and `out` must be zero on entry.
#include "common.h"
#include "dense_tile.h"   // the cell -> row map, the tile geometry and the LDS stagings (shared with bev_bn.hip)
#include <cstdint>

namespace {

constexpr int kThreads = 256;

template <typename T>
__global__ __launch_bounds__(kThreads) void dense_scatter_kernel(const T *__restrict__ feats, const int *__restrict__ coords,
                                                                 const int *__restrict__ n_rows, int cap, int C, int D, int H,
                                                                 int W, T *__restrict__ out) {
    const int n = min(*n_rows, cap);
    const long long total = (long long)n * C;
    const long long vol = (long long)D * H * W;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const int row = (int)(t / C), c = (int)(t % C);
        const int4 cd = reinterpret_cast<const int4 *>(coords)[row];
        const long long sp = ((long long)cd.y * H + cd.z) * W + cd.w;
        out[((long long)cd.x * C + c) * vol + sp] = feats[t];
    }
}

// T: element type (2 or 4 bytes); row bytes must be a multiple of 4.  One tile = 64*VEC consecutive cells
// of a (b,z) plane; lane l owns cells VEC*l .. VEC*l+VEC-1 and stores them with one VEC*sizeof(T)-byte
// store per channel plane (a wave store covers 64*VEC*sizeof(T) contiguous bytes).
// LDS: kSlots rows of C*sizeof(T) + 4 bytes (the + 4 spreads the rows over the banks): the occupied
// cells of a tile (~10 %) get consecutive slots; a tile with more than kSlots of them is written in VEC
// passes of one cell per lane (element stores) — rare, and still each element exactly once.
constexpr int kSlots = kDenseSlots;

template <typename T, int VEC>
__global__ __launch_bounds__(kThreads) void dense_write_kernel(const T *__restrict__ feats, const int *__restrict__ index, int C,
                                                               int B, int D, long long plane, int tiles_per_plane,
                                                               T *__restrict__ out, const float *__restrict__ fill) {
    // fill (optional, per channel): the value of a cell without a row instead of 0 — the BEV map behind a convolution whose
    // epilogue (BatchNorm shift, ReLU) gives cells with no input in reach a constant per channel
    extern __shared__ __attribute__((aligned(16))) unsigned char fnp_dense_smem[];
    typedef T TVec __attribute__((ext_vector_type(VEC)));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long tile = blockIdx.x;
    const long long bz = tile / tiles_per_plane;                 // = b*D + z
    const long long l0 = (tile % tiles_per_plane) * (64 * VEC);  // first cell of the tile inside the plane
    const int b = (int)(bz / D), z = (int)(bz % D);
    const bool in = l0 + (long long)VEC * lane < plane;          // (plane % VEC == 0: all of the lane's cells or none)
    int r[VEC];
    fnp_dense_tile_rows<VEC>(index, bz * plane + l0 + (long long)VEC * lane, in, r);
    unsigned long long occ[VEC];                                  // same in all four waves
    int total = 0;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        occ[j] = __ballot(r[j] >= 0);
        total += __popcll(occ[j]);
    }
    const int row_bytes = C * (int)sizeof(T), stride = row_bytes + 4;
    T *o = out + ((long long)b * C * D + z) * plane + l0 + (long long)VEC * lane;   // channel c adds c * D * plane
    const long long cstep = (long long)D * plane;
    const unsigned long long below = (1ull << lane) - 1ull;

    auto stage = [&](unsigned long long m, const int rj, int first) {
        return fnp_dense_stage_rows(fnp_dense_smem, feats, row_bytes, stride, m, rj, first, lane, wave);
    };

    if (total == 0) {
        if (!in) return;
        for (int c = wave; c < C; c += 4) {
            const T bg = fill ? (T)fill[c] : (T)0;
            TVec v;
#pragma unroll
            for (int j = 0; j < VEC; ++j) v[j] = bg;
            *reinterpret_cast<TVec *>(o + c * cstep) = v;
        }
    } else if (total <= kSlots) {
        int first = 0, myslot[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            myslot[j] = first + __popcll(occ[j] & below);
            first = stage(occ[j], r[j], first);
        }
        __syncthreads();
        if (!in) return;
        for (int c = wave; c < C; c += 4) {
            const T bg = fill ? (T)fill[c] : (T)0;
            TVec v;
#pragma unroll
            for (int j = 0; j < VEC; ++j)
                v[j] = ((occ[j] >> lane) & 1ull) ? reinterpret_cast<const T *>(fnp_dense_smem + myslot[j] * stride)[c] : bg;
            *reinterpret_cast<TVec *>(o + c * cstep) = v;
        }
    } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j) {   // (workgroup-uniform path: the barriers match)
            stage(occ[j], r[j], 0);
            __syncthreads();
            if (in) {
                const bool has = (occ[j] >> lane) & 1ull;
                const T *mine = reinterpret_cast<const T *>(fnp_dense_smem + __popcll(occ[j] & below) * stride);
                for (int c = wave; c < C; c += 4) o[c * cstep + j] = has ? mine[c] : (fill ? (T)fill[c] : (T)0);
            }
            __syncthreads();
        }
    }
}

// (cells per lane: kDenseVec, dense_tile.h)
template <typename T, int VEC>
int launch_dense_write(const void *feats, const int *index, int C, int B, int D, long long plane, void *out, const float *fill, hipStream_t s) {
    const int row_bytes = C * (int)sizeof(T);
    const int tiles_per_plane = (int)((plane + 64 * VEC - 1) / (64 * VEC));
    const long long tiles = (long long)B * D * tiles_per_plane;
    if (tiles > 0x7fffffffll) return FNP_ERR_ARG;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(dense_write_kernel<T, VEC>), dim3((unsigned)tiles), dim3(kThreads), kSlots * (row_bytes + 4), s,
                       (const T *)feats, index, C, B, D, plane, tiles_per_plane, (T *)out, fill);
    FNP_LAUNCH_CHECK();
    return FNP_OK;
}

template <typename T>
int run_dense(const void *feats, const int *coords, const int *n_rows, int cap, int C, int B, int D, int H, int W, void *out,
              void *ws, int64_t ws_bytes, hipStream_t s, const float *fill = nullptr) {
    const long long plane = (long long)H * W, cells = (long long)B * D * plane;
    const int row_bytes = C * (int)sizeof(T);
    const bool tiled = ws != nullptr && row_bytes % 4 == 0 && 64 * (row_bytes + 4) <= 64 * 1024;
    if (!tiled) {
        if (fill) return FNP_ERR_ARG;   // (a per-channel background needs the single-pass writer: workspace + a row size it takes)
        if (ws) {   // (workspace given: out may be dirty)
            const long long bytes = cells * C * (long long)sizeof(T);
            if (bytes % 4 == 0 && ((uintptr_t)out & 3) == 0) {
                const int frc = fnp_fill_words(out, bytes / 4, 0u, s);
                if (frc) return frc;
            } else {
                FNP_HIP_TRY(hipMemsetAsync(out, 0, (size_t)bytes, s));   // (odd sizes only: not a shape of the backbone)
            }
        }
        const int grid = fnp_grid_for((long long)cap * C, kThreads, 256 * 16);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(dense_scatter_kernel<T>), dim3(grid), dim3(kThreads), 0, s, (const T *)feats, coords,
                           n_rows, cap, C, D, H, W, (T *)out);
        FNP_LAUNCH_CHECK();
        return FNP_OK;
    }
    if (ws_bytes < cells * 4) return FNP_ERR_WORKSPACE;
    int *index = (int *)ws;
    {
        const int frc = fnp_fill_words(index, cells, 0xffffffffu, s);
        if (frc) return frc;
    }
    hipLaunchKernelGGL(fnp_dense_index_kernel, dim3(fnp_grid_for(cap, kThreads)), dim3(kThreads), 0, s, coords, n_rows, cap, B, D, H,
                       W, index);
    FNP_LAUNCH_CHECK();
    // widest store (<= 16 bytes per lane) that the plane size and the buffer alignment allow
    const bool al = ((uintptr_t)out % 16 == 0) && ((uintptr_t)ws % 16 == 0);
    constexpr int kMaxVec = 16 / (int)sizeof(T) < kDenseVec ? 16 / (int)sizeof(T) : kDenseVec;
    if constexpr (kMaxVec >= 8) {
        if (al && plane % 8 == 0) return launch_dense_write<T, 8>(feats, index, C, B, D, plane, out, fill, s);
    }
    if constexpr (kMaxVec >= 4) {
        if (al && plane % 4 == 0) return launch_dense_write<T, 4>(feats, index, C, B, D, plane, out, fill, s);
    }
    if constexpr (kMaxVec >= 2) {
        if (al && plane % 2 == 0) return launch_dense_write<T, 2>(feats, index, C, B, D, plane, out, fill, s);
    }
    return launch_dense_write<T, 1>(feats, index, C, B, D, plane, out, fill, s);
}

// ---------------------------------------------------------------------------------------------------------------------
// The adjoint of the writer (training through HeightCompression): grad_feats[r, :] = grad_out[b, :, z, y, x] for every
// row r < n whose (b, z, y, x) lies in the grid, a plain copy; every other row gets 0 (the forward wrote nothing for it).
// Same tiling as dense_write_kernel, read instead of written: one workgroup per 64*VEC consecutive cells of a (b,z) plane;
// a tile without rows reads nothing; otherwise the lanes that own an occupied cell read their VEC cells of every channel
// plane (coalesced, VEC*sizeof(T) bytes per lane) and park the occupied ones in padded LDS slots, then the workgroup writes
// each staged row whole (C*sizeof(T) contiguous bytes, 16-byte stores where the row size and buffer allow).  A tile with
// more than kSlots rows is done in passes of kSlots slots (each pass re-reads only the lanes whose cells it stages).

// rows r < n: cell -> row in `index` (in the grid) or a zero row (outside); rows n .. cap-1: zero.  After this launch the
// tile kernel writes exactly the rows the index map names, so every row of grad_feats is written once.
template <typename T>
__global__ __launch_bounds__(kThreads) void dense_grad_index_kernel(const int *__restrict__ coords, const int *__restrict__ n_rows,
                                                                    int cap, int C, int B, int D, int H, int W, int *__restrict__ index,
                                                                    T *__restrict__ grad_feats) {
    const int n = min(*n_rows, cap);
    for (int r = blockIdx.x * kThreads + threadIdx.x; r < n; r += gridDim.x * kThreads) {
        const int4 c = reinterpret_cast<const int4 *>(coords)[r];
        if (c.x < 0 || c.x >= B || c.y < 0 || c.y >= D || c.z < 0 || c.z >= H || c.w < 0 || c.w >= W) {
            for (int e = 0; e < C; ++e) grad_feats[(long long)r * C + e] = (T)0;
            continue;
        }
        index[(((long long)c.x * D + c.y) * H + c.z) * W + c.w] = r;
    }
    const long long end = (long long)cap * C;
    for (long long t = (long long)n * C + (long long)blockIdx.x * kThreads + threadIdx.x; t < end; t += (long long)gridDim.x * kThreads)
        grad_feats[t] = (T)0;
}

template <typename T, int VEC>
__global__ __launch_bounds__(kThreads) void dense_grad_kernel(const T *__restrict__ grad_out, const int *__restrict__ index, int C,
                                                              int D, long long plane, int tiles_per_plane, int quad,
                                                              T *__restrict__ grad_feats) {
    extern __shared__ __attribute__((aligned(16))) unsigned char fnp_dense_smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long tile = blockIdx.x;
    const long long bz = tile / tiles_per_plane;
    const long long l0 = (tile % tiles_per_plane) * (64 * VEC);
    const int b = (int)(bz / D), z = (int)(bz % D);
    const bool in = l0 + (long long)VEC * lane < plane;
    int r[VEC];
    fnp_dense_tile_rows<VEC>(index, bz * plane + l0 + (long long)VEC * lane, in, r);
    const unsigned long long below = (1ull << lane) - 1ull;
    int total = 0, slot[VEC];                                    // slot of cell j (when occupied): rank among the tile's rows
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        const unsigned long long occ = __ballot(r[j] >= 0);    // (same in all four waves: they own the same cells)
        slot[j] = total + __popcll(occ & below);
        total += __popcll(occ);
    }
    if (total == 0) return;                                      // (workgroup-uniform)

    const int row_bytes = C * (int)sizeof(T), stride = row_bytes + 4;
    int *slot_row = reinterpret_cast<int *>(fnp_dense_smem + kSlots * stride);
    const T *g = grad_out + ((long long)b * C * D + z) * plane + l0 + (long long)VEC * lane;   // channel c adds c * D * plane
    const long long cstep = (long long)D * plane;
    for (int p0 = 0; p0 < total; p0 += kSlots) {                 // one pass unless the tile holds more than kSlots rows
        bool mine[VEC], any = false;
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            mine[j] = r[j] >= 0 && slot[j] >= p0 && slot[j] < p0 + kSlots;
            any |= mine[j];
            if (mine[j] && wave == 0) slot_row[slot[j] - p0] = r[j];
        }
        if (any) {
            fnp_dense_gather_tile<T, VEC>(fnp_dense_smem, g, cstep, C, stride, wave, mine, slot, p0);
        }
        __syncthreads();
        const int cnt = min(total - p0, kSlots);
        unsigned char *dst0 = reinterpret_cast<unsigned char *>(grad_feats);
        if (quad) {   // row_bytes % 16 == 0, grad_feats 16-byte aligned
            const int qpr = row_bytes >> 4;
            for (int i = threadIdx.x; i < cnt * qpr; i += kThreads) {
                const int k = i / qpr, q = i - k * qpr;
                const unsigned *src = reinterpret_cast<const unsigned *>(fnp_dense_smem + k * stride) + 4 * q;
                const uint4 v = make_uint4(src[0], src[1], src[2], src[3]);
                *reinterpret_cast<uint4 *>(dst0 + (size_t)slot_row[k] * row_bytes + 16 * q) = v;
            }
        } else {
            const int wpr = row_bytes >> 2;
            for (int i = threadIdx.x; i < cnt * wpr; i += kThreads) {
                const int k = i / wpr, q = i - k * wpr;
                reinterpret_cast<unsigned *>(dst0 + (size_t)slot_row[k] * row_bytes)[q] =
                    reinterpret_cast<const unsigned *>(fnp_dense_smem + k * stride)[q];
            }
        }
        __syncthreads();                                         // (before the next pass overwrites the slots)
    }
}

// Rows without a workspace, or whose size the tile kernel does not take: one thread per element of grad_feats.
template <typename T>
__global__ __launch_bounds__(kThreads) void dense_grad_rows_kernel(const T *__restrict__ grad_out, const int *__restrict__ coords,
                                                                   const int *__restrict__ n_rows, int cap, int C, int B, int D, int H,
                                                                   int W, T *__restrict__ grad_feats) {
    const int n = min(*n_rows, cap);
    const long long total = (long long)cap * C;
    const long long vol = (long long)D * H * W;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const int row = (int)(t / C), c = (int)(t % C);
        T v = (T)0;
        if (row < n) {
            const int4 cd = reinterpret_cast<const int4 *>(coords)[row];
            if (cd.x >= 0 && cd.x < B && cd.y >= 0 && cd.y < D && cd.z >= 0 && cd.z < H && cd.w >= 0 && cd.w < W)
                v = grad_out[((long long)cd.x * C + c) * vol + ((long long)cd.y * H + cd.z) * W + cd.w];
        }
        grad_feats[t] = v;
    }
}

template <typename T, int VEC>
int launch_dense_grad(const void *grad_out, const int *index, int C, int B, int D, long long plane, void *grad_feats, hipStream_t s) {
    const int row_bytes = C * (int)sizeof(T);
    const int tiles_per_plane = (int)((plane + 64 * VEC - 1) / (64 * VEC));
    const long long tiles = (long long)B * D * tiles_per_plane;
    if (tiles > 0x7fffffffll) return FNP_ERR_ARG;
    const int quad = row_bytes % 16 == 0 && (uintptr_t)grad_feats % 16 == 0;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(dense_grad_kernel<T, VEC>), dim3((unsigned)tiles), dim3(kThreads),
                       kSlots * (row_bytes + 4) + kSlots * 4, s, (const T *)grad_out, index, C, D, plane, tiles_per_plane, quad,
                       (T *)grad_feats);
    FNP_LAUNCH_CHECK();
    return FNP_OK;
}

template <typename T>
int run_dense_backward(const void *grad_out, const int *coords, const int *n_rows, int cap, int C, int B, int D, int H, int W,
                       void *grad_feats, void *ws, int64_t ws_bytes, hipStream_t s) {
    const long long plane = (long long)H * W, cells = (long long)B * D * plane;
    const int row_bytes = C * (int)sizeof(T);
    const bool tiled = ws != nullptr && row_bytes % 4 == 0 && kSlots * (row_bytes + 4) + kSlots * 4 <= 64 * 1024;
    if (!tiled) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(dense_grad_rows_kernel<T>), dim3(fnp_grid_for((long long)cap * C, kThreads, 256 * 16)),
                           dim3(kThreads), 0, s, (const T *)grad_out, coords, n_rows, cap, C, B, D, H, W, (T *)grad_feats);
        FNP_LAUNCH_CHECK();
        return FNP_OK;
    }
    if (ws_bytes < cells * 4) return FNP_ERR_WORKSPACE;
    int *index = (int *)ws;
    {
        const int frc = fnp_fill_words(index, cells, 0xffffffffu, s);
        if (frc) return frc;
    }
    hipLaunchKernelGGL(HIP_KERNEL_NAME(dense_grad_index_kernel<T>), dim3(fnp_grid_for(cap, kThreads)), dim3(kThreads), 0, s, coords,
                       n_rows, cap, C, B, D, H, W, index, (T *)grad_feats);
    FNP_LAUNCH_CHECK();
    const bool al = ((uintptr_t)grad_out % 16 == 0) && ((uintptr_t)ws % 16 == 0);
    constexpr int kMaxVec = 16 / (int)sizeof(T) < kDenseVec ? 16 / (int)sizeof(T) : kDenseVec;
    if constexpr (kMaxVec >= 8) {
        if (al && plane % 8 == 0) return launch_dense_grad<T, 8>(grad_out, index, C, B, D, plane, grad_feats, s);
    }
    if constexpr (kMaxVec >= 4) {
        if (al && plane % 4 == 0) return launch_dense_grad<T, 4>(grad_out, index, C, B, D, plane, grad_feats, s);
    }
    if constexpr (kMaxVec >= 2) {
        if (al && plane % 2 == 0) return launch_dense_grad<T, 2>(grad_out, index, C, B, D, plane, grad_feats, s);
    }
    return launch_dense_grad<T, 1>(grad_out, index, C, B, D, plane, grad_feats, s);
}

}  // namespace

extern "C" int64_t fnp_sparse_to_dense_workspace_bytes(int B, int D, int H, int W) {
    if (B <= 0 || D <= 0 || H <= 0 || W <= 0) return 0;
    return (int64_t)B * D * H * W * 4;
}

extern "C" int fnp_sparse_to_dense(const void *feats, int dtype, const int *coords, const int *n_rows, int cap, int C,
                                   int B, int D, int H, int W, void *out, void *workspace, int64_t workspace_bytes,
                                   fnp_stream_t stream) {
    if (!feats || !coords || !n_rows || !out || cap <= 0 || C <= 0 || B <= 0 || D <= 0 || H <= 0 || W <= 0)
        return FNP_ERR_ARG;
    if (dtype == FNP_F32)
        return run_dense<float>(feats, coords, n_rows, cap, C, B, D, H, W, out, workspace, workspace_bytes, (hipStream_t)stream);
    if (dtype == FNP_BF16)
        return run_dense<__bf16>(feats, coords, n_rows, cap, C, B, D, H, W, out, workspace, workspace_bytes, (hipStream_t)stream);
    if (dtype == FNP_F16)
        return run_dense<_Float16>(feats, coords, n_rows, cap, C, B, D, H, W, out, workspace, workspace_bytes, (hipStream_t)stream);
    return FNP_ERR_ARG;
}

// fnp_sparse_to_dense with a per-channel value for the cells without a row (fill: C floats in device memory).  Needs the
// workspace (the single-pass writer).  The first BaseBEVBackbone block evaluated on sparse rows ends with it.
extern "C" int fnp_sparse_to_dense_fill(const void *feats, int dtype, const int *coords, const int *n_rows, int cap, int C,
                                        int B, int D, int H, int W, void *out, const float *fill, void *workspace,
                                        int64_t workspace_bytes, fnp_stream_t stream) {
    if (!feats || !coords || !n_rows || !out || !fill || !workspace || cap <= 0 || C <= 0 || B <= 0 || D <= 0 || H <= 0 || W <= 0)
        return FNP_ERR_ARG;
    if (dtype == FNP_F32)
        return run_dense<float>(feats, coords, n_rows, cap, C, B, D, H, W, out, workspace, workspace_bytes, (hipStream_t)stream, fill);
    if (dtype == FNP_BF16)
        return run_dense<__bf16>(feats, coords, n_rows, cap, C, B, D, H, W, out, workspace, workspace_bytes, (hipStream_t)stream, fill);
    if (dtype == FNP_F16)
        return run_dense<_Float16>(feats, coords, n_rows, cap, C, B, D, H, W, out, workspace, workspace_bytes, (hipStream_t)stream, fill);
    return FNP_ERR_ARG;
}

// The adjoint of fnp_sparse_to_dense (backward of HeightCompression's densification): grad_out (B,C,D,H,W) -> grad_feats
// (cap, C), same dtype.  Every row is written: rows r < n in the grid get a copy of their cell's C values, the rest 0.
// With a workspace (the cell -> row map, rebuilt here) the plane-tiled gather runs; without one, a row-driven gather.
extern "C" int fnp_sparse_to_dense_backward(const void *grad_out, int dtype, const int *coords, const int *n_rows, int cap, int C,
                                            int B, int D, int H, int W, void *grad_feats, void *workspace, int64_t workspace_bytes,
                                            fnp_stream_t stream) {
    if (!grad_out || !coords || !n_rows || !grad_feats || cap <= 0 || C <= 0 || B <= 0 || D <= 0 || H <= 0 || W <= 0)
        return FNP_ERR_ARG;
    if (dtype == FNP_F32)
        return run_dense_backward<float>(grad_out, coords, n_rows, cap, C, B, D, H, W, grad_feats, workspace, workspace_bytes,
                                         (hipStream_t)stream);
    if (dtype == FNP_BF16)
        return run_dense_backward<__bf16>(grad_out, coords, n_rows, cap, C, B, D, H, W, grad_feats, workspace, workspace_bytes,
                                          (hipStream_t)stream);
    if (dtype == FNP_F16)
        return run_dense_backward<_Float16>(grad_out, coords, n_rows, cap, C, B, D, H, W, grad_feats, workspace, workspace_bytes,
                                            (hipStream_t)stream);
    return FNP_ERR_ARG;
}
