/*
 * fnp.h — C ABI of libfnp_hip.so, the MI355X (gfx950) drop-in for the point-cloud hot path of
 * djamahl99/findnpropagate (an OpenPCDet fork).
 *
 * Every entry point is what the reference's FFI for this path binds today (pybind11 torch
 * extensions and the third-party spconv package); the reference interface each one replaces is
 * cited as  <file>:<line>  relative to the reference tree.
 *
 * Conventions:
 *   - all pointers are DEVICE pointers borrowed from the caller (torch tensors), unless a
 *     parameter is documented as "host"; the caller allocates every output and every workspace;
 *   - no hidden allocation, no host synchronisation, no exit(): 0 = success, <0 = error code;
 *   - every launch goes to the hipStream_t handed in (the reference launches on the legacy
 *     default stream, roiaware_pool3d_kernel.cu:348, iou3d_nms_kernel.cu:394);
 *   - row counts that are data-dependent (voxels, active output sites) live in device memory
 *     (`const int *n_rows`), kernels grid-stride over them, so a whole forward is sync-free
 *     and hipGraph-capturable.
 */
#ifndef FNP_H
#define FNP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *fnp_stream_t; /* hipStream_t */

enum {
    FNP_OK = 0,
    FNP_ERR_ARG = -1,      /* bad shape / null pointer / unsupported channel count */
    FNP_ERR_LAUNCH = -2,   /* hipGetLastError() after a launch */
    FNP_ERR_HIP = -3,      /* a HIP runtime call failed */
    FNP_ERR_WORKSPACE = -4 /* workspace too small */
};

enum { FNP_F32 = 0, FNP_BF16 = 1, FNP_F16 = 2 };

/* Library / build identification: returns a static string "fnp-hip gfx950 <abi version>". */
const char *fnp_version(void);
int fnp_abi_version(void);

/* ------------------------------------------------------------------------------------------
 * roiaware_pool3d — replaces pcdet/ops/roiaware_pool3d/src/roiaware_pool3d.cpp:98-118
 * (points_in_boxes_gpu) and its kernel roiaware_pool3d_kernel.cu:16-36,313-359.
 * ------------------------------------------------------------------------------------------ */

/* boxes (B,T,7) [x,y,z,dx,dy,dz,heading], pts (B,M,3); box_idx_of_points (B,M) receives the
 * first (lowest) box index containing the point, else -1 (the reference needs the caller to
 * pre-fill -1, roiaware_pool3d_utils.py:38; this entry point writes every element). */
int fnp_points_in_boxes(const float *boxes, const float *pts, int *box_idx_of_points,
                        int B, int T, int M, fnp_stream_t stream);

/* Batched form of the Box Seeker's hot loop 4 (frustum_proposals_v1.py:930-932): for each of
 * T candidate boxes count the points (M,3) inside it, with the same test as above.
 * counts (T,) int32.  One launch instead of T launches + T host syncs. */
int fnp_points_in_boxes_count(const float *boxes, const float *pts, int *counts,
                              int T, int M, fnp_stream_t stream);

/* Dense (T,M) 0/1 membership with the reference's CPU margin 1e-2 and z test
 * (roiaware_pool3d.cpp:121-168, points_in_boxes_cpu) — device-side equivalent. */
int fnp_points_in_boxes_dense(const float *boxes, const float *pts, int *pts_indices,
                              int T, int M, fnp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * iou3d_nms — replaces pcdet/ops/iou3d_nms/src/iou3d_nms.cpp:49-209 and
 * iou3d_nms_kernel.cu (box_overlap :104-225, iou_bev :227-234, iou_normal :327-338,
 * nms_kernel :280-324, nms_normal_kernel :341-385).
 * ------------------------------------------------------------------------------------------ */

/* boxes_overlap_bev_gpu (iou3d_nms.cpp:71-89): a (N,7), b (M,7) -> ans (N,M) overlap area. */
int fnp_boxes_overlap_bev(const float *boxes_a, int num_a, const float *boxes_b, int num_b,
                          float *ans_overlap, fnp_stream_t stream);
/* boxes_iou_bev_gpu (iou3d_nms.cpp:91-111): -> ans (N,M) rotated BEV IoU. */
int fnp_boxes_iou_bev(const float *boxes_a, int num_a, const float *boxes_b, int num_b,
                      float *ans_iou, fnp_stream_t stream);
/* boxes_aligned_overlap_bev_gpu (iou3d_nms.cpp:49-69): a (N,7), b (N,7) -> ans (N,). */
int fnp_boxes_aligned_overlap_bev(const float *boxes_a, const float *boxes_b, int num,
                                  float *ans_overlap, fnp_stream_t stream);
/* Fused boxes_iou3d_gpu (iou3d_nms_utils.py:48-81): BEV overlap x height overlap / union,
 * z = box centre.  ans (N,M). */
int fnp_boxes_iou3d(const float *boxes_a, int num_a, const float *boxes_b, int num_b,
                    float *ans_iou, fnp_stream_t stream);

/* boxes_aligned_iou3d_gpu (iou3d_nms_utils.py:83-117) fused: a (N,7), b (N,7) -> ans (N,) 3D IoU of pair i. */
int fnp_boxes_aligned_iou3d(const float *boxes_a, const float *boxes_b, int num, float *ans_iou, fnp_stream_t stream);

/* Recall bookkeeping of one frame, Detector3DTemplate.generate_recall_record
 * (pcdet/models/detectors/detector3d_template.py:314-399, called per frame by tools/extract_pseudo_labels.py:124),
 * accumulated on the device: counters (5 + 6*num_thresh) int64 DEVICE, layout
 *   [gt, num_3known, num_6known, num_4unknown, num_7unknown] then per threshold
 *   [roi, rcnn, rcnn_3known, rcnn_6known, rcnn_4unknown, rcnn_7unknown]   (added to, never zeroed here).
 * preds: rows of pred_stride floats starting with a (7) box; pred_count: DEVICE float holding the number of live rows
 * (the header cell of an extraction record) or NULL = max_preds.  gt (num_gt, gt_stride >= 8): box (7) ... class label
 * (1-based) in the LAST column; trailing all-zero rows are padding (:342-346).  rois: optional (num_rois, rois_stride).
 * thresh: HOST floats (num_thresh <= 8).  known3_bits / known6_bits: bit l set iff label l is a known class. */
int fnp_recall_counters(const float *preds, int pred_stride, int max_preds, const float *pred_count,
                        const float *gt, int num_gt, int gt_stride, const float *rois, int num_rois, int rois_stride,
                        const float *thresh, int num_thresh, unsigned known3_bits, unsigned known6_bits,
                        int64_t *counters, fnp_stream_t stream);

/* Host-side dense point-in-box test of the pseudo-label mixing (PseudoSampler.points_in_boxes,
 * pcdet/datasets/augmentor/pseudo_loader.py:270-316): points (N,C>=3), boxes (T,7) -> in_box (T,N) u8 with
 * INCLUSIVE faces, and optionally the points in each box frame (T,N,C) (points_out may be NULL). */
int fnp_host_points_in_boxes_frame(const float *points, int n, int C, const float *boxes, int t,
                                   unsigned char *in_box, float *points_out);

/* The same membership in compact form (no (T, N) matrix): counts (T,) int32, the rows inside box t; box after box, in row order,
 * the row indices (int32) and the box-frame rows (C f32 each) of those rows: the entries of fnp_host_points_in_boxes_frame's
 * in_box and points_out, bit for bit.  indices (capacity,) and rows (capacity, C) receive the first `capacity` of them; counts
 * are always complete, and the call returns FNP_ERR_WORKSPACE when their sum exceeds capacity (call again with that size).
 * The pending cut (cut_m == 0: none): rows i with cut_from <= i < cut_to that lie inside one of the cut_m records
 * (fnp_host_cut_records; the test of fnp_host_points_outside_boxes and the device cut) are left out; indices still number the
 * input rows.  n < 2^31.  Host pointers, no device. */
int fnp_host_points_in_boxes_compact(const float *points, int64_t n, int C, const float *boxes, int t,
                                     const float *cut_records, int cut_m, int64_t cut_from, int64_t cut_to,
                                     int *counts, int64_t capacity, int *indices, float *rows);

/* Host-side rotated BEV IoU (no device, no stream): replaces boxes_iou_bev_cpu (N x M) and
 * boxes_aligned_iou_bev_cpu (N pairs) of pcdet/ops/iou3d_nms/src/iou3d_cpu.cpp:232-272, called by the
 * pseudo-label mixing in dataloader workers (pseudo_loader.py:29-55).  Host pointers, (n,7) boxes. */
int fnp_host_boxes_iou_bev(const float *boxes_a, int na, const float *boxes_b, int nb, float *iou_out);
int fnp_host_boxes_aligned_iou_bev(const float *boxes_a, const float *boxes_b, int n, float *iou_out);
/* The host twin of fnp_boxes_overlap_bev: overlap_out (na, nb) f32 = the BEV overlap AREA, the same function as the IoU above
 * before its division (additive, ABI 14).  The golden generator of the target assignment feeds it to the reference. */
int fnp_host_boxes_overlap_bev(const float *boxes_a, int na, const float *boxes_b, int nb, float *overlap_out);

/* Bytes of the u64 suppression-mask workspace for N boxes. */
int64_t fnp_nms_workspace_bytes(int num_boxes);
/* nms_gpu / nms_normal_gpu (iou3d_nms.cpp:113-209): boxes (N,7) pre-sorted by score desc.
 * keep (N,) int64 DEVICE, num_keep (1,) int32 DEVICE.  The greedy sweep that the reference
 * runs on the host after a synchronous cudaMemcpy (iou3d_nms.cpp:139-155,189-205) runs on
 * the device, so the call is asynchronous. */
int fnp_nms_rotated(const float *boxes, int num_boxes, float thresh, void *workspace,
                    int64_t *keep, int *num_keep, fnp_stream_t stream);
int fnp_nms_normal(const float *boxes, int num_boxes, float thresh, void *workspace,
                   int64_t *keep, int *num_keep, fnp_stream_t stream);
/* (ABI 12) Several score-sorted lists in one launch pair — the per-class NMS of multi_classes_nms (model_nms_utils.py:30-66): list z holds
 * counts[z] (a DEVICE array, each <= cap) boxes at boxes + z * cap * 7; keep (lists, cap) int64 and num_keep (lists) int32 receive,
 * per list, what fnp_nms_rotated (rotated != 0) / fnp_nms_normal gives for its first counts[z] boxes.  workspace:
 * fnp_nms_batched_workspace_bytes(lists, cap).  No host synchronisation. */
int64_t fnp_nms_batched_workspace_bytes(int lists, int cap);
int fnp_nms_batched(const float *boxes, const int *counts, int lists, int cap, float thresh, int rotated, void *workspace,
                    int64_t *keep, int *num_keep, fnp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Rank grid — the voxel index behind voxelisation and rulebook building.  A grid of
 * (B, D, H, W) cells is cut into 4x4x4 blocks; block w owns one u64 occupancy word
 * (bit = (z&3)*16 + (y&3)*4 + (x&3)) and one u32 exclusive popcount prefix, so
 *     row(cell) = base[w] + popc(bits[w] & below(bit))
 * is a collision-free lookup (at most 8 words for a 3x3x3 neighbourhood).  A second level,
 * one summary bit per block, lets the prefix scan, the coordinate emission and the clearing
 * visit only occupied blocks (a 41x1440x1440 lidar grid is ~1.5 % occupied at block level).
 * Replaces spconv's hash / direct table (call sites pcdet/utils/spconv_utils.py:3-10).
 * ------------------------------------------------------------------------------------------ */
typedef struct fnp_rankgrid {
    int B, D, H, W;     /* cells */
    uint64_t *bits;     /* (nblk)  occupancy words; all zero before a build */
    uint32_t *base;     /* (nblk)  exclusive popcount prefix, defined where bits != 0 */
    uint64_t *summary;  /* (nsum)  bit j of word i set iff bits[64*i + j] != 0; zero before a build */
    int *perm;          /* (cap)   rank -> row, or NULL when rows are stored in rank order */
    uint32_t *counters; /* (ABI 13, nullable) fnp_rankgrid_counter_words() words, ALL ZERO before a build: the marking kernels of
                         * fnp_voxelize / fnp_rulebook_strided add the cells they set to per-unit / per-group / per-chunk counters
                         * here (one atomic per workgroup and counter), and the rank prefix is ONE launch instead of three (count
                         * pass, totals, prefix pass).  The fnp_rankgrid_clear* calls zero them again.  NULL: the three-launch prefix. */
} fnp_rankgrid;

int64_t fnp_rankgrid_num_blocks(int B, int D, int H, int W);   /* nblk */
int64_t fnp_rankgrid_num_summary(int B, int D, int H, int W);  /* nsum = ceil(nblk / 64) */
int64_t fnp_rankgrid_counter_words(int B, int D, int H, int W); /* (ABI 13) uint32 words of fnp_rankgrid.counters */
int64_t fnp_rankgrid_workspace_bytes(int B, int D, int H, int W);

/* Index an existing coordinate list (N,4) [b,z,y,x] (e.g. a SparseConvTensor built from user
 * tensors): sets bits/summary/base and, when grid->perm != NULL, perm[rank] = row. */
int fnp_rankgrid_build(const int *coords, const int *n_rows, int cap, const fnp_rankgrid *grid,
                       void *workspace, int64_t workspace_bytes, fnp_stream_t stream);

/* Zero the occupancy + summary words touched by `coords` (O(rows) instead of O(grid)). */
int fnp_rankgrid_clear(const int *coords, const int *n_rows, int cap, const fnp_rankgrid *grid,
                       fnp_stream_t stream);

/* fnp_rankgrid_clear for up to 8 grids in one launch (HOST arrays of `count` device pointers / capacities / grids). */
int fnp_rankgrid_clear_multi(int count, const int *const *coords, const int *const *n_rows, const int *caps,
                             const fnp_rankgrid *grids, fnp_stream_t stream);

/* (ABI 13) Zero up to 8 grids through their SUMMARY level in one launch: every occupancy word a summary bit names, the summary
 * words, the counters.  No coordinate list: whatever was marked goes (cells of dropped voxels and of rows beyond a capacity too). */
int fnp_rankgrid_clear_summary(int count, const fnp_rankgrid *grids, fnp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Voxelisation + MeanVFE — replaces spconv.utils.Point2VoxelCPU3d.point_to_voxel as called
 * at pcdet/datasets/processor/data_processor.py:38-61 and MeanVFE.forward
 * (pcdet/models/backbones_3d/vfe/mean_vfe.py:14-31).
 * ------------------------------------------------------------------------------------------ */
typedef struct fnp_voxel_cfg {
    float range_min[3];  /* x,y,z of POINT_CLOUD_RANGE[0:3] */
    float voxel_size[3]; /* x,y,z */
    int grid[3];         /* x,y,z = round((max-min)/voxel_size), data_processor.py:257-258 */
    int num_features;    /* C of points (N,C); xyz are columns 0..2 */
    int max_points;      /* MAX_POINTS_PER_VOXEL (10) */
    int max_voxels;      /* MAX_NUMBER_OF_VOXELS per scene */
} fnp_voxel_cfg;

/* The rank grid the voxels are indexed in may be larger than the voxel grid
 * {cfg.grid[2], cfg.grid[1], cfg.grid[0]} (the backbone's sparse_shape adds one z layer,
 * spconv_backbone.py:191); grid->B is the number of scenes. */
int64_t fnp_voxelize_workspace_bytes(int64_t n_points, const fnp_voxel_cfg *cfg, const fnp_rankgrid *grid);

/* A frame into the STATIC inputs of a captured forward (a hipGraph reads fixed addresses), one launch: dst_points[0, n) = points,
 * dst_points[n, n_prev) = pad in every column (rows the previous frame filled: pad lies outside every range, the voxeliser drops such
 * points), dst_offsets = batch_offsets (n_offsets words).  All device pointers; (n, num_features) f32 rows, contiguous.
 * The reference's loops hand a frame to the model through load_data_to_gpu (pcdet/models/__init__.py:23-37). */
int fnp_stage_points(const float *points, int64_t n_points, int64_t n_prev_points, int num_features, float pad, float *dst_points,
                     const int *batch_offsets, int n_offsets, int *dst_offsets, fnp_stream_t stream);

/* points (N,C) f32, scenes concatenated; batch_offsets (B+1,) int32 device (scene b owns
 * points [off[b], off[b+1])).  Outputs, all capacity `cap` rows (cap >= N is always enough):
 *   coords (cap,4) int32 [b,z,y,x] in the sequential first-come order of the reference,
 *   num_points (cap,) int32, mean_feats (cap,C) f32 = MeanVFE, voxels (cap,max_points,C) f32
 *   zero padded (nullable), n_voxels (1,) int32 device.
 * The grid (bits/summary zero on entry, perm != NULL) is left describing the voxels for the first
 * rulebook: perm[rank] = voxel row, -1 for a cell whose voxel fell to the max_voxels cut.
 * n_cells (1,) int32 device, nullable: number of occupied cells (>= n_voxels); rows
 * [n_voxels, n_cells) of coords then list the cells of the dropped voxels in no particular order, so
 * that fnp_rankgrid_clear(coords, n_cells, ...) wipes every word the voxeliser set in a persistent grid. */
int fnp_voxelize(const float *points, int n_points, const int *batch_offsets,
                 const fnp_voxel_cfg *cfg, const fnp_rankgrid *grid,
                 void *workspace, int64_t workspace_bytes,
                 int *coords, int *num_points, float *mean_feats, float *voxels,
                 int *n_voxels, int *n_cells, int cap, fnp_stream_t stream);

/* HOST voxeliser (no device, no stream; host pointers): spconv.utils.Point2VoxelCPU3d.point_to_voxel as DataProcessor
 * calls it inside DataLoader worker processes (data_processor.py:38-61,255-302), where a GPU context cannot be created
 * after a fork.  One scene: points (n, C) -> voxels (max_rows, max_points, C) zero padded, coords (max_rows, 3) [z,y,x],
 * num_points (max_rows); rows = first-come order, capped at min(cfg->max_voxels, max_rows).  Returns the number of
 * voxels or a negative error code.  Results equal fnp_voxelize's bit for bit. */
int fnp_host_voxelize(const float *points, int n_points, const fnp_voxel_cfg *cfg, float *voxels, int *coords,
                      int *num_points, int max_rows);

/* ------------------------------------------------------------------------------------------
 * Point preparation in front of fnp_voxelize — replaces, on the device, the world augmentations of DataAugmentor
 * (pcdet/datasets/augmentor/data_augmentor.py:59-181: random_world_flip / _rotation / _scaling / _translation),
 * the points half of mask_points_and_boxes_outside_range (data_processor.py:80-94, common_utils.py:78-81) and
 * shuffle_points (data_processor.py:96-106), which the reference runs in numpy inside DataLoader workers.
 * ------------------------------------------------------------------------------------------ */
enum { FNP_SHUFFLE_NONE = 0, FNP_SHUFFLE_DEVICE = 1, FNP_SHUFFLE_EXPLICIT = 2 };
enum { FNP_PREP_MAX_STEPS = 6 };

int64_t fnp_prepare_points_workspace_bytes(int64_t n_points);

/* points (N, C) f32, scenes concatenated, batch_offsets (B+1,) int32 (scene b owns rows [off[b], off[b+1])).
 * program (B, K, 4) f32, K <= FNP_PREP_MAX_STEPS (nullable when K = 0): scene b's ops in the order the config lists them,
 *   one row {op, a, b, c} per step: 0 none, 1 flip x (y = -y), 2 flip y (x = -x), 3 rotate about z (a = cos, b = sin of the
 *   f32 angle, computed on the host), 4 scale xyz by a, 5 translate xyz by (a, b, c).  f32 arithmetic of the reference.
 * The range (host values): a point is kept iff x_min <= x <= x_max and y_min <= y <= y_max after its program (in f64, as numpy
 *   compares an f32 array with the f64 range); z is not tested.
 * shuffle_mode: FNP_SHUFFLE_NONE keeps the kept rows in order; FNP_SHUFFLE_DEVICE places the k-th kept row of scene b at a
 *   keyed bijection of k in [0, m_b) (seed and b are the key: reproducible, independent of the rest of the batch);
 *   FNP_SHUFFLE_EXPLICIT writes out[j] = kept[perm[j]] with perm (n_perm,) int32 device, perm[o_b + j] in [0, m_b) the scene's
 *   own permutation of its kept rows (numpy's np.random.permutation order after the mask).
 * Outputs: out_points (N, C) f32: the kept rows, scene after scene, then rows [kept, N) = pad in every column (pad must lie
 *   outside every range: fnp_voxelize over all N rows drops them); out_offsets (B+1,) int32: the new scene offsets, and
 *   out_offsets[B] the total kept count.  Everything stays on the device; no host synchronisation. */
int fnp_prepare_points(const float *points, int64_t n_points, int num_features, const int *batch_offsets, int batch_size,
                       const float *program, int program_steps, double x_min, double y_min, double x_max, double y_max,
                       int shuffle_mode, const int *perm, int64_t n_perm, uint64_t seed, float pad,
                       void *workspace, int64_t workspace_bytes, float *out_points, int *out_offsets, fnp_stream_t stream);

/* gt_sampling's cut (DataBaseSampler.add_sampled_boxes_to_scene: box_utils.remove_points_in_boxes3d over the sampled boxes enlarged
 * by REMOVE_EXTRA_WIDTH, i.e. roiaware_pool3d.cpp points_in_boxes_cpu).  A cut record is 8 f32 {cx, cy, cz, dx, dy, dz, cos(-h),
 * sin(-h)}; a point is inside when fabsf(z - cz) <= dz / 2.0 and, with the f32 rotation lx = sx*c + sy*(-s), ly = sx*s + sy*c
 * (sx = x - cx, sy = y - cy), |lx| < dx / 2.0 + 1e-2f and |ly| < dy / 2.0 + 1e-2f, compared in double: the reference's test bit
 * for bit.  Host and device share that one definition.
 *
 * fnp_host_cut_records: boxes (m, 7) f32 host -> records (m, 8) f32 host, cos / sin by the C library's cosf / sinf.
 * fnp_host_points_outside_boxes: keep[i] = 1 iff point i of points (n, C) f32 host lies in none of the m records (host). */
int fnp_host_cut_records(const float *boxes, int m, float *records);
int fnp_host_points_outside_boxes(const float *points, int64_t n, int num_features, const float *records, int m,
                                  unsigned char *keep);

/* fnp_prepare_points with the cut in front of the program: row i of scene b is dropped when i >= off[b] + cut_from[b] and the
 * raw row lies inside one of the records [cut_offsets[b], cut_offsets[b+1]) of cut_records (device, 4-byte aligned; NULL only
 * when no scene has a record).  cut_offsets (B+1,) and cut_from (B,) are int32 device arrays.  Same workspace, outputs and
 * guarantees as fnp_prepare_points: no atomics, no host synchronisation, any number of records per scene, capturable. */
int fnp_prepare_points_cut(const float *points, int64_t n_points, int num_features, const int *batch_offsets, int batch_size,
                           const float *program, int program_steps, const float *cut_records, const int *cut_offsets,
                           const int *cut_from, double x_min, double y_min, double x_max, double y_max,
                           int shuffle_mode, const int *perm, int64_t n_perm, uint64_t seed, float pad,
                           void *workspace, int64_t workspace_bytes, float *out_points, int *out_offsets, fnp_stream_t stream);

/* fnp_prepare_points_cut with a window: row i of scene b is tested against the scene's records only when
 * cut_from[b] <= i - off[b] < cut_to[b] (cut_to (B,) int32 device, not NULL; INT32_MAX: to the end of the scene), so rows that
 * unknowns_copy_paste appended behind the scene rows are never cut.  Everything else as fnp_prepare_points_cut. */
int fnp_prepare_points_cut_window(const float *points, int64_t n_points, int num_features, const int *batch_offsets, int batch_size,
                                  const float *program, int program_steps, const float *cut_records, const int *cut_offsets,
                                  const int *cut_from, const int *cut_to, double x_min, double y_min, double x_max, double y_max,
                                  int shuffle_mode, const int *perm, int64_t n_perm, uint64_t seed, float pad,
                                  void *workspace, int64_t workspace_bytes, float *out_points, int *out_offsets, fnp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Multi-sweep assembly in front of fnp_prepare_points — replaces, on the device, NuScenesDataset.get_lidar_with_sweeps and
 * get_sweep (pcdet/datasets/nuscenes/nuscenes_dataset.py:88-121), which the reference runs in numpy inside DataLoader workers.
 * ------------------------------------------------------------------------------------------ */
enum { FNP_SWEEP_DROP_EGO = 1, FNP_SWEEP_TRANSFORM = 2, FNP_SWEEP_FINISHED = 4 /* fnp_assemble_sweeps_window only */ };

int64_t fnp_assemble_sweeps_workspace_bytes(int64_t n_rows);

/* A batch of B scenes holding T sweeps in all (every key frame counts as a sweep).  All arrays on the device:
 * raw (R, 5) f32, 16-byte aligned: the rows of all sweep files as read from disk, sweep after sweep, scene after scene
 *   (column 4, the ring index, is dropped, as the reference's [:, :4] does);
 * sweep_offsets (T+1,) int32: sweep t owns rows [sweep_offsets[t], sweep_offsets[t+1]);
 * scene_sweeps (B+1,) int32: scene b owns sweeps [scene_sweeps[b], scene_sweeps[b+1]);
 * xform (T, 12) f64: rows 0-2 of the sweep's 4x4 matrix, row-major;  flags (T,) int32: FNP_SWEEP_DROP_EGO drops the rows with
 *   |x| < center_radius && |y| < center_radius (both strict, the raw f32 values against the f64 radius), FNP_SWEEP_TRANSFORM
 *   moves x, y, z by xform: fma(m2, z, fma(m1, y, m0*x)) + m3 in f64 (the accumulation of BLAS's dgemm, which numpy's dot
 *   runs for the reference), rounded to f32 once
 *   (a sweep without a matrix does not carry the flag: an identity would turn -0.0 into +0.0);  a key frame carries neither;
 * time_lag (T,) f32: the fifth output column of the sweep's rows.  Intensity passes through.
 * Outputs, the contract of fnp_prepare_points: out_points (R, 5) f32: every scene's kept rows in raw order, scene after scene,
 *   then rows [kept, R) = pad in every column; out_offsets (B+1,) int32: the scene offsets, out_offsets[B] the kept count.
 * No atomics, no host synchronisation, fixed launch sequence for fixed shapes: capturable. */
int fnp_assemble_sweeps(const float *raw, int64_t n_rows, const int *sweep_offsets, int num_sweeps, const int *scene_sweeps,
                        int batch_size, const double *xform, const int *flags, const float *time_lag, double center_radius,
                        float pad, void *workspace, int64_t workspace_bytes, float *out_points, int *out_offsets,
                        fnp_stream_t stream);

/* fnp_assemble_sweeps with finished-row sweeps and a cut window per scene (same workspace, same four launches).
 * FNP_SWEEP_FINISHED: the sweep's rows are finished (x, y, z, intensity, lag) rows — gt-sampled database objects in front of
 *   the scene, pasted objects behind it: all five columns leave as they came, bit for bit; time_lag[t] is not read, and
 *   FNP_SWEEP_DROP_EGO / FNP_SWEEP_TRANSFORM on the same sweep are ignored (the caller should not set them).
 * window_sweeps (B, 2) int32 device: the rows of scene b that gt_sampling's cut may drop are those of the sweeps
 *   [window_sweeps[b][0], window_sweeps[b][1]), sweep indices into the T sweeps, clamped into the scene's own range.
 * out_window (B, 2) int32 device: {kept rows of scene b in front of the window's first raw row, kept rows of scene b in front
 *   of the window's end row}, both relative to out_offsets[b]: the cut_from / cut_to arrays of fnp_prepare_points_cut_window
 *   and fnp_rows_in_boxes as out_window[2 * b] and out_window[2 * b + 1].
 * No atomics, no host synchronisation: capturable. */
int fnp_assemble_sweeps_window(const float *raw, int64_t n_rows, const int *sweep_offsets, int num_sweeps, const int *scene_sweeps,
                               int batch_size, const double *xform, const int *flags, const float *time_lag, double center_radius,
                               float pad, void *workspace, int64_t workspace_bytes, float *out_points, int *out_offsets,
                               const int *window_sweeps, int *out_window, fnp_stream_t stream);

/* The rows inside boxes, compact, for a batch on the device: fnp_host_points_in_boxes_compact for the scenes that
 * fnp_assemble_sweeps leaves on the card (unknowns_copy_paste feeds its queue from them).  All arrays on the device:
 * points (N, 5) f32, 16-byte aligned, and batch_offsets (B+1,) int32: the assembly's output (rows behind batch_offsets[B] are
 *   ignored); num_features must be 5;
 * box_records (T, 8) f32 in the layout of fnp_host_cut_records {cx, cy, cz, dx, dy, dz, cos(-h), sin(-h)} and box_offsets (B+1,)
 *   int32: scene b's boxes are [box_offsets[b], box_offsets[b+1]) and are tested against that scene's rows only, with the
 *   INCLUSIVE test of fnp_host_points_in_boxes_frame (same expressions, f32, uncontracted);
 * the pending cut (num_cut_records == 0: none): cut_records (M, 8), cut_offsets (B+1,), cut_from (B,), cut_to (B,) as
 *   fnp_prepare_points_cut_window takes them; a row with cut_from[b] <= i - batch_offsets[b] < cut_to[b] inside one of the
 *   scene's cut records is left out.
 * Outputs: counts (T,) int32, always complete; total (1,) int32, their sum; indices (capacity,) int32 and rows (capacity, 5) f32:
 *   the first `capacity` rows inside, box after box, in row order inside a box: the scene-relative row index and the RAW row
 *   (the host form returns box-frame rows; the caller makes them).  When total > capacity call again with that size.
 * Deterministic, no atomics, no host synchronisation, fixed launch sequence for fixed shapes: capturable.
 * num_boxes * ceil(N / 256) < 2^31. */
int64_t fnp_rows_in_boxes_workspace_bytes(int64_t n_points, int num_boxes);
int fnp_rows_in_boxes(const float *points, int64_t n_points, int num_features, const int *batch_offsets, int batch_size,
                      const float *box_records, int num_boxes, const int *box_offsets, const float *cut_records,
                      int num_cut_records, const int *cut_offsets, const int *cut_from, const int *cut_to, int64_t capacity,
                      void *workspace, int64_t workspace_bytes, int *counts, int *total, int *indices, float *rows,
                      fnp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Rulebooks — replace spconv's indice-pair generation for SubMConv3d / SparseConv3d
 * (call sites pcdet/models/backbones_3d/spconv_backbone.py:12-17,39-46,193-234).
 * Output-stationary layout: nbr[k*cap + o] = input row feeding output row o through kernel
 * offset k, or -1.
 * ------------------------------------------------------------------------------------------ */
typedef struct fnp_conv_geom {
    int ksize[3];   /* kD,kH,kW */
    int stride[3];
    int padding[3];
    int in_shape[3];  /* D,H,W of the input grid */
    int out_shape[3]; /* D,H,W of the output grid ( = in_shape for SubM ) */
} fnp_conv_geom;

/* SubM: outputs = inputs, same order. */
int fnp_rulebook_subm(const int *coords, const int *n_rows, int cap, const fnp_conv_geom *geom,
                      const fnp_rankgrid *grid, int *nbr, fnp_stream_t stream);

/* Strided SparseConv3d: builds the output rank grid (bits/summary zero on entry; perm unused),
 * the output coordinate list (rows in rank-grid order: spatially blocked, deterministic) and
 * nbr (nullable: only grid + coordinates, for fnp_spconv_forward_strided).  workspace:
 * fnp_rankgrid_workspace_bytes of the output grid. */
int fnp_rulebook_strided(const int *in_coords, const int *n_in, int cap_in, const fnp_conv_geom *geom,
                         const fnp_rankgrid *in_grid, const fnp_rankgrid *out_grid,
                         int *out_coords, int *n_out, int cap_out, int *nbr,
                         void *workspace, int64_t workspace_bytes, fnp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Sparse convolution forward (implicit GEMM, output-stationary, no atomics) with the
 * BatchNorm1d(eval) + residual + ReLU epilogue of spconv_backbone.py:51-67 fused in.
 *   feat_in  (n_in_rows, Cin) in_dtype  weight (K, Cout, Cin) packed, w_dtype = in_dtype
 *   feat_out (n_out, Cout) out_dtype    residual (n_out, Cout) out_dtype or NULL
 *   scale/shift (Cout,) f32 or NULL (identity).  out = act(acc*scale + shift + residual)
 * bf16 x bf16 -> fp32 accumulate runs on MFMA (v_mfma_f32_16x16x32_bf16); f32 x f32 runs on the f32 MFMA
 * (v_mfma_f32_16x16x4_f32: bit for bit the offset-ascending, channel-ascending fmaf chain of the CPU oracle) for the
 * backbone's channel pairs, on VALU fma chains of the same order otherwise.
 * hints: performance only, never changes results.  FNP_HINT_ROWS_RANKED states that neighbour row
 * ids lie close to the output row ids (input and output rows both in rank-grid order, i.e. a
 * SubM convolution on the output of fnp_rulebook_strided): the kernel then keeps a window of
 * input rows in LDS instead of gathering every (site, offset) pair from L2.
 * ------------------------------------------------------------------------------------------ */
#define FNP_HINT_ROWS_RANKED 1
/* f32 only: take the thread-per-element fmaf chain (validation path) instead of the f32 MFMA kernel; the two are
 * bit-identical, this only selects which one computes */
#define FNP_HINT_VALU 2
/* f32 MFMA path only: `weight` is stored with every group of 16 input channels transposed 4 x 4 — position 4q + r of a
 * group holds channel 4r + q (q, r in 0..3) — so that a lane's 16-byte load holds its channels of four consecutive
 * MFMA steps.  Layout statement, not a numerical option: results are bit-identical to the plain layout.  Shapes the
 * f32 MFMA kernel does not cover return FNP_ERR_ARG with this hint (the other kernels read the plain layout). */
#define FNP_HINT_W_PERMUTED 4
int fnp_spconv_forward(const void *feat_in, int in_dtype, int n_in_rows, const void *weight,
                       const int *nbr, int nbr_stride, int K,
                       const int *n_out, int cap_out,
                       void *feat_out, int out_dtype,
                       const float *scale, const float *shift, const void *residual, int relu,
                       int hints, int Cin, int Cout, fnp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The same convolution on a TILE RULEBOOK, for the ranked 16-bit 32 -> 32 and 64 -> 64 layers of 3x3x3 kernels (the SubM
 * convolutions of stages 2 and 3 of VoxelResBackBone8x, spconv_backbone.py:210-219: one rulebook per stage, indice_keys
 * 'subm2' / 'subm3', each used four times per forward).  fnp_tile_rulebook_build restates the (27, cap) int32 table once,
 * per tile of FNP_TILE_ROWS (32 channels) / FNP_TILE64_ROWS (64 channels) output rows, as 16-bit addresses into an LDS
 * image of the tile's neighbourhood (a window of input rows around the tile + up to 256 / 128 far rows, deduplicated) —
 * FNP_TILE_RECORD_BYTES / FNP_TILE64_RECORD_BYTES per tile, 58 bytes per row instead of 108 — and
 * fnp_spconv_forward_tiled sweeps the offsets from LDS alone (64 channels: with the weight slabs streamed).  Bit-identical to fnp_spconv_forward on the int32
 * table for ANY row order; the tiled form is the faster one when rows are in rank-grid order (FNP_HINT_ROWS_RANKED's
 * condition): with the tile rulebook written by fnp_rulebook_subm_tiled, four tiled convolutions + that rulebook were ahead
 * of four gather convolutions + fnp_rulebook_subm from 1 to 64 scenes of the backbone (1-4 % at 1-3 scenes, 10 % at 32-64).
 *   tile_rb  fnp_tile_rulebook_bytes(cap_out, channels) bytes, 16-byte aligned; valid for the (nbr, n_out) it was built from
 *   nbr      the int32 table itself: read only for entries the tile record could not hold (more distinct far rows in a tile than its
 *            image has overflow rows: arbitrary row orders)
 * K must be 27, Cin == Cout == 32 or 64 (the channel count the tile rulebook was built for), dtype FNP_BF16 or FNP_F16 (features, weights, residual and output alike);
 * FNP_ERR_ARG otherwise, and for tensors beyond 32-bit byte offsets.
 * ------------------------------------------------------------------------------------------ */
#define FNP_TILE_ROWS 256            /* 32 channels */
#define FNP_TILE_RECORD_BYTES 14864
#define FNP_TILE64_ROWS 128          /* 64 channels */
#define FNP_TILE64_RECORD_BYTES 7440
/* Diagnostic: the 32-channel kernel hands tile images between its producer and consumer waves through counters in LDS; a
 * wait that times out (2^20 polls, tens of milliseconds; never, unless that protocol is broken) ends the workgroup with
 * wrong output and counts here.  fnp_spconv_tiled_aborts synchronises the device (>= 0, or a negative error code);
 * fnp_spconv_tiled_aborts_copy enqueues a device-to-device copy of the counter (one int32) on `stream`, for a caller that
 * reads it with its other per-forward counts (the host layer raises when it has grown); fnp_debug_tile_hold(1) is the
 * test hook that makes every hand-over time out (producers stop publishing), fnp_debug_tile_hold(0) restores them. */
int fnp_spconv_tiled_aborts(void);
int fnp_spconv_tiled_aborts_copy(int *dst, fnp_stream_t stream);
/* dst[i] = *srcs[i] for n <= 16 one-word device counters (srcs: HOST array of device pointers), the time-out counter above where
 * srcs[i] is NULL: what a forward hands to the host in its one synchronisation, in one launch (capturable).  Bit i of reset_mask:
 * *srcs[i] = 0 after it is read (a counter its owner keeps across forwards, e.g. fnp_rulebook_ell's pool_used). */
int fnp_gather_counts(int *const *srcs, int n, unsigned reset_mask, int *dst, fnp_stream_t stream);
/* The same launch, handing the counts to the HOST itself (ABI 14): besides dst (device) it stores them into host_dst — PINNED host
 * memory of >= FNP_COUNTS_SEQ_SLOT + 1 words, addressed by the device through its host pointer — and then, behind a system-scope fence,
 * ++*seq (a device word the caller zeroed once) into host_dst[FNP_COUNTS_SEQ_SLOT].  A host thread that has counted its launches polls that
 * word and reads the counts when it arrives: no event, no device-to-host copy, and the launch may sit in the MIDDLE of a hipGraph — the
 * captured forward is one graph, its counts leave where they are final (in front of the last SubM stage) and the host sizes the
 * outputs while the rest of the graph runs.  The reference synchronises once per forward where spconv reads its pair counts
 * (pcdet/models/backbones_3d/spconv_backbone.py:193-234 through spconv's indice-pair call). */
#define FNP_COUNTS_SEQ_SLOT 16
int fnp_gather_counts_host(int *const *srcs, int n, unsigned reset_mask, int *dst, int *host_dst, unsigned *seq, fnp_stream_t stream);
int fnp_debug_tile_hold(int on);
long long fnp_tile_rulebook_bytes(int cap_out, int channels);
int fnp_tile_rulebook_build(const int *nbr, int nbr_stride, int K, const int *n_out, int cap_out, int channels,
                            void *tile_rb, fnp_stream_t stream);
/* fnp_rulebook_subm for a 3x3x3 kernel that writes the tile rulebook (for `channels` = 32 or 64) in the same pass: what
 * fnp_rulebook_subm followed by fnp_tile_rulebook_build leaves, without reading the table back. */
int fnp_rulebook_subm_tiled(const int *coords, const int *n_rows, int cap, const fnp_conv_geom *geom,
                            const fnp_rankgrid *grid, int *nbr, int channels, void *tile_rb, fnp_stream_t stream);
/* The same, but the int32 table receives only the rows of tiles whose record holds an escape entry (the only rows
 * fnp_spconv_forward_tiled ever looks up in it; ~1e-5 of the tiles of a rank-ordered tensor): for a caller whose every
 * consumer of this rulebook is fnp_spconv_forward_tiled — the fused inference backbone; the int32 table was 108 of the 166
 * bytes per row this kernel stores.  nbr must still be a (27, cap) buffer; rows outside such tiles stay unwritten. */
int fnp_rulebook_subm_tiled_lean(const int *coords, const int *n_rows, int cap, const fnp_conv_geom *geom,
                                 const fnp_rankgrid *grid, int *nbr, int channels, void *tile_rb,
                                 const fnp_rankgrid *mark_grid, const fnp_conv_geom *mark_geom, int *escape_groups,
                                 fnp_stream_t stream);
/* escape_groups (ABI 10, nullable): a device counter that receives += the number of 32-row groups whose entries hold an escape:
 * the statistic the tiled convolutions' advantage rests on (a group with an escape fetches through the int32 table).  Measured
 * on the synthetic scenes: ~1e-5 of the groups at single-sweep density (tiled kernels 1.15-2.1x the gather kernels), 2 % / 11 %
 * (32 / 64 channels) at the 10-sweep density of transfusion_lidar.yaml (tiled kernels 4-8 % SLOWER): the fused engine reads
 * the counter with its per-forward counts and runs a stage on the gather kernels while it exceeds 0.4 %. */
/* mark_grid / mark_geom (both NULL: none; also on fnp_rulebook_subm_masked): the rows whose rulebook is built are the input
 * sites of the NEXT strided convolution (mark_geom, in_shape = their grid); while the kernel has their coordinates in its
 * registers it also marks that convolution's output sites in mark_grid (all zero on entry), so that
 * fnp_rulebook_strided_premarked — fnp_rulebook_strided without its marking launch — can follow: the separate pass over the
 * coordinates, a chain of dependent loads and atomics per wave, goes.  Geometries with at most two outputs per input cell and
 * axis (ceil(k / s) <= 2); FNP_ERR_ARG otherwise. */
int fnp_rulebook_strided_premarked(const int *in_coords, const int *n_in, int cap_in, const fnp_conv_geom *geom,
                                   const fnp_rankgrid *in_grid, const fnp_rankgrid *out_grid, int *out_coords, int *n_out,
                                   int cap_out, int *nbr, void *workspace, int64_t workspace_bytes, fnp_stream_t stream);
int fnp_spconv_forward_tiled(const void *feat_in, int dtype, int n_in_rows, const void *weight,
                             const void *tile_rb, const int *nbr, int nbr_stride,
                             const int *n_out, int cap_out, void *feat_out,
                             const float *scale, const float *shift, const void *residual, int relu,
                             int Cin, int Cout, fnp_stream_t stream);

/* f32 rows -> two bf16 tensors hi = bf16(x), lo = bf16(x - hi) (ABI 10): hi + lo equals x to 2^-17 of |x|.  The activation
 * format of the fused backbone's "bf16x3" precision (FNP_DTYPE: bf16x3): every convolution is three fnp_spconv_forward launches
 * with f32 outputs chained through `residual` — lo x W_hi, hi x W_lo, hi x W_hi — on the bf16 matrix pipe, the f32 result to
 * ~1e-5 relative.  Rows >= *n_rows are not touched; C a multiple of 4. */
int fnp_split_bf16(const float *x, const int *n_rows, int cap_rows, int C, void *hi, void *lo, fnp_stream_t stream);
/* The same behind y = x + float(t) (t: a bf16 tensor of the same shape; then ReLU if relu != 0), y written as f32 (y == x allowed):
 * where the two cross terms of a bf16x3 convolution were summed in bf16 by the fast bf16-out kernels (they are 2^-8 of the result
 * and need bf16 precision only) and only the main product ran with an f32 output. */
int fnp_split_bf16_add(const float *x, const void *t, int relu, const int *n_rows, int cap_rows, int C, float *y, void *hi,
                       void *lo, fnp_stream_t stream);

/* The bf16x3 engine's MAIN product with the sum and the split in its epilogue (ABI 11): fnp_spconv_forward with 16-bit features and
 * weights and an f32 output,
 *     y = act( conv * scale + shift + residual (f32, nullable) + float(addend) (16-bit rows of the features' dtype, nullable) ),
 * written as f32 rows (feat_out) AND as their split out_hi = 16bit(y), out_lo = 16bit(y - out_hi) — what fnp_spconv_forward (f32 out,
 * no ReLU) followed by fnp_split_bf16_add computes, bit for bit, without the pass over the rows in between (it was 12 % of a
 * bf16x3 forward).  feat_out may be NULL: only the split is written (a layer whose f32 rows nobody reads).  Shapes of the matrix
 * kernel only (FNP_ERR_ARG otherwise).  fnp_spconv_forward_tiled_split: the same on the
 * tile rulebook (fnp_spconv_forward_tiled's arguments and conditions; Cin == Cout == 32 or 64); fnp_spconv_forward_sorted_split:
 * the same as the class-sorted sweep of the 128 -> 128 layers (fnp_spconv_forward_sorted's arguments and conditions). */
int fnp_spconv_forward_split(const void *feat_in, int in_dtype, int n_in_rows, const void *weight, const int *nbr, int nbr_stride,
                             int K, const int *n_out, int cap_out, float *feat_out, const float *scale, const float *shift,
                             const float *residual, const void *addend, int relu, int hints, int Cin, int Cout, void *out_hi,
                             void *out_lo, fnp_stream_t stream);
int fnp_spconv_forward_sorted_split(const void *feat_in, int dtype, int n_in_rows, const void *weight, const int *nbr, int nbr_stride,
                                    const int *perm, const unsigned *blockmask, const int *n_out, int cap_out, float *feat_out,
                                    const float *scale, const float *shift, const float *residual, const void *addend, int relu,
                                    int Cin, int Cout, void *out_hi, void *out_lo, fnp_stream_t stream);
int fnp_spconv_forward_tiled_split(const void *feat_in, int dtype, int n_in_rows, const void *weight, const void *tile_rb,
                                   const int *nbr, int nbr_stride, const int *n_out, int cap_out, float *feat_out,
                                   const float *scale, const float *shift, const float *residual, const void *addend, int relu,
                                   int Cin, int Cout, void *out_hi, void *out_lo, fnp_stream_t stream);

/* COMPACT RULEBOOK for the sparse-neighbourhood layers (conv_input 5 -> 16, the four 16 -> 16 SubM layers, the strided
 * 16 -> 32 layer: spconv_backbone.py:193-210).  A stage-1 voxel has 3.6 of its 27 neighbours, an output site of the first
 * strided layer 2.1 of 27 inputs: the (27, cap) int32 table spends 108 bytes per row on that and the matrix kernel a gather
 * and a matrix step per (16-row block, offset).  fnp_rulebook_ell writes 32 bytes per row instead —
 *     record = 8 x uint32: (k << 27) | input row, ascending k; 0xFFFFFFFF = empty; slot 7 may be (31 << 27) | e = link to
 *     extension record e of a pool behind the cap_rows row records (rows with more than 8 neighbours)
 * — and fnp_spconv_forward_ell sums sum_k W_k^T x over the entries that exist, on the VALU (v_dot2c_f32_bf16 /
 * v_dot2_f32_f16 for 16-bit rows; the oracle's fmaf chain, bit for bit, for the f32 point features of conv_input), with the
 * BatchNorm(eval) scale / shift, residual and ReLU epilogue of fnp_spconv_forward.
 *   records    fnp_ell_bytes(cap_rows, pool_records) bytes, 16-byte aligned
 *   coords     the rows' cells: the tensor's own coordinates (SubM: geom with in_shape == out_shape, stride 1, padding 1) or
 *              the output coordinates of fnp_rulebook_strided(nbr = NULL) (strided 3x3x3: geom as given there)
 *   pool_used  one int32 (device): ends as the number of extension records the rows asked for; above pool_records the
 *              chains were cut and the caller must discard the result and come back with a larger pool.
 *              pool_used_is_zero != 0: the word already holds zero (a counter the caller keeps and has reset when it is read,
 *              fnp_gather_counts): the call does not spend a launch on clearing it
 *   nbr        optional (27, cap) int32 table of the same rows (fnp_rulebook_subm's / fnp_rulebook_strided's), written in the
 *              same pass: measured on MI355X the VALU convolution wins 2.3x on conv_input (5 input channels) and loses 30 %
 *              on the 16-channel layers (256 products per pair are v_dot2c work at a quarter of the FMA rate), so the
 *              backbone reads the records in conv_input and keeps the table for the four 16 -> 16 layers
 * fnp_spconv_forward_ell: K = 27; (in_dtype FNP_F32, Cin 4 or 5, Cout 16, any out_dtype) or (in_dtype = out_dtype = FNP_BF16
 * / FNP_F16, Cin 16, Cout 16 or 32); FNP_ERR_ARG otherwise.  weight: packed (27, Cout, Cin) in in_dtype. */
long long fnp_ell_bytes(int cap_rows, int pool_records);
int fnp_rulebook_ell(const int *coords, const int *n_rows, int cap, const fnp_conv_geom *geom, const fnp_rankgrid *in_grid,
                     void *records, int pool_records, int *pool_used, int pool_used_is_zero, int *nbr, fnp_stream_t stream);
int fnp_spconv_forward_ell(const void *feat_in, int in_dtype, int n_in_rows, const void *weight, const void *records,
                           int cap_rows, int pool_records, const int *n_out, void *feat_out, int out_dtype,
                           const float *scale, const float *shift, const void *residual, int relu, int Cin, int Cout,
                           fnp_stream_t stream);
/* The same call for the 16-input-channel layers (Cin 16, Cout 16 or 32, FNP_BF16 / FNP_F16 in = out) ON THE MATRIX PIPE (ABI 8):
 * the MFMA kernel of fnp_spconv_forward with the entries of a tile's rows expanded from the records into LDS at the top of
 * the tile — no (27, cap) table is written or read (108 of the ~170 bytes a row of those layers moves), no entry load shares
 * the gathers' in-order queue.  Values: fnp_spconv_forward's on the table of the same rows, bit for bit. */
int fnp_spconv_forward_ell_mfma(const void *feat_in, int in_dtype, int n_in_rows, const void *weight, const void *records,
                                int cap_rows, int pool_records, const int *n_out, void *feat_out, int out_dtype,
                                const float *scale, const float *shift, const void *residual, int relu, int Cin, int Cout,
                                fnp_stream_t stream);

/* CLASS-SORTED sweep of the 128 -> 128 SubM layers (the four 3x3x3 convolutions of stage 4, spconv_backbone.py:219-224).
 * After three stride-2 layers a lidar surface is two cells thick: ~36 % of the stage-4 sites have neighbours only in the
 * plane above, ~36 % only in the plane below.  fnp_rulebook_classsort orders the rows each persistent workgroup of the
 * convolution sweeps concurrently by that class (once per forward; the four convolutions share it): perm[position] = row, and
 * blockmask[position / 16] = union of the 27-bit neighbour masks of 16 consecutive positions.  fnp_spconv_forward_sorted
 * then sweeps, per tile, only the kernel offsets some row of the tile has a neighbour at (on lidar scenes 20 % of the
 * (tile, offset) pairs go, with their slab loads, barriers, gathers and matrix work); every row still sums its own
 * neighbours in ascending offset order, so the values equal fnp_spconv_forward's.
 * The convolution's workgroups that share an XCD (blocks b, b + 8, ...) own one contiguous run of rows together and take
 * its tiles round-robin; the sort orders the rows of each ROUND of tiles, so that the tiles in flight on an XCD cover one
 * contiguous region of the feature map (its L2) and all but the two or three tiles at the class boundaries are of one class.
 *   rowmask    (cap_out) uint32, bit k = row has a neighbour at offset k: written by fnp_rulebook_subm_masked (the SubM
 *              rulebook kernel with that one extra store per row); NULL: classsort derives it from nbr into `workspace`
 *              (fnp_classsort_workspace_bytes(cap_out) bytes)
 *   perm       (cap_out) int32, blockmask (cap_out / 16 + 1) uint32: written by classsort, read by the convolution; valid
 *              for the (nbr, n_out, cap_out) they were built from
 * K must be 27, (Cin, Cout) = (128, 128), dtype FNP_BF16 or FNP_F16 for features, weights, residual and output alike;
 * FNP_ERR_ARG otherwise. */
long long fnp_classsort_workspace_bytes(int cap_out);
int fnp_rulebook_subm_masked(const int *coords, const int *n_rows, int cap, const fnp_conv_geom *geom,
                             const fnp_rankgrid *grid, int *nbr, unsigned *rowmask,
                             const fnp_rankgrid *mark_grid, const fnp_conv_geom *mark_geom, fnp_stream_t stream);
int fnp_rulebook_classsort(const int *nbr, int nbr_stride, int K, const unsigned *rowmask, const int *n_out, int cap_out, int Cin, int Cout,
                           int *perm, unsigned *blockmask, void *workspace, long long workspace_bytes, fnp_stream_t stream);
int fnp_spconv_forward_sorted(const void *feat_in, int dtype, int n_in_rows, const void *weight, const int *nbr, int nbr_stride,
                              const int *perm, const unsigned *blockmask, const int *n_out, int cap_out, void *feat_out,
                              const float *scale, const float *shift, const void *residual, int relu, int Cin, int Cout,
                              fnp_stream_t stream);

/* The f32 engine's form of the class sort (the f32 3x3x3 SubM layers, 16 / 32 / 64 / 128 channels, run on v_mfma_f32_16x16x4_f32
 * and are bound by the matrix pipe; the kernel skips the MFMAs of a (16-row block, offset) pair without any neighbour).
 * fnp_rulebook_classsort_f32 orders the rows of every workgroup range of that kernel's grid by class (perm (cap_out) int32;
 * rowmask as written by fnp_rulebook_subm_masked), fnp_spconv_forward_f32_sorted sweeps the ranges in that order.  Cin == Cout;
 * wperm != 0: weight in the 4 x 4-transposed layout (FNP_HINT_W_PERMUTED).  Bit-identical to fnp_spconv_forward on f32. */
int fnp_rulebook_classsort_f32(const unsigned *rowmask, const int *n_out, int cap_out, int Cin, int Cout, int *perm, fnp_stream_t stream);
int fnp_spconv_forward_f32_sorted(const void *feat_in, int n_in_rows, const void *weight, const int *nbr, int nbr_stride, const int *perm,
                                  const int *n_out, int cap_out, void *feat_out, const float *scale, const float *shift,
                                  const void *residual, int relu, int wperm, int Cin, int Cout, fnp_stream_t stream);

/* The same convolution for a STRIDED 3x3x3 layer whose rulebook has no other user (the three down-sampling
 * layers of VoxelResBackBone8x, spconv_backbone.py:207,214,221): the kernel computes the rulebook rows of its
 * tiles itself from the input rank grid and the output coordinates (fnp_rulebook_strided with nbr = NULL builds
 * those), so no (27, cap) table is written and read back.  bf16 in/out, (Cin, Cout) in {(16,32), (32,64),
 * (64,128)}; FNP_ERR_ARG otherwise (take the table path).  Results are identical to the table path. */
int fnp_spconv_forward_strided(const void *feat_in, int in_dtype, int n_in_rows, const void *weight,
                               const fnp_rankgrid *in_grid, const fnp_conv_geom *geom, const int *out_coords,
                               const int *n_out, int cap_out, void *feat_out, int out_dtype,
                               const float *scale, const float *shift, int relu, int Cin, int Cout,
                               fnp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Backward of the sparse convolution (spconv's autograd behind SubMConv3d / SparseConv3d in the
 * self-training step, tools/train_st.py; modules at spconv_backbone.py:12-17,39-46).
 *   dgrad: dx[i] = sum_k W_k dy[nbrT[k][i]] = fnp_spconv_forward on the transposed rulebook with the
 *          transposed slabs (weight (K, Cin, Cout) passed as (K, "Cout"=Cin, "Cin"=Cout)).
 *   fnp_rulebook_transpose: nbr (K, nbr_stride) over output rows -> nbr_t (K, cap_in) over input rows
 *          (nbr_t[k][i] = o iff nbr[k][o] = i, else -1).
 *   fnp_spconv_wgrad: grad_weight (K, Cout, Cin) f32 = sum_o grad_out[o] (x) feat_in[nbr[k][o]];
 *          deterministic (per-chunk partials in `workspace`, added in chunk order).
 * ------------------------------------------------------------------------------------------ */
int fnp_rulebook_transpose(const int *nbr, int nbr_stride, int K, const int *n_out, int cap_out,
                           int *nbr_t, int cap_in, fnp_stream_t stream);
int64_t fnp_spconv_wgrad_workspace_bytes(int K, int Cin, int Cout);
int fnp_spconv_wgrad(const void *feat_in, int in_dtype, const void *grad_out, int grad_dtype,
                     const int *nbr, int nbr_stride, int K, const int *n_out, int cap_out,
                     float *grad_weight, int grad_layout, int Cin, int Cout,
                     void *workspace, int64_t workspace_bytes, fnp_stream_t stream);
/* grad_layout (ABI 9): 0 = grad_weight is the packed (K, Cout, Cin), 1 = the module parameter's (Cout, K, Cin) (the final
 * reduction writes the .grad tensor itself: no permute-copy per layer afterwards).
 * fnp_pack_weight: the module's f32 weight (Cout, K, Cin) -> the packed (K, Cout, Cin) slabs in `dtype`, and in the same launch
 * the slabs the data gradient of a SubM layer reads: mirror_mode 1 = (K-1-k, Cout, Cin) for fnp_spconv_dgrad on the forward's
 * table (which transposes them itself), 2 = (K-1-k, Cin, Cout): the forward kernel run on the gradient of a SubM layer, 3 =
 * (k, Cin, Cout): the same for a strided layer on its transposed table (fnp_rulebook_transpose); 0 = none (mirror NULL). */
int fnp_pack_weight(const float *weight, int Cout, int K, int Cin, int dtype, void *packed, void *mirror, int mirror_mode,
                    fnp_stream_t stream);
/* the same for count <= 32 layers in one launch (host arrays of device pointers and shapes; one dtype for all) */
int fnp_pack_weight_multi(int count, const float *const *weights, const int *couts, const int *ks, const int *cins, int dtype,
                          void *const *packed, void *const *mirrors, const int *mirror_modes, fnp_stream_t stream);
/* PAIR LISTS of a rulebook (ABI 8), for the weight gradient: offset k only sums over the output rows that HAVE a neighbour
 * at k (44-54 % of the rows on lidar scenes); fnp_rulebook_pairs compacts every column of the table once per rulebook —
 * pair_o[k][j] = the j-th such output row (ascending), pair_i[k][j] = its neighbour, pair_count[k] — and
 * fnp_spconv_wgrad_pairs runs fnp_spconv_wgrad's sum over them (16-bit features and gradients, the MFMA channel pairs;
 * FNP_ERR_ARG otherwise: take fnp_spconv_wgrad).  pair_o / pair_i: (K, pair_stride) int32, pair_stride >= cap_out = the rows the
 * caller knows to exist (not the table's stride: a strided layer's table is sized for 27 outputs per input); order-preserving. */
int64_t fnp_rulebook_pairs_workspace_bytes(int K, int cap_out);
int fnp_rulebook_pairs(const int *nbr, int nbr_stride, int K, const int *n_out, int cap_out, int *pair_o, int *pair_i,
                       int pair_stride, int *pair_count, void *workspace, int64_t workspace_bytes, fnp_stream_t stream);
int fnp_spconv_wgrad_pairs(const void *feat_in, int in_dtype, const void *grad_out, int grad_dtype, const int *pair_o,
                           const int *pair_i, const int *pair_count, int pair_stride, int K, const int *n_out, int cap_out,
                           float *grad_weight, int grad_layout, int Cin, int Cout, void *workspace, int64_t workspace_bytes,
                           fnp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * BatchNorm1d in TRAINING mode on sparse rows, fused with the ReLU / residual add that follow it in post_act_block and
 * SparseBasicBlock (pcdet/models/backbones_3d/spconv_backbone.py:8-27,51-67; norm_fn = BatchNorm1d(eps 1e-3, momentum
 * 0.01), :189) — forward and backward of the dense part of the self-training step (tools/train_st.py).
 *   x, residual, y, grad_* : (cap, C) rows of `dtype` (f32 / bf16 / fp16), C in {8, 16, 32, 64, 128, 256}; the n_rows valid
 *   rows (DEVICE scalar) form the batch.  gamma, beta, running_*, save_*, grad_gamma, grad_beta: (C,) f32.
 *   forward : y = act((x - mean) * invstd * gamma + beta [+ residual]); biased variance for the normalisation, running
 *             statistics updated in place like torch (momentum, unbiased variance); running_* may both be NULL.
 *   backward: g = grad_out * [y > 0] (relu) ; grad_beta = sum g ; grad_gamma = sum g * xhat ;
 *             grad_x = gamma * invstd * (g - grad_beta / n - xhat * grad_gamma / n) ; grad_residual (nullable) = g.
 * Two passes per direction, f64 partial sums added in a fixed order: deterministic, no atomics, no host sync.
 * workspace: fnp_bn_workspace_bytes(C).
 * ------------------------------------------------------------------------------------------ */
int64_t fnp_bn_workspace_bytes(int C);
int fnp_bn_train_forward(const void *x, int dtype, const int *n_rows, int cap, int C, const float *gamma, const float *beta,
                         float *running_mean, float *running_var, float momentum, float eps, const void *residual, int relu,
                         void *y, float *save_mean, float *save_invstd, long long *num_batches_tracked, void *workspace,
                         int64_t workspace_bytes, fnp_stream_t stream);
/* num_batches_tracked (ABI 9, nullable): nn.BatchNorm1d's int64 counter, advanced by one on the device with the statistics. */
int fnp_bn_train_backward(const void *grad_out, const void *x, const void *y, int dtype, const int *n_rows, int cap, int C,
                          const float *gamma, const float *save_mean, const float *save_invstd, int relu, void *grad_x,
                          void *grad_residual, float *grad_gamma, float *grad_beta, void *workspace, int64_t workspace_bytes,
                          fnp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * BatchNorm2d in TRAINING mode + ReLU on rows that stand for a dense map (csrc/bev_bn.hip): the tail of the first
 * BaseBEVBackbone block (pcdet/models/backbones_2d/base_bev_backbone.py:31-40) behind a bias-free convolution that ran on
 * sparse rows.  Additive in ABI 14.
 *   x, grad_x : (cap, C) rows of `dtype` (f32 / bf16 / fp16) on the sites coords (cap, 4) [b, 0, y, x], unique and inside
 *   the (B, H, W) grid; the n_rows valid rows (DEVICE scalar) are the cells that hold a value, every other of the
 *   N = B * H * W cells holds 0 and COUNTS in the batch.  y, grad_out: (B, C, H, W) of `dtype`, contiguous.
 *   gamma, beta, running_*, save_*, fill, grad_gamma, grad_beta: (C,) f32.  C a power of two in [8, 256] whose 64 rows fit
 *   64 KB of LDS (C = 256: 16-bit rows only); anything else returns FNP_ERR_ARG.
 *   forward : mean = sum_r x / N, var = sum_r x^2 / N - mean^2 (biased, f64), invstd = 1 / sqrt(var + eps); running
 *             statistics like torch (momentum, var * N / (N - 1); both may be NULL); num_batches_tracked (nullable) += 1;
 *             fill_c = relu((0 - mean) * invstd * gamma + beta), the f32 sequence of a row with x = 0;
 *             y = relu((x - mean) * invstd * gamma + beta) at the row cells, fill_c elsewhere, every element written once.
 *   backward: g = grad_out * [y > 0] (row cells: y recomputed from x by the forward's f32 sequence and rounded to `dtype`,
 *             the bits the forward stored; other cells: fill_c > 0);  T = sum over all cells of grad_out, R = over row cells;
 *             grad_beta = sum_rows g + [fill > 0] (T - R);  grad_gamma = sum_rows g xhat + [fill > 0] xhat_bg (T - R),
 *             xhat_bg = (0 - mean) * invstd;  grad_x[r] = gamma * invstd * (g_r - grad_beta / N - xhat_r grad_gamma / N)
 *             for r < n and 0 for n <= r < cap (every row is written).
 * f64 partial sums added in a fixed order by a finishing launch: no atomics, bit-identical from run to run; no host
 * synchronisation, no allocation, capturable.  5 launches forward, 6 backward.  workspace: fnp_bev_bn_workspace_bytes()
 * (cell -> row map + partials), rebuilt by each call.
 * ------------------------------------------------------------------------------------------ */
int64_t fnp_bev_bn_workspace_bytes(int C, int B, int H, int W);
int fnp_bev_bn_train_forward(const void *x, int dtype, const int *coords, const int *n_rows, int cap, int C, int B, int H,
                             int W, const float *gamma, const float *beta, float *running_mean, float *running_var,
                             float momentum, float eps, void *y, float *save_mean, float *save_invstd, float *fill,
                             long long *num_batches_tracked, void *workspace, int64_t workspace_bytes, fnp_stream_t stream);
int fnp_bev_bn_train_backward(const void *grad_out, const void *x, int dtype, const int *coords, const int *n_rows, int cap,
                              int C, int B, int H, int W, const float *gamma, const float *beta, const float *save_mean,
                              const float *save_invstd, const float *fill, void *grad_x, float *grad_gamma, float *grad_beta,
                              void *workspace, int64_t workspace_bytes, fnp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * CLIP-crop scoring, geometry half (CLIPBoxClassification.forward,
 * pcdet/models/dense_heads/clip_box_classification.py:230-379): which camera sees which box and the
 * square image crop CLIP looks at.
 *   fnp_clipcrop_plan: boxes (N,7) device; lidar_aug_rot_inv (9) and lidar_aug_trans (3) HOST floats
 *       (torch.inverse of the augmentation rotation is the caller's, like the reference :205-207);
 *       lidar2image, img_aug (6,4,4) device -> rect (N,6,4) f32 [x1, y1, side, has_crop] and
 *       cam_mask (N,6) u8 (box visible in the camera, set even when the crop is < min_crop px).
 *   fnp_clipcrop_sample: images (6, C, H, W) f32/f16 device, pairs (M,2) i32 [box, cam] in the caller's
 *       order, unit_grid (out_size) f32 = the [0,1] sampling positions (F.affine_grid normalised as in
 *       :318-319) -> crops (M, C, out_size, out_size), F.grid_sample arithmetic (bilinear,
 *       align_corners = False, zeros padding).
 * ------------------------------------------------------------------------------------------ */
int fnp_clipcrop_plan(const float *boxes, int n, const float *lidar_aug_rot_inv, const float *lidar_aug_trans,
                      const float *lidar2image, const float *img_aug, int image_h, int image_w, int min_crop,
                      float *rect, unsigned char *cam_mask, fnp_stream_t stream);
int fnp_clipcrop_sample(const void *images, int dtype, int channels, int image_h, int image_w,
                        const float *rect, const int *pairs, int num_pairs, const float *unit_grid,
                        int out_size, void *crops, fnp_stream_t stream);

/* SparseConvTensor.dense() as used by HeightCompression (height_compression.py:20-24):
 * feats (n,C) -> out (B,C,D,H,W) of the same dtype (FNP_F32, FNP_BF16 or FNP_F16) (viewed as (B, C*D, H, W) by the caller).
 * With a workspace of fnp_sparse_to_dense_workspace_bytes() (a cell -> row map) every element of
 * `out` is written exactly once, zeros included, in 128-byte segments: `out` need not be zeroed.
 * With workspace == NULL a row-driven scatter runs and `out` must be zero on entry. */
int64_t fnp_sparse_to_dense_workspace_bytes(int B, int D, int H, int W);
int fnp_sparse_to_dense(const void *feats, int dtype, const int *coords, const int *n_rows, int cap,
                        int C, int B, int D, int H, int W, void *out,
                        void *workspace, int64_t workspace_bytes, fnp_stream_t stream);
/* The same with a per-channel value (fill: C floats, device) for the cells WITHOUT a row instead of 0: the dense map behind
 * a convolution whose epilogue gives unreached cells a constant — relu(BatchNorm shift) — i.e. the output of the first
 * BaseBEVBackbone block (base_bev_backbone.py:31-40) evaluated on the sparse rows.  Needs the workspace. */
int fnp_sparse_to_dense_fill(const void *feats, int dtype, const int *coords, const int *n_rows, int cap, int C,
                             int B, int D, int H, int W, void *out, const float *fill, void *workspace,
                             int64_t workspace_bytes, fnp_stream_t stream);
/* The adjoint of fnp_sparse_to_dense (the backward of SparseConvTensor.dense() / HeightCompression): grad_out (B,C,D,H,W),
 * contiguous -> grad_feats (cap, C), both of `dtype` (FNP_F32, FNP_BF16 or FNP_F16, as the two calls above).  A row r < n
 * whose (b, z, y, x) lies in the grid gets grad_out[b, :, z, y, x], copied bit for bit; every other row (r >= n, or outside
 * the grid) gets 0.  Every row of grad_feats is written (it need not be zeroed); grad_out is read only inside its bounds.
 * No host synchronisation, no atomics, capturable.  The workspace (fnp_sparse_to_dense_workspace_bytes()) is rebuilt by the
 * call itself as the cell -> row map: the plane-tiled gather reads each element of an occupied 64*VEC-cell tile at most once;
 * workspace == NULL (or a row size the tile kernel does not take: C * sizeof(T) not a multiple of 4) runs a row-driven
 * gather.  Coordinates must be unique per site (spconv's contract); duplicates are memory-safe only. */
int fnp_sparse_to_dense_backward(const void *grad_out, int dtype, const int *coords, const int *n_rows, int cap, int C,
                                 int B, int D, int H, int W, void *grad_feats, void *workspace,
                                 int64_t workspace_bytes, fnp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Greedy Box Seeker — replaces hot loops 2-4 of FrustumProposerOG.get_proposals
 * (pcdet/models/dense_heads/frustum_proposals_v1.py:593-1048) for topk = 1: per 2D detection
 * ("frustum") select the points inside the 2D box, take the depth quantiles, build the frustum,
 * generate num_mags x num_rotations x num_sizes candidate boxes, score them by 2D IoU of their
 * projected corners and by point density, return the best one.  One launch for all frustums of
 * a batch of scenes; no host synchronisation.
 * ------------------------------------------------------------------------------------------ */
typedef struct fnp_seeker_params {
    float lq, uq, cq;            /* depth quantiles: frustum near, far, centre (PARAMS lq/uq/cq) */
    float iou_w, dst_w, dns_w;   /* score weights (:997) */
    float min_cam_iou;           /* :904 */
    float max_dist;              /* :871, also caps the frustum depth (:647) */
    int num_mags, num_rotations, num_sizes;
    int topk;                    /* boxes per frustum: the first topk of the 3D NMS in score order (:1030-1045); >= 1 */
    int clamp_bottom;            /* :817 */
    int image_h, image_w;        /* 900, 1600 (:205) */
    int point_stride;            /* floats per point row */
    int xyz_offset;              /* column of x in a point row */
    int has_img_aug;             /* cam_mats carries a non-identity img_aug_matrix (:1456-1458, :1525-1527) */
    int mult;                    /* MODEL_CFG.MULT: product instead of sum of the score terms (:997-1000) */
    float ego_w;                 /* PARAMS ego_w: + ego_w * ||centre|| / max ||centre|| (:1017-1021) */
    /* ABI 8 — the options no shipped configuration sets (:154-196) */
    float nms_normal;            /* threshold of that NMS on the axis-aligned BEV footprints (nms_normal_gpu, :1030) */
    float search_depth;          /* > 0: frustum far plane = near quantile + search_depth, search axis of that length (:617-622,:841) */
    float occl_w;                /* + occl_w * (1 - occl / max occl), occl = calc_occl_scores as it runs (:1007-1014, :408-477) */
    int occl_mult;               /* MODEL_CFG.OCCL_MULT: score = density * IoU * occl (:1022-1027) */
    int multicam;                /* MODEL_CFG.MULTICAM_IOU: IoU averaged over the cameras of the scene's same-label frustums (:885, :1413) */
    int count_only;              /* pre-pass of multicam: only dbg_npts (points per frustum) is written */
    int num_frustums;            /* rows of npts_all (= num_frustums of the call) */
    const int *npts_all;         /* multicam: points per frustum from the count_only pre-pass (device) */
    const float *rand_noise;     /* rand_center (:847): (num_frustums, num_mags, 3) draws added to the weighted centre, or NULL */
} fnp_seeker_params;

int64_t fnp_boxseeker_workspace_bytes(int num_frustums, int max_points_per_scene);

/* scene_mats (S,21) / cam_mats (S,6,45) of fnp_boxseeker made ON THE DEVICE (ABI 8) from the batch's own device tensors —
 * lidar_aug (S,4,4), lidar2image / camera2lidar / intrinsics (S,6,4,4), img_aug (S,6,4,4) or NULL (identity) — the matrix
 * algebra of project_to_camera / get_geometry_at_image_coords (frustum_proposals_v1.py:1431-1475, :1509-1545; the reference
 * calls torch.inverse on 3x3 blocks: here a Gauss-Jordan elimination with partial pivoting in f32).  No host copy, no sync. */
int fnp_seeker_prepare_matrices(const float *lidar_aug, const float *lidar2image, const float *camera2lidar,
                                const float *intrinsics, const float *img_aug, int num_scenes, float *scene_mats,
                                float *cam_mats, fnp_stream_t stream);

/* HOST function (all pointers are host memory, no GPU work): frustum enumeration of :561-594 —
 * per scene, per camera in image_order, torchvision.batched_nms (coordinate trick, f32) on the
 * 2D detections, then the score threshold.  boxes (D,4) xyxy f32, labels/batch_idx/cam_idx (D,)
 * int64, scores (D,) f32 (the CPU tensors PreprocessedGLIP returns, preprocessed_detector.py:47-101).
 * rows (max_rows,8) f32 receives [scene, cam, x1, y1, x2, y2, label, score]; returns the number
 * of rows or a negative error code. */
int fnp_host_enumerate_frustums(const float *boxes, const int64_t *labels, const float *scores,
                                const int64_t *batch_idx, const int64_t *cam_idx, int num_dets,
                                int num_scenes, const int *image_order, int num_cams,
                                float nms_thr, float score_thr, float *rows, int max_rows);

/* points: rows of `point_stride` floats, scenes concatenated; scene_offsets (S+1,) int32.
 * scene_mats (S,21) f32: lidar_aug rotation (9, row major) | its inverse (9) | translation (3).
 * cam_mats (S,6,45) f32: lidar2image[:3,:3] (9) | lidar2image[:3,3] (3) |
 *                        camera2lidar_rot @ inv(intrinsics) (9) | camera2lidar_trans (3) |
 *                        img_aug[:3,:3] (9) | img_aug[:3,3] (3) | inv(img_aug[:3,:3]) (9)   (the last 21 are read only
 *                        when params->has_img_aug)
 *                        (the matrices of :1431-1475 and :1509-1545, prepared on the host).
 * frustums (F,8) f32: scene, camera, x1, y1, x2, y2, label (1-based), score — already NMS'ed,
 *                        score-filtered and in the reference's enumeration order (:582-594).
 * base_boxes (10,R,7), base_corners (10,R,8,3), R = num_rotations*num_sizes (:284-298); mags (num_mags,).
 * Outputs per frustum: out_valid (number of boxes, 0 .. topk), out_box (topk, 7), out_score (topk: second-stage
 * scores), out_best (topk: candidate indices, -1 past out_valid).  dbg_* are optional (NULL) per-candidate dumps:
 * dbg_npts (F), dbg_frust (F,8,3), dbg_cand (F,NC,7), dbg_iou (F,NC), dbg_count (F,NC),
 * dbg_valid (F,NC: 0 dropped by max_dist, 1 dropped by min_cam_iou, 2 scored). */
int fnp_boxseeker(const float *points, const int *scene_offsets, int num_scenes, int max_points_per_scene,
                  const fnp_seeker_params *params, const float *scene_mats, const float *cam_mats,
                  const float *frustums, int num_frustums,
                  const float *base_boxes, const float *base_corners, const float *mags,
                  void *workspace, int64_t workspace_bytes,
                  int *out_valid, float *out_box, float *out_score, int *out_best,
                  int *dbg_npts, float *dbg_frust, float *dbg_cand, float *dbg_iou, int *dbg_count, int *dbg_valid,
                  fnp_stream_t stream);

/* Exchange records of the sharded extraction (BASELINE.json configs[3]; the reference gathers pickled objects or files,
 * pcdet/utils/commu_utils.py:50-111, common_utils.py:229-250): packs the fnp_boxseeker outputs of a batch of scenes
 * into records (num_scenes, rows_per_scene, 9) f32 — row 0 = [count, tags[scene], 0 ...], rows 1.. =
 * [box (7), 2D detection score, label] of the scene's frustums with out_valid != 0, in frustum order; all other rows
 * zero.  frustums / out_valid / out_box as in fnp_boxseeker (device); tags: HOST floats (num_scenes <= 64). */
int fnp_seeker_pack_records(const float *frustums, const int *out_valid, const float *out_box, int num_frustums,
                            const float *tags, int num_scenes, int rows_per_scene, float *records, fnp_stream_t stream);

/* Dense heatmap targets and heatmap loss of TransFusionHead (transfusion_head.py:446-470, :492-498; additive, ABI 14).
 * All three steps take a stream, allocate nothing and do not synchronise.
 *
 * fnp_heatmap_box_params: gt_boxes (B, M, ncol) f32, x y z dx dy dz ... label (last column, 1-based, 0 = padding) ->
 * out_params (B, M, 4) int32 {class (0-based), cx, cy, r}, 16-byte aligned.  class = -1 marks a skipped box: dx or dy <= 0, a
 * non-finite x, y, dx or dy, or a label outside 1..num_classes (the reference raises on a label above num_classes and wraps
 * on one below 1; both are out of contract here).  voxel_*, range_* are voxel_size[0:2] and point_cloud_range[0:2] rounded to
 * f32; overlap = GAUSSIAN_OVERLAP, min_radius = MIN_RADIUS; unknown_mask has bit (label - 1) set for every 1-based label in
 * unknown_labels (0 when use_pseudo is off), whose radius becomes int(r * unknown_mult) in f64.  The arithmetic is the
 * reference's as torch runs it on the CPU, bit for bit.  A radius is clamped to 2^20 and a centre to +-2^30 cells.
 *
 * fnp_heatmap_draw: params as above -> heatmap (B, C, H, W) f32 (H along y, W along x), every element written exactly once
 * (no clear pass, no atomics, independent of box order), and num_pos (1) int32 = the number of elements equal to 1.
 * workspace: fnp_heatmap_draw_workspace_bytes(B, C, H, W), 4-byte aligned.
 *
 * fnp_heatmap_loss_forward: loss (1) f32 = sum(GaussianFocalLoss(alpha 2, gamma 4)(clip_sigmoid(logits), target)) /
 * max(*num_pos, 1).  logits: n values of `dtype` (FNP_F32, FNP_F16, FNP_BF16), upcast exactly and NOT modified (the
 * reference's sigmoid_ overwrites them); target n f32; arithmetic in f32, the sum in f64 in a fixed order: bit-identical from
 * run to run.  workspace: fnp_heatmap_loss_workspace_bytes(n), 8-byte aligned.
 * fnp_heatmap_loss_backward: grad_logits (n, `dtype`) = dT/dlogit * (*grad_out / max(*num_pos, 1)), recomputed from logits
 * and target; exactly 0 where the sigmoid lies outside the clamp. */
int fnp_heatmap_box_params(const float *gt_boxes, int batch_size, int max_boxes, int ncol, int num_classes, float voxel_x,
                           float voxel_y, int stride, float range_x, float range_y, double overlap, int min_radius,
                           uint64_t unknown_mask, double unknown_mult, int *out_params, fnp_stream_t stream);
int64_t fnp_heatmap_draw_workspace_bytes(int batch_size, int num_classes, int height, int width);
int fnp_heatmap_draw(const int *params, int batch_size, int max_boxes, int num_classes, int height, int width,
                     void *workspace, int64_t workspace_bytes, float *heatmap, int *num_pos, fnp_stream_t stream);
int64_t fnp_heatmap_loss_workspace_bytes(int64_t n);
int fnp_heatmap_loss_forward(const void *logits, int dtype, const float *target, int64_t n, const int *num_pos,
                             void *workspace, int64_t workspace_bytes, float *loss, fnp_stream_t stream);
int fnp_heatmap_loss_backward(const void *logits, int dtype, const float *target, int64_t n, const int *num_pos,
                              const float *grad_out, void *grad_logits, fnp_stream_t stream);

/* Inference side of TransFusionHead around its decoder (transfusion_head.py:201-324 and :616-728; additive, ABI 14).  Every
 * call takes a stream, allocates nothing and does not synchronise; all tensors are f32 unless stated.
 *
 * fnp_proposals: heatmap (B, C, H, W), logits when from_logits != 0 (the sigmoid is fused: 1.0f / (1.0f + expf(-x)), not
 * contracted, no fast-math) and probabilities >= 0 otherwise -> top_class, top_index (B, K) int64, top_score (B, K) and
 * query_heatmap_score (B, C, K).  1 <= C <= 64, 1 <= K <= min(2048, C*H*W), C*H*W < 2^31.
 *   1. Masked value.  s = the probability.  An ordinary class keeps s at an interior cell where s equals the maximum of its
 *      3 x 3 neighbourhood, and is 0 elsewhere, border cells included (NMS_KERNEL_SIZE is 3; the caller asserts it).
 *   2. Point classes, bit c of point_class_mask, keep s at every cell, border included.
 *   3. Order: masked value descending, then flat index c*H*W + h*W + w ascending.  The reference's argsort is not stable, so
 *      among tied values the rule is this library's; where values are distinct it is the reference's order.
 *   4. Zero fill.  Masked-out cells take part with value 0: with P < K positive cells, the remaining K - P places go to the
 *      lowest flat indices that are no positive cell, ascending (all of them below K).
 *   5. top_class = flat / (H*W), top_index = flat % (H*W), top_score = the masked value.
 *   6. query_heatmap_score[b, c, k] = the masked value of class c at top_index[b, k], from the same device function as the
 *      selecting pass.
 *   7. Finite values and +-inf are in contract; NaN is out of contract (a NaN cell is never selected as positive, and may
 *      spoil its neighbours' maxima).  Results are bit-identical from run to run.
 * workspace: fnp_proposals_workspace_bytes(B, C, H, W, K) bytes, 8-byte aligned (negative: the shape is out of contract).
 *
 * fnp_query_init: query_feat[b, f, k] = lidar_feat[b, f, top_index[b, k]] + (enc_weight[f, top_class[b, k]] + enc_bias[f]),
 * in that association (the one-hot Conv1d class encoding), and query_pos[b, k, :] = bev_pos[top_index[b, k], ::-1], gathered
 * from the caller's table: bev_pos is (num_cells, 2), or (B, num_cells, 2) when bev_pos_batched != 0.  lidar_feat
 * (B, F, num_cells), F >= 2; enc_weight (F, C); outputs (B, F, K) and (B, K, 2).  An index or class outside its range yields
 * NaN and is never followed.
 *
 * fnp_tf_decode: get_bboxes + decode_bbox(filter=True).  heatmap (logits) and query_heatmap_score (B, C, K), center (B, 2, K),
 * height (B, 1, K), dim (B, 3, K), rot (B, 2, K: sin, cos), vel (B, 2, K) or NULL, query_labels (B, K) int64.  Per query, with
 * q = query_labels[b, k]: v = sigmoid(heatmap[b, q, k]) * query_heatmap_score[b, q, k]; label = q when v > 0, else 0 (the
 * reference's maximum over an all-zero column); x = center_x * stride * voxel_x + range_x in f32, two multiplications and
 * one addition, not contracted (y alike); z = height; sizes exp(dim); yaw atan2(sin, cos); the score, the sizes and the yaw
 * are formed in f64 and rounded once to f32 (closer to the true value than expf / atan2f).  A query is kept when
 * score > score_thresh (score_thresh_unk when bit `label` of unknown_mask is set, i.e. the 1-based label is an unknown
 * class) and post_center_range[0:3] <= (x, y, z) <= post_center_range[3:6] (a HOST array of 6 floats), all in f32.  Kept rows are written
 * per scene in query order: boxes (B, K, 7 or 9), scores (B, K), labels (B, K) int32 = label + 1, mapped through relabel
 * (C + 1 int32 on the device, or NULL); counts (B) int32; the rows behind a scene's count are zero. */
int64_t fnp_proposals_workspace_bytes(int batch_size, int num_classes, int height, int width, int num_proposals);
int fnp_proposals(const float *heatmap, int batch_size, int num_classes, int height, int width, int num_proposals,
                  int from_logits, uint64_t point_class_mask, void *workspace, int64_t workspace_bytes, int64_t *top_class,
                  int64_t *top_index, float *top_score, float *query_heatmap_score, fnp_stream_t stream);
int fnp_query_init(const float *lidar_feat, const float *bev_pos, int bev_pos_batched, const float *enc_weight,
                   const float *enc_bias, const int64_t *top_class, const int64_t *top_index, int batch_size, int num_features,
                   int64_t num_cells, int num_classes, int num_proposals, float *query_feat, float *query_pos,
                   fnp_stream_t stream);
int fnp_tf_decode(const float *heatmap, const float *query_heatmap_score, const float *center, const float *height,
                  const float *dim, const float *rot, const float *vel, const int64_t *query_labels, int batch_size,
                  int num_classes, int num_proposals, int feature_map_stride, float voxel_x, float voxel_y, float range_x,
                  float range_y, float score_thresh, float score_thresh_unk, uint64_t unknown_mask,
                  const float *post_center_range, const int *relabel, float *boxes, float *scores, int *labels, int *counts,
                  fnp_stream_t stream);

/* TransFusionHead's decoder layer and prediction heads (transfusion_utils.py:29-101, transfusion_head.py:20-54, eval mode;
 * additive, ABI 14; csrc/tfdecoder.hip).  All tensors f32; every product runs on the f32 MFMA (a k-ordered fmaf chain), no
 * atomics: results are bit-identical from run to run, and a scene's result does not depend on the batch around it.  Every call
 * takes a stream, allocates nothing and does not synchronise.  Pointers are 16-byte aligned.
 *
 * fnp_tf_attention: q (B, Kq, 128), k and v (B, N, 128) row-major -> out (B, Kq, 128), eight heads, head h = columns
 * 16h .. 16h + 15, scores 0.25 * (q . k) (q is scaled first; the factor is exact), softmax over the N keys, before any output
 * projection.  1 <= Kq <= 2048, 1 <= N < 2^31 / 128, finite inputs.
 *   1. Geometry (fnp_tf_attention_geometry, a function of N alone): tile_len = 64;
 *      split_len = max(256, 64 * ceil(ceil(N / 64) / 64)); split s holds keys [s * split_len, min(N, (s + 1) * split_len)).
 *      N = 32 400 gives 64 splits of 512, i.e. 8 heads x 64 = 512 workgroups per scene, two per CU; N <= 256 is one split.
 *   2. One workgroup per (split, head, scene x query chunk: 256 queries, 64 when N <= 256 makes one split) walks its keys in tiles of tile_len with the online softmax:
 *      per tile m' = max(m, tile maximum), acc = acc * exp(m - m') + sum_k exp(s_k - m') v_k, l alike; exp is expf.
 *   3. With more than one split the partials (m, l, 16 accumulators) per (scene, split, head, query) go to the workspace and
 *      a second launch merges them in split order: M = max m_s, out = (sum_s acc_s exp(m_s - M)) / (sum_s l_s exp(m_s - M)).
 *      With one split the first launch divides and writes out itself.
 *   4. A query whose scores are all equal gets the mean of v; a score that leads the others by more than 104 gets that key's
 *      v row bit for bit (exp of the difference is 0 in f32).
 * workspace: fnp_tf_attention_workspace_bytes(B, Kq, N) bytes (0 with one split; negative: the shape is out of contract).
 *
 * fnp_tf_decoder: the whole forward in seven launches (front, self-attention, mid, kv_proj, cross-attention, merge, tail) for
 * K <= 256 and eight for 256 < K <= 2048, where the self-attention has several splits and a merge launch of its own.
 * query_feat (B, 128, K) and lidar_feat (B, 128, N) channel-major as the head holds them, query_pos (B, K, 2), key_pe (128, N)
 * = cross_posembed(bev_pos), channel-major, or (B, 128, N) when key_pe_batched != 0 (it depends on weights and bev_pos only: the
 * caller computes it once) ->
 * out_query_feat (B, 128, K) and out_heads: head h is a contiguous (B, head_out[h], K) array at float offset
 * B * K * (head_out[0] + .. + head_out[h - 1]).  head_out is a HOST array of n_heads entries (0 <= n_heads <= 8, each 1..64);
 * center_head (or -1) names the head with two outputs that gets query_pos added.  ffn: a multiple of 16 in [16, 1024].
 *   front  x = query_feat^T; qpe = W2 relu(W1' pos + b1') + b2 (self_posembed, BatchNorm folded); q, k, v = (x + qpe) Win^T + bin
 *   self   attention(q, k, v) as above with N = K
 *   mid    x1 = LN1(x + (attn Wo^T + bo)); qc = (x1 + qpe) Wq^T + bq
 *   kv     K = (lidar_feat^T + key_pe^T) Wk^T + bk, V alike with Wv, bv (the feature map is read channel-major as it is)
 *   cross  attention(qc, K, V), then the merge
 *   tail   x2 = LN2(x1 + (attn Wo^T + bo)); x3 = LN3(x2 + (W2 relu(W1 x2 + b1) + b2)) -> out_query_feat;
 *          head h: W2h relu(W1h' x3 + b1h') + b2h (BatchNorm folded), center += query_pos
 * LayerNorm: mean, then the biased variance of the centred values, (x - mean) * (1 / sqrt(var + eps)) * gamma + beta, in f32.
 * Sums over input channels run in ascending channel order per output element.
 * params: one block of params_floats f32, in this order (row-major, sizes in floats):
 *   eps of norm1, norm2, norm3, 0 (4) | self_posembed W1' (128 x 2), b1' (128), W2 (128 x 128), b2 (128) |
 *   self_attn in_proj_weight (384 x 128), in_proj_bias (384), out_proj.weight (128 x 128), out_proj.bias (128) |
 *   norm1 weight, bias (128, 128) | multihead_attn in_proj_weight, in_proj_bias, out_proj.weight, out_proj.bias (as self_attn) |
 *   norm2 weight, bias | linear1.weight (ffn x 128), bias (ffn), linear2.weight (128 x ffn), bias (128) | norm3 weight, bias |
 *   heads' first convolutions stacked (64 n_heads x 128) and biases (64 n_heads), BatchNorm folded: W' = W * s,
 *   b' = (b - running_mean) * s + beta, s = gamma / sqrt(running_var + eps) |
 *   heads' last convolutions, head h padded with zero rows to 16 * ceil(head_out[h] / 16) rows of 64, then the biases padded alike.
 * Out of contract: training mode (dropout, batch statistics), masks, d_model != 128, nhead != 8, non-finite inputs.
 * workspace: fnp_tf_decoder_workspace_bytes(B, K, N, ffn, n_head_out = the sum of head_out) bytes.
 *
 * fnp_tf_decoder_stages: fnp_tf_decoder's arguments and a mask of the stages to launch (bit 0 front, 1 self-attention, 2 mid,
 * 3 kv_proj, 4 cross-attention with its merge, 5 tail; 63 is fnp_tf_decoder).  A stage reads what the stages in front of it left in
 * the workspace: on the workspace of a complete call any single stage can be launched again, which is how tools/bench_decoder.py
 * times each kernel on its own.  (After a complete call the attention output buffer holds the cross attention's rows, so `mid`
 * run alone is good for its time, not for its values.) */
int fnp_tf_attention_geometry(int64_t n_keys, int *split_len, int *tile_len);
int64_t fnp_tf_attention_workspace_bytes(int batch_size, int num_queries, int64_t num_keys);
int fnp_tf_attention(const float *q, const float *k, const float *v, int batch_size, int num_queries, int64_t num_keys,
                     void *workspace, int64_t workspace_bytes, float *out, fnp_stream_t stream);
int64_t fnp_tf_decoder_workspace_bytes(int batch_size, int num_queries, int64_t num_keys, int ffn, int n_head_out);
int fnp_tf_decoder_stages(const float *query_feat, const float *lidar_feat, const float *query_pos, const float *key_pe,
                          int key_pe_batched, const float *params, int64_t params_floats, int batch_size, int num_queries,
                          int64_t num_keys, int ffn, int n_heads, const int *head_out, int center_head, void *workspace,
                          int64_t workspace_bytes, float *out_query_feat, float *out_heads, int stages, fnp_stream_t stream);
int fnp_tf_decoder(const float *query_feat, const float *lidar_feat, const float *query_pos, const float *key_pe,
                   int key_pe_batched, const float *params, int64_t params_floats, int batch_size, int num_queries, int64_t num_keys, int ffn,
                   int n_heads, const int *head_out, int center_head, void *workspace, int64_t workspace_bytes,
                   float *out_query_feat, float *out_heads, fnp_stream_t stream);

/* The attention core softmax(0.25 q . k^T) v as a differentiable operator (additive, ABI 14; the forward's statistics come from
 * the kernels of csrc/tfdecoder.hip, the backward is csrc/tfattn_grad.hip).  Conventions and shapes are those of fnp_tf_attention:
 * f32, every product on the f32 MFMA, no atomics, a stream, no allocation, no synchronisation, bit-identical from run to run, a
 * scene's results independent of the batch around it, 16-byte aligned pointers.  The score matrix is never stored: the backward
 * recomputes it tile by tile with the forward's arithmetic (q scaled by 0.25 first, the same k-ordered chain per score).
 *
 * fnp_tf_attention_stats: fnp_tf_attention (same kernels, same workspace, `out` bit for bit) that also writes
 * stats (B, 8, Kq, 2): per (scene, head, query) the pair (M, L), M = the maximum score, L = sum_j exp(s_j - M) as the forward
 * summed it (with several splits: the merge's M and L).  The pair and not the log-sum-exp: s - M is exact near the maximum and
 * 1 / L carries one rounding, whereas an f32 log-sum-exp of magnitude 11 (N = 32 400) alone is half an ulp = 5e-7 off, a
 * relative error common to a query's whole row of probabilities.
 *
 * fnp_tf_attention_backward: with P_ij = exp(s_ij - M_i) * (1 / L_i), D_i = sum_d dO_id O_id (per head), dP_ij = dO_i . v_j and
 * dS_ij = P_ij (dP_ij - D_i):  dV_j = sum_i P_ij dO_i,  dK_j = 0.25 sum_i dS_ij q_i,  dQ_i = 0.25 sum_j dS_ij k_j.
 * q, out, d_out, dq (B, Kq, 128); k, v, dk, dv (B, N, 128); stats as above; all contiguous.  Any of dq, dk, dv may be NULL: that
 * result is not written, and its kernel (dq) or its products (dk, dv) are skipped.
 *   1. Prologue: D_i per (scene, head, query) into the workspace, the diagonal of dO O^T on the MFMA.
 *   2. dK and dV, key-stationary (fnp_tf_attention_backward_geometry, constants: key_block = 256, wave_keys = 64): one workgroup
 *      per (block of key_block keys, head, scene), wave w of its four owns the wave_keys keys from key_block * block +
 *      wave_keys * w as four MFMA column blocks of 16, walks ALL queries in blocks of 16 in ascending order and keeps the dK and
 *      dV rows of its keys in registers: every row has one owner, so there is no reduction across workgroups.  Query rows past Kq
 *      enter with P = 0.
 *   3. dQ, query-stationary, on the forward's geometry (fnp_tf_attention_geometry; the same splits, tiles and query chunks): one
 *      workgroup per (split, head, scene x query chunk) accumulates its split's part of dQ over tiles of 64 keys in ascending
 *      order; with several splits the parts go to the workspace and a second launch adds them in split order.  The factor 0.25
 *      is applied last.
 * workspace: fnp_tf_attention_backward_workspace_bytes(B, Kq, N) bytes (D, and with several splits the dQ parts: 16 floats per
 * (scene, split, head, query); negative: the shape is out of contract).  It does not depend on which results are asked for. */
int fnp_tf_attention_stats(const float *q, const float *k, const float *v, int batch_size, int num_queries, int64_t num_keys,
                           void *workspace, int64_t workspace_bytes, float *out, float *stats, fnp_stream_t stream);
int fnp_tf_attention_backward_geometry(int64_t n_keys, int *key_block, int *wave_keys);
int64_t fnp_tf_attention_backward_workspace_bytes(int batch_size, int num_queries, int64_t num_keys);
int fnp_tf_attention_backward(const float *q, const float *k, const float *v, const float *out, const float *stats,
                              const float *d_out, int batch_size, int num_queries, int64_t num_keys, void *workspace,
                              int64_t workspace_bytes, float *dq, float *dk, float *dv, fnp_stream_t stream);

/* Attention dropout inside the differentiable attention core (additive, ABI 14; csrc/tfattn_dropout.h states the mask, the
 * kernels are the dropout instantiations of the ones above).  Dropout sits after the softmax: O = (P o Z) V with
 * Z_ij = keep_ij / (1 - p_eff).  The statistics (M, L) do not see the mask.  Backward: dV_j = sum_i P_ij Z_ij dO_i,
 * dS_ij = P_ij (Z_ij dP_ij - D_i) with D_i = dO_i . O_i of the DROPPED output (sum_j P_ij Z_ij dP_ij = dO_i . O_i), dK and dQ
 * from dS as above.  No mask is stored: every kernel regenerates its bits.
 *
 * The mask.  keep(seed, scene, head, query, key) is a pure function of those five integers; it depends on nothing of a launch
 * (split length, query chunk, batch size, which kernel asks).  seed is a uint64, scene the index in the batch, head 0..7, query
 * and key the row indices.
 *   generator  Philox4x32-10 (Salmon et al. 2011): multipliers 0xD2511F53 (on word 0) and 0xCD9E8D57 (on word 2), the key words
 *              advance by 0x9E3779B9 and 0xBB67AE85 after every round, ten rounds; a round maps (c0, c1, c2, c3) to
 *              (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)).
 *   key        (seed & 0xffffffff, seed >> 32)
 *   counter    (key >> 2, query, scene * 8 + head, 0)
 *   word       output word (key & 3) of that call belongs to `key`: one call serves an aligned group of four keys of a query
 *   keep       iff word >= T, T = (uint32)((double)p * 2^32) with p the f32 argument; p_eff = T / 2^32 (|p_eff - p| < 2^-32;
 *              p = 0.5 gives exactly 0.5), and the scale 1 / (1 - p_eff) is evaluated in double and rounded to f32 once (2 at
 *              p = 0.5, 1 at p = 0).
 * Because the scene index is part of the counter, a scene alone has the mask of scene 0: a batch and its FIRST scene alone agree
 * bit for bit, other scenes get other masks (unlike the plain entry points, whose results do not depend on the position in a batch).
 * Same seed, same bits, from run to run.
 *
 * seed is a DEVICE pointer to one uint64, 8-byte aligned; the kernels read it (no host read, and a captured graph does not
 * freeze the mask: it replays with whatever the word holds then).  0 <= p < 1, anything else (NaN included) is FNP_ERR_ARG.
 *
 * fnp_tf_attention_dropout_stats: fnp_tf_attention_stats' arguments, workspace and launches; out is the dropped output, stats are
 * bit for bit what fnp_tf_attention_stats writes.  fnp_tf_attention_dropout_backward: fnp_tf_attention_backward's arguments,
 * workspace, launches and NULL-result rules; out is the dropped output and p, seed those of the forward.  With p = 0 (T = 0,
 * every word kept, scale 1) both give the bits of the plain entry points.  In the key-stationary kernel a lane holds four queries
 * against one key: lane i of a quad calls the generator for (query 4g + (i & 3), the quad's common key group) and the four lanes
 * exchange their keep bits by quad permutes.  Rows past Kq and keys past N enter with P = 0; their mask bits are computed like any
 * other and index nothing.
 *
 * fnp_tf_attention_dropout_mask: keep as one byte (0 or 1) per element of (B, 8, Kq, N), from the same device function the three
 * kernels call; B * 8 <= 65535.  For tests and tools: nothing on a training path launches it. */
int fnp_tf_attention_dropout_stats(const float *q, const float *k, const float *v, int batch_size, int num_queries, int64_t num_keys,
                                   void *workspace, int64_t workspace_bytes, float *out, float *stats, float p, const uint64_t *seed,
                                   fnp_stream_t stream);
int fnp_tf_attention_dropout_backward(const float *q, const float *k, const float *v, const float *out, const float *stats,
                                      const float *d_out, int batch_size, int num_queries, int64_t num_keys, void *workspace,
                                      int64_t workspace_bytes, float *dq, float *dk, float *dv, float p, const uint64_t *seed,
                                      fnp_stream_t stream);
int fnp_tf_attention_dropout_mask(const uint64_t *seed, float p, int batch_size, int num_queries, int64_t num_keys, uint8_t *keep,
                                  fnp_stream_t stream);

/* Hungarian assignment and per-query targets of TransFusionHead (transfusion_head.py:352-444, hungarian_assigner.py:61-132;
 * additive, ABI 14; csrc/tfassign.hip).  The batch goes in four launches (valid rows, cost, match, targets); every device call
 * takes a stream, allocates nothing, calls no synchronising HIP function and uses no atomics: results are bit-identical from
 * run to run, and a scene's results are the same alone or in a batch.  Parity is with the reference run on the CPU.
 *
 * fnp_tf_assign_cost: the head outputs heatmap (logits, B, C, K), center (B, 2, K), height (B, 1, K), dim (B, 3, K), rot
 * (B, 2, K: sin, cos), vel (B, 2, K; required when ncol == 10, else ignored), all f32, and gt_boxes (B, Mcap, ncol) f32,
 * ncol = 10 (x y z dx dy dz yaw vx vy label) or 8 (no velocities), label 1-based, 0 = padding.
 *   1. Valid rows: dx > 0 and dy > 0 (the reference's "filter empty boxes"), a label inside 1..num_classes (a fraction is
 *      truncated, as the reference's .long() does) and finite x, y, dx, dy.  The reference wraps on a label below 1 and raises on one above num_classes; both are out of contract here and
 *      skipped, the rule of fnp_heatmap_box_params.  num_valid (B) int32 = their number; valid_map (B, Mcap) int32 = their row
 *      indices in ascending order, -1 behind them.
 *   2. Decode (decode_bbox, filter = False): the sequence of fnp_tf_decode (one device function, csrc/tfdecode.h): centres bit
 *      for bit, exp(dim) and atan2 in f64 rounded once.  boxes (B, K, 9 or 7) or NULL receives the decoded rows.
 *   3. cost[b, k, j] for j < num_valid[b], the box being row valid_map[b, j]: cls + reg + iou_cost, f32, in that order.
 *      cls = (pos - neg) * cls_weight with p = sigmoid(heatmap[b, label - 1, k]), neg = -log(1 - p + eps) * (1 - alpha) * p^gamma,
 *      pos = -log(p + eps) * alpha * (1 - p)^gamma (f32 expf / logf; p^2 is a product);  reg = (|dx| + |dy|) * reg_weight of the
 *      centres normalised as (v - range[0:2]) / (range[3:5] - range[0:2]);  iou_cost = -iou * iou_weight.
 *   4. iou[b, k, j] = the reference's overlaps(): BEV overlap (the function behind fnp_boxes_overlap_bev, csrc/boxoverlap.h)
 *      times the height overlap with z as the BOTTOM of a box, over clamp(vol_q + vol_g - overlap, 1e-8); plain IEEE f32 in the
 *      reference's operand order.  Columns j >= num_valid[b] of cost and iou are 0: every element is written.
 * point_cloud_range: a HOST array of 6 floats.  Python scalars (weights, alpha, 1 - alpha, eps) meet the tensors as their f32
 * roundings.  Every argument is checked before the first launch: a call that returns an error has written nothing.  B <= 65535, C <= 64, K <= 2048, Mcap <= 1024.  Two launches.
 *
 * fnp_tf_assign_targets (transfusion_head.py:401-444): assigned (B, K) int32 as fnp_tf_assign_match writes it (original row
 * of gt_boxes or -1) -> labels (B, K) int64: the box's label - 1 at a match, num_classes elsewhere; label_weights (B, K) f32:
 * 1 everywhere (the reference's outcome for positives and negatives alike); bbox_targets (B, K, ncol) f32: encode_bbox at a
 * match ((x - range_x) / f32(stride * voxel_x), y alike, z, log of the sizes, sin and cos of the yaw, the velocities when
 * ncol == 10; the divisions, log, sin and cos formed in f64 and rounded once), 0 elsewhere; bbox_weights (B, K, ncol): 1 at a
 * match, else 0; unknown (B, K) bytes 0 / 1: the matched label has its bit (label - 1) set in unknown_mask; num_pos (1) int32:
 * the number of matches of the batch, an integer sum.  One launch.
 *
 * The matching: both functions below reproduce scipy.optimize.linear_sum_assignment (scipy >= 1.4, the
 * shortest-augmenting-path solver) exactly, ties included: the matrix is transposed when it has fewer columns than rows, the
 * reduced costs are formed in f64 on the f32 costs widened, in scipy's operand order, and scipy's scan order and tie rule
 * are kept (csrc/lsap.h states them).  Costs must be finite; with a NaN or an infinity the result is unspecified, but every
 * loop is bounded: each inner step removes a column.
 *
 * fnp_host_lsap: HOST arrays, serial.  cost (nr, nc) f32 row-major -> rows, cols (min(nr, nc)) int32, rows ascending, as
 * scipy returns them.  FNP_ERR_ARG when no finite assignment exists.
 *
 * fnp_tf_assign_match: cost (B, K, Mcap) f32 on the device, of which scene b uses the K x num_valid[b] leading columns
 * (num_valid (B) int32 on the device, clamped to 0..Mcap; the columns are the scene's valid boxes, compacted in ascending row
 * order) -> assigned (B, K) int32: per query the matched box, or -1.  The box is named by valid_map[b, column] (valid_map
 * (B, Mcap) int32, compact column -> original row of gt_boxes) or, with valid_map NULL, by the column itself.  matched_iou
 * (B, K) f32 or NULL: iou[b, k, column] (iou (B, K, Mcap) f32) at the match, clamped to [0, 1], else 0.  A scene with
 * num_valid 0 gets no match.  K <= 2048, Mcap <= 1024.  One launch for the batch, one wave per scene; takes a stream,
 * allocates nothing, calls no synchronising HIP function and uses no atomics: results are bit-identical from run to run,
 * and a scene's result is the same alone or in a batch. */
int fnp_host_lsap(const float *cost, int nr, int nc, int *rows, int *cols);
int fnp_tf_assign_match(const float *cost, const float *iou, const int *num_valid, const int *valid_map, int batch_size,
                        int num_queries, int max_boxes, int *assigned, float *matched_iou, fnp_stream_t stream);
int fnp_tf_assign_cost(const float *heatmap, const float *center, const float *height, const float *dim, const float *rot,
                       const float *vel, const float *gt_boxes, int batch_size, int num_classes, int num_queries, int max_boxes,
                       int ncol, int feature_map_stride, float voxel_x, float voxel_y, const float *point_cloud_range,
                       double cls_weight, double alpha, double gamma, double eps, double reg_weight, double iou_weight,
                       int *num_valid, int *valid_map, float *cost, float *iou, float *boxes, fnp_stream_t stream);
int fnp_tf_assign_targets(const int *assigned, const float *gt_boxes, int batch_size, int num_classes, int num_queries,
                          int max_boxes, int ncol, int feature_map_stride, double voxel_x, double voxel_y, float range_x,
                          float range_y, uint64_t unknown_mask, int64_t *labels, float *label_weights, float *bbox_targets,
                          float *bbox_weights, unsigned char *unknown, int *num_pos, fnp_stream_t stream);

/* The two losses behind the per-query targets (transfusion_head.py:500-504, :561-597, the default configuration:
 * SigmoidFocalClassificationLoss without label smoothing or balanced reweighting, L1Loss; additive, ABI 14; csrc/tfassign.hip).
 * heatmap (logits, B, C, K) and the n_heads <= 8 regression heads in HEAD_ORDER, head h (B, head_channels[h], K), all of `dtype`
 * (FNP_F32, FNP_F16, FNP_BF16; upcast exactly), read where they lie: no cat, no permute.  heads, head_channels, code_weights and
 * unknown_code_weights (or NULL) are HOST arrays; the channels sum to code_size <= 16.  labels, label_weights, bbox_targets,
 * bbox_weights, unknown and num_pos as fnp_tf_assign_targets writes them.
 * forward: loss[0] = sum(focal * bce * w) / max(*num_pos, 1), loss[1] = sum(|pred - target| * rw) / max(*num_pos, 1), with
 * t = 1 at column labels[b, k]; p = sigmoid(x); focal = (t alpha + (1 - t)(1 - alpha)) * pt^gamma, pt = t (1 - p) + (1 - t) p;
 * bce = max(x, 0) - x t + log1p(exp(-|x|)); w = label_weights, times unknown_cls_weight where unknown is set (pass 1 when not
 * configured); rw = bbox_weights * code_weights, times unknown_code_weights where unknown is set.  f32 per element, f64 partial
 * sums in a fixed order: bit-identical from run to run.  Two launches.  workspace: fnp_tf_query_loss_workspace_bytes(), 8-byte
 * aligned.
 * backward: grad_heatmap and grad_heads[h] (`dtype`, the layouts of their inputs) = the derivative, recomputed, times
 * grad_out[0 or 1] / max(*num_pos, 1) (grad_out: 2 f32 on the device).  The focal weight is differentiated through; the L1
 * gradient is sign(pred - target), 0 at equality.  One launch.  Neither call allocates or synchronises. */
int64_t fnp_tf_query_loss_workspace_bytes(void);
int fnp_tf_query_loss_forward(const void *heatmap, const void *const *heads, const int *head_channels, int n_heads, int dtype,
                              int batch_size, int num_classes, int num_queries, int code_size, const int64_t *labels,
                              const float *label_weights, const float *bbox_targets, const float *bbox_weights,
                              const unsigned char *unknown, const int *num_pos, double alpha, double gamma,
                              const float *code_weights, const float *unknown_code_weights, double unknown_cls_weight,
                              void *workspace, int64_t workspace_bytes, float *loss, fnp_stream_t stream);
int fnp_tf_query_loss_backward(const void *heatmap, const void *const *heads, const int *head_channels, int n_heads, int dtype,
                               int batch_size, int num_classes, int num_queries, int code_size, const int64_t *labels,
                               const float *label_weights, const float *bbox_targets, const float *bbox_weights,
                               const unsigned char *unknown, const int *num_pos, double alpha, double gamma,
                               const float *code_weights, const float *unknown_code_weights, double unknown_cls_weight,
                               const float *grad_out, void *grad_heatmap, void *const *grad_heads, fnp_stream_t stream);

/* The optimizer step of the reference's adam_onecycle recipe (tools/train_utils/train_utils.py:173-176 around
 * optimization/fastai_optim.py OptimWrapper.step with true_wd and torch's Adam; additive, ABI 14; csrc/optim.hip): unscale,
 * non-finite check, gradient norm, clip, decoupled weight decay, Adam and the loss-scale update in THREE launches whatever the
 * number of tensors, with no host read, no allocation and no atomics: results are bit-identical from run to run.
 *
 * Host inputs, by value: lr, beta1, beta2, eps, wd, max_norm (doubles; lr and beta1 move every step with the OneCycle schedule;
 * max_norm = +infinity: no clipping), growth_factor, backoff_factor, growth_interval (the loss scaler's; ignored when scale is NULL).
 * Device state: per tensor i of num_tensors: params[i], exp_avg[i], exp_avg_sq[i] (f32, contiguous, 4-byte aligned, the
 * tensor's length each) and steps[i] (int32); the scaler's scale (1 f32) and growth_tracker (1 int32), both NULL without a
 * scaler (the scale is then 1); outputs grad_norm (1 f32) and found_inf (1 int32).  params, grads, exp_avg and exp_avg_sq are
 * DEVICE tables of num_tensors pointers each; grads[i] == NULL: tensor i has no gradient this step.  Gradients are f32 and are
 * left as they came (scaled, unclipped).
 * chunks: a DEVICE table of num_chunks struct fnp_optim_chunk, made once per parameter list: workgroup c works on elements
 * [offset, offset + length) of tensor `tensor`; 0 < length, offset a multiple of 4, every element of every tensor in exactly
 * one chunk (an empty tensor has none), chunks of a tensor in ascending order.  The chunk length is the caller's choice.
 *
 * The step (m = exp_avg, v = exp_avg_sq, t = steps):
 *   1. inv = (float)(1.0 / (double)scale);  g^ = g * inv (f32);  found_inf = any g^ of any present gradient is not finite.
 *   2. N = sqrt(sum g^ * g^) over all present gradients, the squares formed and summed in f64: per chunk by a fixed tree, the
 *      chunks' partial sums in a fixed order;  c = (float)min(1, max_norm / (N + 1e-6)).
 *   3. found_inf: no byte of any p, m, v, t is written;  scale <- scale * backoff_factor;  growth_tracker <- 0.
 *   4. otherwise every tensor, with a gradient or not: p <- p * (float)(1 - wd * lr).
 *   5. then every tensor with a gradient: t <- t + 1;  g' = g^ * c;  m <- m + (g' - m) * (float)(1 - beta1);
 *      v <- (float)beta2 * v + (float)(1 - beta2) * g' * g';
 *      p <- p - (float)(lr / (1 - beta1^t)) * (m / (sqrt(v) / (float)sqrt(1 - beta2^t) + (float)eps)),
 *      the bias corrections in f64 from the tensor's own t and this step's beta1; f32 IEEE multiply, add, divide and square
 *      root, no fused multiply-add.
 *   6. then growth_tracker <- growth_tracker + 1, and when that equals growth_interval: scale <- scale * growth_factor if that
 *      is finite, growth_tracker <- 0.
 * grad_norm <- (float)N and found_inf are written by every step.  A non-finite gradient skips the step also without a scaler.
 * workspace: fnp_adam_onecycle_workspace_bytes(num_chunks) bytes, 8-byte aligned; its contents mean nothing between steps.
 * Every host-visible argument is checked before the first launch (lr, eps >= 0 and wd finite, the betas in [0, 1), max_norm >= 0
 * or +infinity, the scaler's factors positive and finite, growth_interval >= 1; FNP_ERR_ARG otherwise): a call that returns an
 * error has written nothing.  What the device tables hold is the caller's to get right. */
struct fnp_optim_chunk {
    int32_t tensor;
    int32_t length;
    int64_t offset;
};
int64_t fnp_adam_onecycle_workspace_bytes(int64_t num_chunks);
int fnp_adam_onecycle_step(int num_tensors, int64_t num_chunks, const struct fnp_optim_chunk *chunks, float *const *params,
                           const float *const *grads, float *const *exp_avg, float *const *exp_avg_sq, int32_t *steps,
                           float *scale, int32_t *growth_tracker, double lr, double beta1, double beta2, double eps, double wd,
                           double max_norm, double growth_factor, double backoff_factor, int growth_interval, void *workspace,
                           int64_t workspace_bytes, float *grad_norm, int32_t *found_inf, fnp_stream_t stream);

/* Capacity overflow: data-dependent counts (n_voxels, n_out) always hold the TRUE count; every
 * kernel clamps to the capacity it was given, so a count larger than its capacity means rows
 * were dropped and the caller must re-run with larger buffers. */

#ifdef __cplusplus
}
#endif
#endif /* FNP_H */
