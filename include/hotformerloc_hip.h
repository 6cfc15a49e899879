/*
 * hotformerloc_hip.h -- C-ABI of libhotformerloc_hip.so (gfx950 / MI355X).
 *
 * Drop-in boundary for the native side of the HOTFormerLoc hot path.  Every entry
 * point takes plain device pointers and sizes (no torch types), enqueues work on
 * the given HIP stream WITHOUT synchronising (the reference's extension launches
 * on the current stream: libs/dwconv/csrc/dwconv.cu:92,106,124) and returns 0 on
 * success or a hipError_t value (> 0) / a negative HFL_E* code on failure; the
 * reference aborts on launch errors (libs/dwconv/csrc/utils.h:12-24), the host
 * wrapper turns non-zero into a Python exception.
 *
 * All feature matrices are row-major float32.  "neigh" tables hold row indices,
 * -1 = no neighbour.  Tables may be int64 (the reference's dtype, dwconv.cu:27)
 * or int32 (what this library builds itself): `idx64` selects.
 *
 * The reference interface each function replaces is cited as file:line of
 * csiro-robotics/HOTFormerLoc; ocnn==2.2.2 is the un-vendored dependency
 * (requirements.txt:6) whose behaviour SURVEY.md Appendix A restates.
 */
#ifndef HOTFORMERLOC_HIP_H
#define HOTFORMERLOC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* hfl_stream_t; /* hipStream_t */

#define HFL_OK 0
#define HFL_EINVAL (-1)      /* unsupported shape / argument            */
#define HFL_ECAPACITY (-2)   /* input exceeds a documented kernel limit */
#define HFL_EBACKEND (-100)  /* hipBLASLt refused the problem: code = -100 - hipblasStatus_t */

/* library / device identification: returns the version as major*100+minor */
int hfl_version(void);
/* name of the code-object architecture this library was compiled for */
const char* hfl_arch(void);

/* ------------------------------------------------------------------------
 * 1. Octree depth-wise convolution  (replaces dwconv.core, libs/dwconv)
 * ---------------------------------------------------------------------- */

/* out[h,c] = sum_k [neigh[h,k] >= 0] * weight[k,c] * data[neigh[h,k], c]
 *   replaces  Tensor dwconv_forward_backward(Tensor data, Tensor weight, Tensor neigh)
 *             libs/dwconv/csrc/dwconv.h:13, dwconv.cu:24-42,99-113, pybind.cpp:11
 *   data (n_in,C) ; weight (K,1,C) ; neigh (n_out,K) ; out (n_out,C).  Also used for
 *   the input gradient with the inverse table (libs/dwconv/dwconv/nn.py:36-38).
 *   Unchecked precondition: with n_out > 0, `data` holds at least one row (n_in >= 1, not NULL).  The kernel reads row 0
 *   for every dead tap and drops the value; the API has no n_in to check this against. */
int hfl_dwconv_forward_backward(float* out, const float* data, const float* weight,
                                const void* neigh, int idx64, int64_t n_out,
                                int64_t channels, int kngh, hfl_stream_t stream);

/* out[h,c] = sum_k [slot[h,k] >= 0] part[slot[h,k], c] [+ bias[c]]  (round 6): the per-row sum of the partial products of an
 * octree convolution over its live (row, tap) pairs -- ocnn's octree2col + mm scatters nothing, it multiplies the zero-padded
 * column matrix (models/layers/octformer_layers.py:89-95); here every output row adds the products of its own live taps in tap
 * order -- and the convolution's bias.  part (P, C) f32, slot (n_out, K <= 32) int32, -1 = no such neighbour, bias (C) or
 * NULL.  Only live slots are loaded; a row without one reads nothing from part.
 * Equals hfl_dwconv_forward_backward with unit weights (what rounds 1-5 launched) bit for bit. */
int hfl_slot_sum(float* out, const float* part, const int32_t* slot, const float* bias, int64_t n_out, int64_t channels, int kngh,
                 hfl_stream_t stream);

/* hfl_slot_sum with the caller's LayerNorm [+ ReLU] over the channel axis folded into the same pass: the norm that follows every
 * stem convolution and every Downsample (models/layers/octformer_layers.py:80-98, models/octformer_backbone.py:464-477), on the
 * sum while it is in registers.  f32 rows (out_f32, (n_out, C)) or the split2 operand of the next GEMM (out_split2, (n_out, 2C)
 * bf16); exactly one of the two is non-NULL.  channels in {32, 64, 128, 256} (one 16-B cell per lane), kngh <= 32; anything
 * else is HFL_EINVAL.  Bit for bit hfl_slot_sum followed by hfl_layer_norm (relu = 0) / hfl_layer_norm_relu (relu = 1). */
int hfl_slot_sum_norm(float* out_f32, uint16_t* out_split2, const float* part, const int32_t* slot, const float* bias,
                      const float* gamma, const float* beta, int64_t n_out, int64_t channels, int kngh, float eps, int relu,
                      hfl_stream_t stream);

/* gW[k,c] = sum_h [neigh[h,k] >= 0] data[neigh[h,k], c] * grad[h,c]
 *   replaces  Tensor dwconv_weight_backward(Tensor grad, Tensor data, Tensor neigh)
 *             libs/dwconv/csrc/dwconv.h:14, dwconv.cu:44-72,115-131, pybind.cpp:12
 *   out (K,1,C).  `workspace` must hold hfl_dwconv_weight_backward_workspace() bytes.
 *   Unchecked precondition: with n_rows > 0, `data` holds at least one row (not NULL): row 0 is read for every dead tap
 *   and dropped by a select; the API has no source row count to check this against. */
int64_t hfl_dwconv_weight_backward_workspace(int64_t n_rows, int64_t channels, int kngh);
int hfl_dwconv_weight_backward(float* out, const float* grad, const float* data,
                               const void* neigh, int idx64, int64_t n_rows,
                               int64_t channels, int kngh, void* workspace,
                               hfl_stream_t stream);

/* ineigh[neigh[h,k], k] = h on a -1-filled (n_rows,K) table
 *   replaces  Tensor inverse_neigh(Tensor neigh)
 *             libs/dwconv/csrc/dwconv.h:15, dwconv.cu:74-97, pybind.cpp:13 */
int hfl_inverse_neigh(void* ineigh, const void* neigh, int idx64, int64_t n_rows,
                      int kngh, hfl_stream_t stream);

/* Fused conditional position encoding:
 *   y = LayerNorm_C( dwconv(x) ) * gamma + beta ;  out = residual ? x + y : y
 *   replaces  CPE.forward + the residual of its callers
 *             models/layers/octformer_layers.py:138-142,
 *             models/octformer_backbone.py:258, models/hotformerloc_backbone.py:204,351
 *   x,out (n,C) with C in {128,256} (C % 64 == 0, C <= 512); neigh int32 (n,27). */
int hfl_cpe_forward(float* out, const float* x, const float* weight, const float* gamma,
                    const float* beta, const int32_t* neigh, int64_t n_rows,
                    int64_t channels, int kngh, float eps, int residual,
                    hfl_stream_t stream);
/* The same launch for the training forward: additionally writes conv_out (n, C) = dwconv(x), the input of the LayerNorm
 * backward (hfl_layer_norm_bwd_add), so that loss.backward() through CPE (training/trainer.py:344-362) needs no second
 * pass over the neighbourhoods; conv_out = NULL is hfl_cpe_forward. */
int hfl_cpe_forward_save(float* out, float* conv_out, const float* x, const float* weight, const float* gamma,
                         const float* beta, const int32_t* neigh, int64_t n_rows,
                         int64_t channels, int kngh, float eps, int residual,
                         hfl_stream_t stream);
/* The convolution alone through the same gather (live taps compacted per row): out = dwconv(data, weight, neigh) [+ add].
 * The data gradient of CPE in loss.backward(): data = gradient of the convolution's output, neigh = the INVERSE neighbour
 * table (hfl_inverse_neigh, libs/dwconv/dwconv/nn.py:36-38), add = the skip connection's gradient (or NULL).
 * int32 tables, C in {32, 64, 128, 256}, kngh <= 27; out must not alias data. */
int hfl_dwconv_add(float* out, const float* data, const float* weight, const int32_t* neigh, const float* add,
                   int64_t n_out, int64_t channels, int kngh, hfl_stream_t stream);

/* ------------------------------------------------------------------------
 * 2. Octree construction  (replaces ocnn.octree.Octree.build_octree /
 *    merge_octrees / construct_all_neigh; call sites datasets/dataset_utils.py:89-94,
 *    eval/pnv_evaluate.py:173-175,123, misc/torch_utils.py:47-51)
 * ---------------------------------------------------------------------- */

/* Limits of the one-workgroup-per-cloud builder. */
#define HFL_OCTREE_MAX_POINTS (1 << 20) /* points per cloud; <= 16384 sort entirely in LDS */
#define HFL_OCTREE_MAX_DEPTH 10         /* 30-bit shuffled keys                            */

/* Bytes of scratch hfl_octree_build_clouds needs. */
int64_t hfl_octree_scratch_bytes(int64_t total_points, int batch, int max_points, int depth);

/* Stage 1: one workgroup per cloud.  points (P,3) in [-1,1]; cloud_offsets (B+1)
 * int64 on the DEVICE; total_points = P and max_points = the largest cloud are the
 * host's copies of the same numbers (they size the scratch strides and the LDS sort).
 * Writes per-cloud sorted unique node keys and child slots for depths
 * full_depth..depth into `scratch`, the per-leaf point averages (scaled to
 * [0,2^depth], ocnn's `points[depth]`) into leaf_points (P,3) at the cloud's point
 * offset, and counts[(depth+1) * B] int32 = non-empty nodes per depth and cloud
 * (`batch_nnum_nempty`, layout (depth+1,B) as models/octree.py:163 reads it).
 * Returns HFL_ECAPACITY when max_points > HFL_OCTREE_MAX_POINTS. */
int hfl_octree_build_clouds(const float* points, const int64_t* cloud_offsets, int batch,
                            int64_t total_points, int max_points, int depth, int full_depth,
                            void* scratch, float* leaf_points, int32_t* counts,
                            hfl_stream_t stream);

/* Stage 2 (after the host has read `counts` and allocated exact-size outputs):
 * merge into batch arrays, ocnn `merge_octrees` layout.  For every depth d in
 * [0,depth], pointers indexed by d:
 *   keys[d]     int64 (nnum_d)      shuffled key | batch << 48      (may be NULL)
 *   children[d] int32 (nnum_d)      index among non-empty nodes of depth d, or -1
 *   nkeys[d]    int64 (nne_d)       keys of the non-empty nodes only
 *   nidx[d]     int32 (nne_d)       position of each non-empty node among all nodes
 * children[d] for d >= full_depth must be pre-filled with -1 by the caller.
 * points_out (nne_depth,3) receives the compacted leaf averages.
 * cum_nne (depth+1, B+1) int32 DEVICE: exclusive prefix of counts over clouds. */
int hfl_octree_merge(const void* scratch, const int64_t* cloud_offsets, const int32_t* cum_nne,
                     int batch, int depth, int full_depth, int64_t total_points,
                     int64_t* const* keys, int32_t* const* children,
                     int64_t* const* nkeys, int32_t* const* nidx,
                     const float* leaf_points, float* points_out, hfl_stream_t stream);

/* 27-neighbour table of the non-empty nodes of one depth, equal to ocnn
 * `get_neigh(depth,'333',stride=1,nempty=True)`:
 *   depth <= full_depth : by key arithmetic (children_d maps key -> non-empty rank)
 *   depth  > full_depth : parent walk through neigh_parent (nne_{d-1},27),
 *                         nidx_d and children_d.
 * neigh_out int32 (nne_d,27). */
int hfl_octree_neigh(int32_t* neigh_out, const int32_t* neigh_parent, const int32_t* nidx,
                     const int32_t* children, const int64_t* nkeys, int64_t nne, int depth,
                     int full_depth, hfl_stream_t stream);

/* tok_meta (n,2) uint32 per non-empty node of one depth: [x | y<<10 | z<<20, batch id]
 * (ocnn key2xyz / batch_id as read by models/octree.py:132,273-275). */
int hfl_token_meta(uint32_t* tok_meta, const int64_t* nkeys, int64_t n, int depth,
                   hfl_stream_t stream);

/* Raw-cloud pre-steps in front of the octree build, for a whole batch (eval/pnv_evaluate.py:158-171,
 * datasets/dataset_utils.py:84-90): bounding-box normalisation into [-1,1] (datasets/augmentation.py:213-223,
 * scale_factor=None, unit_sphere_norm=False, zero_mean=True) when `normalize`, the |coordinate| <= 1 mask, the
 * |xy| <= 1 mask when `cylindrical_mask`, and -- when `cylindrical_transform` -- (x,y,z) -> (rho,phi,z) rescaled
 * to [-1,1] (datasets/coordinate_utils.py:68-116).  points (P,3) with cloud b at rows
 * [cloud_offsets[b], cloud_offsets[b+1]); the kept points of cloud b are written, in order, from row
 * cloud_offsets[b] of out_points (P,3) on, and out_counts[b] says how many.  Normalisation and masks are
 * bit-exact with the reference's fp32 torch sequence; the transform's atan2f is the device library's (see
 * csrc/preprocess.hip).  out_points must not alias points. */
int hfl_prepare_clouds(float* out_points, int32_t* out_counts, const float* points,
                       const int64_t* cloud_offsets, int batch, int normalize, int cylindrical_mask,
                       int cylindrical_transform, hfl_stream_t stream);

/* The training augmentation of the reference for a whole batch, fused with the pre-steps above (csrc/augment.hip):
 * per cloud Normalize, JitterPoints(0.001, clip 0.002), RemoveRandomPoints, [RandomRotation about z],
 * RandomTranslation, RemoveRandomBlock (datasets/CSWildPlaces/CSWildPlaces_train.py:19-57, datasets/augmentation.py)
 * and the masks of datasets/base_datasets.py:77-83; then the batch-wide TrainSetTransform (z rotation, flip;
 * datasets/dataset_utils.py:111-116) and the cylindrical transform.
 *
 * The random scalars come in a table, one row per cloud (hotformerloc_amd/augment.py draws them): */
typedef struct hfl_augment_cloud {
  int32_t remove_k;      /* RemoveRandomPoints: int(n * r) points are set to (0,0,0); 0 <= remove_k <= n */
  int32_t block;         /* RemoveRandomBlock's coin: 1 = erase */
  float rot_cos, rot_sin;/* RandomRotation: float32(cos theta), float32(sin theta); x' = x cos + y sin, y' = y cos - x sin */
  float trans[3];        /* RandomTranslation: float32(max_delta * N(0,1)) */
  float block_u[4];      /* RemoveRandomBlock: U(scale), U(ratio), U(0,1) for x, U(0,1) for y, rounded to float32 */
  float reserved;
} hfl_augment_cloud;

typedef struct hfl_augment_config {
  int32_t normalize;             /* bounding-box Normalize first */
  int32_t cylindrical_mask;      /* also drop |xy| > 1 */
  int32_t cylindrical_transform; /* (x,y,z) -> (rho,phi,z) last */
  int32_t augment;               /* 0: none of jitter / removal / rotation / translation / block (aug_mode 0) */
  int32_t rotate;                /* the per-cloud z rotation (aug_mode 2) */
  int32_t set_rotate;            /* the batch-wide z rotation (set_aug_mode 1) */
  int32_t flip_axis;             /* batch-wide flip: -1 none, 0 x, 1 y, 2 z */
  float set_cos, set_sin;
  float jitter_sigma, jitter_clip;
} hfl_augment_config;

/* points (P,3) with cloud b at rows [cloud_offsets[b], cloud_offsets[b+1]); the kept points of cloud b are written, in
 * order, from row cloud_offsets[b] of out_points (P,3) on, out_counts[b] says how many, and out_index (P, may be null)
 * receives the index within its cloud of every kept point.  cloud_offsets and table are device memory;
 * host_cloud_offsets and host_table are the same values in host memory, which the launcher validates
 * (HFL_EINVAL: a null or aliased buffer, a negative cloud size, remove_k outside [0, n]).
 * Per-point random numbers are Philox4x32-10 keyed by `seed` with counter (point index in its cloud, cloud index +
 * cloud_base, stream, 0): a point's numbers depend on (seed, cloud, point) only.  RemoveRandomPoints removes the
 * remove_k points with the smallest 32-bit selection keys, ties to the lower index; selection_keys (P, device, may be
 * null = Philox stream 1) lets a caller with a generator of its own supply the keys. */
int hfl_augment_clouds(float* out_points, int32_t* out_counts, int32_t* out_index, const float* points,
                       const int64_t* cloud_offsets, const int64_t* host_cloud_offsets, int batch,
                       const hfl_augment_cloud* table, const hfl_augment_cloud* host_table,
                       const hfl_augment_config* config, uint64_t seed, int64_t cloud_base,
                       const uint32_t* selection_keys, hfl_stream_t stream);

/* ------------------------------------------------------------------------
 * 2b. Raw submaps: voxel-grid downsampling and the PointNetVLAD normalisation (csrc/voxel.hip; replaces
 *     datasets/CSWildPlaces/postprocess_submaps.py's processing_utils.voxel_down_sample -- open3d's
 *     PointCloud.voxel_down_sample -- and processing_utils.normalise_pcl with downsample_number=None)
 * ---------------------------------------------------------------------- */
#define HFL_VOXEL_MAX_CLOUDS 32767        /* the cloud id has 15 bits of a positive int64 key          */
#define HFL_VOXEL_MAX_CELLS 65535         /* cells a cloud may span along an axis (16 bits, see below) */
#define HFL_VOXEL_MAX_POINTS 2147483646LL /* points of a batch: sorted positions are kept as int32     */
/* keys[i] = cloud << 48 | ix << 32 | iy << 16 | iz for every point of points (P,3), cloud b at rows
 * [cloud_offsets[b], cloud_offsets[b+1]), every cloud non-empty and cloud_offsets[batch] == n_points.  Per cloud
 * origin = double(min p) - 0.5 v and cell = floor((double(p) - origin) / v) per axis, a float64 subtract and divide as open3d
 * computes them, so membership is bit-identical to a float64 restatement, points on a cell face included.  bounds
 * (batch, 6) uint32 is workspace (ordered-integer images of the per-cloud minimum and maximum, found with integer atomics
 * by as many workgroups as the cloud needs).  flags[b] = 1 when cloud b spans HFL_VOXEL_MAX_CELLS + 1 = 65 536 or more
 * cells along an axis: its keys are then clamped, still carry its own cloud id, and its output must be discarded.
 * points and keys 16-byte aligned.  A memset and two launches on `stream`, no synchronisation.  Non-finite coordinates:
 * undefined values, nothing out of bounds.  voxel_size <= 0 or not finite, batch < 1, n_points < batch or a NULL pointer:
 * HFL_EINVAL; more than HFL_VOXEL_MAX_CLOUDS clouds or HFL_VOXEL_MAX_POINTS points: HFL_ECAPACITY. */
int hfl_voxel_keys(int64_t* keys, int32_t* flags, uint32_t* bounds, const float* points, const int64_t* cloud_offsets,
                   int batch, int64_t n_points, double voxel_size, hfl_stream_t stream);
/* bytes of workspace hfl_voxel_reduce needs for n_points points (0 for n_points outside 1..HFL_VOXEL_MAX_POINTS) */
int64_t hfl_voxel_reduce_workspace(int64_t n_points);
/* sorted_keys = the keys of hfl_voxel_keys in ascending order, perm[j] = the row of `points` that sorted position j came from
 * (a stable sort: members of a cell stay in input order).  One output row per distinct key, in key order, i.e. per cloud
 * in ascending (ix, iy, iz): the mean of the cell's points, summed in float64 in a fixed order, divided by the count and
 * rounded once to fp32.  out_points (P,3) receives M <= P rows; out_offsets (batch + 1) int64: cloud b's rows are
 * [out_offsets[b], out_offsets[b+1]), so its output count is their difference and out_offsets[batch] = M;
 * out_cell_counts (P, may be NULL): members per output row; out_keys (P, may be NULL): the row's key.  No floating-point
 * atomics: the same input gives the same bits, and a cloud gives the same bits alone or in a batch.  Four launches on
 * `stream`, no synchronisation.  perm is trusted (values in [0, n_points)).  out_points must not alias points;
 * workspace 16-byte aligned, workspace_bytes >= hfl_voxel_reduce_workspace(n_points), else HFL_EINVAL. */
int hfl_voxel_reduce(float* out_points, int64_t* out_offsets, int32_t* out_cell_counts, int64_t* out_keys,
                     const int64_t* sorted_keys, const int64_t* perm, const float* points, int64_t n_points, int batch,
                     void* workspace, int64_t workspace_bytes, hfl_stream_t stream);
/* normalise_pcl without padding, in float64 per cloud: c = mean q, d = mean |q - c|, s = 0.5 / d, q' = s (q - c); the rows
 * with every |q'| <= 1 are written in order, rounded once to fp32, from row cloud_offsets[b] of out_points (P,3) on and
 * out_counts[b] says how many.  flags[b] = 1 when d is not > 0 (a single point, coincident points) or the cloud is empty:
 * its output is then meaningless.  cloud_offsets (batch + 1) int64 may be hfl_voxel_reduce's out_offsets.  One workgroup
 * per cloud, fixed-order float64 reductions (no atomics), one launch on `stream`.  out_points must not alias points. */
int hfl_submap_normalise(float* out_points, int32_t* out_counts, int32_t* flags, const float* points,
                         const int64_t* cloud_offsets, int batch, hfl_stream_t stream);
/* The padding loop of normalise_pcl (downsample_number set): rows drawn from the raw cloud go through the transform of
 * hfl_submap_normalise -- the same device code, so the same bits: c and s come from the same fixed-order float64
 * reductions over cloud b of `points`, q' = s (q - c) in float64 rounded once to fp32.  Row j of cloud b, j in
 * [row_offsets[b], row_offsets[b+1]), is raw row raw_offsets[b] + row_index[j]; out_rows (R,3) receives q' and keep[j] = 1
 * when every |q'| <= 1.  An index outside the raw cloud, or a cloud whose d is not > 0, gives a zero row with keep = 0.
 * One workgroup per cloud, one launch on `stream`. */
int hfl_submap_normalise_rows(float* out_rows, int32_t* keep, const float* points, const int64_t* cloud_offsets,
                              const float* raw_points, const int64_t* raw_offsets, const int64_t* row_index,
                              const int64_t* row_offsets, int batch, hfl_stream_t stream);
/* out_points[r] = points[index[r]] for r < n_rows (the random rows of the fixed-size downsamplers); an index outside
 * [0, n_points) gives a zero row.  One launch on `stream`. */
int hfl_voxel_gather_rows(float* out_points, const float* points, int64_t n_points, const int64_t* index, int64_t n_rows,
                          hfl_stream_t stream);
/* The first half of hfl_voxel_keys alone: bounds (batch, 6) uint32 receives the ordered-integer images of every cloud's
 * minimum and maximum ([0..2] = ~enc(min), [3..5] = enc(max); enc(f) = bits(f) ^ (sign ? ~0 : 1 << 31)).  Same argument
 * rules as hfl_voxel_keys.  A memset and one launch on `stream`. */
int hfl_voxel_bounds(uint32_t* bounds, const float* points, const int64_t* cloud_offsets, int batch, int64_t n_points,
                     hfl_stream_t stream);
/* One candidate of hfl_voxel_occupancy: cloud `cloud` on a grid of voxel size `voxel`, nx x ny x nz cells (each
 * 1..HFL_VOXEL_MAX_CELLS; the caller derives them from the cloud's bounds with the formula of hfl_voxel_keys), whose bitmap
 * of nx ny nz bits starts at 32-bit word `word_offset` of the call's bitmap area.  Bitmaps must not overlap. */
typedef struct {
  int32_t cloud;
  int32_t nx, ny, nz;
  double voxel;
  int64_t word_offset;
} hfl_voxel_candidate;
#define HFL_VOXEL_OCC_MAX_CANDIDATES 65535    /* one grid row per candidate                       */
#define HFL_VOXEL_OCC_MAX_WORDS 67108863LL    /* < 2^31 bits per call, so a count fits its int32 */
/* bytes of workspace for n_candidates candidates whose bitmaps take bitmap_words 32-bit words together (0 when out of range) */
int64_t hfl_voxel_occupancy_workspace(int n_candidates, int64_t bitmap_words);
/* counts[k] = the number of distinct cells that candidate k's cloud occupies at its voxel size, with a point's cell exactly
 * the one hfl_voxel_keys computes (same device functions), so counts[k] = the rows hfl_voxel_reduce would return for that
 * cloud and size.  `candidates` is HOST memory (n_candidates rows): it is checked here -- every bitmap inside the bitmap
 * area -- and copied into the workspace; bounds is what hfl_voxel_bounds / hfl_voxel_keys left for the same points.  A point
 * whose cell lies outside a candidate's nx x ny x nz (a table that does not match the bounds) is skipped, never written.
 * max_cloud_points (the largest cloud) only sizes the grid.  Integer OR atomics on bitmaps (in LDS when a bitmap fits
 * 32 KiB, else in global memory), then a popcount: exact and order-independent, no workgroup waits for another.  A copy,
 * a memset and two launches on `stream`.  workspace 16-byte aligned, workspace_bytes >= hfl_voxel_occupancy_workspace. */
int hfl_voxel_occupancy(int32_t* counts, const hfl_voxel_candidate* candidates, int n_candidates, int64_t bitmap_words,
                        const uint32_t* bounds, const float* points, const int64_t* cloud_offsets, int batch,
                        int64_t n_points, int64_t max_cloud_points, void* workspace, int64_t workspace_bytes,
                        hfl_stream_t stream);

/* ------------------------------------------------------------------------
 * 2c. Raw submaps: ground removal by the Cloth Simulation Filter (csrc/ground.hip; replaces
 *     datasets/CSWildPlaces/postprocess_submaps.py --remove_ground, i.e. processing_utils.remove_ground and the pip CSF
 *     package behind it).  The filter is defined in hotformerloc_amd/ground.py and DESIGN.md section 7f: fp32, z up,
 *     u = -z, every operation rounded once; bit parity with the pip package is not claimed.
 * ---------------------------------------------------------------------- */
#define HFL_CLOTH_MAX_PARTICLES 10240     /* width * height of one cloth: u, u_prev, t and the flags stay in LDS (130 KiB) */
/* One cloud's cloth: particle (i, j), i < width, j < height, stands at (ox + i r, oy + j r) and is element
 * cell_offset + j * width + i of the particle arrays; u0 is the start height max(-z) + 0.05.  The caller derives the
 * fields from the cloud's fp32 bounds (hfl_voxel_bounds) as the definition says. */
typedef struct {
  float ox, oy, u0;
  int32_t width, height;
  int32_t reserved;
  int64_t cell_offset;
} hfl_cloth_desc;
/* Every hfl_cloth_* call takes the table twice: descs_host (HOST memory, batch rows) is checked before anything runs --
 * 2 <= width, height, width * height <= HFL_CLOTH_MAX_PARTICLES, the cloth inside [0, n_cells), finite ox, oy, u0, else
 * HFL_EINVAL -- and descs is the same table in device memory, which the kernels read.
 *
 * terrain (n_cells) receives every particle's terrain value t: -z of the point that maps to the particle
 * (col = int((x - ox) / r + 0.5), likewise row, clamped into the cloth) with the smallest squared horizontal distance to
 * it, ties to the lowest point index -- one 64-bit integer atomic min per point on keys (n_cells, scratch), exact and
 * order-independent -- and for a particle no point maps to, the value of the rastered particle the definition names
 * (same row towards larger i, then smaller i, same column towards smaller j, then larger j, then the nearest in index
 * distance with ties to the lowest j, then i).  A memset and two launches on `stream`. */
int hfl_cloth_raster(float* terrain, uint64_t* keys, const hfl_cloth_desc* descs_host, const hfl_cloth_desc* descs, int batch,
                     int64_t n_cells, const float* points, const int64_t* cloud_offsets, int64_t n_points, float resolution,
                     hfl_stream_t stream);
/* The simulation and (slope_smooth != 0) the slope smoothing, one workgroup per cloud with its state in LDS: heights
 * (n_cells) fp32 receives u, movable (n_cells) uint8 the flags and steps_run (batch) the number of steps.  f_one and f_two
 * are the one- and two-sided pair factors, gravity_step = -(0.2 dt^2) and velocity_keep = 1 - damping, all rounded to
 * fp32 by the caller.  One launch on `stream`; no workgroup waits for another. */
int hfl_cloth_simulate(float* heights, uint8_t* movable, int32_t* steps_run, const float* terrain,
                       const hfl_cloth_desc* descs_host, const hfl_cloth_desc* descs, int batch, int64_t n_cells, float f_one,
                       float f_two, float gravity_step, float velocity_keep, int iterations, int slope_smooth,
                       hfl_stream_t stream);
/* keep[p] = 0 where point p is ground -- |(-z) - h| < threshold, h the bilinear cloth height at the point -- else 1.
 * One launch on `stream`.  Non-finite coordinates: undefined values, nothing out of bounds. */
int hfl_cloth_classify(uint8_t* keep, const float* heights, const hfl_cloth_desc* descs_host, const hfl_cloth_desc* descs,
                       int batch, int64_t n_cells, const float* points, const int64_t* cloud_offsets, int64_t n_points,
                       float resolution, float threshold, hfl_stream_t stream);

/* ------------------------------------------------------------------------
 * 2d. Raw submaps: statistical outlier removal and the radius trim (csrc/outliers.hip; replaces
 *     datasets/CSWildPlaces/processing_utils.py remove_outliers, i.e. open3d's remove_statistical_outlier, and the radius
 *     cut of postprocess_wildplaces_ground.py).  The filter is defined in hotformerloc_amd/outliers.py and DESIGN.md
 *     section 7g: fp32 squared distances (dx dx + dy dy) + dz dz, every operation rounded once; bit parity with open3d is
 *     not claimed.
 * ---------------------------------------------------------------------- */
#define HFL_KNN_MAX_NEIGHBOURS 32         /* k of one cloud: the register list of the query is 8, 16 or 32 floats long */
#define HFL_KNN_MAX_CELLS 268435455LL     /* cells of all grids of a call: the cell-start table holds one int32 per cell */
#define HFL_KNN_PHASE_STARTS 1            /* the launches of hfl_knn_mean_dist, for running them one at a time */
#define HFL_KNN_PHASE_QUERY 2
#define HFL_KNN_PHASE_FALLBACK 4
#define HFL_KNN_PHASE_ALL 7
/* One cloud's search grid: nx x ny x nz cubic cells of edge `cell` from the corner (ox, oy, oz) = the cloud's fp32 minimum;
 * a point's cell along an axis is int((p - o) / cell) in fp32, clamped into the grid; cell (ix, iy, iz) is entry
 * cell_base + (iz ny + iy) nx + ix of the cell-start table.  k = min(nb_neighbors, points of the cloud).  mx, my, mz >= 0
 * are the absolute margins by which the query shrinks its distance to a face of the scanned block along each axis
 * (the caller sets 2^-20 of the grid's extent: sixteen times the worst rounding error of the cell assignment). */
typedef struct {
  float ox, oy, oz, cell;
  float mx, my, mz;
  int32_t k;
  int32_t nx, ny, nz;
  int32_t reserved;
  int64_t cell_base;
} hfl_knn_grid;
/* flags[b] = 1 when cloud b holds a coordinate that is not finite, else 0 (the bounds of hfl_voxel_bounds cannot say: fminf
 * and fmaxf drop a NaN).  A memset and one launch on `stream`; integer OR atomics. */
int hfl_cloud_nonfinite(int32_t* flags, const float* points, const int64_t* cloud_offsets, int batch, int64_t n_points,
                        hfl_stream_t stream);
/* Every hfl_knn_* call takes the grids twice, as the hfl_cloth_* calls take their table: grids_host (HOST memory, batch
 * rows) is checked before anything runs -- 1 <= nx, ny, nz, 1 <= k <= HFL_KNN_MAX_NEIGHBOURS, the grid inside
 * [0, n_cells), finite corner, cell > 0, margins >= 0, else HFL_EINVAL -- and grids is the same table in device memory.
 *
 * keys[p] = the global cell of point p (cell_base of its cloud + its cell).  One launch on `stream`. */
int hfl_knn_cell_keys(int64_t* keys, const hfl_knn_grid* grids_host, const hfl_knn_grid* grids, int batch, int64_t n_cells,
                      const float* points, const int64_t* cloud_offsets, int64_t n_points, hfl_stream_t stream);
/* avg[p] = the mean over the k nearest points of p's own cloud, p itself included, of the distance to them: the k smallest
 * fp32 squared distances, the correctly rounded root of each, added in ascending order from 0, divided by (float)k.  Exact
 * (no approximate search) and a pure function of the input: the same bits for any grid.  sorted_keys / perm are the keys of
 * hfl_knn_cell_keys in ascending order and the permutation of the sort (sorted position j came from row perm[j]);
 * sorted_points (P,3) = points[perm].  cell_starts (n_cells + 1) int32, pending (P) int32 and counter (1) int32 are
 * workspace; after the call *counter is the number of points the 3 x 3 x 3 block did not resolve, which the whole-cloud
 * scan finished.  `phases` selects the launches (HFL_KNN_PHASE_ALL for the whole; a later phase needs the workspace an
 * earlier one left).  A memset and three launches on `stream`, no synchronisation, no floating-point atomics. */
int hfl_knn_mean_dist(float* avg, int32_t* pending, int32_t* counter, int32_t* cell_starts, const float* sorted_points,
                      const int64_t* sorted_keys, const int64_t* perm, const hfl_knn_grid* grids_host,
                      const hfl_knn_grid* grids, int batch, int64_t n_cells, const int64_t* cloud_offsets, int64_t n_points,
                      int phases, hfl_stream_t stream);
/* Surface normals by the same search (csrc/normals.hip; defined in hotformerloc_amd/normals.py and DESIGN.md section 7j).
 * With r2 the k-th smallest fp32 squared distance of point p and N(p) every point of its cloud with d2 <= r2 (ties at the
 * k-th place all included, p itself too): counts[p] = |N(p)|; in float64 about p itself S1 = sum e, S2 = sum e e^T over
 * e = q - p, C = S2 / m - (S1 / m)(S1 / m)^T; a one-sided cyclic Jacobi of fixed sweep count gives the eigenvalues
 * l0 <= l1 <= l2; normals[p] (3 floats) = the unit eigenvector of l0, curvature[p] = l0 / (l0 + l1 + l2).  m < 3 or
 * l1 <= 1e-12 l2: normal (0, 0, 0), curvature 0 -- a zero normal says "no normal".  Sign: viewpoints (DEVICE, batch x 3
 * float64, one per cloud) not NULL: n . (viewpoint - p) >= 0; NULL: n_z > 0, else n_y > 0, else n_x > 0.  The other
 * arguments, the workspace and `phases` are those of hfl_knn_mean_dist; outputs are in INPUT order (row perm[j]).  counts is
 * a pure function of the input; the float64 sums run in an order fixed by the sort and the grid, so two calls give the
 * same bits and two grids agree to rounding.  A memset and three launches on `stream`, no floating-point atomics. */
int hfl_knn_normals(float* normals, float* curvature, int32_t* counts, int32_t* pending, int32_t* counter,
                    int32_t* cell_starts, const float* sorted_points, const int64_t* sorted_keys, const int64_t* perm,
                    const hfl_knn_grid* grids_host, const hfl_knn_grid* grids, int batch, int64_t n_cells,
                    const int64_t* cloud_offsets, int64_t n_points, const double* viewpoints, int phases,
                    hfl_stream_t stream);
/* Radius and hybrid neighbourhoods on the same search.  radius2 is R2, the largest fp32 squared
 * distance that counts as "within the radius" (what sqrtf(d2) <= radius admits), one value for every cloud of the call;
 * >= 0, +inf allowed, a NaN or a negative value: HFL_EINVAL.  radius_only == 0 (hybrid): r2 = min(k-th smallest, R2), so
 * |N(p)| may lie below k, down to 1; with R2 = +inf this is hfl_knn_normals bit for bit, which calls it so.
 * radius_only != 0: r2 = R2 for every point, |N(p)| has no cap, the grids' k is checked (1 .. HFL_KNN_MAX_NEIGHBOURS) but
 * not read; no register list and no first scan -- one pass over the 3 x 3 x 3 block where the completeness bound proves
 * that it holds every point within R2 (always, when cell >= about the radius), one pass of a wave over the cloud for the
 * others.  Everything else as hfl_knn_normals. */
int hfl_knn_normals_radius(float* normals, float* curvature, int32_t* counts, int32_t* pending, int32_t* counter,
                           int32_t* cell_starts, const float* sorted_points, const int64_t* sorted_keys,
                           const int64_t* perm, const hfl_knn_grid* grids_host, const hfl_knn_grid* grids, int batch,
                           int64_t n_cells, const int64_t* cloud_offsets, int64_t n_points, const double* viewpoints,
                           float radius2, int radius_only, int phases, hfl_stream_t stream);
/* counts[p] (INPUT order) = the number of points of p's own cloud with d2 <= radius2, p itself included: the radius-only
 * search of hfl_knn_normals_radius with a count for its work (csrc/outliers.hip; open3d's remove_radius_outlier counts this
 * set).  An integer and a pure function of the input: the same for any grid.  Workspace and `phases` as hfl_knn_mean_dist. */
int hfl_knn_radius_count(int32_t* counts, int32_t* pending, int32_t* counter, int32_t* cell_starts,
                         const float* sorted_points, const int64_t* sorted_keys, const int64_t* perm,
                         const hfl_knn_grid* grids_host, const hfl_knn_grid* grids, int batch, int64_t n_cells,
                         const int64_t* cloud_offsets, int64_t n_points, float radius2, int phases, hfl_stream_t stream);
/* keep[p] = counts[p] > nb_points (nb_points >= 0).  One launch on `stream`. */
int hfl_count_mask(uint8_t* keep, const int32_t* counts, int64_t n_points, int32_t nb_points, hfl_stream_t stream);
/* ISS keypoints (csrc/keypoints.hip; defined in hotformerloc_amd/keypoints.py and DESIGN.md section 7t): two radius-only
 * searches on ONE sorted batch laid out for the larger of the two radii.  Workspace and `phases` as hfl_knn_mean_dist.
 *
 * hfl_iss_saliency: over N(p) = { q : d2 <= radius2 } (p itself included, m = |N(p)|) the float64 sums and the ordered
 * eigenvalues l0 <= l1 <= l2 of hfl_knn_normals; the saliency is float(l0) where m >= max(min_neighbors, 3), l1 < gamma_21 l2
 * and l0 < gamma_32 l1 (float64 products, a NaN fails), else 0.  It is written twice: sorted_saliency (P) by SORTED position,
 * for hfl_iss_select, and saliency (P) in INPUT order; counts (P) int32 = m in INPUT order.  gamma_21, gamma_32 in (0, 1],
 * min_neighbors >= 1, radius2 >= 0 (+inf allowed), else HFL_EINVAL.  counts and the set of zeros do not depend on the grid,
 * the values do to rounding; two runs give the same bits. */
int hfl_iss_saliency(float* saliency, float* sorted_saliency, int32_t* counts, int32_t* pending, int32_t* counter,
                     int32_t* cell_starts, const float* sorted_points, const int64_t* sorted_keys, const int64_t* perm,
                     const hfl_knn_grid* grids_host, const hfl_knn_grid* grids, int batch, int64_t n_cells,
                     const int64_t* cloud_offsets, int64_t n_points, float radius2, double gamma_21, double gamma_32,
                     int min_neighbors, int phases, hfl_stream_t stream);
/* hfl_iss_select: mask (P) uint8 in INPUT order, 1 where the point's saliency s is > 0, at least min_neighbors points of its
 * cloud lie within radius2 (itself included), and none of them has a saliency > s, or == s at a lower input row.
 * sorted_saliency (P) is indexed by SORTED position (saliency[perm]); any fp32 values, a NaN is no candidate and beats
 * nobody.  Integers and comparisons only: a pure function of the points and the saliency, the same for any grid. */
int hfl_iss_select(uint8_t* mask, int32_t* pending, int32_t* counter, int32_t* cell_starts, const float* sorted_points,
                   const int64_t* sorted_keys, const int64_t* perm, const float* sorted_saliency,
                   const hfl_knn_grid* grids_host, const hfl_knn_grid* grids, int batch, int64_t n_cells,
                   const int64_t* cloud_offsets, int64_t n_points, float radius2, int min_neighbors, int phases,
                   hfl_stream_t stream);
/* FPFH descriptors by the same search (csrc/fpfh.hip; defined in hotformerloc_amd/fpfh.py and DESIGN.md section 7k), in
 * three calls that share the workspace of hfl_knn_mean_dist.  Everything but the last output is indexed by SORTED position.
 *
 * hfl_fpfh_radius: r2[j] = the k-th smallest fp32 squared distance of sorted point j within its cloud (itself included);
 * proven[j] = 1 when the 3 x 3 x 3 block of cells round j holds every point with d2 <= r2[j], else 0 and j is in pending;
 * *counter = the number of such points.  The cell-start table, a memset and two launches on `stream`. */
int hfl_fpfh_radius(float* r2, uint8_t* proven, int32_t* pending, int32_t* counter, int32_t* cell_starts,
                    const float* sorted_points, const int64_t* sorted_keys, const hfl_knn_grid* grids_host,
                    const hfl_knn_grid* grids, int batch, int64_t n_cells, const int64_t* cloud_offsets, int64_t n_points,
                    hfl_stream_t stream);
/* hfl_fpfh_radius with radius2 and radius_only as hfl_knn_normals_radius takes them.  Hybrid: r2[j] = min(k-th smallest,
 * R2).  Radius-only: r2[j] = R2 for every point, proven[j] from the completeness bound alone, one launch and no scan.
 * hfl_fpfh_spfh and hfl_fpfh_combine read r2 and proven and never k, so they follow either unchanged. */
int hfl_fpfh_radius_capped(float* r2, uint8_t* proven, int32_t* pending, int32_t* counter, int32_t* cell_starts,
                           const float* sorted_points, const int64_t* sorted_keys, const hfl_knn_grid* grids_host,
                           const hfl_knn_grid* grids, int batch, int64_t n_cells, const int64_t* cloud_offsets,
                           int64_t n_points, float radius2, int radius_only, hfl_stream_t stream);
/* hist (P, 33) int32 and pairs (P) int32: the SPFH histogram of every point over N(j) = { q : d2 <= r2[j] } and the number
 * of pairs binned; three groups of 11 bins (theta, f2, f3 of the Darboux frame).  sorted_normals (P, 3) = normals[perm]; a
 * zero row, or one with a component that is not finite, is "no normal".  theta_table_host: HOST memory, 10 rows of
 * (cos e_k, sin e_k) float64 for the bin edges e_k = -pi + 2 pi k / 11, k = 1 .. 10 (passed on by value; not finite:
 * HFL_EINVAL).  r2, proven, pending, counter and cell_starts as hfl_fpfh_radius left them.  Integers only: the result
 * depends on no order and no grid.  Two launches on `stream`, 33 KiB of LDS a workgroup. */
int hfl_fpfh_spfh(int32_t* hist, int32_t* pairs, const float* r2, const uint8_t* proven, const int32_t* pending,
                  const int32_t* counter, const int32_t* cell_starts, const float* sorted_points,
                  const float* sorted_normals, const int64_t* sorted_keys, const hfl_knn_grid* grids_host,
                  const hfl_knn_grid* grids, int batch, int64_t n_cells, const int64_t* cloud_offsets, int64_t n_points,
                  const double* theta_table_host, hfl_stream_t stream);
/* fpfh (P, 33) fp32 in INPUT order (row perm[j]): SPFH_j(b) = 100 hist[j][b] / pairs[j] (0 without pairs) plus, per group,
 * (100 / s) W(b) when s > 0, with W(b) = the sum over q in N(j), q != j, d2 > 0, pairs[q] > 0 of
 * hist[q][b] ((100 / pairs[q]) / d2) in float64 and s the sum of W over the group.  The sums run in an order fixed by the
 * sort and the grid: two calls give the same bits, two grids agree to an fp32 ulp.  Two launches on `stream`. */
int hfl_fpfh_combine(float* fpfh, const int32_t* hist, const int32_t* pairs, const float* r2, const uint8_t* proven,
                     const int32_t* pending, const int32_t* counter, const int32_t* cell_starts, const float* sorted_points,
                     const int64_t* sorted_keys, const int64_t* perm, const hfl_knn_grid* grids_host,
                     const hfl_knn_grid* grids, int batch, int64_t n_cells, const int64_t* cloud_offsets, int64_t n_points,
                     hfl_stream_t stream);
#define HFL_FEATURE_ROWS 512              /* query rows of a 256-thread workgroup of hfl_feature_nn (two per thread) */
#define HFL_FEATURE_MAX_DIM 64            /* columns of a feature row */
/* Nearest neighbour in feature space for ragged pairs, brute force (csrc/fpfh.hip): queries (Nq, dim) and targets (Nt, dim)
 * fp32 with (n_pairs + 1) int64 offsets each, 1 <= dim <= HFL_FEATURE_MAX_DIM; tiles (n_tiles, 2) int64 rows of (pair, first
 * query row), HFL_FEATURE_ROWS rows of one pair per workgroup.  dist2[r] = the smallest squared distance from query row r to
 * a target row of its pair, in fp32 on the differences: d0 d0, then fmaf(dc, dc, .) for c = 1 .. dim - 1; idx[r] = that
 * row's index within the pair's targets, the lowest of equal distances; +inf and -1 for an empty target.  Inputs must be
 * finite (a query whose every d2 is +inf or NaN reports -1).  Rows the table does not cover stay unwritten.  One launch on
 * `stream`, no atomics.  n_targets, n_tiles or n_pairs at 2^31 or more: HFL_ECAPACITY. */
int hfl_feature_nn(float* dist2, int32_t* idx, const float* queries, const int64_t* q_offsets, int64_t n_queries,
                   const float* targets, const int64_t* t_offsets, int64_t n_targets, int dim, const int64_t* tiles,
                   int64_t n_tiles, int64_t n_pairs, hfl_stream_t stream);
/* stats (batch, 4) float64 = (mean, std, mean + std_ratio std, n_valid) over the valid rows (avg > 0) of every cloud, std
 * with n_valid - 1 in the denominator; float64, summed in the order of hfl_pair_stats.  No valid row: mean = NaN; one: std =
 * NaN.  One workgroup per cloud, one launch on `stream`.  std_ratio <= 0 or not finite: HFL_EINVAL. */
int hfl_outlier_threshold(double* stats, const float* avg, const int64_t* cloud_offsets, int batch, int64_t n_points,
                          double std_ratio, hfl_stream_t stream);
/* keep[p] = 1 when avg[p] > 0 and double(avg[p]) < the threshold of p's cloud (stats[b][2]; NaN keeps nothing), else 0. */
int hfl_outlier_mask(uint8_t* keep, const float* avg, const double* stats, const int64_t* cloud_offsets, int batch,
                     int64_t n_points, hfl_stream_t stream);
/* keep[p] = 1 when sqrt(x x + y y) <= radius_max, evaluated in float64 from the fp32 coordinates, every operation rounded
 * once (what numpy's norm over the first two columns computes), else 0.  radius_max <= 0 or not finite: HFL_EINVAL. */
int hfl_radius_mask(uint8_t* keep, const float* points, int64_t n_points, double radius_max, hfl_stream_t stream);

/* ------------------------------------------------------------------------
 * 3. Octree convolution gather  (ocnn.nn.OctreeConv's octree2col; call sites
 *    models/layers/octformer_layers.py:89-95, models/octformer_backbone.py:470-475)
 * ---------------------------------------------------------------------- */

/* out[m, k*C + c] = neigh[m,k] >= 0 ? data[neigh[m,k], c] : 0 ;  out (n_out, K*C) */
int hfl_octree_gather(float* out, const float* data, const int32_t* neigh, int64_t n_out,
                      int kngh, int64_t channels, hfl_stream_t stream);

/* Live-tap lists of a (rows, taps) int32 index table, taps <= 32 (ocnn.nn.OctreeConv multiplies an (N, K*Cin)
 * octree2col matrix that is 80-94 % zeros on surface-like clouds; the convolutions here run over the live
 * (row, tap) pairs only):
 *   src   (rows*taps capacity) input row of every live pair, pairs ordered by tap then by row; the first
 *         edges[taps] entries are written
 *   slot  (rows, taps)         position of (row, tap) in that list, -1 where the neighbour is missing
 *   edges (taps + 1)           pairs of tap k are [edges[k], edges[k+1])          -- all on the device
 * No atomics, fixed order, no host synchronisation; `workspace` holds hfl_tap_lists_workspace() bytes. */
int64_t hfl_tap_lists_workspace(int64_t rows, int taps);
int hfl_tap_lists(int32_t* src, int32_t* slot, int32_t* edges, const int32_t* table, int64_t rows, int taps,
                  void* workspace, hfl_stream_t stream);
/* The same for n <= 16 tables in THREE launches in all (count, scan, fill over every table: the convolution depths of one
 * batch); arrays of n pointers / sizes, workspace[i] = hfl_tap_lists_workspace(rows[i], taps[i]) bytes. */
int hfl_tap_lists_multi(int n, int32_t* const* src, int32_t* const* slot, int32_t* const* edges, const int32_t* const* table,
                        const int64_t* rows, const int32_t* taps, void* const* workspace, hfl_stream_t stream);
/* Row tiles of the grouped tap GEMM (section 9b, hfl_linear_x3_grouped) from the device-side tap edges hfl_tap_lists wrote:
 * tiles (n_tiles, 3) int32 = {first pair, pairs (<= tile_rows), tap * w_rows}, n_tiles = sum_k ceil(pairs_k / tile_rows). */
int hfl_tap_tiles(int32_t* tiles, const int32_t* edges, int taps, int tile_rows, int w_rows, hfl_stream_t stream);
/* Padded gather index of a ragged per-cloud row stream (pooling head, models/layers/pooling.py:209-233): out (batch * nmax)
 * int64, row_off[b] + j inside cloud b, row_off[batch] (a zero row the caller appends) beyond it. */
int hfl_pad_index(int64_t* out, const int64_t* row_off, int batch, int64_t nmax, hfl_stream_t stream);
/* The padded copy itself in one pass: out (batch, nmax, channels) f32, rows of cloud b = x[row_off[b] ..), zeros beyond
 * (the per-cloud split + zero padding of models/layers/pooling.py:209-233 without an index table or an appended zero row). */
int hfl_pad_rows(float* out, const float* x, const int64_t* row_off, int batch, int64_t nmax, int64_t channels,
                 hfl_stream_t stream);
/* Attentional pooling of a level's ragged per-cloud rows by learned queries as ONE launch (+ a combine when the rows of a
 * cloud are split over workgroups) -- AdaptivePooling.forward, models/layers/salsa.py:25-55, per level from
 * PyramidAttnPoolWrapper.forward, models/layers/pooling.py:209-233:
 *     out[b, q, :] = sum_r softmax_r(scale * <query[q], x[r]>) x[r],   r over rows row_off[b] .. row_off[b + 1] of x (n_rows, C)
 * out + b * out_cloud_stride + q * C is row q of cloud b (so a level can write its slice of the concatenated token matrix).
 * Products as bf16 (hi, lo) splits with fp32 accumulation, softmax in fp32.  channels in {128, 256} (hfl_attn_pool_ok);
 * workspace: hfl_attn_pool_workspace bytes (without it a cloud's rows stay in one workgroup per 64 queries). */
/* Tail of the Mixer aggregator, models/layers/salsa.py:104-111 (channel_proj over the token axis, row_proj over the channel
 * axis, flatten) in one launch: out (batch, k_out * out_d), x (batch, k_tokens, channels), channel_w (k_out, k_tokens),
 * row_w (out_d, channels); out_d <= 8.  row_proj is applied first (the two maps commute): same value up to fp32 summation
 * order. */
int hfl_mixer_tail(float* out, const float* x, const float* channel_w, const float* channel_b, const float* row_w,
                   const float* row_b, int batch, int k_tokens, int channels, int k_out, int out_d, hfl_stream_t stream);
/* Every FeatureMixerLayer of the Mixer aggregator (models/layers/salsa.py:58-111) and row_proj as ONE launch
 * (csrc/mixer_chain.hip), x (M, 256) f32 rows:
 *     for l < layers:  x = x + fc2_l(gelu(fc1_l(LN_l(x))))        u[row, j] = sum_c x[row, c] row_w[j, c],  j < out_d
 * with the arithmetic of `layers` calls of hfl_ln_mlp_fused_h at every hand-off (only f32 summation orders differ) and the
 * f32 dot of hfl_mixer_tail.  hfl_mixer_chain_ok: 1 for channels = hidden = 256, 1 <= layers <= 4, 0 <= out_d <= 8.
 * packs: hfl_mixer_chain_pack_bytes(layers) bytes (0 = unsupported) written by hfl_mixer_chain_pack from the fp32 weights
 * w1[l] (256, 256), w2[l] (256, 256), once per parameter set.  gamma / beta / b1 / b2 / w1 / w2: host arrays of `layers` device
 * pointers.  out_x (M, 256) and out_u (M, out_d) are each written only when given: out_d > 0 needs out_u and row_w, out_d = 0
 * needs out_x and no out_u.  out_x may be x.  Anything else: HFL_EINVAL, nothing launched. */
int hfl_mixer_chain_ok(int channels, int hidden, int layers, int out_d);
int64_t hfl_mixer_chain_pack_bytes(int layers);
int hfl_mixer_chain_pack(void* dst, const float* const* w1, const float* const* w2, int layers, hfl_stream_t stream);
int hfl_mixer_chain_x3(float* out_x, float* out_u, const float* x, const void* packs, const float* const* gamma,
                       const float* const* beta, const float* const* b1, const float* const* b2, float eps, const float* row_w,
                       int64_t M, int layers, int out_d, hfl_stream_t stream);
/* The rest of hfl_mixer_tail for u (batch, k_tokens, out_d) = row_proj without its bias (hfl_mixer_chain_x3's out_u):
 *     out[b, o * out_d + j] = sum_t channel_w[o, t] u[b, t, j] + channel_b[o] sum_c row_w[j, c] + row_b[j]
 * in hfl_mixer_tail's order and arithmetic; normalize != 0: the row divided by max(||row||_2, 1e-12) (F.normalize(out, dim=1)),
 * the norm summed in a fixed order.  One workgroup per cloud. */
int hfl_descriptor_tail(float* out, const float* u, const float* channel_w, const float* channel_b, const float* row_w,
                        const float* row_b, int batch, int k_tokens, int channels, int k_out, int out_d, int normalize,
                        hfl_stream_t stream);
int hfl_attn_pool_ok(int channels);
int64_t hfl_attn_pool_workspace(int batch, int n_queries, int channels, int64_t n_rows);
int hfl_attn_pool(float* out, int64_t out_cloud_stride, const float* x, const int64_t* row_off, const float* query, int batch,
                  int n_queries, int channels, int64_t n_rows, float scale, void* workspace, int64_t workspace_bytes,
                  hfl_stream_t stream);

/* ------------------------------------------------------------------------
 * 4. Windowed multi-head attention over z-order octree windows
 *    (replaces OctreeAttention.forward's bias build + SDPA,
 *     models/octformer_backbone.py:59-88, RPE models/layers/octformer_layers.py:159-170,
 *     masks models/octree.py:186-222,267-283, window (un)packing models/octree.py:346-386)
 * ---------------------------------------------------------------------- */
typedef struct {
  int64_t n_tokens;     /* N_t: real tokens of this depth (rows 0..N_t-1 of qkv/out)    */
  int64_t rt_row0;      /* first relay-token row in qkv/out (G=1), ignored when G=0     */
  int32_t n_windows;    /* W = ceil(N_t / (K*D_pad)) * D_pad   (models/octree.py:73-75) */
  int32_t patch_size;   /* K  (48 or 64)                                                 */
  int32_t dilation;     /* D  (1, or the stage dilation 4 for odd OctFormer blocks)     */
  int32_t n_relay;      /* G  (0 or 1)                                                   */
  int32_t n_heads;      /* H, head dim is fixed at 16                                    */
  int32_t pos_bnd;      /* int(0.8*K*sqrt(D)), rpe table has 3*(2*pos_bnd+1) rows        */
  int32_t batch_size;   /* B: batch id given to padding                                  */
  float scale;          /* 16^-0.5                                                       */
  int32_t depth;        /* octree depth of the tokens (coords < 2^depth); 0 = unknown    */
  const float* rpe_expanded; /* optional: hfl_window_rpe_expand(rpe_table, depth) output, enables
                              * the two-lookup forward kernel; NULL = three axis lookups     */
} hfl_window_attn_desc;

/* qkv (rows, 3*H*16): per row [q(H,16) | k(H,16) | v(H,16)], the layout produced by
 * `self.qkv(data).reshape(-1, K+G, 3, H, C//H)`.  tok_meta (N_t) uint2 per token:
 * .x = x | y<<10 | z<<20 (node coords at this depth), .y = batch id.
 * rpe_table (3*(2*pos_bnd+1), H) float32 or NULL (disable_RPE).
 * out (rows, H*16).  Window w covers tokens  w*K+k  (D=1)  or
 * (w/D)*K*D + k*D + (w%D)  (dilated), k in [0,K).  Relay token of window w is row
 * rt_row0 + w and carries the batch id of the window's first token. */
int hfl_window_attention_fwd(float* out, const float* qkv, const uint32_t* tok_meta,
                             const float* rpe_table, const hfl_window_attn_desc* desc,
                             hfl_stream_t stream);

/* As hfl_window_attention_fwd, for the split-precision Linear path: qkv comes from a bias-free GEMM
 * and `qkv_bias` (3*H*16) is added to q, k, v on load (NULL = none); with out_split3 != 0 `out` is the
 * bf16 A operand [hi | hi | lo] (rows, 3*H*16) of the output projection (section 9). */
/* 1 when hfl_window_attention_fwd_ex takes the fp16 (hi, lo) qkv layout of hfl_linear_x3_qkv for this configuration
 * (`out_split3 | 0x100`; depth <= 5 with coordinates inside pos_bnd, <= 72 KiB of LDS), else 0: use fp32 qkv. */
int hfl_window_attention_f16_ok(const hfl_window_attn_desc* desc, int64_t n_rows_total);
int hfl_window_attention_fwd_ex(void* out, const float* qkv, const float* qkv_bias,
                                const uint32_t* tok_meta, const float* rpe_table,
                                const hfl_window_attn_desc* desc, int out_split3, hfl_stream_t stream);
/* n (<= 4) independent attention problems on fp16 (hi, lo) qkv operands (out_split3 carries 0x100) as ONE launch when they
 * have one shape (patch_size, n_relay, n_heads, table form), else one launch each: arrays of the arguments of
 * hfl_window_attention_fwd_ex (no qkv_bias).  Small problems ride along with a large one instead of paying a launch each. */
int hfl_window_attention_fwd_multi(int n, void* const* out, const float* const* qkv, const uint32_t* const* tok_meta,
                                   const float* const* rpe_table, const hfl_window_attn_desc* const* desc, int out_split3,
                                   hfl_stream_t stream);

/* Expanded relative-position table for the forward kernels, scaled by log2(e); which form is built depends on the consumer:
 *   f16_operand = 0 (fp32 qkv kernel): per head the x-axis table restricted to |dx| <= R = 2^depth - 1 followed by the
 *     pre-added (dy, dz) table of (2R+1)^2 entries; valid when R <= pos_bnd and depth <= 5 (size() returns 0 otherwise:
 *     the three-lookup kernel reads rpe_table itself)
 *   f16_operand = 1 (fp16 (hi, lo) qkv kernel, flag 0x100 of hfl_window_attention_fwd_ex): that form up to depth 4; from
 *     depth 5 (and whenever R > pos_bnd) three 1-D tables over the full coordinate range with the reference's clamp baked
 *     in (depth <= 7)
 *   f16_operand = 2: the three 1-D tables at every depth <= 7 (what the fp16 kernel reads from depth 5 on, for any depth)
 * out holds hfl_window_rpe_expand_size() floats; rebuild it whenever rpe_table changes.  A table built for one consumer
 * must not be handed to the other. */
int64_t hfl_window_rpe_expand_size(int n_heads, int pos_bnd, int depth, int f16_operand);
int hfl_window_rpe_expand(float* out, const float* rpe_table, int n_heads, int pos_bnd, int depth, int f16_operand,
                          hfl_stream_t stream);

/* Linear on the split operands through hipBLASLt, with the block's epilogue in the same launch:
 *   out (n_rows, out_features) f32 = a (n_rows, k_concat) bf16 . w (out_features, k_concat)^T bf16
 *                                    [+ bias (out_features) f32] [+ residual (n_rows, out_features) f32]
 * a / w are the K-concatenated [hi|hi|lo] / [hi|lo|hi] operands of section 9 (k_concat = 3 * in_features),
 * fp32 accumulation.  Replaces `x = x + proj(attn)` / `x = x + mlp(x)` of
 * models/octformer_backbone.py:275-278 and models/hotformerloc_backbone.py:213-216 (Linear + bias +
 * residual add) without a separate pass over the residual stream.  bias / residual may be NULL;
 * residual must not alias out.  Returns HFL_EBACKEND - status when the library rejects the problem. */
int hfl_gemm_bf16(float* out, const uint16_t* a, const uint16_t* w, const float* bias, const float* residual,
                  int64_t n_rows, int out_features, int k_concat, hfl_stream_t stream);

/* Weight gradient of that Linear (training path): out (n_out, k_out) f32 = a^T b with the contraction over the
 * n_rows_stacked = 3M rows of  a = [dy_hi; dy_hi; dy_lo] (3M, n_out) bf16  and  b = [x_hi; x_lo; x_hi] (3M, k_out)
 * bf16, i.e. dW = dy^T x to the same 2^-17 operand accuracy as the forward (torch autograd of nn.Linear). */
int hfl_gemm_bf16_tn(float* out, const uint16_t* a, const uint16_t* b, int64_t n_rows_stacked, int n_out,
                     int k_out, hfl_stream_t stream);

/* Test / measurement hook: select a kernel variant at run time.  The keys are the seams that the test suite and bench.py use:
 *   "reset"                       every key below back to its default, the per-launch timing recorders off
 *   "window_attention"            4 = default; any other value selects the three-lookup fp32 kernels and makes
 *                                 hfl_window_attention_f16_ok return 0
 *   "window_rpe_form1_max_depth"  deepest level at which the fp16 window kernel takes table form 1 (default 4; 0 = form 2 always)
 *   "relay_fast"                  0 = the general loop of the fp16 relay-token attention for every sequence length
 *   "window_bwd_rt"               0 = scatter-add table gradient in the window attention backward (-1 = by depth)
 *   "tail_split"                  0 = no split of the left-over rows in the fused MLP and the fused LN -> qkv launches
 *   "x3_dbg"                      0x100 | nt: non-temporal stores of the x3 GEMM output (bit 0 f32, bit 1 split2); any other
 *                                 value is accepted and ignored
 * Every variant that lost its A/B measurement is gone from the library together with its key (knob history); the logs
 * are under profiles/.  Returns HFL_EINVAL for an unknown key. */
int hfl_set_variant(const char* key, int value);

/* ------------------------------------------------------------------------
 * 5. Relay-token self-attention, ragged per cloud
 *    (replaces concat_and_pad_rt + RTAttention SDPA + unpad_and_split_rt,
 *     models/relay_token_utils.py:12-79, models/hotformerloc_backbone.py:83-119,
 *     mask models/octree.py:229-265)
 * ---------------------------------------------------------------------- */
/* qkv (rows, 3*H*16), out (rows, H*16).  Cloud b attends over the rows
 * seq_rows[seq_off[b] .. seq_off[b+1]) (its relay tokens of all pyramid depths,
 * fine to coarse; relay tokens of pure-padding windows are in no sequence).  Rows not
 * listed in seq_rows are left untouched (the caller zero-fills `out`).  max_seq_len = the
 * longest per-cloud sequence (host copy; sizes the grid). */
int hfl_relay_attention_fwd(float* out, const float* qkv, const int32_t* seq_rows,
                            const int32_t* seq_off, int batch, int n_heads, float scale,
                            int max_seq_len, hfl_stream_t stream);
/* The same attention on the fp16 (hi, lo) operand rows hfl_ln_qkv_fused writes (queries pre-multiplied by 16^-0.5 * log2 e),
 * writing attention.proj's bf16 split2 operand (rows, 2C) directly; `orphan_rows` (n_orphans of them, may be 0): rows of no
 * sequence, written as zeros (models/hotformerloc_backbone.py:83-119 on the padded sequences gives those rows no consumer). */
int hfl_relay_attention_f16_fwd(void* out_split2, const void* qkv_f16, const int32_t* seq_rows, const int32_t* seq_off, int batch,
                                int n_heads, int max_seq_len, const int32_t* orphan_rows, int n_orphans, hfl_stream_t stream);

/* ------------------------------------------------------------------------
 * 6. Relay-token initialisation and window statistics
 * ---------------------------------------------------------------------- */
/* rt[w,:] = mean over tokens k of window w with batch id == id of the window's first
 * token (models/hotformerloc_backbone.py:352-360, mask models/octree.py:142-145).
 * Windows past the last token give 0.  x (N_t,C), rt (W,C). */
int hfl_relay_token_init(float* rt, const float* x, const uint32_t* tok_meta,
                         int64_t n_tokens, int32_t n_windows, int32_t patch_size,
                         int64_t channels, hfl_stream_t stream);

/* ADaPE window statistics, mode 'cov' (models/octree.py:285-344): per window mean (3)
 * and upper-triangular Bessel covariance (6) of the owner's node coordinates rescaled
 * to [-1,1] (misc/utils.py:293-304).  stats (W,9). */
int hfl_window_stats(float* stats, const uint32_t* tok_meta, int64_t n_tokens,
                     int32_t n_windows, int32_t patch_size, int depth, hfl_stream_t stream);

/* ------------------------------------------------------------------------
 * 7. Attentional pooling helpers (models/layers/salsa.py:25-55,
 *    models/layers/pooling.py:209-233)
 * ---------------------------------------------------------------------- */
/* In place, per cloud b and pooled token q: scores[r, q] over rows
 * r in [row_off[b], row_off[b+1]) -> softmax over r of scores * scale.
 * scores (rows, n_queries). */
int hfl_segment_softmax(float* scores, const int64_t* row_off, int batch, int n_queries,
                        float scale, hfl_stream_t stream);

/* ------------------------------------------------------------------------
 * 8. LayerNorm over the channel axis, optionally fused with the residual add that precedes it
 *    (torch.nn.LayerNorm call sites: models/octformer_backbone.py:275-278,
 *     models/hotformerloc_backbone.py:213-216,288-291; eps 1e-5, two-pass statistics)
 * ---------------------------------------------------------------------- */
/* out = LN(x) * gamma + beta ;  channels in {16,32,64,128,256,512,1024} */
int hfl_layer_norm(float* out, const float* x, const float* gamma, const float* beta, int64_t n_rows,
                   int64_t channels, float eps, hfl_stream_t stream);
/* x_out = x + y (+ bias, may be NULL) ; h_out = LN(x_out) * gamma + beta.  x_out may alias x. */
int hfl_add_layer_norm(float* x_out, float* h_out, const float* x, const float* y, const float* bias,
                       const float* gamma, const float* beta, int64_t n_rows, int64_t channels,
                       float eps, hfl_stream_t stream);

/* ------------------------------------------------------------------------
 * 9. Operand producers of the split-precision Linear path.
 *    An fp32 Linear y = x W^T (torch.nn.Linear call sites: models/octformer_backbone.py:70,91,
 *    models/layers/octformer_layers.py:54,57) is evaluated as ONE bf16 matrix-core GEMM with fp32
 *    accumulation and fp32 output over K-concatenated operands
 *        A3 = [x_hi | x_hi | x_lo]  (rows, 3K) bf16,   W3 = [w_hi | w_lo | w_hi]  (N, 3K) bf16,
 *    i.e. x_hi w_hi + x_hi w_lo + x_lo w_hi with x = x_hi + x_lo to 2^-17 (measured GEMM error
 *    4e-6 relative, descriptors 1.5e-5 vs the 1e-3 bar).  These kernels write A3 directly from the
 *    op that produces x, so the split costs no extra pass.
 * ---------------------------------------------------------------------- */
/* A3 = split3(LN(x)) */
int hfl_layer_norm_split3(uint16_t* out, const float* x, const float* gamma, const float* beta,
                          int64_t n_rows, int64_t channels, float eps, hfl_stream_t stream);
/* x_out = x + y (+ bias) ; A3 = split3(LN(x_out)) */
int hfl_add_layer_norm_split3(float* x_out, uint16_t* h_out, const float* x, const float* y,
                              const float* bias, const float* gamma, const float* beta, int64_t n_rows,
                              int64_t channels, float eps, hfl_stream_t stream);
/* out = x + y + bias (fp32; out may alias x or y) */
int hfl_add_bias(float* out, const float* x, const float* y, const float* bias, int64_t n_rows,
                 int64_t channels, hfl_stream_t stream);
/* A3 = split3(gelu(x + bias)), exact erf GELU */
int hfl_bias_gelu_split3(uint16_t* out, const float* x, const float* bias, int64_t n_rows,
                         int64_t channels, hfl_stream_t stream);
/* A3 = split3(x) */
int hfl_split3(uint16_t* out, const float* x, int64_t n_rows, int64_t channels, hfl_stream_t stream);

/* 9b. Hand-written split-precision Linear (csrc/gemm_x3.hip): y = x W^T [+ bias] [GELU] [+ residual] with
 * fp32-equivalent accuracy on the bf16 matrix cores (x_lo w_hi + x_hi w_lo + x_hi w_hi, fp32 accumulation).
 * Replaces torch.nn.Linear and the element-wise op after it (models/octformer_backbone.py:70,91,275-278;
 * models/layers/octformer_layers.py:53-59; models/hotformerloc_backbone.py:213-216).
 * Operands are PRE-SPLIT in the "split2" layout (rows, K/32, 2, 32) bf16: per 32-wide k-block [32 x hi | 32 x lo]
 * (hi = RNE(v), lo = RNE(v - hi)); hfl_split2 converts an fp32 matrix, hfl_layer_norm_split2 and the attention
 * kernel (out_split = 2) write it directly.  in_features % 32 == 0, out_features % 128 == 0.
 *   gelu_split_out = 0: out is float (n_rows, out_features) = acc + bias [+ residual]  (residual may alias out)
 *   gelu_split_out = 1: out is split2 bf16 (n_rows, out_features/32, 2, 32) of gelu(acc + bias), exact erf GELU */
int hfl_linear_x3(void* out, const uint16_t* x_split2, const uint16_t* w_split2, const float* bias,
                  const float* residual, int64_t n_rows, int in_features, int out_features, int gelu_split_out,
                  hfl_stream_t stream);
int hfl_split2(uint16_t* out, const float* x, int64_t n_rows, int64_t channels, hfl_stream_t stream);
/* A logical (n_rows, C) f32 matrix whose rows live in up to four separate arrays: rows [row0[i], row0[i + 1]) at ptr[i] (C floats
 * per row, row-major), row0[0] = 0, 1 <= n <= 4.  The [tokens | relay rows] buffer of an H-OSA block, whose relay rows arrive
 * from the relay-token block, and the relay-token block's input, the concatenation of the pyramid levels' relay rows
 * (models/hotformerloc_backbone.py:593-633: `torch.cat` / index assignment there), are read through it where they are. */
typedef struct hfl_row_segments {
  int32_t n;
  const float* ptr[4];
  int64_t row0[4];
} hfl_row_segments;
/* hfl_linear_x3 (f32 output) with the residual rows read through a segment table. */
int hfl_linear_x3_seg(float* out, const uint16_t* x_split2, const uint16_t* w_split2, const float* bias,
                      const hfl_row_segments* residual, int64_t n_rows, int in_features, int out_features, hfl_stream_t stream);
/* Grouped form: ONE launch over row tiles that use DIFFERENT weight blocks -- the per-tap products of an octree convolution
 * over its live (row, tap) pairs (models/layers/octformer_layers.py:89-95; model.OctreeConv._forward_live_taps), which were
 * 27 library GEMM launches.  tiles (n_tiles, 3) int32 = {first row, rows (1..128), first row of the tile's weight block in
 * w_split2}; out (n_rows, out_features) f32 = x W_block^T for the rows of every tile (rows outside all tiles are not
 * written).  out_features % 128 == 0, or out_features == 64 with every weight block padded to 128 rows (zeros). */
int hfl_linear_x3_grouped(float* out, const uint16_t* x_split2, const uint16_t* w_split2, const int32_t* tiles,
                          int64_t n_tiles, int64_t n_rows, int in_features, int out_features, hfl_stream_t stream);
/* The same with the octree convolution's gather done by the GEMM's tile loader: row m of the A operand is
 * x_split2[gather[m]] -- x_split2 (n_src_rows, 2 K) bf16 is the split2 form of the convolution's INPUT rows, gather (n_rows)
 * int32 the input row of every live (row, tap) pair (src of hfl_tap_lists).  Replaces hfl_octree_gather + hfl_linear_x3_grouped:
 * the gathered (pairs x Cin) matrix never exists in memory.  n_src_rows * K * 4 < 2^32. */
int hfl_linear_x3_grouped_gather(float* out, const uint16_t* x_split2, const int32_t* gather, int64_t n_src_rows,
                                 const uint16_t* w_split2, const int32_t* tiles, int64_t n_tiles, int64_t n_rows,
                                 int in_features, int out_features, hfl_stream_t stream);
/* Per-row scaled forms for per-cloud stochastic depth (OctreeDropPath, models/layers/octformer_layers.py:213-289) inside the
 * fused residual branches: out = (x W^T + bias) * row_scale[m] + residual, and split2(x * row_scale[row]) for the branch's
 * incoming gradient.  row_scale (n_rows) may be NULL (= 1). */
int hfl_linear_x3_rows(float* out, const uint16_t* x_split2, const uint16_t* w_split2, const float* bias,
                       const float* residual, const float* row_scale, int64_t n_rows, int in_features, int out_features,
                       hfl_stream_t stream);
int hfl_split2_rows(uint16_t* out, const float* x, const float* row_scale, int64_t n_rows, int64_t channels,
                    hfl_stream_t stream);
/* Training forms of the MLP's first Linear (models/layers/octformer_layers.py:53-59 under autograd):
 *   _gelu_fwd: out_split2 = split2(gelu(x W^T + b)) AND preact (n_rows, out_features) f32 = x W^T + b in one launch (GELU's
 *              backward needs the pre-activation);
 *   _gelu_bwd: out_split2 = split2((dy W) * gelu'(preact)): the input gradient of fc2 multiplied by the GELU derivative and
 *              written as the operand of fc1's gradient GEMMs -- wt_split2 is the split2 layout of W^T (in_features x
 *              out_features of the forward = (out_features, in_features) here). */
int hfl_linear_x3_gelu_fwd(uint16_t* out_split2, float* preact, const uint16_t* x_split2, const uint16_t* w_split2,
                           const float* bias, int64_t n_rows, int in_features, int out_features, hfl_stream_t stream);
int hfl_linear_x3_gelu_bwd(uint16_t* out_split2, const uint16_t* dy_split2, const uint16_t* wt_split2,
                           const float* preact, int64_t n_rows, int in_features, int out_features,
                           hfl_stream_t stream);
/* Weight and bias gradient of the same Linear (csrc/wgrad_x3.hip): dw (N,K) = dy^T x, db (N) = column sums of dy, both
 * operands in the split2 layout (dy (n_rows, N) and x (n_rows, K)), three-term products, fp32 accumulation, slabs of rows
 * reduced in a fixed order (bitwise reproducible).  Replaces autograd's fp32 GEMM + bias reduction for torch.nn.Linear in
 * loss.backward() (training/trainer.py:335-352).  N % 128 == 0, K % 128 == 0; db may be NULL;
 * workspace >= hfl_wgrad_x3_workspace(n_rows, N, K) bytes. */
int64_t hfl_wgrad_x3_workspace(int64_t n_rows, int64_t out_features, int64_t in_features);
int hfl_wgrad_x3(float* dw, float* db, const uint16_t* dy_split2, const uint16_t* x_split2, int64_t n_rows,
                 int64_t out_features, int64_t in_features, void* workspace, hfl_stream_t stream);
/* The same weight and bias gradient from f32 operands on the fp32 matrix cores (csrc/wgrad_f32.hip): dw (N,K) = dy^T x,
 * db (N) = column sums of dy, dy (n_rows, N) and x (n_rows, K) f32 row-major, every product one f32 FMA
 * (v_mfma_f32_16x16x4_f32, the reference's arithmetic), slabs of rows reduced in a fixed order (bitwise reproducible).  The
 * weight gradient of the matched-precision training path (GEMM mode x6).  N % 128 == 0, K % 128 == 0; db may be NULL;
 * workspace >= hfl_wgrad_f32_workspace(n_rows, N, K) bytes. */
int64_t hfl_wgrad_f32_workspace(int64_t n_rows, int64_t out_features, int64_t in_features);
int hfl_wgrad_f32(float* dw, float* db, const float* dy, const float* x, int64_t n_rows, int64_t out_features,
                  int64_t in_features, void* workspace, hfl_stream_t stream);
/* The qkv projection written straight into the operand layout of the fp16-MFMA window attention kernel
 * (hfl_window_attention_fwd_ex with flag 0x100): out (n_rows, out_features) 4-byte cells, every row = [Q | K | V] regions
 * of C = out_features / 3 features, per head 16 dims stored as [16 x hi | 16 x lo] fp16 (hi = RTZ(v), lo = RTZ(v - hi):
 * 22 significant bits) = 64 B, v = acc + bias, the queries multiplied by q_scale (softmax scale * log2 e).
 * Replaces qkv = Linear(x) + the reshape/permute of models/octformer_backbone.py:70-73.  C % 128 == 0. */
int hfl_linear_x3_qkv(void* out, const uint16_t* x_split2, const uint16_t* w_split2, const float* bias,
                      int64_t n_rows, int in_features, int out_features, float q_scale, hfl_stream_t stream);
/* split2(LayerNorm(x)) in one pass (the LayerNorm in front of qkv / fc1: models/octformer_backbone.py:275-278) */
int hfl_layer_norm_split2(uint16_t* out, const float* x, const float* gamma, const float* beta,
                          int64_t n_rows, int64_t channels, float eps, hfl_stream_t stream);
/* ReLU(LayerNorm(x)) in one pass: f32 rows (out_f32) or the split2 operand of the next GEMM (out_split2); exactly one of
 * the two is non-NULL.  Replaces norm -> relu behind every stem convolution (models/layers/octformer_layers.py:80-98). */
int hfl_layer_norm_relu(float* out_f32, uint16_t* out_split2, const float* x, const float* gamma, const float* beta,
                        int64_t n_rows, int64_t channels, float eps, hfl_stream_t stream);

/* 9b'. MATCHED-PRECISION Linear (csrc/gemm_x6.hip): y = x W^T [+ bias] [GELU] [* row_scale] [+ residual], all f32 in memory,
 * with fp32-grade products on the bf16 matrix cores: every operand is the EXACT sum of three bf16 planes (h, m, l) and the six
 * plane products >= 2^-16 are accumulated smallest first in fp32 (what is dropped, m l + l m + l l <= 2^-23 |x w|, is the size of
 * one fp32 rounding of the product).  Replaces torch.nn.Linear (fp32) and the element-wise op after it in the transformer blocks
 * (models/octformer_backbone.py:70,91,275-278; models/layers/octformer_layers.py:53-59; models/hotformerloc_backbone.py:213-216)
 * for callers that want the reference's own arithmetic rather than the 16-bit-operand split of section 9b.
 *   w3 (3, out_features, Kp) bf16 = hfl_linear_x6_pack(w (out_features, in_features) f32), once per parameter;
 *      Kp = hfl_linear_x6_padded_k(in_features) = in_features rounded up to a multiple of 64 (zero padding);
 *   x (n_rows, in_features) f32 as any producer left it (the split happens on the way into LDS);
 *   gelu = 1: out = gelu(acc + bias), exact-erf GELU (residual and row_scale must be NULL);
 *   gelu = 0: out = (acc + bias) [* row_scale[row]] [+ residual] (residual may alias out).
 * in_features % 32 == 0, out_features % 128 == 0. */
int64_t hfl_linear_x6_padded_k(int64_t in_features);
int hfl_linear_x6_pack(uint16_t* w3, const float* w, int64_t out_features, int64_t in_features, hfl_stream_t stream);
int hfl_linear_x6(float* out, const float* x, const uint16_t* w3, const float* bias, const float* residual,
                  const float* row_scale, int64_t n_rows, int in_features, int out_features, int gelu, hfl_stream_t stream);
/* Training forms of hfl_linear_x6 for the MLP (models/layers/octformer_layers.py:53-59 under autograd), the counterparts of
 * hfl_linear_x3_gelu_fwd / _bwd with f32 rows in and out:
 *   _gelu_fwd: out = gelu(x W^T + bias) AND preact = x W^T + bias (n_rows, out_features) in one launch; out is bitwise
 *              hfl_linear_x6(..., gelu = 1), preact bitwise hfl_linear_x6(..., gelu = 0);
 *   _gelu_bwd: out = (dy W) * gelu'(preact): the input gradient of fc2 times the GELU derivative; wt3 = hfl_linear_x6_pack of
 *              W^T (in_features = fc2's out_features, out_features = fc2's in_features), preact (n_rows, out_features). */
int hfl_linear_x6_gelu_fwd(float* out, float* preact, const float* x, const uint16_t* w3, const float* bias, int64_t n_rows,
                           int in_features, int out_features, hfl_stream_t stream);
int hfl_linear_x6_gelu_bwd(float* out, const float* dy, const uint16_t* wt3, const float* preact, int64_t n_rows,
                           int in_features, int out_features, hfl_stream_t stream);

/* Grouped form of hfl_linear_x6 with the gather done by the tile loader: the per-tap products of an octree convolution over
 * its live (row, tap) pairs (models/layers/octformer_layers.py:89-95: ocnn's octree2col + mm) at matched precision -- the
 * stem / downsample convolutions of the matched-precision step.  As hfl_linear_x3_grouped_gather: tiles (n_tiles, 3) int32 =
 * {first row, rows (1..128), first row of the tile's weight block in w3}; row m of the x operand is x[gather[m]] (x: the
 * convolution's input rows, f32, in_features wide); w3 = hfl_linear_x6_pack of the stacked per-tap blocks W[k]^T, each padded
 * to a multiple of 128 rows (w_rows rows in all); out (n_rows, out_features) f32, out_features % 128 == 0 or == 64. */
int hfl_linear_x6_grouped_gather(float* out, const float* x, const int32_t* gather, const uint16_t* w3, int64_t w_rows,
                                 const int32_t* tiles, int64_t n_tiles, int64_t n_rows, int in_features, int out_features,
                                 hfl_stream_t stream);

/* 9e'. norm1 -> attention.qkv -> window attention of a RELAY-TOKEN block (models/hotformerloc_backbone.py:197-216,
 *      models/octformer_backbone.py:52-93: C = 256, 16 heads, K = 48 tokens + 1 relay token per window, dilation 1) as ONE launch
 *      with specialised waves (csrc/attn_ws.hip: six waves run the qkv GEMM of 96 rows head pair by head pair, six run the
 *      window attention of the pair before from LDS): q, k, v of the token rows never cross HBM.
 *        out_split2 (rows, 2C) bf16 split2: the attention output of the token rows [0, n_tokens) and of the relay rows
 *                   [rt_row0, rt_row0 + n_windows) -- the operand of attention.proj (hfl_linear_x3)
 *        x          (n_tokens, C) f32 token rows (after the CPE); gamma / beta / eps: norm1
 *        qkv_pack   hfl_qkv_fused_pack image of attention.qkv.weight; qkv_bias (3C); q_scale = head_dim^-0.5 * log2(e)
 *        relay_qkv  (n_windows, 3C) fp16 (hi, lo) operand rows of the relay tokens = hfl_ln_qkv_fused over the relay rows
 *        rpe_tables3  hfl_window_rpe_expand(..., f16_operand = 2) of the block's RPE table, or NULL (disable_RPE)
 *      hfl_attn_ws_ok: 1 when the configuration is taken (channels 256, 16 heads, n_relay 1, dilation 1, K = 48, depth <= 7),
 *      else 0 -- the caller then runs hfl_ln_qkv_fused + hfl_window_attention_fwd_ex. */
int hfl_attn_ws_ok(const hfl_window_attn_desc* desc, int channels);
int hfl_attn_ws_fwd(void* out_split2, const float* x, const float* gamma, const float* beta, float eps, const void* qkv_pack,
                    const float* qkv_bias, float q_scale, const void* relay_qkv, const uint32_t* tok_meta,
                    const float* rpe_tables3, const hfl_window_attn_desc* desc, hfl_stream_t stream);

/* 9c. The pre-norm MLP branch of a transformer block as ONE launch (csrc/mlp_fused.hip):
 *       out (n_rows, C) = x + fc2(gelu(fc1(LayerNorm(x; gamma, beta, eps)) + b1)) + b2        fc1: C -> 4C, fc2: 4C -> C
 * Replaces norm2 -> mlp.fc1 -> GELU -> mlp.fc2 -> residual add (models/octformer_backbone.py:275-278,
 * models/hotformerloc_backbone.py:213-216, models/layers/octformer_layers.py:38-59).  Same split-precision arithmetic as
 * hfl_linear_x3 (three-term bf16 products, fp32 accumulation, exact-erf GELU); the 4C-wide hidden activation never leaves the
 * register file.  C in {128, 256}; out must not alias x.
 * `pack` is the weight image hfl_mlp_fused_pack writes ONCE per parameter pair from the fp32 weights w1 (4C, C) and w2 (C, 4C)
 * (hfl_mlp_fused_pack_bytes(C) bytes; 0 = unsupported C): the (hi, lo) bf16 split of both matrices cut into 32-hidden-feature
 * stages in the order the kernel streams them through LDS. */
int64_t hfl_mlp_fused_pack_bytes(int channels);
int hfl_mlp_fused_pack(void* pack, const float* w1, const float* w2, int channels, hfl_stream_t stream);
int hfl_ln_mlp_fused(float* out, const float* x, const float* gamma, const float* beta, float eps, const void* pack,
                     const float* b1, const float* b2, int64_t n_rows, int channels, hfl_stream_t stream);
/*     The same launch with a workspace of hfl_ln_mlp_fused_workspace(n_rows, C) bytes (0: none needed): rows are dealt to
 *     the workgroups in whole passes (128 rows at C = 256), and the rows left over after the last whole round -- fewer than
 *     one pass per workgroup -- are computed with the HIDDEN dimension split over several workgroups per row set, whose fc2
 *     partial sums go through the workspace and are added in a fixed order (bitwise reproducible).  Without a workspace the
 *     left-over rows cost every workgroup that holds some a whole extra pass of the weight stream. */
int64_t hfl_ln_mlp_fused_workspace(int64_t n_rows, int channels);
int hfl_ln_mlp_fused_ws(float* out, const float* x, const float* gamma, const float* beta, float eps, const void* pack,
                        const float* b1, const float* b2, int64_t n_rows, int channels, void* workspace,
                        int64_t workspace_bytes, hfl_stream_t stream);
/*     The same launches for a hidden width other than 4C: `hidden` = rows of w1 = columns of w2.  Supported: 4C (C = 128,
 *     256: the transformer blocks, identical to the entry points above) and C = hidden = 256 (the Mixer layers of the pooling
 *     head, models/layers/salsa.py:58-75: LayerNorm -> Linear -> GELU -> Linear -> residual with mlp_ratio 1). */
int64_t hfl_mlp_fused_pack_bytes_h(int channels, int hidden);
int hfl_mlp_fused_pack_h(void* pack, const float* w1, const float* w2, int channels, int hidden, hfl_stream_t stream);
int64_t hfl_ln_mlp_fused_workspace_h(int64_t n_rows, int channels, int hidden);
int hfl_ln_mlp_fused_h(float* out, const float* x, const float* gamma, const float* beta, float eps, const void* pack,
                       const float* b1, const float* b2, int64_t n_rows, int channels, int hidden, void* workspace,
                       int64_t workspace_bytes, hfl_stream_t stream);

/* 9d. LayerNorm -> qkv projection as ONE launch, written as the fp16 (hi, lo) operand rows of the window kernel
 *     (= hfl_layer_norm_split2 + hfl_linear_x3_qkv: norm1 -> attention.qkv, models/octformer_backbone.py:70,
 *     models/hotformerloc_backbone.py:213-216; csrc/qkv_fused.hip).  C = 128 or 256.  `pack` = hfl_qkv_fused_pack_bytes(C)
 *     bytes laid out once per parameter by hfl_qkv_fused_pack from the f32 weight (3C, C); bias (3C); qkv_out (n_rows, 3C)
 *     4 B per element; q_scale (softmax scale x log2 e) is folded into the queries. */
int64_t hfl_qkv_fused_pack_bytes(int channels);
int hfl_qkv_fused_pack(void* pack, const float* w_qkv, int channels, hfl_stream_t stream);
int hfl_ln_qkv_fused(void* qkv_out, const float* x, const float* gamma, const float* beta, float eps, const void* pack,
                     const float* bias, float q_scale, int64_t n_rows, int channels, hfl_stream_t stream);
/* ... with the input rows read through a segment table (hfl_row_segments above). */
int hfl_ln_qkv_fused_seg(void* qkv_out, const hfl_row_segments* x, const float* gamma, const float* beta, float eps,
                         const void* pack, const float* bias, float q_scale, int64_t n_rows, int channels, hfl_stream_t stream);

/* 9e. LayerNorm -> qkv projection -> window attention as ONE launch (csrc/attn_fused.hip): norm1 -> attention.qkv -> mask /
 *     RPE bias / SDPA of `x = x + attn(norm1(x))` (models/octformer_backbone.py:52-93,275-276) up to the attention output,
 *     q, k, v never in HBM.  Built for the OctFormer stage: C = 128 (8 heads of 16), patch_size 48, no relay tokens,
 *     dilation 1 / 2 / 4, octree depth <= 7, RPE through the three clamped 1-D expanded tables
 *     (hfl_window_rpe_expand with f16_operand = 1 at a depth where it builds that form) or none.  hfl_attn_fused_ok says
 *     whether a configuration is taken.  x (n_tokens, C) f32; qkv_pack = hfl_qkv_fused_pack image; out_split2 (n_tokens, 2 C)
 *     bf16 = the operand of the proj GEMM (hfl_linear_x3), bitwise what hfl_ln_qkv_fused + hfl_window_attention_fwd_ex
 *     (out_split3 = 2 | 0x100) produce. */
int hfl_attn_fused_ok(const hfl_window_attn_desc* desc, int channels, int has_rpe);
int hfl_attn_fused_fwd(void* out_split2, const float* x, const float* gamma, const float* beta, float eps, const void* qkv_pack,
                       const float* qkv_bias, float q_scale, const uint32_t* tok_meta, const float* rpe_table,
                       const hfl_window_attn_desc* desc, hfl_stream_t stream);

/* ------------------------------------------------------------------------
 * 10. Backward kernels (training path; autograd glue in hotformerloc_amd/autograd.py).
 *     The reference gets these from PyTorch autograd over its materialised formulation and from
 *     dwconv.cu for the depth-wise conv (section 1 already covers dwconv's two gradients).
 * ---------------------------------------------------------------------- */
/* Gradient of hfl_window_attention_fwd.  dout (rows, H*16) -> dqkv (rows, 3*H*16), fully written for
 * every token and relay row; drpe_table (3*(2*pos_bnd+1), H) is ACCUMULATED into (zero it first; float
 * atomics, so its low bits are not run-to-run reproducible) and may be NULL when rpe_table is NULL. */
int hfl_window_attention_bwd(float* dqkv, float* drpe_table, const float* qkv, const float* dout,
                             const uint32_t* tok_meta, const float* rpe_table,
                             const hfl_window_attn_desc* desc, hfl_stream_t stream);
/* The same with a REPRODUCIBLE RPE-table gradient: every grid column writes its partial table to `workspace`
 * (hfl_window_attention_bwd_workspace(desc) bytes; 0 = this launch configuration has no deterministic form, use the entry
 * above) and a second launch adds the partials in a fixed order -- no float atomics; drpe_table need not be zeroed. */
int64_t hfl_window_attention_bwd_workspace(const hfl_window_attn_desc* desc);
int hfl_window_attention_bwd_det(float* dqkv, float* drpe_table, const float* qkv, const float* dout,
                                 const uint32_t* tok_meta, const float* rpe_table, const hfl_window_attn_desc* desc,
                                 void* workspace, hfl_stream_t stream);
/* (All three backward entry points, round 6: with desc->depth in 1..5 -- token coordinates < 32 -- the RPE-table gradient
 * of models/layers/octformer_layers.py:144-174 is computed on the matrix cores as the diagonal sums of OHQ^T dS OHK, one-hot
 * coordinate matrices of the window, summed over every window of a wave and reduced once in a fixed order; deeper levels or
 * depth 0 = unknown keep the fixed-point LDS scatter-add.  The grid is the resident workgroup count of the instantiation.)
 * The same (workspace = NULL: the float-atomic table gradient of hfl_window_attention_bwd) with dqkv written as the split2
 * operand (rows, 2 * 3 H 16) bf16 of the qkv layer's data- and weight-gradient GEMMs (round 6): bit for bit what hfl_split2
 * makes of the f32 gradient, which is never in memory (the training step spent 2 ms in that pass). */
int hfl_window_attention_bwd_split2(uint16_t* dqkv_split2, float* drpe_table, const float* qkv, const float* dout,
                                    const uint32_t* tok_meta, const float* rpe_table, const hfl_window_attn_desc* desc,
                                    void* workspace, hfl_stream_t stream);
/* Gradient of hfl_relay_attention_fwd.  dqkv (rows, 3*H*16): rows listed in seq_rows are written, the
 * others left untouched (the caller zero-fills).  max_seq_len * 268 B of LDS per workgroup: returns
 * HFL_ECAPACITY beyond 611 relay tokens per cloud. */
int hfl_relay_attention_bwd(float* dqkv, const float* qkv, const float* dout, const int32_t* seq_rows,
                            const int32_t* seq_off, int batch, int n_heads, float scale,
                            int max_seq_len, hfl_stream_t stream);
/* ----------------------------------------------------------------------
 * 12. A whole transformer block of the inference path in one call (csrc/capi.hip): OctFormerBlock / HOTFormerBlock forward
 *     (models/octformer_backbone.py:232-281, models/hotformerloc_backbone.py:130-236 with layer scale and stochastic depth
 *     off) = CPE -> [relay rows] -> LN1 -> qkv -> window attention -> proj + residual -> LN2 -> fc1 + GELU -> fc2 +
 *     residual, on the entry points above (split-precision GEMMs, fp16 (hi, lo) attention operands: the caller checks
 *     hfl_window_attention_f16_ok first).  Weights in the layouts those entry points take; `rpe_table` may be NULL.
 *     io->x_in: (n_rows, C) input buffer [tokens | relay rows]; io->relay: optional fresh relay rows (n_rows - n_tokens, C)
 *     that replace x_in's; io->out (n_rows, C); io->arena >= hfl_block_forward_x3_arena(n_rows, C) bytes of scratch.
 * ---------------------------------------------------------------------- */
typedef struct hfl_block_weights {
  int64_t channels;
  float eps, q_scale;
  const float *cpe_weight, *cpe_gamma, *cpe_beta;
  const float *norm1_gamma, *norm1_beta, *norm2_gamma, *norm2_beta;
  const uint16_t *qkv_w, *proj_w, *fc1_w, *fc2_w;     /* split2 */
  const float *qkv_b, *proj_b, *fc1_b, *fc2_b;
  const float* rpe_table;                              /* (3 (2 pos_bnd + 1), H) or NULL */
  const void* mlp_pack;                                /* hfl_mlp_fused_pack image of (fc1, fc2) or NULL: when set, LN2 -> fc1 ->
                                                          GELU -> fc2 -> residual run as ONE launch (hfl_ln_mlp_fused) and fc1_w /
                                                          fc2_w are not read */
  const void* qkv_pack;                                /* hfl_qkv_fused_pack image of qkv_w or NULL: when set, phase 1 runs LN1 -> qkv
                                                          of the token rows as ONE launch (hfl_ln_qkv_fused); qkv_w is still
                                                          read for the relay rows */
  int32_t fuse_attention;                              /* bit 0: a whole-block call (phase 0) of a block WITHOUT relay rows runs LN1
                                                          -> qkv -> window attention as ONE launch (hfl_attn_fused_fwd) when
                                                          hfl_attn_fused_ok takes the configuration; needs qkv_pack.
                                                          bit 1: a block WITH relay rows runs LN1 -> qkv -> window attention of its
                                                          token rows as ONE launch (hfl_attn_ws_fwd) when hfl_attn_ws_ok takes the
                                                          configuration; needs qkv_pack and rpe_tables3.  Phase 1 is then the CPE
                                                          alone (the launch reads the relay rows' q / k / v). */
  const float* rpe_tables3;                            /* hfl_window_rpe_expand(..., f16_operand = 2) of rpe_table, or NULL */
} hfl_block_weights;
typedef struct hfl_block_io {
  const float* x_in;
  const float* relay;                                  /* also in phase 4: proj's residual reads the relay rows there */
  float* out;
  void* arena;
  const int32_t* neigh;                                /* (n_tokens, 27) */
  const uint32_t* tok_meta;
  int64_t n_rows, n_tokens;
  int32_t phase;                                       /* 0: the whole block.  1: only what does not depend on the relay rows --
                                                          CPE, LN1 and the qkv projection of the TOKEN rows (may run while the
                                                          relay-token self-attention of the iteration is still in flight);
                                                          2: the rest -- relay rows in, their LN1 / qkv, window attention, proj,
                                                          MLP.  3 + 4 split phase 2 around the attention: 3 = relay rows in and
                                                          their LN1 / qkv, 4 = proj and MLP; between them the caller runs the
                                                          attention of this and other blocks with hfl_block_attention_x3_multi.
                                                          All phases of a block share `arena`. */
} hfl_block_io;
int64_t hfl_block_forward_x3_arena(int64_t n_rows, int64_t channels);
int hfl_block_forward_x3(const hfl_block_weights* w, const hfl_block_io* io, const hfl_window_attn_desc* desc,
                         hfl_stream_t stream);
/* The window attention of n (<= 4) blocks that have finished phases 1 and 3, in ONE launch when they share an attention shape
 * (patch size, relay tokens, heads, table form: the pyramid levels of an H-OSA iteration,
 * models/hotformerloc_backbone.py:466-473), else one launch each; then run each block's phase 4. */
int hfl_block_attention_x3_multi(int n, const hfl_block_weights* const* w, const hfl_block_io* const* io,
                                 const hfl_window_attn_desc* const* desc, hfl_stream_t stream);

/* The relay-token transformer block (RTSA, models/hotformerloc_backbone.py:239-302) of the inference path as ONE call: LN1 ->
 * split2, qkv GEMM, ragged relay attention (hfl_relay_attention_fwd), split2, proj GEMM + residual, LN2 -> split2, fc1 GEMM +
 * GELU, fc2 GEMM + residual -- eight launches and a memset issued back to back from native code (the rows are the few
 * thousand relay tokens of a batch: the launches are tiny, the Python issue time was the cost).
 * arena >= hfl_relay_block_forward_x3_arena(n_rows, channels) bytes; out (n_rows, C) must not alias x_in. */
typedef struct hfl_relay_block_weights {
  int64_t channels;
  int32_t n_heads;
  float eps;
  const float *norm1_gamma, *norm1_beta, *norm2_gamma, *norm2_beta;
  const uint16_t *qkv_w, *proj_w, *fc1_w, *fc2_w;     /* split2 */
  const float *qkv_b, *proj_b, *fc1_b, *fc2_b;
  const void* mlp_pack;                                /* hfl_mlp_fused_pack image of (fc1, fc2) or NULL: when set (C = 128 / 256) the MLP
                                                          branch is ONE launch (hfl_ln_mlp_fused_ws) and fc1_w / fc2_w are not read */
  const void* qkv_pack;                                /* hfl_qkv_fused_pack image of qkv_w or NULL: when set, LN1 -> qkv is ONE launch
                                                          (hfl_ln_qkv_fused) and the attention reads its fp16 (hi, lo) rows and
                                                          writes proj's split2 operand itself (hfl_relay_attention_f16_fwd): three
                                                          launches up to proj's input instead of six */
  const void* relay_pack;                              /* hfl_relay_block_pack image of (qkv, proj, fc1, fc2) or NULL: what
                                                          hfl_relay_block_fused_x3 reads; hfl_relay_block_forward_x3 ignores it */
} hfl_relay_block_weights;
typedef struct hfl_relay_block_io {
  const float* x_in;
  float* out;
  void* arena;
  const int32_t* seq_rows;                             /* as hfl_relay_attention_fwd */
  const int32_t* seq_off;
  int64_t n_rows;
  int32_t batch, max_seq_len;
  const int32_t* orphan_rows;                          /* rows that belong to no sequence (relay tokens of pure padding windows):
                                                          their attention output is zero; read when qkv_pack is set */
  int32_t n_orphans;
  const hfl_row_segments* x_segments;                  /* optional, needs qkv_pack: the input rows where the pyramid levels left
                                                          them (no concatenation launch); x_in is then not read */
} hfl_relay_block_io;
int64_t hfl_relay_block_forward_x3_arena(int64_t n_rows, int64_t channels);
int hfl_relay_block_forward_x3(const hfl_relay_block_weights* w, const hfl_relay_block_io* io, hfl_stream_t stream);
/* The same block as ONE launch (csrc/relay_block.hip): a workgroup per (cloud, 16-row query tile) and per 16 orphan rows, no
 * communication between workgroups, arithmetic at every hand-off as in the five launches of hfl_relay_block_forward_x3 (only
 * f32 summation orders differ).  hfl_relay_block_fused_ok: 1 when the launch takes the problem -- channels = 256, 16 heads,
 * relay_pack, every bias and LayerNorm parameter present, max_seq_len <= 64.  io->arena is not used.  out must not overlap any
 * input rows (the other rows of a cloud are read after some were written): HFL_EINVAL.
 * hfl_relay_block_pack: the weight image (hfl_relay_block_pack_bytes(channels) bytes; 0 = unsupported width) from the fp32
 * Linear weights qkv (3C, C), proj (C, C), fc1 (4C, C), fc2 (C, 4C): bf16 (hi, lo) MFMA fragments, once per parameter set. */
int hfl_relay_block_fused_ok(const hfl_relay_block_weights* w, const hfl_relay_block_io* io);
int hfl_relay_block_fused_x3(const hfl_relay_block_weights* w, const hfl_relay_block_io* io, hfl_stream_t stream);
int64_t hfl_relay_block_pack_bytes(int channels);
int hfl_relay_block_pack(void* pack, const float* qkv_w, const float* proj_w, const float* fc1_w, const float* fc2_w, int channels,
                         hfl_stream_t stream);

/* Weight gradient of an octree convolution over its live (row, tap) pairs (csrc/tapconv.hip; replaces autograd over
 * ocnn's octree2col + mm, models/layers/octformer_layers.py:89-95): dw[k] (cin, cout) = g_k^T dpart_k over the pairs of tap
 * k.  g (P, cin), dpart (P, cout) fp32 pair-major; chunks (n_chunks, 3) int32 = {tap, first pair, end pair}, ascending, no
 * chunk straddles a tap; tap_chunk_off (taps + 1) int32 = first chunk of every tap; workspace n_chunks * cin * cout floats.
 * cin % 64 == 0, cout % 64 == 0.  fp32 MFMA, fixed summation order. */
int hfl_tap_wgrad(float* dw, const float* g, const float* dpart, const int32_t* chunks, int n_chunks,
                  const int32_t* tap_chunk_off, int taps, int cin, int cout, float* workspace, hfl_stream_t stream);
/* The same with the pair-major operands read through row tables (round 6): pair p contracts row g_rows[p] of g (the layer
 * input, (n_src, cin)) with row d_rows[p] of dpart (the output gradient, (n_out, cout)); a NULL table = pair-major operand as
 * above.  With both tables neither octree2col copy of the backward is written (ocnn materialises both). */
int hfl_tap_wgrad_gather(float* dw, const float* g, const int32_t* g_rows, const float* dpart, const int32_t* d_rows,
                         const int32_t* chunks, int n_chunks, const int32_t* tap_chunk_off, int taps, int cin, int cout,
                         float* workspace, hfl_stream_t stream);
/* Inverse of a gather table whose source and destination row counts differ (stride-2 conv:
 * table (n_dst, K) with entries in [0, n_src)): inverse (n_src, K), inverse[table[m,k], k] = m, -1 else. */
int hfl_inverse_table(int32_t* inverse, int64_t n_src_rows, const int32_t* table, int64_t n_dst_rows,
                      int kngh, hfl_stream_t stream);
/* Gradient of hfl_octree_gather w.r.t. data through the INVERSE table (hfl_inverse_neigh of the
 * forward table, int32): ddata[n,c] = sum_k dcol[ineigh[n,k], k*C + c]. */
int hfl_octree_gather_bwd(float* ddata, const float* dcol, const int32_t* ineigh, int64_t n_rows,
                          int kngh, int64_t channels, hfl_stream_t stream);
/* Gradient of hfl_relay_token_init: dx (N_t,C) fully written. */
int hfl_relay_token_init_bwd(float* dx, const float* drt, const uint32_t* tok_meta, int64_t n_tokens,
                             int32_t n_windows, int32_t patch_size, int64_t channels,
                             hfl_stream_t stream);

/* Gradient of LayerNorm over the channel axis (training path; replaces torch's native_layer_norm_backward behind
 * the LayerNorms of models/octformer_backbone.py:275-278 etc.): dx (n_rows, C); dgamma_partial / dbeta_partial
 * (hfl_layer_norm_bwd_blocks(n_rows, C), C) per-workgroup partial sums the caller adds up (fixed order, no atomics).
 * Statistics are recomputed from x. */
int hfl_layer_norm_bwd_blocks(int64_t n_rows, int64_t channels);
int hfl_layer_norm_bwd(float* dx, float* dgamma_partial, float* dbeta_partial, const float* dy, const float* x,
                       const float* gamma, int64_t n_rows, int64_t channels, float eps, hfl_stream_t stream);
/* The same with dx = dres + (LayerNorm input gradient): the skip path of a pre-norm residual branch y = x + f(LN(x))
 * (models/octformer_backbone.py:275-278) joins inside the kernel; dres (n_rows, channels) may be NULL and may alias dx. */
int hfl_layer_norm_bwd_add(float* dx, float* dgamma_partial, float* dbeta_partial, const float* dy, const float* x,
                           const float* gamma, const float* dres, int64_t n_rows, int64_t channels, float eps,
                           hfl_stream_t stream);
int hfl_layer_norm_bwd_finalize(float* dgamma, float* dbeta, const float* dgamma_partial, const float* dbeta_partial,
                                int n_blocks, int64_t channels, hfl_stream_t stream);

/* ------------------------------------------------------------------------
 * 11. TruncatedSmoothAP ranking core (replaces the (B,P,B) tensor algebra of
 *     models/losses/truncated_smoothap.py:44-93 and its autograd graph)
 * ---------------------------------------------------------------------- */
/* sim (B,B) f32 = E E^T, pos_mask / neg_mask (B,B) uint8 (0/1), closest_pos (B,P) int64 = top-P positives of
 * every query by similarity (entries that are not positives are skipped, as the reference zeroes them,
 * :85-87).  ap (B): sum_j valid r_j / n_valid (0 for a query without positives); dap_ds (B,B): d ap[q] / d sim[q,z]
 * with the clamped-sigmoid gradient of loss_utils.py:40-48.  HFL_ECAPACITY beyond 17066 rows (9 B of LDS each). */
int hfl_smoothap_rows(float* ap, float* dap_ds, const float* sim, const uint8_t* pos_mask,
                      const uint8_t* neg_mask, const int64_t* closest_pos, int batch, int positives_per_query,
                      float tau, hfl_stream_t stream);

/* ------------------------------------------------------------------------
 * 11b. Euclidean affinity of TruncatedSmoothAP (models/losses/loss_utils.py:55-60: -torch.cdist(E, E), the similarity
 *      every shipped training config resolves to, misc/utils.py:204)
 * ---------------------------------------------------------------------- */
/* dist (B,B) f32: dist[i,j] = sqrt(sum_k (emb[i,k] - emb[j,k])^2), summed over the differences themselves (never
 * |x|^2 + |y|^2 - 2 x.y, which cancels for the near pairs the loss depends on).  The diagonal and every pair of equal rows
 * are exactly 0, dist is bitwise symmetric, every element has one writer (two launches agree bitwise).  emb (B,D) f32
 * row-major; any B >= 1 and D >= 1, else HFL_EINVAL. */
int hfl_pairwise_dist(float* dist, const float* emb, int batch, int dim, hfl_stream_t stream);

/* d_emb (B,D) f32: d_emb[i] = sum_j (grad_dist[i,j] + grad_dist[j,i]) (emb[i] - emb[j]) / dist[i,j], the gradient of
 * sum_ij grad_dist[i,j] dist[i,j] for an arbitrary (B,B) grad_dist; terms with dist[i,j] == 0 contribute 0 (torch.cdist's
 * convention for coincident rows).  dist: what hfl_pairwise_dist wrote for emb.  j ascending in a fixed order, one writer
 * per element, no atomics.  Any B >= 1 and D >= 1, else HFL_EINVAL. */
int hfl_pairwise_dist_bwd(float* d_emb, const float* grad_dist, const float* dist, const float* emb, int batch, int dim,
                          hfl_stream_t stream);

/* ------------------------------------------------------------------------
 * 11b'. Batch-hard triplet and contrastive losses (models/losses/loss.py:27-135 with pytorch-metric-learning's
 *       LpDistance(p = 2, power = 1), TripletMarginLoss(swap = True), ContrastiveLoss and AvgNonZeroReducer).  Every distance
 *       below carries the bits hfl_pairwise_dist writes for that entry.  Any B >= 1 and D >= 1, else HFL_EINVAL.  No float
 *       atomics; every output element has one writer and a fixed summation order (two launches agree bitwise).
 * ---------------------------------------------------------------------- */
/* Bytes of workspace hfl_batch_hard_mine needs for a batch (the partial results of its column splits). */
int64_t hfl_batch_hard_mine_workspace(int batch);

/* Per row a: p[a] the column with the largest dist[a, j] among pos_mask[a, j] != 0 and d_ap[a] that distance, n[a] the column
 * with the smallest dist[a, j] among neg_mask[a, j] != 0 and d_an[a]; the lowest column wins a tie; index -1 and distance 0
 * where the row has none.  The (B, B) matrix is never written: two launches, the second combines the column splits in
 * ascending order.  emb (B,D) f32, masks (B,B) u8 row-major, p and n (B,) i32, d_ap and d_an (B,) f32. */
int hfl_batch_hard_mine(int* p, float* d_ap, int* n, float* d_an, void* workspace, const float* emb, const uint8_t* pos_mask,
                        const uint8_t* neg_mask, int batch, int dim, hfl_stream_t stream);

/* Bytes of workspace hfl_batch_hard_terms needs for a batch (one set of partial sums per 64 rows; 8-byte aligned). */
int64_t hfl_batch_hard_terms_workspace(int batch);

/* Loss terms of the mined triples; one entry point for both losses, selected by `mode`.  Two launches: a workgroup per 64
 * rows, then one wave that adds the workgroups' partial sums in a fixed order.  A row is kept iff 0 <= p[a] < B and
 * 0 <= n[a] < B; the terms are float64 expressions of the f32 distances.
 *   mode 0 (triplet): d_pn[a] = dist[p[a], n[a]]; v = d_ap - min(d_an, d_pn) + margin0 (d_pn is taken iff d_pn < d_an);
 *     flags[a] = 1 kept | 2 v > 0 | 4 v > 0 and d_pn taken; loss = mean of the v > 0.
 *   mode 1 (contrastive): flags[a] = 1 kept | 2 d_ap - margin0 > 0 | 4 margin1 - d_an > 0; d_pn = 0;
 *     loss = mean of the positive d_ap - margin0 + mean of the positive margin1 - d_an.
 * stats (16,) f64: 0 kept rows, 1 and 2 the counts of flag 2 and flag 4, 3 and 4 the sums of the two term sets, 5-7 mean, max,
 * min of the kept d_ap, 8-10 of the kept d_an (NaN without a kept row), 11 the mean row norm, 12 loss, 13 and 14 the two
 * means of mode 1, 15 zero.  scale (4,) f32: 1 / count of each term set (0 for an empty set), the loss, zero. */
int hfl_batch_hard_terms(double* stats, float* scale, float* d_pn, int* flags, void* workspace, const float* emb, const int* p,
                         const float* d_ap, const int* n, const float* d_an, int batch, int dim, int mode, double margin0,
                         double margin1, hfl_stream_t stream);

/* d_emb (B,D) f32: the gradient of the loss of hfl_batch_hard_terms (same mode) for unit upstream gradient, from what mine and
 * terms wrote.  A pair at distance 0 contributes nothing.  Row i sums, anchors ascending, w (emb[i] - emb[other]) with
 * w = +-scale / distance by fmaf. */
int hfl_batch_hard_grad(float* d_emb, const float* emb, const int* p, const int* n, const float* d_ap, const float* d_an,
                        const float* d_pn, const int* flags, const float* scale, int batch, int dim, int mode,
                        hfl_stream_t stream);

/* ------------------------------------------------------------------------
 * 11c. The batch's positives / negatives masks (datasets/dataset_utils.py:118-123, the collate function's two nested list
 *      comprehensions over in_sorted_array, :201-206; the lists are TrainingTuple.positives / .non_negatives,
 *      datasets/base_datasets.py:11-28)
 * ---------------------------------------------------------------------- */
/* Entries of EACH of a row's two lists that the kernel stages in LDS; a longer list is searched in global memory. */
#define HFL_BATCH_MASKS_LDS_ENTRIES 4096
/* pos_mask[i][j] = labels[j] in positives[labels[i]], neg_mask[i][j] = labels[j] not in non_negatives[labels[i]], both (B,B)
 * bytes that are exactly 0 or 1 (they may be the storage of bool tensors); no special case for the diagonal or for repeated
 * labels.  counts (B,2) int32 or NULL: the row sums of pos_mask and of neg_mask.  labels (B) int64 element ids, may repeat.
 * The lists of all n_elems elements as CSR: pos_off / nn_off (n_elems + 1) int64 offsets into pos_idx / nn_idx, int32 ids,
 * every list non-decreasing (repeats allowed).  The CSR is trusted; a row whose label lies outside [0, n_elems) is treated as
 * having two empty lists and nothing is read out of bounds for it.  One launch on `stream`, no synchronisation.  batch <= 0,
 * n_elems <= 0 or a NULL pointer other than counts: HFL_EINVAL. */
int hfl_batch_masks(uint8_t* pos_mask, uint8_t* neg_mask, int32_t* counts, const int64_t* labels, int batch,
                    const int64_t* pos_off, const int32_t* pos_idx, const int64_t* nn_off, const int32_t* nn_idx, int n_elems,
                    hfl_stream_t stream);

/* ------------------------------------------------------------------------
 * 11d. Tuple lists / evaluation truth from poses: a fixed-radius join of 2-D positions in float64 (the KDTree.query_radius
 *      calls and the per-anchor np.setdiff1d / np.sort loop of datasets/{pointnetvlad,WildPlaces}/generate_training_tuples*.py,
 *      generate_test_sets.py and datasets/CSWildPlaces/generate_train_test_tuples.py:92-212)
 * ---------------------------------------------------------------------- */
/* Query rows (one wave each) of a workgroup, and database positions of the LDS tile they share (12 B each). */
#define HFL_RADIUS_ROWS 8
#define HFL_RADIUS_TILE 2048
/* Two CSR list families over queries (Q,2) and database (N,2), float64 row-major: list A of query i holds the ids j with
 * dx*dx + dy*dy <= r_a*r_a, list B the same at r_b, every operation rounded to float64 (no FMA); a NaN coordinate is in no
 * list.  exclude_self != 0 drops j == i from list A only (for queries == database).  Every list is strictly ascending in j.
 * Count pass (ids_a == NULL and ids_b == NULL): counts (Q,2) int32 = the lengths of A and B.  Fill pass (either ids pointer
 * set): each non-NULL ids_x receives the int32 ids of list x of query i from off_x[i] on, off_x (Q+1) int64 being the
 * exclusive prefix sum of that family's counts; an id that would land at or past off_x[i+1] is dropped, so nothing is
 * written outside [off_x[0], off_x[Q]).  No atomics: two runs give the same bits.  One launch on `stream`, no
 * synchronisation.  Q < 1, N < 1, N >= 2^31, a radius that is negative or NaN, r_a > r_b, NULL positions, NULL counts in the
 * count pass or ids_x without off_x in the fill pass: HFL_EINVAL. */
int hfl_radius_lists(int32_t* counts, int32_t* ids_a, int32_t* ids_b, const int64_t* off_a, const int64_t* off_b,
                     const double* queries, int64_t n_queries, const double* database, int64_t n_database, double r_a,
                     double r_b, int exclude_self, hfl_stream_t stream);

/* ------------------------------------------------------------------------
 * 11e. Ground-to-aerial submap overlap: align, nearest neighbours, Chamfer sums (misc/compute_ground_aerial_overlap.py:
 *      apply_transform and the chamfer_distance the script leaves as a TODO)
 * ---------------------------------------------------------------------- */
/* Query rows of a 256-thread workgroup of hfl_nn_dist (HFL_OVERLAP_ROWS / 256 per thread, in registers), target points of
 * the LDS tile they share (12 B each), and the most thresholds hfl_pair_stats counts in one launch. */
#define HFL_OVERLAP_ROWS 512
#define HFL_OVERLAP_TILE 2048
#define HFL_OVERLAP_MAX_TAUS 8
/* All three take a ragged batch of P pairs: the points of all clouds concatenated as (N, 3) fp32 row-major and (P + 1)
 * int64 DEVICE offsets, cloud p at rows [offsets[p], offsets[p + 1]), offsets[0] = 0, non-decreasing, offsets[P] = N (the
 * caller checks; the kernels clamp what they read of them to the arrays).  Inputs must be finite; this is not checked.  No
 * atomics, one writer per output element, a fixed evaluation order: two runs give the same bits.  One launch each on
 * `stream`, no synchronisation.  A NULL pointer, a negative count or P < 1: HFL_EINVAL; a total that does not fit (P, a
 * grid or the targets of hfl_nn_dist at 2^31 or more): HFL_ECAPACITY. */
/* out[i] = R_p x[i] + t_p for the pair p that owns row i; transforms (P, 12) fp32, a row-major 3 x 4 (R | t) per pair.  Per
 * coordinate c one fmaf chain: acc = fmaf(R[c][0], x, t[c]); acc = fmaf(R[c][1], y, acc); out = fmaf(R[c][2], z, acc). */
int hfl_transform_points(float* out, const float* points, const int64_t* offsets, const float* transforms, int64_t n_pairs,
                         int64_t n_points, hfl_stream_t stream);
/* For every query row of pair p: dist = the distance to the nearest point of pair p's target cloud, idx = that point's
 * index within the cloud (int32); +inf and -1 where the target cloud is empty.  d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx)) in
 * fp32 on the differences, one correctly rounded square root of the minimum; of equal d2 the lowest index wins.  tiles
 * (n_tiles, 2) int64 on the DEVICE, built by the host from the query offsets: (pair, first query row) per workgroup, which
 * then owns the rows [first, min(first + HFL_OVERLAP_ROWS, q_offsets[pair + 1])).  Rows no tile covers are not written. */
int hfl_nn_dist(float* dist, int32_t* idx, const float* queries, const int64_t* q_offsets, int64_t n_queries,
                const float* targets, const int64_t* t_offsets, int64_t n_targets, const int64_t* tiles, int64_t n_tiles,
                int64_t n_pairs, hfl_stream_t stream);
/* Per pair p over dist[offsets[p] .. offsets[p + 1]): sums (P, 2) float64 = the sum of the distances and of their squares,
 * both from the stored fp32 values widened to float64; counts (P, K + 1) int64 = for each of the K thresholds of the HOST
 * array taus (0 <= K <= HFL_OVERLAP_MAX_TAUS, by value in the kernel arguments) how many distances are <= taus[k], compared
 * in fp32, and in column K how many are +inf.  +inf distances are in no sum and no threshold count.  One workgroup per
 * pair, a fixed reduction order. */
int hfl_pair_stats(double* sums, int64_t* counts, const float* dist, const int64_t* offsets, int64_t n_dist, int64_t n_pairs,
                   const float* taus, int n_taus, hfl_stream_t stream);

/* ------------------------------------------------------------------------
 * 11f. Rigid point-to-point ICP registration of submap pairs (csrc/registration.hip; the "6-DoF metric localisation" step
 *      that follows retrieval; no counterpart in the reference).  Definition: hotformerloc_amd/registration.py, DESIGN.md
 *      section 7i.
 * ---------------------------------------------------------------------- */
/* The float64 quantities a workgroup of hfl_icp_correspond reduces its inlier rows to: n, Sp (3), Sq (3), Spq (9, row-major,
 * p' down and q across), sum d^2; and what a pair's status says. */
#define HFL_ICP_SUMS 17
#define HFL_ICP_RUNNING 0
#define HFL_ICP_CONVERGED 1
#define HFL_ICP_MAX_ITERATIONS 2
#define HFL_ICP_TOO_FEW 3
#define HFL_ICP_DEGENERATE 4
/* Both take the ragged batches of section 11e (source and target clouds of P pairs, DEVICE offsets, clamped to the arrays)
 * and the state of the P pairs in two DEVICE arrays: state (P, 16) float64 = the pose as a row-major 3 x 4 (R | t), fitness,
 * rmse, previous fitness, previous rmse; istate (P, 2) int32 = iterations, status.  A pair whose status is not
 * HFL_ICP_RUNNING is left alone by both.  No atomics, one writer per output element, a fixed evaluation order: two runs give
 * the same bits.  One launch each on `stream`, no synchronisation, no host read.  A NULL pointer (but for the outputs named
 * optional), a negative count or P < 1: HFL_EINVAL; P, the tiles or the targets at 2^31 or more: HFL_ECAPACITY. */
/* One evaluation.  Every source row of a RUNNING pair p is moved by the fp32 rounding of the pair's pose with the fmaf chain
 * of hfl_transform_points, and its nearest target is found exactly as hfl_nn_dist finds it (the same bits; tiles is that
 * function's table, built from the source offsets).  dist and idx are optional: where not NULL they receive what
 * hfl_nn_dist would write for the moved cloud.  A row is an inlier when it has a target and dist <= max_dist, compared in
 * fp32.  partials (n_tiles, HFL_ICP_SUMS) float64: row i holds the sums over the inlier rows of tile i -- a thread adds its
 * rows in row order, a wave its lanes by the xor butterfly 32 .. 1, the four waves are added in wave order.  The rows of a
 * pair that is not RUNNING are not written. */
int hfl_icp_correspond(double* partials, float* dist, int32_t* idx, const float* source, const int64_t* s_offsets,
                       int64_t n_source, const float* targets, const int64_t* t_offsets, int64_t n_targets,
                       const int64_t* tiles, int64_t n_tiles, const double* state, const int32_t* istate, float max_dist,
                       int64_t n_pairs, hfl_stream_t stream);
/* One decision and update per RUNNING pair p, one wave each, in float64.  The pair's partials, rows [tile_offsets[p],
 * tile_offsets[p + 1]) (DEVICE, (P + 1) int64), are added in ascending order; sums (P, HFL_ICP_SUMS) is optional and
 * receives them.  With k = iterations, n the inlier count and N = s_offsets[p + 1] - s_offsets[p]: fitness = n / N and
 * rmse = sqrt(sum d^2 / n) are stored; n < min_correspondences: rmse = NaN, status TOO_FEW; k >= 1 and |fitness - previous
 * fitness| < relative_fitness and |rmse - previous rmse| < relative_rmse: CONVERGED; is_last != 0: MAX_ITERATIONS;
 * otherwise H = Spq - Sp Sq^T / n is decomposed by a one-sided cyclic Jacobi of fixed sweep count, R = V diag(1, 1,
 * det(V U^T)) U^T, t = Sq / n - R Sp / n, and pose <- (R | t) . pose, iterations <- k + 1, previous <- (fitness, rmse); a
 * second singular value <= 1e-12 x the largest: DEGENERATE, pose unchanged. */
int hfl_icp_solve(double* state, int32_t* istate, double* sums, const double* partials, const int64_t* tile_offsets,
                  int64_t n_tiles, const int64_t* s_offsets, int64_t n_pairs, int min_correspondences, double relative_fitness,
                  double relative_rmse, int is_last, hfl_stream_t stream);
/* The point-to-plane estimator: the same two launches with 29 sums per tile and pair -- n, sum d^2, g (6), the upper
 * triangle of A row-major (21), where over the inliers r = (p' - q) . nq, J = (p' x nq, nq), A = sum J J^T, g = sum J r,
 * nq = target_normals[idx] (DEVICE, (n_targets, 3) fp32, the rows of `targets`; a zero normal adds nothing to A and g). */
#define HFL_ICP_PLANE_SUMS 29
/* hfl_icp_correspond with the normal gathered at the winning index once the scan is over; dist, idx, the inlier rule and
 * the order of the reduction are unchanged.  partials is (n_tiles, HFL_ICP_PLANE_SUMS). */
int hfl_icp_correspond_plane(double* partials, float* dist, int32_t* idx, const float* source, const int64_t* s_offsets,
                             int64_t n_source, const float* targets, const float* target_normals, const int64_t* t_offsets,
                             int64_t n_targets, const int64_t* tiles, int64_t n_tiles, const double* state,
                             const int32_t* istate, float max_dist, int64_t n_pairs, hfl_stream_t stream);
/* hfl_icp_solve on those partials: the same stop rules; the update solves A x = -g, x = (alpha, beta, gamma, tx, ty, tz),
 * by an LDL^T factorisation without pivoting in a fixed order, R = Rz(gamma) Ry(beta) Rx(alpha), t = (tx, ty, tz),
 * pose <- (R | t) . pose; a pivot <= 1e-12 x its diagonal entry of A (or not a number): DEGENERATE, pose unchanged.  sums
 * (optional) is (P, HFL_ICP_PLANE_SUMS). */
int hfl_icp_solve_plane(double* state, int32_t* istate, double* sums, const double* partials, const int64_t* tile_offsets,
                        int64_t n_tiles, const int64_t* s_offsets, int64_t n_pairs, int min_correspondences,
                        double relative_fitness, double relative_rmse, int is_last, hfl_stream_t stream);
/* The generalized (plane-to-plane) estimator, DESIGN.md section 7r: hfl_icp_correspond_plane with a normal on both sides.
 * source_normals (DEVICE, (n_source, 3) fp32, the rows of `source`) are turned by the fp32 rotation of the pair's pose, the
 * fmaf chain of hfl_transform_points without the translation and without renormalising: a.  b = target_normals[idx].  Both
 * are unit to fp32 rounding, or zero for "no normal" (not checked).  Per inlier row, in float64 from those fp32 values with
 * every operation rounded once: C = 2 I - (1 - epsilon)(a a^T + b b^T), M = C^-1 (adjugate times the reciprocal of the
 * determinant), r = p' - q, J = (-[p']x | I); the HFL_ICP_PLANE_SUMS sums are n, sum d^2, g = sum J^T M r (6), the upper
 * triangle of A = sum J^T M J row-major (21), which hfl_icp_solve_plane takes as they are.  dist, idx, the inlier rule and
 * the order of the reduction are those of hfl_icp_correspond.  A NULL source_normals or target_normals, or an epsilon
 * outside (0, 1]: HFL_EINVAL. */
int hfl_icp_correspond_generalized(double* partials, float* dist, int32_t* idx, const float* source,
                                   const float* source_normals, const int64_t* s_offsets, int64_t n_source,
                                   const float* targets, const float* target_normals, const int64_t* t_offsets,
                                   int64_t n_targets, const int64_t* tiles, int64_t n_tiles, const double* state,
                                   const int32_t* istate, float max_dist, double epsilon, int64_t n_pairs,
                                   hfl_stream_t stream);

/* ------------------------------------------------------------------------
 * 11g. Global registration from point correspondences: a deterministic RANSAC that gives hfl_icp_correspond its starting
 *      pose (csrc/global_registration.hip; no counterpart in the reference).  Definition:
 *      hotformerloc_amd/global_registration.py, DESIGN.md section 7n.
 * ---------------------------------------------------------------------- */
#define HFL_RANSAC_ROWS 512               /* hypotheses of a 256-thread workgroup of hfl_ransac_score (two per thread) */
#define HFL_RANSAC_TILE 1024              /* correspondences of a workgroup of hfl_ransac_score and hfl_ransac_sums */
#define HFL_RANSAC_NO_HYPOTHESIS 5        /* a pair's status beside HFL_ICP_*: no valid hypothesis, the pose is the identity */
/* All four take the correspondences of P pairs as one ragged batch: corr (n_corr, 6) fp32 rows (px, py, pz, qx, qy, qz),
 * source point and target point, with (P + 1) int64 DEVICE offsets, clamped to the array.  A hypothesis is twelve fp32
 * values, the row-major (R | t) of hfl_transform_points; poses is (P, H, 12), valid (P, H) uint8, counts (P, H) int32.
 * tiles (n_tiles, 2) int64 DEVICE rows of (pair, first correspondence), HFL_RANSAC_TILE correspondences of one pair per
 * workgroup.  Launches on `stream`, no synchronisation, no host read, no float atomics: two runs give the same bits.  A NULL
 * pointer, a negative count, P < 1 or H < 1: HFL_EINVAL; n_corr, P, H, P x H or the tiles at 2^31 or more, or more than
 * 65535 x HFL_RANSAC_ROWS hypotheses: HFL_ECAPACITY. */
/* Hypothesis h of pair p: (x0, x1, x2, _) = Philox4x32-10(counter (h, p, 0, 0), key = seed), rows i_k = (x_k * C) >> 32 of
 * the pair's C correspondences (written to draws (P, H, 3) int32 in any case).  Invalid (valid = 0, the pose twelve NaNs)
 * where C < 3, two rows are equal, an edge of the triple fails ls >= rho2 lt and lt >= rho2 ls (squared lengths in float64
 * between the source points and between the target points; rho2 = 0 disables it) or the solve of hfl_icp_solve on the 17
 * sums of the three pairs reports rank < 2; otherwise its (R | t) rounded to fp32. */
int hfl_ransac_hypotheses(float* poses, uint8_t* valid, int32_t* draws, const float* corr, const int64_t* c_offsets,
                          int64_t n_corr, int64_t n_pairs, int64_t n_hypotheses, uint64_t seed, double rho2,
                          hfl_stream_t stream);
/* counts[p, h] = -1 where valid[p, h] = 0, else the number of the pair's correspondences with d2 <= d2_max in fp32, d2 the
 * squared distance of hfl_nn_dist between the moved source point (the fmaf chain of hfl_transform_points) and the target
 * point.  Two launches: the first writes 0 or -1, the second adds every (correspondence tile, hypothesis tile)'s counts by
 * integer atomic adds. */
int hfl_ransac_score(int32_t* counts, const uint8_t* valid, const float* poses, const float* corr, const int64_t* c_offsets,
                     int64_t n_corr, const int64_t* tiles, int64_t n_tiles, int64_t n_pairs, int64_t n_hypotheses,
                     float d2_max, hfl_stream_t stream);
/* One workgroup per pair: the largest count, of equal counts the lowest h.  chosen (P, 3) int32 = that h, its count, the
 * number of counts >= 0; state (P, 16) float64 and istate (P, 2) int32 of section 11f receive the chosen pose, fitness 0,
 * rmse NaN, iteration 0 and HFL_ICP_RUNNING -- or, where every count is -1, the identity, HFL_RANSAC_NO_HYPOTHESIS and
 * chosen = (-1, -1, 0). */
int hfl_ransac_select(double* state, int32_t* istate, int32_t* chosen, const int32_t* counts, const float* poses,
                      int64_t n_pairs, int64_t n_hypotheses, hfl_stream_t stream);
/* hfl_icp_correspond with the correspondences fixed: for every RUNNING pair the inliers (d2 <= d2_max as above) of the fp32
 * rounding of the pose in `state` are reduced to partials (n_tiles, HFL_ICP_SUMS) float64 in the order of
 * hfl_icp_correspond (d = the correctly rounded fp32 root of d2), row i for tile i; hfl_icp_solve with tile offsets over
 * this table and c_offsets as its denominators then decides and updates.  Rows of pairs that are not RUNNING are not
 * written. */
int hfl_ransac_sums(double* partials, const float* corr, const int64_t* c_offsets, int64_t n_corr, const int64_t* tiles,
                    int64_t n_tiles, const double* state, const int32_t* istate, int64_t n_pairs, float d2_max,
                    hfl_stream_t stream);

/* ------------------------------------------------------------------------
 * 11h. Spectral geometric verification: the leading eigenpair of the length-consistency matrix of a pair's point
 *      correspondences by power iteration, for re-ranking retrieved candidates (csrc/spectral.hip; no counterpart in
 *      the reference).  Definition: hotformerloc_amd/spectral.py, DESIGN.md section 7p.
 * ---------------------------------------------------------------------- */
#define HFL_SPECTRAL_ROWS 512             /* rows (correspondences) of a 256-thread workgroup of hfl_spectral_matvec (two per thread) */
#define HFL_SPECTRAL_TILE 1024            /* columns of the LDS tile those rows share: seven fp32 planes */
#define HFL_SPECTRAL_SUMS 3               /* float64 sums of a workgroup: r = sum v w, n = sum v^2, s2 = sum w^2 */
/* Both take the correspondences as section 11g does: corr (n_corr, 6) fp32 rows with (P + 1) int64 DEVICE offsets, clamped
 * to the array.  tiles (n_tiles, 2) int64 DEVICE rows of (pair, first row), HFL_SPECTRAL_ROWS rows of one pair per workgroup,
 * pairs in order; tile_offsets (P + 1) int64 DEVICE: the rows of every pair in that table.  Launches on `stream`, no
 * synchronisation, no host read, no atomics: two runs give the same bits.  A NULL pointer (but for the first step's two),
 * a negative count or P < 1: HFL_EINVAL; n_corr, n_tiles or P at 2^31 or more: HFL_ECAPACITY. */
/* One step of the power iteration.  m_ij = max(0, fmaf(-(e e), inv_sigma2, 1)), e = |p_i - p_j| - |q_i - q_j| with the
 * lengths of hfl_nn_dist (the fmaf chain of d2, the correctly rounded fp32 root), m_ii = 0.  v_j = w_in[j] / fp32(sqrt(s2))
 * with s2 the sum of the pair's rows of partials_in in tile order (v_j = 0 where s2 == 0); w_in == partials_in == NULL is the
 * first step, v = 1.  w_out[i] = the fp32 chain acc = fmaf(m_ij, v_j, acc) from 0 over the pair's j ascending; row t of
 * partials_out (n_tiles, HFL_SPECTRAL_SUMS) float64 = (sum v_i w_i, sum v_i^2, sum w_i^2) over the rows of tile t, reduced in
 * the order of hfl_icp_correspond.  The outputs must not be the inputs.  inv_sigma2 finite and > 0, else HFL_EINVAL. */
int hfl_spectral_matvec(float* w_out, double* partials_out, const float* corr, const int64_t* c_offsets, int64_t n_corr,
                        const int64_t* tiles, int64_t n_tiles, const int64_t* tile_offsets, const float* w_in,
                        const double* partials_in, int64_t n_pairs, float inv_sigma2, hfl_stream_t stream);
/* One wave per pair, after the last step: (r, n, s2) = the pair's rows of `partials` in tile order; eigenvalue[p] = r / n,
 * score[p] = eigenvalue[p] / max(n_source[p], 1), weights[i] = w[i] / fp32(sqrt(s2)) -- or, where s2 == 0 (fewer than two
 * correspondences, or no two of them consistent), eigenvalue 0 and weights 0.  n_source (P) int64 DEVICE. */
int hfl_spectral_finish(double* eigenvalue, double* score, float* weights, const float* w, const double* partials,
                        int64_t n_tiles, const int64_t* tile_offsets, const int64_t* c_offsets, int64_t n_corr,
                        const int64_t* n_source, int64_t n_pairs, hfl_stream_t stream);

/* ------------------------------------------------------------------------
 * 11i. Consensus registration: pose hypotheses from the second-order compatibility of a pair's point correspondences
 *      (csrc/consensus.hip; no counterpart in the reference).  Definition: hotformerloc_amd/consensus.py, DESIGN.md
 *      section 7q.
 * ---------------------------------------------------------------------- */
#define HFL_CONSENSUS_ROWS 512            /* rows (correspondences) of a 256-thread workgroup of hfl_consensus_graph (two per thread) */
#define HFL_CONSENSUS_TILE 1024           /* columns of the LDS tile those rows share: six fp32 planes */
#define HFL_CONSENSUS_MAX_CORRESPONDENCES 16384   /* of one pair: a row of second-order counts fits LDS as 16-bit values */
#define HFL_CONSENSUS_MAX_SIZE 64         /* the largest consensus set, the seed included */
/* Both take the correspondences as section 11g does: corr (n_corr, 6) fp32 rows with (P + 1) int64 DEVICE offsets, clamped
 * to the array.  The compatibility graph of pair p with C correspondences is a bit matrix at bits + word_offsets[p]: C rows
 * of W = 4 ceil(C / 128) 32-bit words, row-major; bit (j & 31) of word (j >> 5) of row i is B_ij = | |p_i - p_j| - |q_i -
 * q_j| | <= distance in fp32 (the d2 fmaf chain, the correctly rounded root), B_ii = 0, the bits from column C on 0.
 * word_offsets (P) int64 DEVICE, multiples of 4; n_words: the length of `bits`, which is 16-byte aligned.  A pair whose
 * matrix does not lie inside [0, n_words), or with more than HFL_CONSENSUS_MAX_CORRESPONDENCES correspondences, is skipped
 * (hfl_consensus_poses: its slots are invalid).  Launches on `stream`, no synchronisation, no host read, no atomics: two
 * runs give the same bits.  A NULL pointer, a negative count, P < 1: HFL_EINVAL; n_corr, P, the tiles or P x S at 2^31 or
 * more: HFL_ECAPACITY. */
/* tiles (n_tiles, 2) int64 DEVICE rows of (pair, first row), HFL_CONSENSUS_ROWS rows of one pair per workgroup.  Writes
 * every word of every pair's matrix and degree[i] = sum_j B_ij (n_corr) int32.  distance finite and > 0, else HFL_EINVAL. */
int hfl_consensus_graph(uint32_t* bits, int32_t* degree, const float* corr, const int64_t* c_offsets, int64_t n_corr,
                        const int64_t* tiles, int64_t n_tiles, const int64_t* word_offsets, int64_t n_words, int64_t n_pairs,
                        float distance, hfl_stream_t stream);
/* One workgroup per (pair, slot): seeds (P, S) int32, a row of the pair or -1 for an unused slot.  n_sj = B_sj sum_k B_sk
 * B_jk; the consensus set is s and the consensus_size - 1 columns of largest n_sj >= 1, the lower j of equal ones; its
 * members in ascending order give the 17 float64 sums (one accumulator each) kabsch_solve takes.  poses (P, S, 12) fp32,
 * valid (P, S) uint8, members (P, S, consensus_size) int32 padded with -1, support (P, S) int32 = the n_sj of the weakest
 * member.  An unused slot, a set of fewer than three members or of rank < 2: twelve NaNs, 0, -1 throughout, 0.
 * consensus_size outside 3 .. HFL_CONSENSUS_MAX_SIZE or S < 1: HFL_EINVAL. */
int hfl_consensus_poses(float* poses, uint8_t* valid, int32_t* members, int32_t* support, const int32_t* seeds,
                        const uint32_t* bits, const int64_t* word_offsets, int64_t n_words, const float* corr,
                        const int64_t* c_offsets, int64_t n_corr, int64_t n_pairs, int64_t n_seeds, int64_t consensus_size,
                        hfl_stream_t stream);

/* ------------------------------------------------------------------------
 * 12. MESA self-distillation (training/trainer.py:161-163, 305-338, 360-361; models/losses/loss.py:138-147)
 * ---------------------------------------------------------------------- */
/* One chunk of one (ema, src) tensor pair: `count` (1..HFL_EMA_CHUNK) fp32 elements at both pointers.  The host cuts each
 * tensor at multiples of HFL_EMA_CHUNK elements, so a chunk is 16-byte aligned exactly when its tensor is. */
#define HFL_EMA_CHUNK 8192
typedef struct hfl_ema_chunk {
  float* ema;
  const float* src;
  int64_t count;
} hfl_ema_chunk;
/* ema <- ema + w * (src - ema) over every chunk of the DEVICE table (n_chunks entries), one launch, one workgroup per
 * chunk.  The table's pointers and counts are trusted: the caller guarantees that every chunk lies inside its tensors and
 * that no ema chunk overlaps another chunk.  0 <= w <= 1, else HFL_EINVAL. */
int hfl_ema_update(const hfl_ema_chunk* table, int n_chunks, float w, hfl_stream_t stream);

/* Distillation rows of kdloss: y, t (B, D) fp32 row-major, p = softmax(y / T), q = softmax(t / T) per row.
 * kl (B): sum_j q_j (log q_j - log p_j);  dkl_dy (B, D): (p - q) / T, the derivative of kl[row] with respect to y[row].
 * One wavefront per row, cross-lane sums in a fixed order (bitwise repeatable).  D a multiple of 64 up to 1024 and
 * T > 0, else HFL_EINVAL. */
int hfl_kd_rows(float* kl, float* dkl_dy, const float* y, const float* t, int batch, int dim, float temperature,
                hfl_stream_t stream);

/* ------------------------------------------------------------------------
 * 12b. Optimizer step: Adam / AdamW with the weight EMA in the same launch (training/trainer.py:140-156, 356, 360-361)
 * ---------------------------------------------------------------------- */
/* One chunk of one parameter: `count` (1..HFL_ADAM_CHUNK) fp32 elements at every non-null pointer.  The host cuts each
 * parameter at multiples of HFL_ADAM_CHUNK elements, so a chunk is 16-byte aligned exactly when its tensors are.
 * grad == NULL: the parameter takes no optimizer step (exp_avg / exp_avg_sq are not touched); ema == NULL: no average.
 * With both NULL the chunk does nothing. */
#define HFL_ADAM_CHUNK 8192
#define HFL_ADAM_MAX_SLOTS 16
typedef struct hfl_adam_chunk {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  float* ema;
  int32_t count;
  int32_t slot; /* index into the launch's slots, 0..HFL_ADAM_MAX_SLOTS-1 */
} hfl_adam_chunk;
/* Hyper-parameters of one (param group, step count) combination.  The host computes every field in double precision from
 * the Python scalars and rounds once to float, as torch's single-tensor path does when it hands its scalars to an op:
 * 1 - beta is therefore its own field (1.f - (float)beta is another number).
 * decay: weight_decay when decoupled == 0 (L2: g += decay * p), 1 - lr * weight_decay when decoupled != 0 (p *= decay). */
typedef struct hfl_adam_slot {
  float step_size; /* lr / (1 - beta1^step) */
  float bias_correction2_sqrt; /* sqrt(1 - beta2^step) */
  float one_minus_beta1;
  float beta2;
  float one_minus_beta2;
  float eps;
  float decay;
  int32_t decoupled;
} hfl_adam_slot;
/* One optimizer step over every chunk of the DEVICE table (n_chunks entries), one launch, one workgroup per chunk; the
 * n_slots (0..HFL_ADAM_MAX_SLOTS) entries of the HOST array `slots` travel by value in the kernel arguments.  Per element,
 * in the order and with the roundings of torch's _single_tensor_adam: decay (see hfl_adam_slot), m += (1 - beta1)(g - m),
 * v = beta2 v + (1 - beta2) g g, p -= step_size m / (sqrt(v) / bias_correction2_sqrt + eps) with correctly rounded sqrt
 * and division; then, where ema != NULL, ema <- ema + w * (p - ema) on the value just stored: bitwise what hfl_ema_update
 * would produce if run afterwards.  The table is trusted as hfl_ema_update's is: every chunk lies inside its tensors, no
 * written chunk overlaps another, every slot index is below n_slots.  n_chunks < 0, a NULL table with chunks present,
 * n_slots outside 0..HFL_ADAM_MAX_SLOTS, NULL slots with n_slots > 0, or w outside [0, 1]: HFL_EINVAL.  Zero chunks:
 * HFL_OK without a launch. */
int hfl_adam_step(const hfl_adam_chunk* table, int n_chunks, const hfl_adam_slot* slots, int n_slots, float w,
                  hfl_stream_t stream);

/* ------------------------------------------------------------------------
 * 13. Retrieval: streamed flat-L2 top-k search (eval/pnv_evaluate.py:199-223, the FAISS GpuIndexFlatL2 search)
 * ---------------------------------------------------------------------- */
/* out (n_rows): squared L2 norm of every row of x (n_rows, dim) fp32 row-major, one fmaf chain per row in column order (a
 * row's value does not depend on n_rows or on the launch).  dim a multiple of 4 in 4..1024, else HFL_EINVAL. */
int hfl_row_sq_norms(float* out, const float* x, int64_t n_rows, int dim, hfl_stream_t stream);

/* For every row of queries (Q, D) the kc = min(k, N) nearest rows of database (N, D) by ||q||^2 + ||d||^2 - 2 q.d, both fp32
 * row-major and 16-byte aligned: dist (Q, kc) fp32 and idx (Q, kc) int32, nearest first, ordered by the lexicographic key
 * (distance, index) -- equal distances by lower index -- in every selection and merge step.  The dot products run on the
 * fp32-input MFMA as one fmaf chain per pair in ascending column order from zero, so a pair's distance is bitwise the same
 * for every Q, N partition and launch shape; it differs from the f64 distance of the same inputs by at most
 * 2^-23 (D + 4) (||q||^2 + ||d||^2).  No (Q, N) matrix is stored: the only device memory besides inputs and outputs is the
 * caller's workspace of hfl_flat_l2_topk_workspace(Q, N, D, k) bytes (both norm vectors and, when the database is split
 * into segments over workgroups, Q x segments x 32 partial entries, segments <= 64; -1 for an unsupported shape).
 * database_sq_norms: hfl_row_sq_norms of the database, or NULL to compute them here.  1 <= k <= 32, D a multiple of 4 in
 * 4..1024, N >= 1, else HFL_EINVAL.  Launches on `stream`, no synchronisation, no host read.  Non-finite inputs: undefined
 * order. */
int64_t hfl_flat_l2_topk_workspace(int64_t n_queries, int64_t n_database, int64_t dim, int k);
int hfl_flat_l2_topk(float* dist, int32_t* idx, const float* queries, const float* database, const float* database_sq_norms,
                     int64_t n_queries, int64_t n_database, int dim, int k, void* workspace, int64_t workspace_bytes,
                     hfl_stream_t stream);

/* The same search with a prefix per query: query q sees the database rows [0, limits[q]) only (limits (Q) int32 on the
 * device, read clamped to [0, N], so no value causes an out-of-range access).  dist, idx are (Q, k) whatever N: the first
 * min(k, limits[q]) slots hold the nearest rows of the prefix under the same key, the rest distance +inf and index -1.  A
 * pair's distance is the value hfl_flat_l2_topk computes for it, so row q of the result is bitwise what hfl_flat_l2_topk
 * returns for that query against the first limits[q] database rows.  The tiles of the database above the largest limit of a
 * 64-query tile are skipped: time-ordered queries with causal limits cost the lower triangle.  Same workspace, same plan,
 * same argument rules; limits NULL: HFL_EINVAL. */
int hfl_flat_l2_topk_prefix(float* dist, int32_t* idx, const float* queries, const float* database,
                            const float* database_sq_norms, const int32_t* limits, int64_t n_queries, int64_t n_database,
                            int dim, int k, void* workspace, int64_t workspace_bytes, hfl_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* HOTFORMERLOC_HIP_H */
