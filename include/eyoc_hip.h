/*
 * eyoc_hip.h - C ABI of libeyoc_hip.so, the MI355X (gfx950) implementation of EYOC's registration
 * hot path.  The reference (liuQuan98/EYOC) has no FFI of its own for this path: its Python calls
 * land in MinkowskiEngine / PyTorch / Open3D.  Every entry point below names the reference call
 * site it stands in for (paths relative to the reference repository root).
 *
 * Conventions
 *   - every function returns 0 on success and a negative eyoc_status on failure;
 *     eyoc_last_error() returns a thread-local message for the last failure on this thread;
 *   - "dev" pointers are device (HBM) pointers owned by the caller; the library never frees them;
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing synchronises
 *     unless stated (eyoc_maps_build does: it must learn the data-dependent level sizes);
 *   - one eyoc_ctx per (process, device); a ctx is not re-entrant (one stream at a time).
 *   - every tensor that crosses this boundary is fp32 (the reference's dtype) and fp32 accumulates every sum; the
 *     sparse-convolution PRODUCTS inside eyoc_model_forward run either as fp32 MFMAs or - "split16", automatic for
 *     batches of >= 8192 rows - as three fp16 MFMAs on hi/lo-split operands (22-bit significands, range-guarded:
 *     eyoc_model_set_math / eyoc_model_range_check); indices are int32 on the device side and int64 where the
 *     reference hands int64 to its callers.
 */
#ifndef EYOC_HIP_H
#define EYOC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct eyoc_ctx eyoc_ctx;
typedef struct eyoc_maps eyoc_maps;
typedef struct eyoc_model eyoc_model;

typedef enum {
  EYOC_OK = 0,
  EYOC_ERR_INVALID = -1,     /* bad argument / unsupported shape            */
  EYOC_ERR_HIP = -2,         /* a HIP runtime call failed                   */
  EYOC_ERR_WORKSPACE = -3,   /* caller-provided workspace too small         */
  EYOC_ERR_DUPLICATE = -4,   /* duplicate coordinates in a sparse tensor    */
  EYOC_ERR_RANGE = -5        /* coordinate / batch index out of key range; split16 activation out of fp16 range */
} eyoc_status;

#define EYOC_MAX_LEVELS 4
/* 111 (round 6): eyoc_model_desc ends with `expanded` (ResUNetExpanded / ResUNetExpBN2C run through eyoc_model_forward too).
 *     Later libraries of 111 add two entry points and change nothing else: eyoc_maps_last_fault_batches and
 *     eyoc_registration_accept_degenerate (a binding checks for the symbols).
 *     Later still, per-pair failure isolation adds eyoc_batch_drop(_workspace_bytes), eyoc_remap_rows and
 *     eyoc_voxelize_batched_isolating(_workspace_bytes), again found by symbol; nothing that existed changes.
 *     Training batches from raw scans add eyoc_cloud_centroids(_workspace_bytes), eyoc_augment_poses and
 *     eyoc_voxelize_batched_posed(_workspace_bytes) the same way.
 *     eyoc_maps_records (what a build kept of its tile records) comes the same way: a read-only accessor, found by symbol.
 *     A fix without a new number: eyoc_voxelize and eyoc_voxelize_batched refuse a point with a NaN coordinate (EYOC_ERR_RANGE), which
 *     earlier libraries of 111 took for cell 0 on that axis; no signature and no output for valid input changes.
 * 110 (round 6): the kernel-selection setters and eyoc_ransac_workspace_bytes take the ctx first (round 5), eyoc_maps_gather_window
 * refuses Z-ordered maps again and eyoc_maps_gather_window_internal exists, eyoc_model_workspace_bytes depends on the maps' size class */
#define EYOC_VERSION 111

/* ------------------------------------------------------------------------------------------------
 * context
 * --------------------------------------------------------------------------------------------- */
int eyoc_version(void);
const char* eyoc_last_error(void);
int eyoc_create(int device, eyoc_ctx** out);
int eyoc_destroy(eyoc_ctx* ctx);
/* The kernel-selection and tiling switches declared further down (eyoc_maps_order_*, eyoc_maps_select_orders, eyoc_maps_internal_order,
 * eyoc_spconv_select_*, eyoc_spconv_st_*, eyoc_spconv_upc_min_rows, eyoc_model_fuse_tail, eyoc_knn_prefilter, eyoc_ransac_select_pruning,
 * eyoc_ransac_transform_store) are state of the ctx they are given: every entry point reads them from ITS ctx (file-scope statics until
 * round 4).  They exist for parity tests and profiling; production code never calls them.  Each returns the previous value (-1 for a
 * NULL ctx) and only queries when the argument is out of range. */
/* Tests only (no production path calls it): fills the whole scratch the ctx currently owns with `byte` on `stream`, ordered on the
 * scratch exactly as a consumer is (the same hand-over between streams).  Returns the scratch size in bytes, 0 when the ctx owns
 * none yet, a negative eyoc_status on error.  The workspace contract tests use it to show that no consumer of the ctx scratch reads
 * what an earlier call - its own or another consumer's - left there. */
long long eyoc_debug_scratch_fill(eyoc_ctx* ctx, int byte, void* stream);

/* ------------------------------------------------------------------------------------------------
 * coordinate maps + rulebooks
 *   replaces: ME.SparseTensor(features, coordinates=) and the coordinate manager it creates
 *             (scripts/test_kitti.py:143-148, util/transform_estimation.py:128-131), and the kernel
 *             maps MinkowskiConvolution / MinkowskiConvolutionTranspose build on first use
 *             (model/resunet.py:31-116, model/residual_block.py:23-33).
 *   coords: int32 [n,4] = (batch, x, y, z), unique rows; |x|,|y|,|z| < 2^17, 0 <= batch < 1024.
 *   Builds the 4 levels (tensor stride 1,2,4,8) and, per level, output-stationary neighbour tables
 *   nbr[27][n_out] (int32 input row or -1): stride-1 (EYOC_MAP_S1), strided ts->2ts
 *   (EYOC_MAP_DOWN, indexed by the fine level) and transposed 2ts->ts (EYOC_MAP_UP, indexed by the
 *   fine level).  Kernel offsets enumerate x fastest.  Row order of level 0 is the input order;
 *   coarser levels are ordered by first occurrence.
 *   The workspace (eyoc_maps_workspace_bytes(n) bytes, 256-byte aligned) is owned by the caller and
 *   must outlive the maps object.  This call synchronises `stream` (3 small read-backs).
 * --------------------------------------------------------------------------------------------- */
typedef enum { EYOC_MAP_S1 = 0, EYOC_MAP_DOWN = 1, EYOC_MAP_UP = 2 } eyoc_map_kind;

typedef struct {
  int32_t n_levels;
  int32_t rows[EYOC_MAX_LEVELS];        /* N1, N2, N4, N8                                   */
  int64_t pairs_s1[EYOC_MAX_LEVELS];    /* valid entries of each stride-1 table             */
  int64_t pairs_down[EYOC_MAX_LEVELS];  /* [l] = table level l -> l+1 (l < n_levels-1)      */
  int64_t pairs_up[EYOC_MAX_LEVELS];    /* [l] = table level l+1 -> l                       */
  int64_t pairs_conv1;                  /* valid (row, offset) pairs of the first conv      */
} eyoc_maps_info_t;

size_t eyoc_maps_workspace_bytes(int n_rows);
int eyoc_maps_build(eyoc_ctx* ctx, const int32_t* coords_dev, int n_rows, void* workspace_dev,
                    size_t workspace_bytes, void* stream, eyoc_maps** out);
/* eyoc_maps_build keeps the CALLER's row order (the accessors below return level coordinates and tables in the caller's
 * rows).  The same with the internal row order chosen by the caller: -1 automatic (Z-order from 8192 rows: what
 * eyoc_model_forward is fastest on), 0 the caller's order (the level coordinates and tables the accessors below return
 * are then in the caller's rows), 1 Z-order.  eyoc_maps_internal_order(ctx, 0 / 1) overrides it for every build of that ctx. */
int eyoc_maps_build_ordered(eyoc_ctx* ctx, const int32_t* coords_dev, int n_rows, void* workspace_dev,
                            size_t workspace_bytes, void* stream, int order, eyoc_maps** out);
/* Which batch indices made the ctx's LAST build fail (eyoc_maps_build / _ordered): dup / range (host arrays of 32 words) get bit b of
 * word b >> 5 for every batch index b < 1024 that holds a duplicate row / a row outside the key range (a row whose own batch index is
 * outside [0, 1024) sets no bit).  Every build clears both masks first; a build that fails with EYOC_ERR_RANGE fills the range mask
 * only, one that fails with EYOC_ERR_DUPLICATE the dup mask only (the range check comes first: with rows out of range the caller-order
 * path does not look for duplicates at all), and any other return leaves both 0.  The build's kernels set the bits from the faulty
 * rows only and the masks come back with the read-back that detects the fault; return codes and messages are unchanged. */
int eyoc_maps_last_fault_batches(const eyoc_ctx* ctx, uint32_t* dup, uint32_t* range);
int eyoc_maps_free(eyoc_maps* maps);
/* Row order the transposed convolutions tile their outputs in: the rows of `level` (a fine level, 0 <= level <
 * n_levels-1) sorted, stably, by the pattern of coarse blocks their transposed map reaches.  Purely a
 * scheduling aid (tiles whose rows share their occupied kernel offsets) - results do not depend on it.
 * out_dev: int32 [rows[level]]. */
int eyoc_maps_copy_up_order(const eyoc_maps* maps, int level, int32_t* out_dev, void* stream);
/* Levels with fewer rows than this keep the natural order (the sorts only pay off for the large-batch kernel;
 * default 65536).  Per ctx; min_rows < 0 only queries.  Returns the previous value.  For tests / profiling. */
int eyoc_maps_order_min_rows(eyoc_ctx* ctx, int min_rows);
/* Z-ordered maps sort their tiling orders inside windows of 2^shift consecutive rows (default 18; the window's rows and
 * their neighbours stay cache-resident while its pattern runs are walked).  Per ctx; shift < 0 only queries.
 * Returns the previous value.  For tests / profiling. */
int eyoc_maps_order_window_shift(eyoc_ctx* ctx, int shift);
/* Which tables get a pattern-sorted tiling order at all: s1 = the stride-1 tables (default 1), down = the strided tables of
 * Z-ordered maps (default 0: natural order wins there).  0 / 1 set, anything else leaves the switch alone.  Returns the
 * previous state (s1 | down << 1).  Per ctx, read when maps are built; for tests / profiling. */
int eyoc_maps_select_orders(eyoc_ctx* ctx, int s1, int down);
/* Internal row order.  From 8192 rows on (mode -1, the default) the maps store level 0 in Z-order (Morton order of
 * (batch, x, y, z)) instead of the caller's order, so that 64 consecutive rows are a compact blob of voxels - what
 * the tile-local input stage of the sparse convolution needs.  eyoc_maps_coords / _table then describe the INTERNAL
 * rows; eyoc_maps_row_order returns the device array perm[i] = caller's row of internal row i (NULL: the caller's order
 * was kept).  eyoc_model_forward reads its input and writes its output in the caller's order either way.
 * eyoc_maps_internal_order(mode): -1 automatic, 0 always the caller's order, 1 always Z-order; returns the previous
 * mode + 2; per ctx, for tests. */
int eyoc_maps_internal_order(eyoc_ctx* ctx, int mode);
/* Lazy tables (round 6, default on): a Z-ordered build of >= eyoc_spconv_upc_min_rows rows derives the tile records of the finest
 * level's stride-1 table and of the transposed tables straight from the octree links and leaves those [27][n] tables unwritten (their
 * only readers on the hot path were the record builders: 0.8 GB per 128-cloud batch).  They are filled on first use - by
 * eyoc_maps_table / _copy_table / _info, by a forward whose layer runs a gathering kernel, by a build whose records overflowed - so
 * nothing a caller can observe changes.  eyoc_maps_lazy_tables(ctx, 0) builds every table eagerly again; returns the previous setting. */
int eyoc_maps_lazy_tables(eyoc_ctx* ctx, int on);
/* EYOC_VERSION >= 111.  Z-ordered builds make the three coarser levels (coordinates, parent and child links) in two launches over the
 * sorted level-0 rows (default, round 6) instead of four short dependent launches per level; the arrays are the same bit for bit.
 * eyoc_maps_fused_levels(ctx, 0) brings the per-level kernels back (tests compare); returns the previous setting. */
int eyoc_maps_fused_levels(eyoc_ctx* ctx, int on);
/* Strided convolutions of a split16 forward on Z-ordered maps of >= eyoc_spconv_upc_min_rows rows: 1 (default, round 6) the staged kernel
 * on 128-row output tiles (tile records built by eyoc_maps_build), 0 the gathering kernel; returns the previous setting. */
int eyoc_spconv_select_down_kernel(eyoc_ctx* ctx, int mode);
const int32_t* eyoc_maps_row_order(const eyoc_maps* maps);
/* stream-ordered copy of the same array (the identity when the caller's order was kept); out_dev: int32 [rows[0]] */
int eyoc_maps_copy_row_order(const eyoc_maps* maps, int32_t* out_dev, void* stream);
int eyoc_maps_rows(const eyoc_maps* maps, int level);
/* What a build kept of its tile records (Z-ordered builds; DESIGN.md "Records that overflow"): 1 when the maps hold records of that
 * family and level, 0 when the build never asked for them or dropped them because a tile did not fit its stage - the layers of that
 * family and level then run on the gathering kernels.  Reads host fields only: no device work, no synchronisation.  EYOC_ERR_INVALID
 * for NULL maps, a family outside the enum or a level outside [0, n_levels).  For tests and diagnostics. */
typedef enum {
  EYOC_RECORDS_S1 = 0,    /* stride-1 table, 256-row tiles                                    */
  EYOC_RECORDS_S1W = 1,   /* stride-1 table, 128-row tiles (the coarsest level)               */
  EYOC_RECORDS_DOWN = 2,  /* strided table level -> level + 1, 128-row tiles                  */
  EYOC_RECORDS_UP = 3,    /* transposed table level + 1 -> level, Morton tiles                */
  EYOC_RECORDS_UPC = 4    /* transposed table level + 1 -> level, class-major tiles           */
} eyoc_records_family;
int eyoc_maps_records(const eyoc_maps* maps, int family, int level);
/* Streams. A maps object may be read on any stream, not only the one it was built on: everything the build writes is complete when
 * eyoc_maps_build returns, and what is filled later on demand (lazy tables, the level-0 hash table) is filled on the stream of the
 * first call that needs it, which records an event; every later reader - eyoc_maps_table / _copy_table / _info, a forward, a window
 * gather - waits for that event, on the host (eyoc_maps_table) or on its own stream (everything else).  The maps' workspace is the
 * caller's: it must not be reused before the work of every stream that read the maps has finished (torch callers: record_stream).
 * eyoc_maps_free waits for fills still pending and may be called while readers are in flight.  Like its ctx, a maps object is
 * single-threaded: one host thread at a time. */
/* device pointers into the workspace; valid while the maps object lives */
const int32_t* eyoc_maps_coords(const eyoc_maps* maps, int level);             /* [rows,4]        */
/* [27][n_out]; a table filled on demand is filled first if need be (NULL stream) and waited for on the host: the pointer is valid for
 * any stream */
const int32_t* eyoc_maps_table(const eyoc_maps* maps, int kind, int level);
/* stream-ordered device-to-device copies of the same arrays into caller-owned buffers (a table filled on demand: filled on `stream`, or
 * `stream` waits for its earlier fill) */
int eyoc_maps_copy_coords(const eyoc_maps* maps, int level, int32_t* out_dev, void* stream);
int eyoc_maps_copy_table(const eyoc_maps* maps, int kind, int level, int32_t* out_dev, void* stream);
/* counts valid pairs (one reduction per table + a sync); conv1_kernel_size 0 skips pairs_conv1 */
int eyoc_maps_info(eyoc_ctx* ctx, const eyoc_maps* maps, int conv1_kernel_size, void* stream,
                   eyoc_maps_info_t* info);

/* ------------------------------------------------------------------------------------------------
 * voxeliser (the step immediately before the path; SURVEY.md 8f "next" row 1)
 *   replaces: ME.utils.sparse_quantize(xyz / voxel_size, return_index=True) followed by
 *             floor(xyz[sel] / voxel_size).int()   (lib/data_loaders.py:940-943,969-979; util/misc.py:80-84)
 *   xyz f32 rows of `stride` floats (3 = xyz, 4 = KITTI .bin xyzr) -> sel int32 [n_out] = index of the
 *   first point of every occupied voxel, ascending; coords int32 [n_out,4] = (batch_index, floor(p / v)).
 *   Outputs need room for n rows.  Synchronises `stream` once (to return n_out).
 *   A NaN or +-inf in x, y or z fails the call with EYOC_ERR_RANGE, like a point outside the key range (a fourth float is never read).
 * --------------------------------------------------------------------------------------------- */
size_t eyoc_voxelize_workspace_bytes(int n_points);
int eyoc_voxelize(eyoc_ctx* ctx, const float* xyz_dev, int n_points, int stride, float voxel_size, int batch_index,
                  int32_t* sel_dev, int32_t* coords_dev, int* n_out, void* workspace_dev, size_t workspace_bytes,
                  void* stream);

/* ------------------------------------------------------------------------------------------------
 * batched voxeliser + collation (SURVEY.md 8f "next": batched voxelise + collate)
 *   replaces: the per-cloud ME.utils.sparse_quantize(xyz / voxel_size, return_index=True) +
 *             floor(xyz[sel] / voxel_size).int() of lib/data_loaders.py:940-943,969-979 for a whole batch,
 *             and the ME.utils.sparse_collate of collate_pair_fn (lib/data_loaders.py:31-85)
 *   xyz_dev: n_clouds clouds packed back to back, rows of `stride` floats (3 = xyz, 4 = KITTI xyzr);
 *   point_offsets (HOST, int64 [n_clouds+1]): cloud b is rows point_offsets[b] .. point_offsets[b+1]; monotone,
 *   point_offsets[0] = 0, point_offsets[n_clouds] = n_points <= 2^30; empty clouds allowed anywhere.
 *   1 <= n_clouds, batch_base + n_clouds <= 1024.
 *   Output: bit for bit the concatenation, in cloud order, of eyoc_voxelize(cloud b, voxel_size, batch_base + b):
 *   sel int32 = index of the kept point WITHIN its cloud (ascending per cloud), coords int32 [.,4] =
 *   (batch_base + b, floor(p / v)), xyz_out f32 [.,3] = the kept points' xyz (or NULL: not written);
 *   voxel_offsets (HOST out, int64 [n_clouds+1]) = the clouds' row ranges of the outputs.  Outputs need room for
 *   n_points rows.  A point outside the key range fails the call (EYOC_ERR_RANGE; the message names the first cloud
 *   holding one).  A NaN or +-inf in x, y or z fails the call with EYOC_ERR_RANGE in the same way.  Synchronises `stream` once per
 *   call; n_points = 0 launches nothing.
 * --------------------------------------------------------------------------------------------- */
size_t eyoc_voxelize_batched_workspace_bytes(int n_points_total, int n_clouds);
int eyoc_voxelize_batched(eyoc_ctx* ctx, const float* xyz_dev, int stride, const int64_t* point_offsets, int n_clouds,
                          int n_points, float voxel_size, int batch_base, int32_t* sel_dev, int32_t* coords_dev,
                          float* xyz_out_dev, int64_t* voxel_offsets, void* workspace_dev, size_t workspace_bytes,
                          void* stream);
/* The same call for a caller that isolates failures: instead of failing on a bad point it counts, per cloud, the finite points
 * outside the key range (cloud_faults[b][0]) and the points with a NaN / +-inf in x, y or z (cloud_faults[b][1]; HOST out, int32
 * [n_clouds][2]) and returns EYOC_OK.  A cloud with a non-zero count contributes NO voxels (its range in voxel_offsets is empty);
 * every other cloud's rows are bit for bit those of eyoc_voxelize_batched, at the same batch index.  The counts come back with the
 * call's one read-back.  The workspace holds two more counters per cloud. */
size_t eyoc_voxelize_batched_isolating_workspace_bytes(int n_points_total, int n_clouds);
int eyoc_voxelize_batched_isolating(eyoc_ctx* ctx, const float* xyz_dev, int stride, const int64_t* point_offsets, int n_clouds,
                                    int n_points, float voxel_size, int batch_base, int32_t* sel_dev, int32_t* coords_dev,
                                    float* xyz_out_dev, int64_t* voxel_offsets, void* workspace_dev, size_t workspace_bytes,
                                    void* stream, int32_t* cloud_faults);

/* ------------------------------------------------------------------------------------------------
 * centroid voxel down-sampling for a batch of clouds.  Added after 111 without a bump, additive only; opt-in, nothing else calls it.
 *   replaces: Open3D's PointCloud::VoxelDownSample as the reference calls it (pcd.voxel_down_sample(voxel_size),
 *             util/pointcloud.py:38,43-44), restated as a contract of this library (parity unpinned: Open3D is not part of any build
 *             here; tests/downsample_restatement.py is the fp64 statement the kernels are held to).  NOT the voxeliser above: that one
 *             keeps the first point of a voxel on a grid anchored at the origin, this one the mean of all its points on a grid
 *             anchored half a voxel below the cloud's minimum corner.
 *   xyz_dev, stride (3 or 4), point_offsets (HOST), n_clouds (1 .. 1024), n_points (<= 2^30): as eyoc_voxelize_batched.  attr_dev f32
 *   [n_points][n_attr] (0 <= n_attr <= 8; NULL or n_attr = 0: none): per-point columns that are averaged like the coordinates.
 *   Per cloud b with rows p_i (f32, widened exactly to f64; every operation below fp64 and rounded on its own, no fused multiply-add):
 *     origin   vmin_k = min_i p_i[k] - 0.5 * voxel_size
 *     cell     c_i[k] = floor((p_i[k] - vmin_k) / voxel_size)
 *     rows     a voxel = the cloud's points with equal c.  The cloud's output rows are its voxels in ascending order of their lowest
 *              point index (the voxeliser's "sel ascending" rule).  first = that index within the cloud, count = the voxel's points,
 *              inverse[i] = the row, within the cloud's output range, that point i went into.
 *     sums     per voxel and column: s = 0.0; for i in ascending point index: s += (double)p_i[k]; out = (float)(s / (double)count) -
 *              one division, one rounding.  attr_out the same over the attribute columns.  This sequential order IS the contract.
 *     status   status_dev[b] = EYOC_ICP_RANGE for a cloud with a NaN or +-inf in x, y or z (a fourth float and the attributes are
 *              never tested), or whose largest cell floor((max_i p_i[k] - vmin_k) / voxel_size) is 2^17 or more on an axis: it
 *              contributes no rows and its inverse entries are -1; every other cloud's rows are unchanged.  Else 0 (empty clouds too).
 *   xyz_out_dev f32 [.,3], attr_out_dev f32 [.,n_attr], first_dev / count_dev int32 [.] need room for n_points rows; inverse_dev int32
 *   [n_points]; first_dev, count_dev, inverse_dev may each be NULL.  voxel_offsets (HOST out, int64 [n_clouds+1]) = the clouds' row
 *   ranges, back with the call's ONE stream synchronisation; rows past voxel_offsets[n_clouds] are not written.  n_points = 0 launches
 *   nothing and writes nothing on the device (voxel_offsets = 0).  EYOC_ERR_INVALID for a voxel_size that is not positive and
 *   finite, a stride other than 3 / 4, n_attr outside [0, 8] or offsets that do not describe n_points.  Caller-owned workspace of
 *   eyoc_voxel_downsample_workspace_bytes, 256-byte aligned: a misaligned or smaller one is EYOC_ERR_WORKSPACE before any launch; its
 *   previous contents do not matter.  No allocation, no floating-point atomics (the bounds use integer min / max, which commute).  A
 *   cloud's bytes are the same from run to run, alone, and at any place in a batch.
 *   eyoc_voxel_downsample_batched_timed (diagnostics, scripts/bench_downsample.py): the same call with events between its stages;
 *   stage_ms (HOST out, float [7]) = bounds + status, keys, sort, run heads, flag scan, row numbers + offsets, sums, in milliseconds.
 * --------------------------------------------------------------------------------------------- */
size_t eyoc_voxel_downsample_workspace_bytes(int n_points_total, int n_clouds, int n_attr);
int eyoc_voxel_downsample_batched(eyoc_ctx* ctx, const float* xyz_dev, int stride, const int64_t* point_offsets, int n_clouds, int n_points,
                                  double voxel_size, const float* attr_dev, int n_attr, float* xyz_out_dev, float* attr_out_dev,
                                  int32_t* first_dev, int32_t* count_dev, int32_t* inverse_dev, int32_t* status_dev,
                                  int64_t* voxel_offsets, void* workspace_dev, size_t workspace_bytes, void* stream);
int eyoc_voxel_downsample_batched_timed(eyoc_ctx* ctx, const float* xyz_dev, int stride, const int64_t* point_offsets, int n_clouds,
                                        int n_points, double voxel_size, const float* attr_dev, int n_attr, float* xyz_out_dev,
                                        float* attr_out_dev, int32_t* first_dev, int32_t* count_dev, int32_t* inverse_dev,
                                        int32_t* status_dev, int64_t* voxel_offsets, void* workspace_dev, size_t workspace_bytes,
                                        void* stream, float* stage_ms);

/* ------------------------------------------------------------------------------------------------
 * per-pair failure isolation: drop clouds from a collated batch
 *   coords_dev int32 [n,4] (batch, x, y, z), feats_dev f32 [n,c] or NULL, rows in any order (clouds may interleave).
 *   drop_mask (HOST, 32 words, the layout of eyoc_maps_last_fault_batches): bit b set = every row of batch index b goes; rows whose
 *   batch index is outside [0, 1024) stay.  Outputs (room for n rows each; not in place): the kept rows' coordinates and features
 *   in input order with their batch indices UNCHANGED (a map build accepts gaps), row_map int32 [n] = old row -> new row, -1 for a
 *   dropped row.  n_kept (HOST out): the kept rows; kept_per_batch (HOST out, int32 [1024], or NULL): the kept rows of every batch
 *   index.  Deterministic (no atomics on the data path).  Stream-ordered on `stream`, which it synchronises once (the counts);
 *   n = 0 launches nothing.  eyoc_remap_rows: out[k] = row_map[idx[k]] (-1 for an index outside [0, n)); out == idx is allowed.
 * --------------------------------------------------------------------------------------------- */
size_t eyoc_batch_drop_workspace_bytes(int n_rows);
int eyoc_batch_drop(eyoc_ctx* ctx, const int32_t* coords_dev, const float* feats_dev, int n_rows, int c, const uint32_t* drop_mask,
                    int32_t* coords_out_dev, float* feats_out_dev, int32_t* row_map_dev, int* n_kept, int32_t* kept_per_batch,
                    void* workspace_dev, size_t workspace_bytes, void* stream);
int eyoc_remap_rows(eyoc_ctx* ctx, const int64_t* idx_dev, int m, const int32_t* row_map_dev, int n_rows, int64_t* out_dev,
                    void* stream);

/* ------------------------------------------------------------------------------------------------
 * one sparse convolution layer (unit tests, profiling)
 *   replaces: one MinkowskiConvolution / MinkowskiConvolutionTranspose forward with the batch norm
 *             that follows it folded in, plus the residual add / ReLU / concat write around it
 *             (model/residual_block.py:37-53, model/resunet.py:142-186).
 *   out[o, :] = act( sum_k in[nbr[k][o], :] @ W[k] + bias (+ res[o, :]) ),  nbr == NULL: K must be
 *   1 and the map is the identity (1x1 convolution).  cin % 32 == 0, cout in {32,64,128,256}; every entry of
 *   nbr must be < 2^24 (the model forward checks its level sizes; ~550 clouds of 30k voxels in one batch).
 *   Weights must be in the packed layout produced by eyoc_spconv_pack_weights (host side).
 * --------------------------------------------------------------------------------------------- */
size_t eyoc_spconv_packed_floats(int K, int cin, int cout);
int eyoc_spconv_pack_weights(const float* w_host /*[K,cin,cout]*/, const float* scale_host /*[cout]|NULL*/,
                             int K, int cin, int cout, float* packed_host);
int eyoc_spconv(eyoc_ctx* ctx, const int32_t* nbr_dev, int K, int n_out, const float* in_dev,
                int ld_in, int cin, const float* wpacked_dev, int cout, const float* bias_dev,
                const float* res_dev, int ld_res, int relu, float* out_dev, int ld_out, void* stream);
/* The same layer on the fp16 matrix pipe at fp32 accuracy ("split16", eyoc_amd/csrc/spconv_wave.hip): math = 1 expects
 * `in_dev` / `res_dev` rows in the SPLIT16 format (eyoc_split16_encode: per 32 channels 64 B of fp16 hi halves + 64 B
 * of fp16 lo halves, x = hi + lo to 2^-22 - the same 4 bytes per channel, so leading dimensions are unchanged; column
 * offsets and widths must be multiples of 32 channels) and
 * weights packed by eyoc_spconv_pack_weights_split16, which also returns the scalar the kernel multiplies its sums
 * with (upload it and pass it as out_scale_dev).  out_split = 1 writes SPLIT16 rows, 0 fp32 rows.  math = 0 is
 * eyoc_spconv.  n_in = rows of the input tensor (0 = unknown: every entry of nbr is assumed < 2^24).  Two kernels
 * implement split16 layers - wave-private (spconv_wave.hip, pair compaction + LDS accumulators) and row-stationary
 * (spconv_rs.hip, register accumulators + zero operands, weights shared through LDS); the launcher picks per layer,
 * eyoc_spconv_select_split16_kernel forces one (0 wave-private, 2 row-stationary, 1 automatic; returns the previous
 * mode; per ctx, for tests and profiling). */
int eyoc_spconv_select_split16_kernel(eyoc_ctx* ctx, int mode);
/* Staged kernel for the transposed 3^3 / stride-2 convolutions on Z-ordered maps (spconv_up.hip: tile rows sorted by
 * parity class, only occupied (16-row group, offset) blocks multiplied): 1 on (default: as fast as the row-stationary
 * kernel in windowed pattern order, 18 GB less HBM traffic per 128-cloud forward), 0 off (gathering kernels), 2 (default since
 * round 4) = the class-major kernel below for batches and this one for small inputs; other values only query.  Returns the
 * previous state.  Per ctx, read when maps are built; for tests and profiling. */
int eyoc_spconv_select_up_kernel(eyoc_ctx* ctx, int on);
/* The same layers in CLASS-MAJOR order (spconv_upc.hip; eyoc_spconv_select_up_kernel(2)): the fine rows are partitioned by parity
 * class (8 classes of 1-8 offsets), a tile is 256 rows of one class and runs the staged kernel's assembly loop over that class's
 * offsets only.  Standalone entry points (the model uses the same kernels through its maps): workspace size for a table with
 * n_out fine rows; build (ws_dev 256-byte aligned; info_host = NULL or 19 ints {tiles, first tile of class 0..8, rows of class
 * 0..7, tiles with more distinct coarse rows than two stage passes hold - the kernel must not be used then}, which
 * synchronises the stream); the layer (split16 rows in, split16 or fp32 rows out, no residual).
 *   replaces: ME.MinkowskiConvolutionTranspose(kernel_size=3, stride=2) of model/resunet.py:83-116 */
/* eyoc_spconv_select_up_kernel(2) (the default) uses the class-major kernel for maps with at least this many level-0 rows (default
 * 2^17; the partition's extra launches cost a single 60 k-voxel pair more than the kernel saves) and spconv_up.hip below; a
 * negative argument only queries; returns the previous value.  Per ctx, read when maps are built. */
int eyoc_spconv_upc_min_rows(eyoc_ctx* ctx, int rows);
/* Rows per tile of the classes with `odd_axes` (0..3) odd axes: 128..256, a multiple of 16 (default 256, and 192 for the
 * 8-offset class, whose 256-row tiles would need two stage passes).  Current device; read when records are built; for
 * measurements (workspace sizes assume >= 128). */
int eyoc_spconv_upc_tile_rows(int odd_axes, int rows);
size_t eyoc_spconv_upc_bytes(int n_out);
int eyoc_spconv_upc_build(eyoc_ctx* ctx, const int32_t* nbr_dev, int n_out, void* ws_dev, int32_t* info_host, void* stream);
int eyoc_spconv_upc(eyoc_ctx* ctx, const int32_t* nbr_dev, const void* ws_dev, int n_out, int n_in, const float* in_dev, int ld_in,
                    int cin, const float* wpacked_dev, int cout, const float* bias_dev, int relu, float* out_dev, int ld_out,
                    int out_split, const float* out_scale_dev, void* stream);
/* First convolution (C_in = 1, 32 output channels) of split16 forwards on Z-ordered maps (default 3): 1 = conv1_bf_kernel - the block
 * feature vectors (8 child features per level-1 row) of a 256-parent tile's neighbourhood staged in LDS through the level-1 tile
 * rulebook, the tile's fine rows grouped by parity class, a K = 27 product over blocks; 0 = conv1_mfma_kernel, which probes
 * the octree per fine row; 2 = the exact-fp32 octree walker (conv1_tree_kernel) even in front of split16 consumers; 3 =
 * conv1_bfp_kernel - the products of 1 in the same order (bit-identical rows and range words) from one persistent 512-thread
 * workgroup per CU: wave = parity class with its weights resident in registers, two tile buffers in LDS, the next tile's loads in
 * flight under the current tile's MFMAs.  Other values only query.  Returns the previous state; per ctx, for tests and profiling. */
int eyoc_spconv_select_conv1_kernel(eyoc_ctx* ctx, int on);
/* Grid of conv1_bfp_kernel: 0 (default) = one workgroup per compute unit, n > 0 = n workgroups (never more than the level-1 tiles;
 * tests make one workgroup walk many tiles with it); negative only queries.  Results do not depend on it.  Returns the previous value; per ctx. */
int eyoc_spconv_conv1_workgroups(eyoc_ctx* ctx, int workgroups);
/* Stride-1 (3^3) split16 layers with a tile-local input stage (spconv_st.hip): per 256-row tile the distinct input rows are
 * copied to LDS once per 32-channel block and all 27 offsets run from there.  Needs the table's per-tile "local
 * rulebooks" (built once per table; *overflow_dev counts 256-row tiles with more than 1278 distinct input rows - the staged
 * kernel must not be used when it is non-zero; rows in Morton order never overflow).  eyoc_model_forward builds and
 * uses them itself; these entry points exist for tests and profiling.
 * eyoc_spconv_select_st_kernel picks the implementation of the offset loop: 1 (default) = hand-scheduled gfx950 assembly
 * with scalar branches around the MFMAs of empty (16-row chunk, offset) blocks; 2 = the same without the branches;
 * 0 = the compiler-scheduled C++ loop.  Any other value only queries.  Returns the previous variant; per ctx, for tests and profiling. */
int eyoc_spconv_select_st_kernel(eyoc_ctx* ctx, int variant);
/* A layer with fewer than `workgroups` 64-output-channel workgroups (default 1024 = two rounds of the chip's 512 slots) runs
 * in 32-channel workgroups instead (twice as many, each half as long: single pairs and small batches).  0 = never (tests force
 * the wide kernels onto small clouds with it); negative only queries.  Returns the previous threshold; per ctx. */
int eyoc_spconv_st_split_below(eyoc_ctx* ctx, int workgroups);
/* Row grouping inside the 256-row tile records (default on): the builder sorts a tile's rows by their neighbour pattern so that the 16
 * rows of an MFMA chunk miss the same offsets - the staged loop skips (chunk, offset) blocks without a neighbour, and 0.81-0.93 of
 * them are non-empty in row order, 0.68-0.72 grouped.  Results are bit-identical either way (only the order of a tile's rows inside
 * its workgroup changes).  1 / 0 set, anything else only queries; returns the previous state; per ctx, read when records are built. */
int eyoc_spconv_st_group_rows(eyoc_ctx* ctx, int on);
/* Small inputs (a single pair: the level-3 layer is 72 workgroups walking 8 input blocks x 27 offsets each): eyoc_model_forward lets
 * the staged kernel split a tile's 32-channel input blocks over several workgroups (partial sums in the forward's workspace, added in
 * share order by a second launch: bit-reproducible).  1 on (default) / 0 off, anything else only queries; returns the
 * previous state; per ctx, for tests and profiling.  Results differ from the unsplit kernel by fp32 rounding (another
 * summation order). */
int eyoc_spconv_st_ksplit(eyoc_ctx* ctx, int on);
size_t eyoc_spconv_local_rulebook_bytes(int n_out);
int eyoc_spconv_build_local_rulebook(eyoc_ctx* ctx, const int32_t* nbr_dev, int K, int n_out, void* out_dev,
                                     int32_t* overflow_dev, void* stream);
int eyoc_spconv_staged(eyoc_ctx* ctx, const int32_t* nbr_dev, const void* local_dev, int n_out, int n_in, const float* in_dev,
                       int ld_in, int cin, const float* wpacked_dev, int cout, const float* bias_dev, const float* res_dev,
                       int ld_res, int relu, float* out_dev, int ld_out, int out_split, const float* out_scale_dev, void* stream);
/* The same two on 128-row tiles - the records and the kernel family of the strided layers and of the wide (>= 128-channel) workgroups -
 * for tests and profiling; arguments as above.  The records of n_out rows take eyoc_spconv_local_rulebook_bytes(2 * n_out) bytes: one
 * record per 128 rows, and cdiv(n, 128) = cdiv(2 n, 256).  eyoc_spconv_select_down_kernel(2 / 3) picks 64- / 128-channel workgroups
 * for layers with >= 128 output channels. */
int eyoc_spconv_build_local_rulebook128(eyoc_ctx* ctx, const int32_t* nbr_dev, int K, int n_out, void* out_dev,
                                        int32_t* overflow_dev, void* stream);
int eyoc_spconv_staged128(eyoc_ctx* ctx, const int32_t* nbr_dev, const void* local_dev, int n_out, int n_in, const float* in_dev,
                          int ld_in, int cin, const float* wpacked_dev, int cout, const float* bias_dev, const float* res_dev,
                          int ld_res, int relu, float* out_dev, int ld_out, int out_split, const float* out_scale_dev, void* stream);
int eyoc_spconv_pack_weights_split16(const float* w_host, const float* scale_host, int K, int cin, int cout,
                                     float* packed_host, float* out_scale_host);
int eyoc_spconv_ex(eyoc_ctx* ctx, const int32_t* nbr_dev, int K, int n_out, int n_in, const float* in_dev, int ld_in, int cin,
                   const float* wpacked_dev, int cout, const float* bias_dev, const float* res_dev, int ld_res, int relu,
                   float* out_dev, int ld_out, int math, int out_split, const float* out_scale_dev, void* stream);
int eyoc_split16_encode(eyoc_ctx* ctx, const float* in_dev, int n, int c, int ld_in, float* out_dev, int ld_out, void* stream);
int eyoc_split16_decode(eyoc_ctx* ctx, const float* in_dev, int n, int c, int ld_in, float* out_dev, int ld_out, void* stream);
/* The bare operator out[o] = sum_k in[nbr[k][o]] W[k] for the training path (forward and input gradient of autograd.sparse_conv;
 * lib/trainer.py:1655-1676 runs them through MinkowskiEngine): no epilogue, fp32 MFMAs, and for small inputs the launcher may split
 * the K offsets over 2-4 workgroups per row tile (scratch of the ctx; shares added in a fixed order) - the summation order then depends
 * on n_out, which eyoc_spconv never lets happen.  Same argument meaning as eyoc_spconv.  The split's shares live in the ctx's ONE
 * grow-only scratch, which kNN / label kernels / RANSAC of the same ctx use too: a call on another stream first waits (event) for
 * the previous user's stream, i.e. offset-split training layers and matching on a second stream of the same ctx serialise there -
 * give concurrent phases their own eyoc_ctx. */
int eyoc_spconv_sum(eyoc_ctx* ctx, const int32_t* nbr_dev, int K, int n_out, const float* in_dev, int ld_in, int cin,
                    const float* wpacked_dev, int cout, float* out_dev, int ld_out, void* stream);
/* Backward of one layer (the reference back-propagates through MinkowskiEngine, lib/trainer.py:1667).
 *   grad-input: dIn[i] = sum_k dOut[o] W[k]^T over the pairs (i -> o, k) is a sparse convolution over the TRANSPOSED
 *     rulebook - for a stride-1 table the same table with mirrored offsets (mirror = 1), for the strided (EYOC_MAP_DOWN)
 *     table the EYOC_MAP_UP table of the same level and vice versa (mirror = 0) - so it runs eyoc_spconv on weights
 *     packed by eyoc_spconv_pack_weights_transposed (C_in and C_out swap roles: the call has cin = C_out, cout = C_in).
 *   grad-weight: dW[k][ci][co] = sum over o with nbr[k][o] >= 0 of in[nbr[k][o]][ci] * dout[o][co], plain [K, cin, cout]
 *     layout, fp32 MFMA, deterministic (fixed reduction order).  C_in, C_out: multiples of 16; nbr == NULL: identity map. */
int eyoc_spconv_pack_weights_transposed(const float* w_host /*[K,cin,cout]*/, int K, int cin, int cout, int mirror,
                                        float* packed_host);
size_t eyoc_spconv_grad_weight_workspace_bytes(int K, int n_out, int cin, int cout);
int eyoc_spconv_grad_weight(eyoc_ctx* ctx, const int32_t* nbr_dev, int K, int n_out, const float* in_dev, int ld_in, int cin,
                            const float* dout_dev, int ld_dout, int cout, float* dw_dev, void* workspace_dev,
                            size_t workspace_bytes, void* stream);
/* Two decompositions implement the operator (workgroup-tiled: spconv.hip, wave-private: spconv_wave.hip);
 * by default the launcher picks by problem size.  mode -1 = automatic (default), 0 = workgroup-tiled,
 * 1 = wave-private.  Per ctx; meant for parity tests and profiling.  Returns the previous mode. */
int eyoc_spconv_select_kernel(eyoc_ctx* ctx, int mode);

/* ------------------------------------------------------------------------------------------------
 * ResUNet2 family (ResUNetBN2C in production)
 *   replaces: Model(in_channels, out_channels, bn_momentum=, conv1_kernel_size=, normalize_feature=)
 *             + load_state_dict + eval + __call__   (model/resunet.py:18-193,
 *             scripts/test_kitti.py:83-93,143-150).
 *   Layers are matched by MinkowskiEngine state_dict names: "conv1", "norm1", "block1.conv1",
 *   "block1.norm1", ... "conv1_tr", "final".  Batch norms are folded into the preceding
 *   convolution (eval mode, eps = bn_eps).
 *   The packed weights live in a caller-owned device blob of eyoc_model_blob_floats() floats so it
 *   can be broadcast between ranks: rank 0 passes `layers`, the others pass layers == NULL after
 *   receiving the blob.
 * --------------------------------------------------------------------------------------------- */
typedef struct {
  int32_t in_channels, out_channels, conv1_kernel_size, normalize_feature;
  int32_t channels[5];     /* CHANNELS    = [-, 32, 64, 128, 256] for BN2C (index 0 unused) */
  int32_t tr_channels[5];  /* TR_CHANNELS = [-, 64, 64, 64, 128]  for BN2C                   */
  float bn_eps;            /* 1e-5 */
  int32_t expanded;        /* EYOC_VERSION >= 111.  1 = ResUNetExpanded (model/resunet.py:254-484): every stage runs
                              block<i> -> norm<i>_2 -> block<i>_2; the layer list then also names "norm<i>_2" (a batch norm that
                              stands alone: one elementwise layer of the plan) and "block<i>_2.conv1" ... for i in 1..4, 4_tr..2_tr */
} eyoc_model_desc;

typedef struct {
  const char* name;        /* "conv1", "block2.conv1", "final", "norm1", "block2.norm2", ... */
  const float* kernel;     /* conv: [K,cin,cout] (K==1 may be [cin,cout]); NULL for norms    */
  int32_t K, cin, cout;
  const float* bias;       /* conv bias [cout] or NULL (only "final")                        */
  const float* bn_weight;  /* norm entries: gamma, beta, running_mean, running_var [c]       */
  const float* bn_bias;
  const float* bn_mean;
  const float* bn_var;
} eyoc_layer_params;

size_t eyoc_model_blob_floats(const eyoc_model_desc* desc);
/* Host-only packing (touches no device): folds the batch norms and writes the blob eyoc_model_create would upload into
 * blob_host (>= eyoc_model_blob_floats() floats).  Lets the broadcasting rank build - and a CPU test verify - the exact
 * bytes that travel over RCCL; eyoc_model_create(layers != NULL) = this + one hipMemcpy. */
int eyoc_model_pack_host(const eyoc_model_desc* desc, const eyoc_layer_params* layers, int n_layers,
                         float* blob_host, size_t blob_floats);
int eyoc_model_create(eyoc_ctx* ctx, const eyoc_model_desc* desc, const eyoc_layer_params* layers,
                      int n_layers, float* blob_dev, size_t blob_floats, eyoc_model** out);
int eyoc_model_destroy(eyoc_model* model);
/* The ResUNetIN2 family (model/resunet.py:229-251: batch norm behind the stage convolutions, MinkowskiInstanceNorm inside every
 * residual block, model/residual_block.py:60-61) as a packed plan; additive to EYOC_VERSION 111, the descriptor is unchanged.  The
 * three calls are their siblings above plus `block_norm`: 0 = batch norm inside the blocks (exactly the sibling), 1 = instance norm.
 * With 1 every "block<i>.norm1" / ".norm2" entry of `layers` carries bn_weight / bn_bias (weight, bias [c]) and NULL bn_mean / bn_var
 * (anything else is refused, naming the layer), and the plan holds two layers per block convolution: the convolution with nothing
 * folded in (packed with scale 1, shift 0, in both the fp32 and the split16 packing) and the instance norm behind it, which keeps its
 * weight and its bias in the blob (pad64(c) floats each) and carries the block's ReLU / residual.  eps = 1e-8 (model/common.py:7-8).
 * The stage convolutions keep their folded batch norm.  eyoc_model_forward then runs eyoc_in_forward's arithmetic per norm on the
 * plan's own rows (fp32 or split16), over instance plans it builds once per maps object without a read-back; eyoc_model_forward_rows
 * computes the full output and takes its rows (an instance norm needs every row).  expanded = 1 is refused. */
size_t eyoc_model_blob_floats_in(const eyoc_model_desc* desc, int block_norm);
int eyoc_model_pack_host_in(const eyoc_model_desc* desc, const eyoc_layer_params* layers, int n_layers,
                            float* blob_host, size_t blob_floats, int block_norm);
int eyoc_model_create_in(eyoc_ctx* ctx, const eyoc_model_desc* desc, const eyoc_layer_params* layers,
                         int n_layers, float* blob_dev, size_t blob_floats, int block_norm, eyoc_model** out);
/* Re-pack on the device (additive to EYOC_VERSION 111): folds and packs `layers` - the same struct and the same name matching as
 * eyoc_model_create, but EVERY pointer is a device pointer to contiguous fp32 on the model's device - into the model's existing
 * blob, in place, on `stream`.  The blob afterwards is byte for byte what eyoc_model_pack_host writes for the same parameters
 * (padding floats zero, the scale words included).  The handle keeps its address, blob, range-guard words, timing and progress
 * events and its math / probe / timing settings.  Shape and name errors are found on the host before anything is enqueued (the
 * messages of eyoc_model_create; the blob is then untouched).  The call only enqueues four kernels whose per-layer descriptors travel
 * as kernel arguments: no host synchronisation, no copy, no allocation, no read-back.  workspace_dev: 256-byte aligned,
 * eyoc_model_repack_workspace_bytes() bytes, free again once the kernels have run.  ORDERING IS THE CALLER'S JOB: a forward of this
 * model on another stream must neither be in flight while the blob is rewritten nor start before the re-pack has finished; on
 * `stream` itself the usual stream order holds. */
size_t eyoc_model_repack_workspace_bytes(const eyoc_model* model);
int eyoc_model_repack_device(eyoc_ctx* ctx, eyoc_model* model, const eyoc_layer_params* layers, int n_layers,
                             void* workspace_dev, size_t workspace_bytes, void* stream);
/* split16 forwards run the network's 1x1 tail (conv1_tr -> ReLU -> final + bias -> row normalisation, model/resunet.py:183-191)
 * as ONE kernel whose 64-channel intermediate never leaves the registers (spconv_tail.hip; BN2C's 96 -> 64 -> 32 widths): mode 1;
 * 2 (default since round 6) = in the epilogue of the last staged stride-1 layer (block2_tr.conv2 of a batch: its 64 output channels
 * go straight into the tail's first product and never reach memory; bit-identical to mode 1), falling back to mode 1 where that
 * layer does not run the 256-row staged kernel; 0 = two launches; other values only query.  Returns the previous state; per ctx. */
int eyoc_model_fuse_tail(eyoc_ctx* ctx, int on);
size_t eyoc_model_workspace_bytes(const eyoc_model* model, const eyoc_maps* maps);
/* feats_dev f32 [N1, in_channels] -> out_dev f32 [N1, out_channels], rows in input order */
int eyoc_model_forward(eyoc_ctx* ctx, const eyoc_model* model, const eyoc_maps* maps,
                       const float* feats_dev, float* out_dev, void* workspace_dev,
                       size_t workspace_bytes, void* stream);
/* The forward for a caller that reads a LIST of output rows (additive to EYOC_VERSION 111).  The reference draws its 5000 matching
 * rows per cloud by index only, after the forward (scripts/test_kitti.py:141-160: the two forwards, then random_sample) - the sample
 * never depends on the features, so a caller knows it before the forward starts.  rows_dev: int64 [n_rows] row numbers in the caller's
 * order, each in [0, N1) (a number outside is clamped into the range; duplicates are allowed and computed twice); out_dev f32
 * [n_rows, out_channels]: row i is, BIT FOR BIT, row rows_dev[i] of what eyoc_model_forward writes for the same inputs - range guard
 * included: a split16 overflow upstream or in a listed row raises the guard's words and gives NaN rows (an overflow confined to rows
 * of the last 3^3 layer that nobody listed is not seen: those values are not computed).
 * Every layer up to the last 3^3 one runs as in eyoc_model_forward.  Where that forward would run the last stride-1 layer on tile
 * records and the 1x1 tail behind it (split16 arithmetic, Z-ordered maps, a 64-channel layer in front of conv1_tr -> final), only the
 * listed rows of that layer and of the tail are computed; in every other case the full forward runs into the workspace and its rows
 * are copied out.  eyoc_model_sampled_tail(ctx, 0) forces the second form (default 1; other values only query; returns the previous
 * state; per ctx).  n_rows == 0 launches nothing.  Timing: the three layers' time is booked on the first, as the fused tail's is;
 * eyoc_model_layer_work reports, after such a forward, for those three layers what it multiplied (below). */
size_t eyoc_model_workspace_bytes_rows(const eyoc_model* model, const eyoc_maps* maps, int n_rows);
int eyoc_model_forward_rows(eyoc_ctx* ctx, const eyoc_model* model, const eyoc_maps* maps, const float* feats_dev,
                            const int64_t* rows_dev, int n_rows, float* out_dev, void* workspace_dev, size_t workspace_bytes,
                            void* stream);
int eyoc_model_sampled_tail(eyoc_ctx* ctx, int on);
/* The launch schedule of ResUNet2.forward (model/resunet.py:143-193) as data: what eyoc_model_forward (rows_dev == NULL) or
 * eyoc_model_forward_rows (rows_dev and n_rows >= 1) WOULD launch for this model, these maps, this workspace and the ctx's switches
 * now.  Same workspace arguments and checks as those two; nothing is launched, no device memory is touched, model and maps stay as
 * they are.  A step is one launch (with what it needs ready in front of it) and covers 1, 2 or 3 consecutive layers; per layer
 * (arrays of eyoc_model_num_layers() entries): step_of_layer the index of its step, kind_of_layer that step's kind - 0 instance norm,
 * 1 stand-alone affine norm, 2 first convolution, 3 sparse convolution, 4 the 1x1 tail as one kernel (2 layers), 5 the last staged
 * layer with the tail in its epilogue (3 layers), 6 that layer for the listed rows + the tail on the compact rows (3 layers) -,
 * path_of_layer the tile-record kernel of a step of kind 3, 5 or 6 (1 staged stride-1, 2 class-major transposed, 3 Morton transposed,
 * 4 strided 128-row tiles, 5 stride-1 128-row tiles, 0 none: a gathering kernel), -1 for the other kinds.  Returns the number of
 * steps - one more than the last layer's step index when a row gather (kind 7, no layer) ends the schedule - or a negative status. */
int eyoc_model_forward_steps(eyoc_ctx* ctx, const eyoc_model* model, const eyoc_maps* maps, const int64_t* rows_dev, int n_rows,
                             void* workspace_dev, size_t workspace_bytes, int32_t* step_of_layer, int32_t* kind_of_layer,
                             int32_t* path_of_layer);
/* per-layer algorithmic work of the last forward geometry (SURVEY.md 8d formulas); arrays of
 * eyoc_model_num_layers() entries, any may be NULL */
/* When the handle's most recent forward was an eyoc_model_forward_rows that computed listed rows only, the entries of the last 3^3
 * layer and of the two 1x1 layers describe THAT forward: the (row, offset) pairs its kernel multiplied (counted on the device) and
 * n_rows rows; flop and bytes by the same formulas.  After any other forward: the geometry's full work. */
int eyoc_model_num_layers(const eyoc_model* model);
int eyoc_model_layer_work(eyoc_ctx* ctx, const eyoc_model* model, const eyoc_maps* maps, void* stream,
                          const char** names, int64_t* pairs, double* flops, double* gather_bytes,
                          double* compulsory_bytes);
/* Arithmetic of the sparse convolutions inside eyoc_model_forward: -1 automatic (default: split16 once the batch
 * has >= 8192 level-0 rows - else fp32), 0 fp32 MFMA, 1 split16 (three fp16 MFMAs per product on
 * hi/lo-split operands: 22-bit significands, fp32 accumulation; activations must stay below 6e4 - guarded, see
 * eyoc_model_range_check).  Returns the
 * previous mode + 2, or a negative status.  eyoc_model_last_math: what the last forward used (0 / 1). */
int eyoc_model_set_math(eyoc_model* model, int mode);
int eyoc_model_last_math(const eyoc_model* model);
/* Range guard of the split16 arithmetic.  Every kernel that stores split16 activations tracks the largest magnitude it
 * writes; once one reaches 6e4 (before any fp16 half became inf) the forward's own device flag is raised - its fp32 output
 * is all-NaN, never plausible-looking garbage (an overflow inside the fused 1x1 tail, whose intermediate never leaves the
 * registers, NaNs the rows it happened in) - together with a sticky flag.  The per-forward flag is cleared, in stream order,
 * when the next split16 forward starts, so forwards enqueued behind an overflowing one are judged on their own.
 * eyoc_model_range_check synchronises `stream`, returns EYOC_ERR_RANGE if ANY forward since the last check overflowed (and
 * clears the sticky flag) else EYOC_OK: a caller that pipelines k forwards and then checks must, on EYOC_ERR_RANGE, treat all
 * k outputs as suspect (the ones that overflowed are the ones holding NaN rows); *max_abs (may be NULL) = largest |activation| stored since eyoc_model_set_probe(model, 1)
 * switched the debug probe on (-1 when the probe is off).  fp32 forwards never raise it. */
int eyoc_model_range_check(eyoc_model* model, void* stream, float* max_abs);
/* The guard's four device words {this forward's overflow flag, max |activation| bits (probe), probe switch, sticky flag} copied
 * to `words_host` (16 bytes of pinned host memory) in stream order, WITHOUT synchronising: enqueued right behind a forward it
 * captures that forward's own verdict (word 0), which a caller that pipelines steps reads once its own event behind the copy has
 * fired - eyoc_model_range_check would queue its read behind everything enqueued since.  Nothing is cleared. */
int eyoc_model_range_snapshot(eyoc_model* model, uint32_t* words_host, void* stream);
/* Every forward records `hip_event` (a hipEvent_t the caller owns; NULL switches it off) on its stream in front of layer `layer`
 * (0-based in launch order, negative counts from the end: -1 = in front of the last layer; == number of layers: behind it).  A
 * caller that pipelines batches lets a side stream wait for it - bench.py starts the next batch's map build there, beside the
 * last layers of the forward instead of behind it. */
int eyoc_model_set_progress_event(eyoc_model* model, int layer, void* hip_event);
int eyoc_model_set_probe(eyoc_model* model, int on);
/* when `on`, eyoc_model_forward brackets every layer with hipEvents on `stream` and
 * eyoc_model_layer_ms returns the per-layer durations of the last forward (synchronises) */
int eyoc_model_set_timing(eyoc_model* model, int on);
int eyoc_model_layer_ms(eyoc_model* model, float* ms /*[num_layers]*/);
/* Two event sets: forwards record into, and eyoc_model_layer_ms reads from, the selected one (0 or 1) - so that a caller
 * can enqueue step k + 1 before it reads step k's durations, and the GPU never waits for the host between steps. */
int eyoc_model_timing_slot(eyoc_model* model, int slot);

/* MFMA pre-filter of eyoc_knn1's plain index query (dist_type 0 or 2, idx only, C = 32): an fp32-MFMA score decides every row
 * whose runner-up is out of rounding reach, the exact kernel recomputes the rest - the indices are identical either way.
 * mode 0: never, 1 (default): when the query fills the chip (>= 512 waves of 64 rows), 2: always; < 0 only queries.
 * Returns the previous mode.  Per ctx; for tests and profiling. */
int eyoc_knn_prefilter(eyoc_ctx* ctx, int mode);
/* The pre-filter's packing of the targets alone, into caller-owned device memory (tests): for the `nseg` segments seg_b[s] ..
 * seg_b[s + 1] of B [*, 32], segment after segment, per tile of 16 targets 3 x 64 float4 - the fp16 hi halves of the power-of-two
 * scaled rows in MFMA operand order, the lo halves, and (|b|^2, 1 / scale, 0, 0) per lane (padding targets: +inf, 0; zero_norm != 0:
 * norm 0) - `packed_floats` >= sum over s of ceil(nb_s / 16) * 768; bmax_dev[s] = bits of the segment's largest |b|^2 (0 if empty). */
int eyoc_knn_pack_targets(eyoc_ctx* ctx, const float* B_dev, const int32_t* seg_b, int nseg, int zero_norm, float* packed_dev,
                          size_t packed_floats, int32_t* bmax_dev, void* stream);
/* ------------------------------------------------------------------------------------------------
 * feature matching
 *   replaces: lib.eval.find_nn_gpu + lib.metrics.pdist (lib/eval.py:18-48, lib/metrics.py:22-29)
 *             and the nearest-neighbour step of Matcher.match_pair (scripts/SC2_PCR/SC2_PCR.py:296-298).
 *   For every row of A the index of the nearest row of B.  dist_type 0: squared L2 (difference
 *   form, fp32, channels left to right, no FMA - bit-exact with oracle/matching.py); 1: L2 =
 *   sqrt(d2 + 1e-7); 2: the GEMM form of Matcher.match_pair, sqrt(2 - 2 S + 1e-6) with S = <A_i, B_j> accumulated by
 *   fp32 FMAs over the channels in order and every later step rounded in fp32 - NOT an L2 distance unless the rows
 *   have unit norm; a NaN distance (S > 1 + 5e-7) is below every number and the first NaN wins, as in torch.argmin.
 *   Ties go to the lowest index.  Segmented form: nseg independent problems,
 *   rows [seg_a[s], seg_a[s+1]) of A against rows [seg_b[s], seg_b[s+1]) of B; indices are local to
 *   the B segment.  seg arrays are HOST arrays; nseg <= 128.  c in {4, 16, 32, 64, 128}.
 * --------------------------------------------------------------------------------------------- */
int eyoc_knn1(eyoc_ctx* ctx, const float* A_dev, const float* B_dev, int c, const int32_t* seg_a,
              const int32_t* seg_b, int nseg, int dist_type, int64_t* idx_dev, float* dist_dev,
              void* stream);

/* Mutual nearest neighbours (additive to EYOC_VERSION 111; no counterpart in the reference, whose use_mutual is stored and never read,
 * scripts/SC2_PCR/SC2_PCR.py:23 - this is the reciprocity check Open3D's registration_ransac_based_on_feature_matching applies with
 * mutual_filter = true).  Same argument rules, arithmetic and tie rule as eyoc_knn1 (host seg arrays, nseg <= 128, c in
 * {4, 16, 32, 64, 128}, dist_type 0 / 1 / 2, scratch on the ctx); seg_a[0] = seg_b[0] = 0.
 *   idx_ab int64 [na]: byte for byte what eyoc_knn1(A, B) writes (local to the B segment);
 *   idx_ba int64 [nb] (NULL: not wanted): byte for byte what eyoc_knn1(B, A) with the segments swapped writes (local to the A segment);
 *   mutual uint8 [na]: bit 1 = row i has a neighbour at all (some comparison of its row succeeded: the B segment is not empty and, for
 *     dist_type 0 / 1, some distance is a number below +inf), bit 0 = it is mutual: j = idx_ab[i] has a neighbour too and idx_ba[j] = i.
 *     So 0 = no neighbour (its index reads 0 like a true neighbour 0, and it is never mutual), 2 = a neighbour that prefers another
 *     row, 3 = mutual; eyoc_mutual_compact's fallback needs bit 1.
 * All three distance forms are symmetric bit for bit, so the two routes give identical bytes: eyoc_knn_mutual_select mode 0 runs
 * eyoc_knn1's machinery in both directions (its MFMA pre-filter included where eyoc_knn1 would use it), 1 one fused sweep that takes the
 * row and the column minima from every distance it computes (knn.hip knn1_mutual_kernel), -1 (default) picks as measured - the fused sweep for c = 32
 * queries below 512 waves of 64 rows in both directions (a single pair), two one-way queries for everything else
 * (EXPERIMENTS.md "Mutual nearest-neighbour filter").  Any other mode only queries; returns the previous mode + 2 (1, 2 or 3), -1 without a
 * ctx.  Per ctx; for tests and profiling. */
int eyoc_knn1_mutual(eyoc_ctx* ctx, const float* A_dev, const float* B_dev, int c, const int32_t* seg_a, const int32_t* seg_b,
                     int nseg, int dist_type, int64_t* idx_ab_dev, int64_t* idx_ba_dev, uint8_t* mutual_dev, void* stream);
int eyoc_knn_mutual_select(eyoc_ctx* ctx, int mode);
/* Stable per-segment compaction of eyoc_knn1_mutual's result: the mutual rows of every segment in their order, back to back -
 * rows int64 (the row INSIDE its A segment), corr int64 (its idx_ab, local to the B segment), both [na] of which the first
 * seg_out[nseg] entries are written; seg_out int32 [nseg + 1] on the DEVICE: segment s owns [seg_out[s], seg_out[s + 1]).  A segment with
 * fewer than min_keep mutual rows keeps all of its rows that have a neighbour instead (Open3D: fewer than ransac_n correspondences
 * survive the mutual filter -> the original set); min_keep 0: no fallback.  A count pass, a flag scan and a fill pass: no atomics, no
 * read-back, the same bytes on every run.  seg_a: host array, seg_a[0] = 0, nseg <= 128; scratch on the ctx. */
int eyoc_mutual_compact(eyoc_ctx* ctx, const int64_t* idx_ab_dev, const uint8_t* mutual_dev, const int32_t* seg_a, int nseg,
                        int min_keep, int64_t* rows_dev, int64_t* corr_dev, int32_t* seg_out_dev, void* stream);

/* Row gather: out[i,:] = F[sel[i], 0:c] (F rows are `ld` floats apart) - the `F[inds]` of
 * scripts/test_kitti.py:30-35,159-160 and of Matcher.match_pair (scripts/SC2_PCR/SC2_PCR.py:291-294).
 * With G_dev != NULL (f32 [n,c]) the gathered row is blended and re-normalised,
 * out[i,:] = (F[sel[i],:] + beta * G[i,:]) / |.|_2 : the synthetic benchmark's descriptor mode (random-init
 * weights carry no geometric signal; G plants it at a stated inlier ratio).  c: power of two in [4,256].
 * sel_dev == NULL: sel[i] = i (rows that are already the sample - eyoc_model_forward_rows' output -, blended in place of a gather). */
int eyoc_gather_rows(eyoc_ctx* ctx, const float* F_dev, int ld, int c, const int64_t* sel_dev, int n,
                     const float* G_dev, float beta, float* out_dev, void* stream);

/* Arg-max of the inner product (replaces ``corr = F0.mm(F1.t()); weight, inds = corr.max(dim=1)`` of
 * util/transform_estimation.py:131-133 without materialising the [N0,N1] matrix - 3.6 GB at 30k voxels):
 * idx int64 [n] (local to the B segment, ties to the lowest index), weight f32 [n] = max_j <A_i, B_j> accumulated
 * with fp32 FMAs over the channels in order. */
int eyoc_dotmax(eyoc_ctx* ctx, const float* A_dev, const float* B_dev, int c, const int32_t* seg_a,
                const int32_t* seg_b, int nseg, int64_t* idx_dev, float* weight_dev, void* stream);

/* Two nearest neighbours for Lowe's ratio test (replaces pytorch3d.ops.knn_points(..., K=2) at
 * lib/trainer.py:1060-1061, squared L2 like knn_points): idx int64 [n] (nearest, local to the B segment), d1 / d2
 * f32 [n] smallest and second smallest squared distance (+inf when the segment has < 2 rows).  Same arithmetic
 * and tie rule as eyoc_knn1; c may also be 4 (xyz padded with a zero column) for the 3-D nearest neighbour
 * of lib/trainer.py:1195. */
int eyoc_knn2(eyoc_ctx* ctx, const float* A_dev, const float* B_dev, int c, const int32_t* seg_a,
              const int32_t* seg_b, int nseg, int64_t* idx_dev, float* d1_dev, float* d2_dev, void* stream);

/* ------------------------------------------------------------------------------------------------
 * label generation
 *   replaces: calculate_ratio_test + get_topk_matches (lib/trainer.py:993-1017, 1066-1084): weight of every
 *   query from its two nearest squared feature distances (cosine = 1 - d/2; x = clamp(1 - cosine, 1e-9);
 *   weight = 1 - x0/x1, fp32 in that order) and the k queries of largest weight, largest first (torch.topk
 *   order; ties in query order).  idx_out int64 [k], w_out f32 [k] or NULL; k <= n.
 *   eyoc_pair_filter: order-preserving filter of index pairs (idx0[i], idx1[i]):
 *     mode 0 (spherical filter, lib/trainer.py:1107-1110): keep iff |P0[idx0]| > radius and |P1[idx1]| > radius;
 *     mode 1 (pose consistency, lib/trainer.py:1203-1206): keep iff |R P0[idx0] + t - P1[idx1]| < radius,
 *            T_dev f32 [16] row-major.  pairs_out int64 [m,2] (first *n_out rows valid), n_out int32 on the device.
 * --------------------------------------------------------------------------------------------- */
int eyoc_lowe_topk(eyoc_ctx* ctx, const float* d1_dev, const float* d2_dev, int n, int k, int64_t* idx_out_dev,
                   float* w_out_dev, void* stream);
int eyoc_pair_filter(eyoc_ctx* ctx, int mode, const float* P0_dev, const float* P1_dev, const int64_t* idx0_dev,
                     const int64_t* idx1_dev, int m, const float* T_dev, float radius, int64_t* pairs_out_dev,
                     int32_t* n_out_dev, void* stream);

/* The "Similarity" spatial filter of match_and_filter_corr (lib/trainer.py:1118-1149): with d0 = |P0[idx0]|, d1 = |P1[idx1]|
 * a pair is kept iff table[min(int(|d0 - d1| / grid1), xlim - 1)][min(int(min(d0, d1) / grid0), ylim - 1)] > thresh.
 * table_dev: fp64 [xlim, ylim] row-major (one frame-distance slice of config/dist_sim_plot/<dataset>_distSimPlot.npz;
 * the reference uses grid0 = 5 and grid1 in {1, 1.5, 2, 2.5} by frame index).  Output like eyoc_pair_filter. */
int eyoc_pair_filter_similarity(eyoc_ctx* ctx, const float* P0_dev, const float* P1_dev, const int64_t* idx0_dev,
                                const int64_t* idx1_dev, int m, const double* table_dev, int xlim, int ylim, float grid0,
                                float grid1, double thresh, int64_t* pairs_out_dev, int32_t* n_out_dev, void* stream);

/* The label stages for every pair of a batch at once.  Added after 111 without a bump, additive only.
 * eyoc_lowe_topk_segmented: d1 / d2 hold the queries of all segments back to back, segment s = rows [seg[s], seg[s+1]) (HOST array of
 * nseg + 1 ints, seg[0] = 0, nseg <= 2^20), one k <= every segment's length.  mode 0: the Lowe weights of eyoc_lowe_topk; mode 1: weight =
 * d1 (feature_filter "None" of lib/trainer.py:1072-1073: the order of a stable descending fp64 argsort, NaN last; d2 may be NULL).
 * idx_out int64 [nseg * k] LOCAL to the segment, w_out f32 [nseg * k] or NULL.  One stable sort whose key holds the segment above the
 * descending weight: segment s is byte for byte eyoc_lowe_topk on it alone (ties in query order), whatever its neighbours hold.
 * eyoc_pair_filter_batched: modes 0 / 1 / 2 (= eyoc_pair_filter_similarity) of eyoc_pair_filter for nseg <= 1024 pairs, one workgroup per
 * pair, 64 pairs per launch.  Pair b owns rows [seg_p0[b], seg_p0[b+1]) of P0, [seg_p1[b], seg_p1[b+1]) of P1 and entries [seg_m[b],
 * seg_m[b+1]) of idx0 / idx1 (all HOST arrays of nseg + 1 ints starting at 0; the indices are LOCAL to the pair's clouds).  Mode 1 reads
 * pair b's pose from T_dev f32 [nseg][16] on the device; a non-finite pose keeps nothing.  Mode 2: tables_dev holds fp64 table slices,
 * slices_host[b] says which one pair b reads (offset in doubles, xlim x ylim row-major, its grid1; grid0 and thresh are the call's).
 * An entry whose index lies outside its cloud (eyoc_posed_nn_grid's -1) is dropped.  Order-preserving: the survivors of pair b are
 * rows [seg_m[b], seg_m[b] + count[b]) of pairs_out int64 [seg_m[nseg], 2], count_dev int32 [nseg].  Nothing is read back. */
typedef struct {
  int64_t table_offset;
  int32_t xlim, ylim;
  float grid1;
  int32_t reserved;
} eyoc_sim_slice;            /* 24 bytes */
int eyoc_lowe_topk_segmented(eyoc_ctx* ctx, const float* d1_dev, const float* d2_dev, const int32_t* seg_host, int nseg, int k, int mode,
                             int64_t* idx_out_dev, float* w_out_dev, void* stream);
int eyoc_pair_filter_batched(eyoc_ctx* ctx, int mode, const float* P0_dev, const float* P1_dev, const int64_t* idx0_dev,
                             const int64_t* idx1_dev, const int32_t* seg_p0_host, const int32_t* seg_p1_host, const int32_t* seg_m_host,
                             int nseg, const float* T_dev, float radius, const double* tables_dev, const eyoc_sim_slice* slices_host,
                             float grid0, double thresh, int64_t* pairs_out_dev, int32_t* count_dev, void* stream);

/* replaces: lib.metrics.pdist (lib/metrics.py:22-29): dense out f32 [n,m]; same arithmetic as eyoc_knn1 */
int eyoc_pdist(eyoc_ctx* ctx, const float* A_dev, int n, const float* B_dev, int m, int c, int dist_type,
               float* out_dev, void* stream);

/* ------------------------------------------------------------------------------------------------
 * pose solvers
 * --------------------------------------------------------------------------------------------- */
/* replaces: rigid_transform_3d (scripts/SC2_PCR/common.py:7-45).  A,B f32 [bs,n,3], w f32 [bs,n] or
 * NULL -> T f32 [bs,4,4] with B ~ R A + t.  Weighted centroids use the reference's 1e-6 epsilon. */
int eyoc_kabsch_batched(eyoc_ctx* ctx, const float* A_dev, const float* B_dev, const float* w_dev,
                        int bs, int n, float* T_dev, void* stream);
/* replaces: est_quad_linear_robust (util/transform_estimation.py:89-116).  p0,p1 f32 [n,3],
 * w f32 [n] or NULL -> T f32 [4,4]. */
int eyoc_irls_quad(eyoc_ctx* ctx, const float* p0_dev, const float* p1_dev, const float* w_dev, int n,
                   int iters, float* T_dev, void* stream);

/* The validation step of the reference (lib/trainer.py:321-403, `_valid_epoch`) behind the neighbour search, for every pair of a batch:
 * the IRLS pose and the loop's metrics.  Added after 111 without a bump, additive only.  Two launches per 64 pairs in all, no host
 * synchronisation, nothing read back.
 *
 * eyoc_irls_quad_batched: eyoc_irls_quad for nseg <= 1024 pairs, one workgroup per pair, 64 pairs per launch.  Pair b owns rows
 * [seg0[b], seg0[b+1]) of p0 f32 [*,3] and of w f32 [*] (or NULL) and rows [seg1[b], seg1[b+1]) of p1 f32 [*,3] (HOST arrays of nseg + 1
 * ints starting at 0, the convention of eyoc_pair_filter_batched).  idx1 int64 [seg0[nseg]] is LOCAL to the pair's p1 segment - what
 * eyoc_knn1 writes -: row i of the pair is the correspondence (p0[i], p1[idx1[i]]), the xyz1[inds1[nn_inds]] of find_corr
 * (lib/trainer.py:405-419), gathered inside the sweep and never materialised.  idx1 == NULL: row i pairs with row i, and the two
 * segment arrays must agree.  T f32 [nseg][16].  Pair b's 64 bytes are exactly what eyoc_irls_quad writes for that pair's gathered
 * arrays alone (the two kernels are one body), whatever the other segments hold and wherever the pair stands in the batch.  An empty
 * segment gets 16 NaNs.  The indices of a pair are checked before any of its points is read: one outside its segment never becomes an
 * address, the pair gets 16 NaNs, the other pairs are untouched.  nseg outside [1, 1024], decreasing offsets, idx1 == NULL with
 * differing segments: EYOC_ERR_INVALID. */
int eyoc_irls_quad_batched(eyoc_ctx* ctx, const float* p0_dev, const float* p1_dev, const int64_t* idx1_dev, const float* w_dev,
                           const int32_t* seg0_host, const int32_t* seg1_host, int nseg, int iters, float* T_dev, void* stream);

/* eyoc_valid_metrics_batched: one record per pair from the correspondence arrays above, the pair's FULL source cloud - rows [segx[b],
 * segx[b+1]) of x0 f32 [*,3] -, T_est f32 [nseg][16] on the device (read where eyoc_irls_quad_batched wrote it) and T_gt f32 [nseg][16].
 * fp64 arithmetic on the fp32 inputs without contraction; sums reduced lane -> wave -> workgroup in a fixed order, so a pair's record is
 * byte-identical alone, in a batch and from run to run.
 *   loss      corr_dist (lib/metrics.py:13-19, weight None): the mean over the full cloud of min(|T_est x - T_gt x|, max_dist)
 *   hits      correspondences with sqrt(|R_gt p0 + t_gt - p1[idx1]|^2 + 1e-6) < hit_thresh (lib/trainer.py:421-424); hit_ratio = hits / n_corr
 *   rte       |t_est - t_gt|
 *   cos_rre   (trace(R_est^T R_gt) - 1) / 2;  rre = acos(cos_rre), NaN when the cosine leaves [-1, 1]: lib/trainer.py:367-370 does not
 *             clamp and skips the NaN (scripts/test_kitti.py's clamp is NOT applied here)
 * status: EMPTY - no correspondences: hit_ratio and loss are NaN.  BAD_INDEX - an index outside the pair's p1 segment (clamped into it
 * before the load): hit_ratio is NaN, hits 0.  POSE_NONFINITE - T_est holds a non-finite entry: loss, rte and rre are NaN, hits are still
 * counted.  An empty x0 segment gives loss NaN and nothing else. */
#define EYOC_VALID_EMPTY 1u
#define EYOC_VALID_BAD_INDEX 2u
#define EYOC_VALID_POSE_NONFINITE 4u
typedef struct {
  double loss, hit_ratio, rte, rre, cos_rre;
  int32_t hits, n_corr, n_points;
  uint32_t status;
  double reserved;
} eyoc_valid_record;         /* 64 bytes */
int eyoc_valid_metrics_batched(eyoc_ctx* ctx, const float* p0_dev, const float* p1_dev, const int64_t* idx1_dev,
                               const int32_t* seg0_host, const int32_t* seg1_host, const float* x0_dev, const int32_t* segx_host, int nseg,
                               const float* T_est_dev, const float* T_gt_dev, double hit_thresh, double max_dist,
                               eyoc_valid_record* records_dev, void* stream);

/* ------------------------------------------------------------------------------------------------
 * training-mode support (lib/trainer.py:1655-1676 back-propagates through the network in train mode)
 * --------------------------------------------------------------------------------------------- */
/* replaces: MinkowskiBatchNorm in training mode (model/common.py:4-6 = nn.BatchNorm1d over the rows): per-channel batch mean
 * and BIASED variance of x f32 [n, c] (rows ld_x floats apart) -> mean_var_dev f32 [2 c] = {mean, variance};
 * y = (x - mean) / sqrt(var + eps) * gamma + beta, then ReLU if `relu`.  c must divide 256 (32 ... 256 in this model family).
 * The statistics are summed in fp64 in a fixed order (bit-reproducible).  The running-statistics update (momentum, unbiased
 * variance) is host glue on the returned 2 c floats.  Workspace: eyoc_bn_workspace_bytes(n, c), caller-owned, 256-byte aligned (a
 * misaligned one is EYOC_ERR_INVALID, a smaller one EYOC_ERR_WORKSPACE, forward and backward alike, before any launch). */
size_t eyoc_bn_workspace_bytes(int n, int c);
int eyoc_bn_train_forward(eyoc_ctx* ctx, const float* x_dev, int n, int c, int ld_x, const float* gamma_dev, const float* beta_dev,
                          float eps, int relu, float* y_dev, int ld_y, float* mean_var_dev, void* workspace_dev, size_t workspace_bytes,
                          void* stream);
/* ... and the running statistics moved in the same call, like nn.BatchNorm1d in training mode: running_mean = (1 - momentum)
 * running_mean + momentum * mean, running_var likewise with the UNBIASED batch variance (n / (n - 1)).  (num_batches_tracked and a
 * momentum of None - the cumulative average - stay with the caller.) */
int eyoc_bn_train_forward_running(eyoc_ctx* ctx, const float* x_dev, int n, int c, int ld_x, const float* gamma_dev, const float* beta_dev,
                                  float eps, int relu, float* y_dev, int ld_y, float* mean_var_dev, float* running_mean_dev,
                                  float* running_var_dev, float momentum, void* workspace_dev, size_t workspace_bytes, void* stream);
/* Its backward: dy' = dy where y > 0 (y_dev = the forward's output when a ReLU was fused, else NULL);
 * dbeta = sum dy', dgamma = sum dy' xhat, dx = gamma / sigma (dy' - dbeta / n - xhat dgamma / n). */
int eyoc_bn_train_backward(eyoc_ctx* ctx, const float* x_dev, int ld_x, const float* y_dev, int ld_y, const float* dy_dev, int ld_dy, int n,
                           int c, const float* gamma_dev, const float* mean_var_dev, float eps, float* dx_dev, int ld_dx,
                           float* dgamma_dev, float* dbeta_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
/* replaces: MinkowskiInstanceNorm (model/common.py:7-8; the norm inside every residual block of the ResUNetIN2 family,
 * model/residual_block.py:60-61).  Additive to EYOC_VERSION 111.  For x f32 [n, c] whose row r belongs to instance b(r) = column 0 of
 * the level's coordinates, n_b rows in instance b:  mean[b] = sum_{r in b} x / n_b, var[b] = sum_{r in b} (x - mean[b])^2 / n_b (biased),
 * y = (x - mean[b]) / sqrt(var[b] + eps) * weight + bias.  No running statistics: eval mode equals training mode.  An instance of one
 * row gives y = bias; an instance id without rows touches nothing.
 *
 * The PLAN of a level groups its rows by instance: eyoc_in_plan_build writes, into caller-owned device memory of
 * eyoc_in_plan_bytes(n, n_inst) bytes, int32 words: a header {identity, n, n_inst, 0}, seg [n_inst + 1] (prefix sums of the row counts)
 * and perm [n] (the rows grouped by instance, ascending row number inside an instance: a stable counting sort), plus internal arrays.
 * eyoc_in_plan_layout gives the byte offsets {header, seg, perm, instance of every row}.  identity = 1: the ids never step down (every
 * collated batch in the caller's order), perm is 0, 1, 2 ... and is not read.  n_inst <= 1024.  The build synchronises the stream once
 * (it reads the header back): an id outside [0, n_inst) is refused with EYOC_ERR_INVALID.
 *
 * eyoc_in_forward: stats f32 [n_inst][2 c] = {mean, biased variance} per instance; with `residual` y = [relu](norm(x) + residual), the
 * tail of a residual block in one pass.  eyoc_in_backward: g = dy where y > 0 (y = the forward's output when a ReLU was fused, else
 * NULL); dx = weight invstd[b] (g - mean_b(g) - xhat mean_b(g xhat)); dres (or NULL) = g, the residual's gradient; dweight = sum g xhat
 * and dbias = sum g over ALL rows.  c must divide 256 (as eyoc_bn_*); every leading dimension a multiple of 4 and >= c, tensors 16-byte
 * aligned; workspace eyoc_in_workspace_bytes(n, c, n_inst), caller-owned, 256-byte aligned (a misaligned one is EYOC_ERR_INVALID, a
 * smaller one EYOC_ERR_WORKSPACE, before any launch).  Three launches forward, four backward, whatever n_inst; no host synchronisation,
 * no floating-point atomics.
 *
 * Batch invariance: sums are fp64 about the instance's first row (plan order), over chunks of eyoc_in_chunk_rows() rows of the
 * instance, added in an order that depends on the instance's row count alone.  The bytes of an instance's stats, y and dx rows do not
 * depend on the other instances, on how the rows interleave, on the grid or on timing; a call on one instance alone (n_inst = 1, its
 * rows in the same relative order) gives the same bytes.  dweight / dbias add the instances in ascending id. */
int eyoc_in_chunk_rows(void);
size_t eyoc_in_plan_bytes(int n, int n_inst);
int eyoc_in_plan_layout(int n, int n_inst, int64_t* offsets_out /* [4] bytes: header, seg, perm, instance of every row */);
int eyoc_in_plan_build(eyoc_ctx* ctx, const int32_t* coords_dev /* [n,4] */, int n, int n_inst, void* plan_dev, size_t plan_bytes,
                       void* stream);
size_t eyoc_in_workspace_bytes(int n, int c, int n_inst);
int eyoc_in_forward(eyoc_ctx* ctx, const float* x_dev, int n, int c, int ld_x, const void* plan_dev, int n_inst, const float* weight_dev,
                    const float* bias_dev, float eps, int relu, const float* residual_dev /* or NULL */, int ld_res, float* y_dev, int ld_y,
                    float* stats_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
/* eyoc_in_forward on SPLIT16 rows (the packed plan's second row format: per 32 channels 32 fp16 hi halves, then 32 fp16 lo halves, the
 * same 4 bytes per channel): x, residual and y are such rows, c and every leading dimension multiples of 32.  The result is, bit for
 * bit, the SPLIT16 encoding of what eyoc_in_forward gives on the decoded rows (the kernels are the same templates); stats as there.
 * range_dev (or NULL): the four range-guard words of eyoc_model_range_snapshot - words 0 and 3 are raised when a stored |y| reaches 6e4. */
int eyoc_in_forward_split16(eyoc_ctx* ctx, const float* x_dev, int n, int c, int ld_x, const void* plan_dev, int n_inst, const float* weight_dev,
                            const float* bias_dev, float eps, int relu, const float* residual_dev /* or NULL */, int ld_res, float* y_dev, int ld_y,
                            float* stats_dev, uint32_t* range_dev /* or NULL */, void* workspace_dev, size_t workspace_bytes, void* stream);
int eyoc_in_backward(eyoc_ctx* ctx, const float* x_dev, int ld_x, const float* y_dev /* or NULL */, int ld_y, const float* dy_dev, int ld_dy,
                     int n, int c, const void* plan_dev, int n_inst, const float* weight_dev, const float* stats_dev, float eps,
                     float* dx_dev, int ld_dx, float* dres_dev /* or NULL */, int ld_dres, float* dweight_dev, float* dbias_dev,
                     void* workspace_dev, size_t workspace_bytes, void* stream);
/* The first convolution's window as a dense matrix (model/resunet.py:31-38, C_in = 1 in production, K = ks^3):
 * out f32 [n, ks^3 * cin], out[row][k * cin + c] = feats[voxel at window offset k of row][c] or 0 (offsets x fastest, like every
 * rulebook) - the convolution and its weight gradient are then plain [n, K cin] x [K cin, C_out] products.  Builds the level-0 hash
 * table on first use.  eyoc_maps_gather_window: feats and out in the CALLER's rows - maps that are Z-ordered internally
 * (eyoc_maps_row_order != NULL) are refused with EYOC_ERR_INVALID; eyoc_maps_gather_window_internal (EYOC_VERSION >= 110): feats and
 * out in the maps' INTERNAL rows (row i = the caller's row eyoc_maps_row_order()[i]). */
int eyoc_maps_gather_window(eyoc_ctx* ctx, eyoc_maps* maps, int ks, const float* feats_dev, int cin, float* out_dev, void* stream);
int eyoc_maps_gather_window_internal(eyoc_ctx* ctx, eyoc_maps* maps, int ks, const float* feats_dev, int cin, float* out_dev, void* stream);

/* replaces: o3d.pipelines.registration.registration_ransac_based_on_feature_matching(..., 4,
 * [EdgeLength(0.9), Distance(d)], RANSACConvergenceCriteria(4000000, 10000))
 * (scripts/test_kitti.py:169-177) given the feature correspondences.  Hypothesis h samples
 * correspondences with the counter hash documented in oracle/ransac.py. */
typedef struct {
  float max_distance;        /* config.voxel_size * 1.0  */
  float edge_similarity;     /* 0.9                      */
  int32_t max_iteration;     /* 4000000                  */
  uint32_t seed;
} eyoc_ransac_params;

typedef struct {
  float T[16];               /* row-major 4x4            */
  int32_t inliers;
  int32_t best_hypothesis;   /* -1 when nothing survived */
  int32_t survivors;
  float inlier_rmse;
} eyoc_ransac_result;

/* src f32 [n,3], tgt f32 [m,3], corr_tgt int64 [n] (target index for source point i);
 * result_dev points to one eyoc_ransac_result in device memory. */
int eyoc_ransac(eyoc_ctx* ctx, const float* src_dev, const float* tgt_dev, const int64_t* corr_tgt_dev,
                int n, const eyoc_ransac_params* params, eyoc_ransac_result* result_dev, void* stream);
/* The same for a batch of independent pairs in a few launches (the per-pair loop of scripts/test_kitti.py:130-225
 * collapsed; SURVEY 8f "batched registration").  Pair b owns source rows / correspondences
 * [seg_src[b], seg_src[b+1]) and target rows starting at seg_tgt[b]; corr_tgt holds target indices LOCAL to the
 * pair's target segment; pair b samples with seed params->seed + b, so results[b] is bit-identical to
 * eyoc_ransac on that pair with that seed.  seg_* are HOST arrays of n_pairs + 1 ints.
 * Up to 64 pairs go through one set of launches (a "chunk"); the scratch holds 12 bytes per hypothesis plus 96 bytes per
 * stored survivor transform (at most 2^20) for every pair of a chunk - 144 MB per pair at 4 000 000 hypotheses.  The results
 * do not depend on the chunk size.
 *
 * eyoc_ransac_batched_ws: CALLER-OWNED scratch (256-byte aligned device memory; nothing is allocated inside the call).
 * eyoc_ransac_workspace_bytes(ctx, n_pairs, total_corr = seg_src[n_pairs], max_iteration, budget) = the bytes of the largest
 * chunk (n_pairs capped at 64, then halved) that stays within `budget` bytes (0 = no limit), never less than a one-pair
 * chunk; the call derives its chunk from workspace_bytes the same way and returns EYOC_ERR_WORKSPACE if not even one pair
 * fits.
 * eyoc_ransac_batched (and eyoc_ransac): the same on the ctx's grow-only scratch, for callers without an allocator - the
 * chunk is sized so that the scratch takes at most a quarter of the device's free memory (hipMemGetInfo) and at most
 * 16 GB, and is halved again (down to one pair) if the allocation fails all the same. */
size_t eyoc_ransac_workspace_bytes(const eyoc_ctx* ctx, int n_pairs, int total_corr, int max_iteration, size_t budget_bytes);
int eyoc_ransac_batched_ws(eyoc_ctx* ctx, const float* src_dev, const float* tgt_dev, const int64_t* corr_tgt_dev,
                           const int32_t* seg_src_host, const int32_t* seg_tgt_host, int n_pairs,
                           const eyoc_ransac_params* params, eyoc_ransac_result* results_dev, void* workspace_dev,
                           size_t workspace_bytes, void* stream);
int eyoc_ransac_batched(eyoc_ctx* ctx, const float* src_dev, const float* tgt_dev, const int64_t* corr_tgt_dev,
                        const int32_t* seg_src_host, const int32_t* seg_tgt_host, int n_pairs,
                        const eyoc_ransac_params* params, eyoc_ransac_result* results_dev, void* stream);
/* Reference pruning of the scorer (k_bucket: a survivor only evaluates the correspondences that can be inliers given its
 * distance to the pair's first survivor; counts are exactly those of the full sweep): 0 off, 1 on, 2 (default since EYOC_VERSION 111)
 * on + a survivor stops counting once its count so far plus the records still ahead of it is below the largest count any survivor of
 * the pair has reached - the result (arg-max by count, RMSE, hypothesis number) is the same, only the counts of survivors that
 * cannot win stay partial; it is applied to launch chunks of >= 32 pairs (every wave polls one word per pair: on fewer words the
 * polling costs more than the skipped work).  Other values only query.  Returns the previous state.  Per ctx; for tests / profiling. */
int eyoc_ransac_select_pruning(eyoc_ctx* ctx, int on);
/* Form of the hypothesis generator: 1 (default) samples from 16-bit fixed-point records (one power-of-two step per pair, from the
 * pair's largest |coordinate|) and rejects a hypothesis only where a rigorous error band proves that the exact edge-length
 * expression rejects it; 0 evaluates the exact fp64 expression on the fp32 records.  Either way the fit kernel re-evaluates the exact
 * expression and drops what fails, so the survivors and every result record are the same bytes.  A pair with a non-finite
 * coordinate, or whose largest |coordinate| lies outside [1e-18, 1e18] (all zeros included), has no usable step: the fit kernel
 * evaluates the exact expression on every hypothesis of that pair.  Launches with more than 12000 correspondences in a pair, or an
 * edge_similarity outside (0, 1], take form 0.  Other values only query.  Returns the previous state.  Per ctx; for tests / profiling. */
int eyoc_ransac_select_generate(eyoc_ctx* ctx, int form);
/* Per-pair failure isolation of the batched back-ends (default 0).  With 1, eyoc_ransac_batched(_ws) accepts pairs with 0..3
 * correspondences and eyoc_sc2pcr_batched pairs with 0..7 rows (empty segments included) instead of failing the call: such a pair
 * gets a defined failed output - RANSAC: T all NaN, best_hypothesis -1, survivors 0, inliers 0, inlier_rmse 0; SC2-PCR: T all NaN,
 * its fitness row 0 -, and its rows are never read.  The other pairs run as they would without it (pair b still samples with
 * seed + b) and give the same bytes.  Other values only query; returns the previous state.  Per ctx. */
int eyoc_registration_accept_degenerate(eyoc_ctx* ctx, int on);
/* How many survivor transforms per pair are stored for the scorer (default 2^20 = 96 MB per pair; survivors beyond it are
 * re-derived from their hypothesis number by k_count_overflow - same counts, more work).  survivors >= 1 sets, anything else
 * only queries; returns the previous value.  Per ctx; tests set it tiny to drive every survivor through the overflow path. */
int eyoc_ransac_transform_store(eyoc_ctx* ctx, int survivors);

/* RANSACConvergenceCriteria(max_iteration, confidence) with confidence below 1: early termination, decided on the device.
 * (Symbols added without a change of EYOC_VERSION, like the other additions since 111.  Opt-in: eyoc_ransac_batched(_ws) is what
 * confidence >= 1 means everywhere else and does not change.)
 *
 * Checkpoints.  With H = params->max_iteration the hypotheses of a pair are evaluated in rounds between checkpoints
 * E_0 < E_1 < ... < E_last = H:  E_0 = min(first_check, H),  E_{j+1} = min(2 E_j, H);  round j covers h in [E_{j-1}, E_j), E_{-1} = 0.
 * Doubling keeps the number of rounds at about log2(H / first_check) - 9 for first_check = 16384 and H = 4 000 000 -, so that all
 * rounds are enqueued without the host waiting, and a pair overshoots its exact stopping point by at most a factor of two.
 * Open3D evaluates the criterion after every iteration, under OpenMP with a sampler seeded from std::random_device, and is not
 * reproducible against itself; here the criterion is looked at only at the checkpoints and what a pair returns is a pure function of
 * (seed, the order of h, first_check).
 *
 * When a pair is finished.  After checkpoint E take the pair's best record over all h < E under the total order of eyoc_ransac (more
 * inliers, then lower fp32 inlier RMSE, then lower h).  With inliers == 0 (nothing survived yet) the pair is not finished.  Otherwise,
 * in fp64 with n the pair's correspondences and c = (double)confidence:  f = inliers / n,  q = (f f)(f f);  the pair is finished if
 * q >= 1, or if (double)E >= log(1 - c) / log(1 - q).  A finished pair evaluates nothing further (the workgroups of the later rounds
 * return on their first test); a pair that never finishes ends at H.
 *
 * What the call returns.  results[b] is byte for byte what eyoc_ransac_batched_ws gives for that pair with max_iteration =
 * iterations[b] and seed params->seed + b, `survivors` included (the sampler is a counter hash that does not depend on H).
 * iterations_dev: int32 [n_pairs] on the device, the checkpoint at which the pair stopped, or H; 0 for a degenerate pair under
 * eyoc_registration_accept_degenerate, which keeps its failed record.  Neither depends on the launch chunk or on the other pairs of
 * the batch.  Nothing is read back, nothing is allocated and the host never waits inside the call.  confidence >= 1 never finishes a
 * pair early: the records are those of eyoc_ransac_batched_ws and iterations = H.
 *
 * Scratch: CALLER-OWNED, 256-byte aligned, as for eyoc_ransac_batched_ws, but the survivor lists are sized for the longest round
 * instead of H (plus 32 bytes of carried state per pair of a chunk).  eyoc_ransac_converging_workspace_bytes(ctx, n_pairs,
 * total_corr, max_iteration, first_check, budget) follows the rules of eyoc_ransac_workspace_bytes (0 for arguments the call refuses).
 * A chunk runs all its rounds before the next chunk starts.
 *
 * Refused: confidence <= 0 or NaN, first_check < 1, a misaligned workspace -> EYOC_ERR_INVALID; a workspace in which not even one
 * pair fits -> EYOC_ERR_WORKSPACE, before the first write. */
size_t eyoc_ransac_converging_workspace_bytes(const eyoc_ctx* ctx, int n_pairs, int total_corr, int max_iteration, int32_t first_check,
                                              size_t budget_bytes);
int eyoc_ransac_converging_batched_ws(eyoc_ctx* ctx, const float* src_dev, const float* tgt_dev, const int64_t* corr_tgt_dev,
                                      const int32_t* seg_src_host, const int32_t* seg_tgt_host, int n_pairs,
                                      const eyoc_ransac_params* params, float confidence, int32_t first_check,
                                      eyoc_ransac_result* results_dev, int32_t* iterations_dev, void* workspace_dev,
                                      size_t workspace_bytes, void* stream);

/* replaces: Matcher.SC2_PCR (scripts/SC2_PCR/SC2_PCR.py:307-384) for bs == 1.
 * src,tgt f32 [n,3] matched correspondences -> T f32 [4,4], seedwise_fitness f32 [int(ratio*n)]. */
typedef struct {
  float inlier_threshold, d_thre, ratio, nms_radius;
  int32_t num_iterations, max_points, k1, k2;
} eyoc_sc2pcr_params;
size_t eyoc_sc2pcr_workspace_bytes(int n, const eyoc_sc2pcr_params* params);
int eyoc_sc2pcr(eyoc_ctx* ctx, const float* src_dev, const float* tgt_dev, int n,
                const eyoc_sc2pcr_params* params, float* T_dev, float* fitness_dev,
                void* workspace_dev, size_t workspace_bytes, void* stream);
/* A batch of independent pairs (the per-pair loop of lib/trainer.py:1157-1166; SURVEY 8f "batched registration"):
 * pair b = rows [seg[b], seg[b+1]) of src / tgt (seg: HOST array of n_pairs + 1 ints), params[b] per pair,
 * T_dev f32 [n_pairs,16], fitness_dev f32 [n_pairs, fitness_stride].  Pairs run concurrently on internal side
 * streams, forked from / joined to `stream`; results are bit-identical to eyoc_sc2pcr on each pair. */
size_t eyoc_sc2pcr_batched_workspace_bytes(int max_n, const eyoc_sc2pcr_params* params);   /* for any n_pairs (16 slices) */
/* ... for a call of exactly n_pairs pairs: min(n_pairs, 16) slices of the largest pair's workspace */
size_t eyoc_sc2pcr_batched_workspace_bytes_n(int max_n, int n_pairs, const eyoc_sc2pcr_params* params);
int eyoc_sc2pcr_batched(eyoc_ctx* ctx, const float* src_dev, const float* tgt_dev, const int32_t* seg_host,
                        int n_pairs, const eyoc_sc2pcr_params* params, float* T_dev, float* fitness_dev,
                        int fitness_stride, void* workspace_dev, size_t workspace_bytes, void* stream);
/* Diagnostics of the per-seed stage (second-order counts + top-k1, sc2pcr.hip), per ctx; neither changes any result - tests run
 * both sides of each and compare bit for bit.  Both return the previous value.
 * _set_shortlist_cap: the top-k1 short list holds at most `cap` <= 1024 entries (default 1024; 0 = every seed takes the histogram
 * selection); _set_dense_threshold: a block of 64 consecutive seeds counts as dense - lane = seed kernel, rows in registers - when
 * its hard rows hold >= x * n candidates together (default 0 = every block, since round 6: with the top-k of dense blocks at 0.1 us per seed
 * the one-wave-per-candidate path of sparse blocks costs more than their share of the dense kernel; 2 in round 5; negative = that kernel off). */
int eyoc_sc2pcr_set_shortlist_cap(eyoc_ctx* ctx, int cap);
int eyoc_sc2pcr_set_dense_threshold(eyoc_ctx* ctx, int x);
/* EYOC_VERSION >= 111.  Round-6 forms of three back-end kernels against their round-5 forms (bit-identical results, tests compare):
 * bit 0 = CSR fill walks the row word by word (default: compacted rows), bit 1 = the mask kernel evaluates both square roots of every
 * cross length exactly (default: v_sqrt_f32 pre-test, exact only for undecided lanes), bit 2 = sqrtf(x) < r in the NMS and the
 * seed-fitness sweeps (default: x < T(r), the exact threshold of the correctly rounded sqrtf), bit 3 = every seed's 3 x 3 Kabsch
 * solve and inlier count inside its wave's kernel (default: lane-per-seed kernels behind it).  0 = default; returns the previous bits. */
int eyoc_sc2pcr_select_kernels(eyoc_ctx* ctx, int legacy_bits);
/* Read-only view of the caller-owned workspace.  Added after 111 without a bump, additive only; host-only: allocates nothing,
 * launches nothing, changes no result.  Every stage of eyoc_sc2pcr leaves its result in the workspace; this reports where (byte
 * offsets from the workspace base, for the same (n, params) the call was made with), so a test can copy the workspace back once and
 * check each stage on its own.  n outside [8, 16384] or a NULL argument: EYOC_ERR_INVALID, *out untouched.
 *   off_ctl     8 x int32: converged (the power iteration reached allclose), iters (sweeps applied), best_seed (first maximum of the
 *               seed-wise fitness), best_fitness (f32), norm (f32: |M v| + 1e-6 of the last sweep), dense (the hard graph has more than
 *               csr_cap edges: ptr_h holds clamped offsets, col_h / val_h are not written, the sweeps recompute the matrix), 2 x pad
 *   off_v       f32 [n]            leading eigenvector after `iters` sweeps (off_y: f32 [n], scratch of the last sweep)
 *   off_score   f32 [n]            dom ? 0 : v
 *   off_seeds   i32 [n_seed]       the first n_seed entries of the stable descending order of score
 *   off_hard, off_tight  u64 [n][words]   bit b of word w of row i: cross(i, 64 w + b) < d_thre resp. < d_thre / 2; columns >= n clear
 *   off_knn     i32 [n_seed][k1]   stable top-k1 of popcount(tight[seed] & tight[j]) * hard[seed][j]
 *   off_Ts      f32 [n_seed][16]   seed hypotheses, row-major 4 x 4: the fp32 storage of an fp64 Kabsch solve of seed_h
 *   off_dom     i32 [n]            non-maximum suppression: some j within nms_radius has a larger v
 *   off_rank    i32 [n]            stable descending rank of score; = off_dom + 4 n, the only offset that is not 256-byte aligned
 *   off_ptr_h   i32 [n + 1]        CSR of the hard graph: exclusive scan of the row popcounts
 *   off_col_h   u16 [nnz]          columns, ascending within a row;  off_val_h  f32 [nnz]: max(0, 1 - c^2 / d_thre^2)
 *   off_cnt     u16 [n_seed][64 words]   second-order counts of the seeds of blocks flagged in blk_dense
 *   off_blk_dense  u8 [ceil(n_seed / 64)]
 *   off_seed_h  f64 [n_seed][16]   centroid a (3), centroid b (3), cross-covariance H (9, row-major), one unused
 * n_seed = int(ratio n); k1 = k2 = 4 when params->k1 > n; total == eyoc_sc2pcr_workspace_bytes(n, params).  n_part column ranges of
 * col_chunk columns split the NMS and rank sweeps.  Batched: pair b of a call (or 16-pair chunk of a call) lives at
 * workspace + (b % 16) * S with S = the largest `total` of the call's pairs rounded up to 256; its layout is that of its own (n, params[b]). */
typedef struct {
  int32_t n, words, n_seed, k1, k2, n_part, col_chunk, reserved;
  int64_t csr_cap;
  uint64_t total;
  uint64_t off_ctl, off_v, off_y, off_score, off_seeds, off_hard, off_tight, off_knn, off_Ts, off_dom, off_rank, off_ptr_h,
      off_col_h, off_val_h, off_cnt, off_blk_dense, off_seed_h;
} eyoc_sc2pcr_layout;
int eyoc_sc2pcr_workspace_layout(int n, const eyoc_sc2pcr_params* params, eyoc_sc2pcr_layout* out);

/* ICP refinement.  Added after 111 without a bump, additive only.
 * replaces: o3d.pipelines.registration.registration_icp(pcd0, pcd1, r, init, TransformationEstimationPointToPoint(),
 * ICPConvergenceCriteria(max_iteration)) at lib/data_loaders.py:485-515 and scripts/SC2_PCR/benchmark_utils.py:40-56, for a batch of
 * independent pairs.  Point-to-point ICP restated from Open3D's published source (parity unpinned):
 *   T = init; res = eval(T); repeat at most max_iteration times { U = Kabsch over the correspondences; T = U T; prev = res;
 *   res = eval(T); stop (CONVERGED) if |prev.fitness - res.fitness| < relative_fitness and |prev.inlier_rmse - res.inlier_rmse| <
 *   relative_rmse }.
 * eval(T): every source point x (fp32, exact in fp64) is posed p = R x + t in fp64; its correspondence is the target row of the pair
 * with the smallest d2 = (p - q)^2 summed in fp64 (x, y, z in that order, no fused multiply-add), the lowest row on an exact tie, kept
 * iff d2 < max_distance^2; fitness = #corr / #source, inlier_rmse = sqrt(sum d2 / #corr) (0 without correspondences).  The posed
 * points are always T x of the ORIGINAL source, and an evaluation with fewer than 3 correspondences stops the pair with its current T
 * and the FEW bit.  The search runs on a cell grid of edge max_distance built once per call (27 cells cover the gate; a posed point
 * within ~1e-16 relative of a cell face AND of the gate at once may miss a neighbour that sits exactly at the gate).
 * Pairs back to back as in eyoc_ransac_batched_ws: pair b owns source rows [seg_src[b], seg_src[b+1]) and target rows [seg_tgt[b],
 * seg_tgt[b+1]) (HOST arrays of n_pairs + 1 ints, n_pairs <= 1024, empty segments accepted: T = init, fitness 0, FEW).  Caller-owned
 * 256-byte aligned workspace of eyoc_icp_workspace_bytes; nothing is allocated and the host never waits inside the call: all
 * max_iteration + 1 evaluations are enqueued, a finished pair's workgroups return at once.  64 pairs share one set of launches (2 per
 * evaluation + the grid build: 3 kernels, 1 fill, 2 radix sorts).  No floating-point atomics and no partition that depends on a pair's neighbours: results[b] is
 * byte-identical from run to run and to a call on pair b alone. */
enum {
  EYOC_ICP_CONVERGED = 1,
  EYOC_ICP_BAD_INIT = 2,   /* non-finite init: T is returned as given, nothing else of the pair is read */
  EYOC_ICP_FEW = 4,        /* an evaluation left fewer than 3 correspondences (or a segment is empty) */
  EYOC_ICP_RANGE = 8,      /* a non-finite source / target point or a target cell outside +-2^17 cells: T = init */
  EYOC_ICP_SINGULAR = 16   /* eyoc_icp_plane_batched only: the correspondences leave a direction of the step unconstrained */
};
typedef struct {
  double max_distance, relative_fitness, relative_rmse;
  int32_t max_iteration;
  int32_t flags;             /* 0 */
} eyoc_icp_params;           /* 32 bytes */
typedef struct {
  double T[16];              /* row-major 4x4 */
  double fitness, inlier_rmse;
  int32_t correspondences, iterations, status, reserved;
} eyoc_icp_result;           /* 160 bytes */
size_t eyoc_icp_workspace_bytes(int n_pairs, int total_src, int total_tgt);
/* init_dev: f64 [n_pairs][16] row-major, NULL = identity.  corr_dev: int32 [total_src], the target row LOCAL to the pair under the
 * returned T or -1; NULL = not wanted. */
int eyoc_icp_batched(eyoc_ctx* ctx, const float* src_dev, const float* tgt_dev, const int32_t* seg_src_host,
                     const int32_t* seg_tgt_host, int n_pairs, const double* init_dev, const eyoc_icp_params* params,
                     eyoc_icp_result* results_dev, int32_t* corr_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
/* One eval(T) and nothing else (iterations 0): corr_dev as above, d2_dev f64 [total_src] (+inf where corr is -1), either may be NULL. */
int eyoc_icp_correspondences(eyoc_ctx* ctx, const float* src_dev, const float* tgt_dev, const int32_t* seg_src_host,
                             const int32_t* seg_tgt_host, int n_pairs, const double* T_dev, double max_distance, int32_t* corr_dev,
                             double* d2_dev, eyoc_icp_result* results_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* Normal estimation for a batch of clouds.  Added after 111 without a bump, additive only.
 * Open3D's estimate_normals(KDTreeSearchParamHybrid(radius, max_nn)) restated as a contract of this library (parity unpinned, like the
 * ICP).  n_clouds <= 1024 clouds back to back: pts_dev f32 [total][3], cloud b owns rows [seg[b], seg[b+1]) (HOST array of n_clouds + 1
 * ints from 0, empty clouds accepted).  For every row x_i of a cloud:
 *   neighbours   the rows j of the SAME cloud, i itself included, with d2 = (dx dx + dy dy) + dz dz < radius * radius, d = x_j - x_i;
 *                all of it fp64 from the fp32 values, every operation rounded on its own (no fused multiply-add), the product
 *                radius * radius formed once; ordered by (d2, j) ascending and cut to the first max_nn.  max_nn = 0 keeps all,
 *                1 <= max_nn <= 64 otherwise (a lane's list lives on chip).  EXACTLY the decision of the n x n sweep: the cell
 *                edge is radius (1 + 2^-20), icp.hip derives the margin.
 *   covariance   k neighbours with offsets d_m in list order: S1 = sum d_m, S2 = sum d_m d_m^T, C = S2 / k - (S1 / k)(S1 / k)^T, fp64,
 *                summed in list order by one lane.
 *   normal       the eigenvector of C's smallest eigenvalue (cyclic Jacobi, fp64), normalised, with the sign that makes n . x_i <= 0
 *                (towards a sensor at the origin); n . x_i == 0: the first non-zero component is positive.  Rounded once to fp32.
 *                k < 3: the zero vector - in eyoc_icp_plane_batched such a target adds nothing to the system.
 * normals_dev f32 [total][3]; count_dev int32 [total] = k, or NULL; status_dev int32 [n_clouds]: 0, or EYOC_ICP_RANGE for a cloud with
 * a non-finite point or a cell floor(v / edge) outside [-2^17, 2^17) - that cloud gets zero normals and count 0, nothing of it is
 * searched.  EYOC_ERR_INVALID for a radius that is not positive and finite or max_nn outside [0, 64].
 * Caller-owned 256-byte aligned workspace of eyoc_normals_workspace_bytes; no allocation, no read-back, no floating-point atomics;
 * every 64-cloud chunk builds its own grid.  A cloud's bytes are the same from run to run, alone, and at any place in a batch. */
size_t eyoc_normals_workspace_bytes(int n_clouds, int total);
int eyoc_normals_batched(eyoc_ctx* ctx, const float* pts_dev, const int32_t* seg_host, int n_clouds, double radius, int max_nn,
                         float* normals_dev, int32_t* count_dev, int32_t* status_dev, void* workspace_dev, size_t workspace_bytes,
                         void* stream);

/* FPFH descriptors for a batch of clouds.  Added after 111 without a bump, additive only.
 * Open3D's compute_fpfh_feature(pcd, KDTreeSearchParamHybrid(radius, max_nn)) restated as a contract of this library (parity unpinned:
 * Open3D is not part of any build here; tests/fpfh_restatement.py is the fp64 statement the kernels are held to).  Clouds, segments
 * and status as eyoc_normals_batched; normals_dev f32 [total][3] are the caller's (eyoc_normals_batched's point to the origin; Open3D's
 * are unoriented unless the caller orients them, and FPFH depends on the orientation).  For every row i of a cloud:
 *   list      L_i = the first max_nn rows of the SAME cloud with d2 < radius * radius by (d2, j) ascending - eyoc_normals_batched's list,
 *             the same fp64 arithmetic, the same cell edge, entry for entry.  N_i = L_i without row i itself, in list order, k_i = |N_i|,
 *             0 <= k_i <= max_nn - 1.  Open3D drops "the first entry" instead: the same unless a duplicate of the point sorts ahead of
 *             the row, where Open3D pairs the row with itself and loses the duplicate.  ONE corner departs from "L_i without row i":
 *             max_nn or more duplicates ahead of the row push it out of L_i, and N_i is then the first max_nn - 1 entries of L_i, not
 *             all max_nn of them.  So k_i <= max_nn - 1 holds everywhere, and in that corner alone N_i is not eyoc_normals_batched's
 *             list without the row.
 *   pair      (p1, n1) = row i, (p2, n2) = row j, fp64, every operation rounded on its own, dots and squared norms as (x + y) + z:
 *             d = p2 - p1, len = |d|; len == 0 -> (0, 0, 0).  a1 = n1.d / len, a2 = n2.d / len.  acos|a1| > acos|a2| (strict): swap n1 and
 *             n2, negate d, f2 = -a2; otherwise f2 = a1.  v = d x n1; |v| == 0 -> (0, 0, 0); v /= |v|, w = n1 x v, f1 = v.n2,
 *             f0 = atan2(w.n2, n1.n2).  A feature of (0, 0, 0) is binned like any other (a zero normal ends there).
 *   SPFH      b0 = clamp(floor(11 (f0 + pi) / (2 pi)), 0, 10), b1 = 11 + clamp(floor(11 (f1 + 1) / 2), 0, 10), b2 = 22 + the same of
 *             f2; cnt_i[33] integer counts over N_i; S_i[b] = cnt_i[b] * (100 / k_i), one division and one product; k_i = 0: S_i = 0.
 *   FPFH      W_i[b] = sum over j in N_i with d2_ij > 0 of S_j[b] / d2_ij and G_i[g] = the sum of the same terms over the 11 bins of
 *             group g = b / 11, both added neighbour by neighbour in list order and, inside a neighbour, bin by bin ascending;
 *             F_i[b] = W_i[b] * (G_i[g] != 0 ? 100 / G_i[g] : 0) + S_i[b]; k_i = 0: F_i = 0.
 *   output    float32(F_i[b]); with normalize != 0 float32(F_i[b] / (sqrt(sum_b F_i[b]^2) + 1e-6)), the sum over b ascending, all fp64
 *             (scripts/SC2_PCR/dataset.py's feature / (norm + 1e-6) on Open3D's float64 rows, rounded once).
 * out_dev f32 [total][out_stride], out_stride 33 or 64 (columns 33..63 are zeros: eyoc_knn1 takes c = 64, and zero columns change no
 * distance); hist_dev uint8 [total][33] = cnt_i, or NULL; count_dev int32 [total] = k_i, or NULL.  status_dev[b] = EYOC_ICP_RANGE for a
 * cloud with a non-finite point, a non-finite normal or a cell outside [-2^17, 2^17): zero rows, zero counts, nothing of it is searched,
 * the other clouds keep their bytes.  EYOC_ERR_INVALID for a radius that is not positive and finite, max_nn outside [2, 128] (counts fit
 * a byte; a radius-only search is not built) or a stride other than 33 / 64.  Caller-owned 256-byte aligned workspace of
 * eyoc_fpfh_workspace_bytes (it holds every row's list: 12 bytes x (max_nn - 1) per row), EYOC_ERR_WORKSPACE before any write when it is
 * short; no allocation, no read-back, no host synchronisation, no floating-point atomics; every 64-cloud chunk builds its own grid.  A
 * cloud's bytes are the same from run to run, alone, and at any place in a batch. */
size_t eyoc_fpfh_workspace_bytes(int n_clouds, int total, int max_nn);
int eyoc_fpfh_batched(eyoc_ctx* ctx, const float* pts_dev, const float* normals_dev, const int32_t* seg_host, int n_clouds, double radius,
                      int max_nn, int normalize, int out_stride, float* out_dev, uint8_t* hist_dev, int32_t* count_dev,
                      int32_t* status_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* Point-to-plane ICP for a batch of pairs.  Added after 111 without a bump, additive only.
 * Open3D's registration_icp with TransformationEstimationPointToPlane restated (parity unpinned).  Call shape, segments, params (flags
 * 0), records, corr_dev and workspace rules are eyoc_icp_batched's; tgt_normals_dev f32 [total_tgt][3] is added (NULL only with no
 * target rows) and the workspace is sized by eyoc_icp_plane_workspace_bytes.
 *   eval(T)  is eyoc_icp_batched's: nearest target by (d2, row), gate d2 < max_distance^2, fitness, Euclidean inlier_rmse, FEW below 3
 *            correspondences, convergence on fitness and rmse.
 *   step     for every correspondence, p = T x in fp64, target q with normal n (fp32, exact in fp64):
 *              r = ((p0 - q0) n0 + (p1 - q1) n1) + (p2 - q2) n2,  a = p x n,  J = (a, n),  A = sum J J^T,  g = sum J r
 *            (21 + 6 sums, reduced lane -> wave -> workgroup -> pair in eyoc_icp_batched's fixed order, no fused multiply-add);
 *            A xi = -g by LDL^T without pivoting in fp64.  A pivot d_k that is not above 2^-30 A_kk (A_kk before elimination) stops
 *            the pair with its current T and EYOC_ICP_SINGULAR.  Otherwise xi = (alpha, beta, gamma, t),
 *            U = [Rz(gamma) Ry(beta) Rx(alpha) | t], T = U T.
 * A non-finite normal sets EYOC_ICP_RANGE for its pair (T = init, nothing searched); a zero normal adds nothing to A and g.
 * Guarantees as eyoc_icp_batched: all max_iteration + 1 evaluations are enqueued, no floating-point atomics, results[b] is
 * byte-identical from run to run and to a call on pair b alone. */
size_t eyoc_icp_plane_workspace_bytes(int n_pairs, int total_src, int total_tgt);
int eyoc_icp_plane_batched(eyoc_ctx* ctx, const float* src_dev, const float* tgt_dev, const float* tgt_normals_dev,
                           const int32_t* seg_src_host, const int32_t* seg_tgt_host, int n_pairs, const double* init_dev,
                           const eyoc_icp_params* params, eyoc_icp_result* results_dev, int32_t* corr_dev, void* workspace_dev,
                           size_t workspace_bytes, void* stream);

/* Posed nearest neighbour with a gate, for a batch of pairs (lib/trainer.py:1198-1211 without the [n0, n1] sweep).  Added after 111
 * without a bump, additive only.  For every query row of every pair: the target row (LOCAL to the pair) that eyoc_knn2(c = 4) returns for
 * the posed point against the pair's targets, if that neighbour passes sqrtf(d2) < max_dist, and -1 otherwise.
 *   posed point  p_r = ((T[4r] x + T[4r+1] y) + T[4r+2] z) + T[4r+3], r = 0..2, every fp32 operation rounded on its own
 *   d2 = (dx dx + dy dy) + dz dz with dx = p_0 - q_x ..., fp32, no fused multiply-add; the minimum is taken over (d2, target row)
 *   lexicographically, so an exact tie goes to the lower row whichever cells the two rows sit in.
 * Pairs back to back like eyoc_icp_batched (seg_src / seg_tgt: HOST arrays of n_pairs + 1 ints from 0, n_pairs <= 1024); T_dev f32
 * [n_pairs][16] row-major, read on the device.  sel_dev NULL: every source row is a query, outputs are indexed like src.  Otherwise
 * sel_dev int64 holds the query rows (LOCAL to the pair's source segment) of all pairs back to back, pair b's are entries [seg_sel[b],
 * seg_sel[b+1]) (HOST), and outputs are indexed like sel_dev.  idx_out int64, d2_out f32 or NULL (+inf where idx is -1).
 * status_dev int32 [n_pairs]: 0, or EYOC_ICP_BAD_INIT (a non-finite pose) / EYOC_ICP_RANGE (a non-finite point among the targets or the
 * queries, a selection outside the source segment, a target or posed query outside +-2^17 cells of max_dist); a pair with a status has
 * every output -1.  The targets are sorted into a cell grid of edge max_dist (1 + 2^-20), built once per call; 27 cells hold every target
 * that passes the fp32 gate (icp.hip derives the margin).  Caller-owned 256-byte aligned workspace, no allocation, no read-back, no
 * floating-point atomics: the result does not depend on slot placement, launch chunking (64 pairs) or the other pairs. */
size_t eyoc_posed_nn_grid_workspace_bytes(int n_pairs, int total_queries, int total_tgt);
int eyoc_posed_nn_grid(eyoc_ctx* ctx, const float* src_dev, const float* tgt_dev, const int32_t* seg_src_host, const int32_t* seg_tgt_host,
                       int n_pairs, const float* T_dev, float max_dist, const int64_t* sel_dev, const int32_t* seg_sel_host,
                       int64_t* idx_out_dev, float* d2_out_dev, int32_t* status_dev, void* workspace_dev, size_t workspace_bytes,
                       void* stream);

/* Ground-truth matching indices by radius search, for a batch of pairs (util/pointcloud.py:53-66, get_matching_indices: Open3D's
 * search_radius_vector_3d around every posed source point; lib/data_loaders.py:948-954 calls it for every training / validation pair,
 * util/pointcloud.py:42-50 with K = 1).  Added after 111 without a bump, additive only.
 * Pairs back to back like eyoc_icp_batched: pair b owns source rows [seg_src[b], seg_src[b+1]) and target rows [seg_tgt[b],
 * seg_tgt[b+1]) (HOST arrays of n_pairs + 1 ints from 0, n_pairs <= 1024, empty segments accepted: no matches).  T_dev f64
 * [n_pairs][16] row-major, read on the device; NULL = the identity for every pair.
 *   posed point  p_k = ((T[4k] x + T[4k+1] y) + T[4k+2] z) + T[4k+3], k = 0..2; fp32 coordinates are exact in fp64
 *   d2 = (dx dx + dy dy) + dz dz with dx = p_0 - q_x ...; all of it fp64, every operation rounded on its own (no fused multiply-add)
 *   match        (i, j) iff d2 < radius * radius, the product formed once in fp64, the comparison strict (what Open3D returns for a
 *                target at exactly the radius is unpinned)
 *   order        inside a source row the matches ascend by (d2, j) - Open3D's sorted radius search, an exact tie in d2 going to the
 *                lower target row; that is the row's list.  max_per_source = K > 0 keeps the first K entries of the list (the
 *                reference's idx[:K]), 0 keeps all.  The result is ordered by pair, then by source row, then by the list; i and j are
 *                LOCAL to the pair.
 * status_dev int32 [n_pairs]: 0, or EYOC_ICP_BAD_INIT (a non-finite pose; nothing else of the pair is read) / EYOC_ICP_RANGE (a
 * non-finite source or target point, a target or posed source whose cell floor(v / edge) lies outside [-2^17, 2^17), edge = radius *
 * (1 + 2^-20) in fp64).  A pair with a status has no matches.
 * The result is EXACTLY the brute-force decision over all n0 x n1 candidates: the cell edge has a margin over the radius, so the 27
 * cells around a source's cell hold every match, also at a cell face (icp.hip derives it).  No floating-point atomics; pair b's slice
 * of the output is byte-identical from run to run, to a call on pair b alone, and for any position of the pair in the batch.
 * The output length is known on the device only, hence two calls:
 *   count  builds the grids, counts every source row's matches (at most K) and writes the exclusive 64-bit scan over ALL source rows
 *          of the call to offsets_dev [total_src + 1]: row r (counted over the whole call) owns entries [offsets[r], offsets[r+1]),
 *          offsets[total_src] is the total.  The grids stay in the workspace.
 *   fill   takes the same arguments, the offsets, the total the host read, and the workspace UNTOUCHED since the count; it searches again
 *          and writes pairs_out_dev int64 [total][2] = (i, j) and d2_out_dev f64 [total].  EYOC_ERR_INVALID for total < 0 or a NULL
 *          output with total > 0; a source row whose slice does not lie inside [0, total) is not written.
 * Caller-owned 256-byte aligned workspace of eyoc_radius_matches_workspace_bytes (every 64-pair chunk keeps its own grid in it);
 * nothing is allocated and the host never waits inside either call. */
size_t eyoc_radius_matches_workspace_bytes(int n_pairs, int total_src, int total_tgt);
int eyoc_radius_matches_count(eyoc_ctx* ctx, const float* src_dev, const float* tgt_dev, const int32_t* seg_src_host,
                              const int32_t* seg_tgt_host, int n_pairs, const double* T_dev, double radius, int max_per_source,
                              int64_t* offsets_dev, int32_t* status_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
int eyoc_radius_matches_fill(eyoc_ctx* ctx, const float* src_dev, const float* tgt_dev, const int32_t* seg_src_host,
                             const int32_t* seg_tgt_host, int n_pairs, const double* T_dev, double radius, int max_per_source,
                             const int64_t* offsets_dev, const int32_t* status_dev, int64_t total, int64_t* pairs_out_dev,
                             double* d2_out_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * training batches from raw scans: the augmentation of the reference's loader for a whole batch (PairDataset.__getitem__ with
 * use_random_rotation, lib/data_loaders.py:912-943, :969-978).  Added after 111 without a bump, additive only.
 * Every fp64 expression below is evaluated as written, left to right inside its brackets, every operation rounded on its own (no fused
 * multiply-add).  fp32 inputs are exact in fp64.
 * --------------------------------------------------------------------------------------------- */

/* replaces: np.mean(pcd, axis=0) of sample_random_trans (lib/data_loaders.py:99), as an fp64 mean.
 * Packed clouds in the layout of eyoc_voxelize_batched (xyz_dev, stride >= 3, HOST point_offsets [n_clouds + 1], empty clouds allowed,
 * n_clouds <= 1024).  centroid_dev f64 [n_clouds][4] = (mean x, mean y, mean z, count); an empty cloud gives four zeros.
 * The sums are reduced lane -> wave -> workgroup -> cloud in an order fixed by the cloud's own size (workgroups of 256 threads take 4096
 * consecutive points each, thread t adds points t, t + 256, ...; a cloud's workgroup sums are added in order, then divided by the count):
 * no floating-point atomics, and a cloud's 32 bytes are the same alone, at any position in a batch and from run to run.
 * Stream-ordered, no synchronisation, no allocation; caller-owned 256-byte aligned workspace. */
size_t eyoc_cloud_centroids_workspace_bytes(int n_points_total, int n_clouds);
int eyoc_cloud_centroids(eyoc_ctx* ctx, const float* xyz_dev, int stride, const int64_t* point_offsets, int n_clouds, int n_points,
                         double* centroid_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* replaces: sample_random_trans's T (lib/data_loaders.py:94-100, the rotation R given) for both clouds of every pair, the pair's pose
 * trans = T1 @ M2 @ np.linalg.inv(T0) (:917) and the scaling of its translation (:933).  One launch, one thread per pair, n_pairs <= 512.
 * rot_dev f64 [2 n_pairs][9] row-major (pair b: clouds 2b, 2b + 1), centroid_dev as eyoc_cloud_centroids wrote it, scale_dev f64
 * [n_pairs] or NULL (no product), M2_dev f64 [n_pairs][16] row-major (its last row is not read).
 *   pose_dev f64 [2 n_pairs][16]:  T_c = [R | t], t_k = (R[k][0] (-m_0) + R[k][1] (-m_1)) + R[k][2] (-m_2), last row 0 0 0 1
 *   T_gt_dev f64 [n_pairs][16] = (T_1 M2) inv(T_0), in this order:
 *     A[i][j] = (T1[i][0] M[0][j] + T1[i][1] M[1][j]) + T1[i][2] M[2][j]                       j < 3
 *     A[i][3] = ((T1[i][0] M[0][3] + T1[i][1] M[1][3]) + T1[i][2] M[2][3]) + T1[i][3]
 *     u[k]    = -((R0[0][k] t0[0] + R0[1][k] t0[1]) + R0[2][k] t0[2])                           inv(T_0) = [R0^T | u], the rigid inverse
 *     G[i][j] = (A[i][0] R0[j][0] + A[i][1] R0[j][1]) + A[i][2] R0[j][2]                       j < 3
 *     G[i][3] = ((A[i][0] u[0] + A[i][1] u[1]) + A[i][2] u[2]) + A[i][3],  then  G[i][3] = s G[i][3]  when scale_dev is given
 *   and the last row 0 0 0 1. */
int eyoc_augment_poses(eyoc_ctx* ctx, const double* rot_dev, const double* centroid_dev, const double* scale_dev, const double* M2_dev,
                       int n_pairs, double* pose_dev, double* T_gt_dev, void* stream);

/* replaces: apply_transform with the fp64 pose (lib/data_loaders.py:134-137, :919-920), scale * xyz (:931-932), the fp64
 * sparse_quantize(xyz / voxel_size) and floor(xyz[sel] / voxel_size).int() (:940-943, :969-970), the .float() of the kept points (:978)
 * and the sparse_collate of collate_pair_fn (:65-66), for a whole batch.
 * eyoc_voxelize_batched's arguments and outputs, plus pose_dev f64 [n_clouds][16] row-major (last row not read), scale_dev f64
 * [n_clouds] or NULL (no product), an fp64 voxel_size and cloud_faults (HOST out int32 [n_clouds][2], or NULL).  Per point (x, y, z):
 *   q_k  = ((T[4k] x + T[4k+1] y) + T[4k+2] z) + T[4k+3]        the posed point of eyoc_radius_matches_*
 *   p'_k = s q_k
 *   c_k  = floor(p'_k / voxel_size)                              IEEE division
 * then key, first-hit de-duplication, row offsets and compaction exactly as eyoc_voxelize_batched: coords int32 [.,4] = (batch_base + b,
 * c), sel ascending per cloud, xyz_out f32 [.,3] = (float)p' of the same p' the key was formed from, voxel_offsets as there.
 * A point is faulty when a p'_k is not finite (a NaN / inf point or pose) or, all p' finite, a c_k lies outside the key range.
 * With cloud_faults: the contract of eyoc_voxelize_batched_isolating - cloud_faults[b][0] counts cloud b's finite posed points out of
 * range, [b][1] its non-finite ones, a cloud with a count has an empty row range and every other cloud's rows are unchanged; EYOC_OK.
 * With NULL: EYOC_ERR_RANGE, the message names the first cloud holding a faulty point.
 * Synchronises `stream` once per call; n_points = 0 launches nothing.  The workspace also holds the posed fp32 points. */
size_t eyoc_voxelize_batched_posed_workspace_bytes(int n_points_total, int n_clouds);
int eyoc_voxelize_batched_posed(eyoc_ctx* ctx, const float* xyz_dev, int stride, const int64_t* point_offsets, int n_clouds, int n_points,
                                const double* pose_dev, const double* scale_dev, double voxel_size, int batch_base, int32_t* sel_dev,
                                int32_t* coords_dev, float* xyz_out_dev, int64_t* voxel_offsets, void* workspace_dev,
                                size_t workspace_bytes, void* stream, int32_t* cloud_faults);

/* ------------------------------------------------------------------------------------------------
 * hardest-contrastive loss and its gradient on device-resident positives (lib/trainer.py:935-991).  Added after 111 without a bump,
 * additive only.
 * replaces: contrastive_hardest_negative_loss and the autograd walk behind it, after the three np.random draws.
 *   F0, F1      f32 [n0, c], [n1, c], c in {16, 32, 64}
 *   pairs       int64 [n_pairs, 2] on the device: all known positives (collated rows)
 *   used        int64 [n_used] indices into pairs (the positive sub-sample), NULL = all of them (n_used == n_pairs)
 *   sel0, sel1  int64 [s0], [s1] candidate rows of F0 / F1
 * Per used positive p = (i, j), a0 = F0[i], a1 = F1[j]; no contraction:
 *   pos_d2 = f32(sum_c (a0_c - a1_c)^2 in fp64), pos_term = max(pos_d2 - pos_thresh, 0) in fp32
 *   01: t* = the t in [0, s1) with the smallest sqrtf(d2(a0, F1[sel1[t]]) + 1e-7f) in fp32, channels left to right, ties to the lowest
 *       t (the arithmetic and the answer of eyoc_knn1 with dist_type 1 on the gathered rows); dist = f32(sqrt(d2 + 1e-7f) in fp64) of
 *       that pair (the search's own fp32 chain is up to 8 ulp off over 64 channels; the value kept is rounded once); masked when i + sel1[t*] * scale, scale = max(n0, n1), is one of the n_pairs keys
 *       pairs[:,0] + pairs[:,1] * scale (an open-addressing table of integer compare-and-swaps: membership does not depend on the order
 *       of pairs), else term = max(neg_thresh - dist, 0)^2
 *   10: the mirror image, a1 against F0[sel0[t]], key sel0[t*] + j * scale.
 * The three sums (pos_term, kept term01, kept term10) are fp64 sums of the fp32 terms in a fixed order: lane -> wave (one workgroup of
 * EYOC_HCLOSS_ANCHORS positives), then the workgroups in order in a final pass.  pos_loss = f32(sum / n_used), neg_loss =
 * f32((s01 / k01 + s10 / k10) / 2); a mean over nothing is NaN.  Every row index of pairs, used, sel0 and sel1 is checked before a
 * feature is read through it: a bad one is skipped, sets EYOC_HCLOSS_BAD_INDEX and makes both losses (and, in the backward, every
 * row that receives a contribution) NaN.  The per-positive results stay in the workspace (eyoc_hcloss_workspace_layout) for the backward.
 *
 * Backward, per positive: d/da0 = g_pos (2 / n_used) [pos_d2 - pos_thresh > 0] (a0 - a1), d/da1 its negative; 01, kept and dist <
 * neg_thresh: w = -g_neg max(neg_thresh - dist, 0) / (k01 dist), d/da0 = w (a0 - b), d/db = -w (a0 - b), b = F1[sel1[t*]]; 10 mirrors it.
 * No floating-point atomics: a row of dF0 sums its own contributions in fp64 and rounds once, in the order (anchor entries by p: positive
 * term, then 01; then candidate entries of direction 10 by p) - dF1: (anchor entries by p: positive term, then 10; then candidate entries
 * of 01) -, entry k of the row's list going to slot k mod (256 / c) and the slots added in order.  A row's bytes depend on its own list
 * only; rows nothing touches are +0.0f.  dF0 [n0, c], dF1 [n1, c] are written completely.
 *
 * Launches: forward 5 (one fill, table build and index check, search, terms, final pass), backward 4 (two fills, weights, row sums), whatever
 * the sizes.  Stream-ordered: no synchronisation, no allocation, no floating-point atomics, nothing read back; caller-owned 256-byte
 * aligned workspace, which the backward reads as the forward of the SAME arguments left it.
 * --------------------------------------------------------------------------------------------- */
#define EYOC_HCLOSS_BAD_INDEX 1u
#define EYOC_HCLOSS_ANCHORS 64      /* positives per workgroup of the search */
#define EYOC_HCLOSS_TILE 128        /* candidate rows staged through LDS at a time */
#define EYOC_HCLOSS_MASKED 1u       /* flags: the direction's hardest negative is a known positive (or there is no candidate) */
#define EYOC_HCLOSS_VALID 2u        /* flags: the positive's own indices were in range */

typedef struct eyoc_hcloss_record {
  double sum_pos, sum01, sum10;
  int32_t n_used, k01, k10;
  uint32_t status;
  float pos_loss, neg_loss;
} eyoc_hcloss_record;               /* 48 bytes */

/* byte offsets into the workspace: record (eyoc_hcloss_record), tstar int32 [2][n_used] (-1: none), dist f32 [2][n_used], pos_d2 f32
 * [n_used], flags uint32 [2][n_used]; [0] is direction 01, [1] direction 10 */
typedef struct eyoc_hcloss_layout {
  int32_t anchors, tile, n_used, table_slots;
  uint64_t total, off_record, off_tstar, off_dist, off_pos_d2, off_flags;
} eyoc_hcloss_layout;

size_t eyoc_hcloss_workspace_bytes(int n_pairs, int n_used, int s0, int s1, int c);
int eyoc_hcloss_workspace_layout(int n_pairs, int n_used, int s0, int s1, int c, eyoc_hcloss_layout* out);
int eyoc_hcloss_forward(eyoc_ctx* ctx, const float* F0_dev, int n0, const float* F1_dev, int n1, int c, const int64_t* pairs_dev,
                        int n_pairs, const int64_t* used_dev, int n_used, const int64_t* sel0_dev, int s0, const int64_t* sel1_dev,
                        int s1, float pos_thresh, float neg_thresh, eyoc_hcloss_record* record_out_dev, void* workspace_dev,
                        size_t workspace_bytes, void* stream);
int eyoc_hcloss_backward(eyoc_ctx* ctx, const float* F0_dev, int n0, const float* F1_dev, int n1, int c, const int64_t* pairs_dev,
                         int n_pairs, const int64_t* used_dev, int n_used, const int64_t* sel0_dev, int s0, const int64_t* sel1_dev,
                         int s1, float pos_thresh, float neg_thresh, const float* g_pos_dev, const float* g_neg_dev, float* dF0_dev,
                         float* dF1_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * triplet and hardest-triplet loss (lib/trainer.py:567-621 and :701-782) and their gradient.  Added after 111 without a bump, additive
 * only.  The arguments of eyoc_hcloss_* plus:
 *   rand_idx    int64 [n_rand] indices into pairs: the random triplets' (anchor, positive) = pairs[rand_idx[r]]
 *   negatives   int64 [n_rand] rows of F1: the random triplets' negatives
 *   margin      the reference's neg_thresh
 *   s0 == s1 == 0 switches the two hardest parts off (the plain TripletLossTrainer); one of them zero alone is EYOC_ERR_INVALID.
 * dist(x, y) = f32(sqrt(sum_c (x_c - y_c)^2 + 1e-7f)) with the sum and the root in fp64: every distance that enters a term or a monitor
 * is rounded to fp32 once.  Keys are i + j * max(n0, n1) in the table of eyoc_hcloss_* (membership does not depend on the order of pairs).
 *   random r:   (a, q) = pairs[rand_idx[r]], n = negatives[r]; dropped when key (a, n) is known, else
 *               term = max((dist(F0[a], F1[q]) + margin) - dist(F0[a], F1[n]), 0) in fp32, in that order
 *   hardest 01: per used positive p = (i, j): t* as in eyoc_hcloss_forward (the search kernel is the same one: eyoc_knn1(dist_type 1)'s
 *               fp32 arithmetic and answer), d01 = dist(F0[i], F1[sel1[t*]]); dropped when key (i, sel1[t*]) is known, else
 *               term = max((dist(F0[i], F1[j]) + margin) - d01, 0)
 *   hardest 10: the mirror, F1[j] against F0[sel0[t]], key (sel0[t*], j), the same positive distance.
 * A term is ACTIVE when kept and (pos + margin) - neg > 0, strictly.  Sums are fp64 sums of the fp32 values in a fixed order: lane -> wave
 * (one workgroup of EYOC_HCLOSS_ANCHORS terms), then the workgroups in order in a final pass.  K = k_rand + k01 + k10 and
 *   loss = f32(((sum_rand + sum01) + sum10) / K), pos_dist_mean = f32(sum_pos_dist / n_used),
 *   neg_dist_mean = f32(sum_rand_neg / k_rand) without the hardest parts (the kept random triplets' negative distances), else
 *                   f32((sum_d01 / n_used + sum_d10 / n_used) / 2) over ALL used positives, dropped or not;
 * a mean over nothing is NaN.  Every index of pairs, used, sel0, sel1, rand_idx and negatives is checked before a feature is read through
 * it: a bad one is skipped, sets EYOC_TRIPLET_BAD_INDEX and makes the three values (and, in the backward, every row that receives a
 * contribution) NaN.  n_used == 0 or n_pairs == 0: the three values are NaN, the gradients exactly +0.0f.
 *
 * Backward.  Every active term (anchor x_a, positive x_q, negative x_n, distances pos, neg; w = g / K) makes three contributions:
 *   anchor row:    (w / pos) (x_a - x_q) + (-w / neg) (x_a - x_n)
 *   positive row:  (w / pos) (x_q - x_a)
 *   negative row:  (-w / neg) (x_n - x_a)
 * with the two factors rounded to fp32.  Term t (random triplets by r, then direction 01 by p, then direction 10 by p) owns the entries
 * 3 t (anchor), 3 t + 1 (positive), 3 t + 2 (negative) of the contribution list: the entry number is the sequence number.  Dropped and
 * inactive terms leave their entries empty and read nothing.  The list is grouped by destination (row, matrix) with one stable radix sort
 * (rocPRIM, its temporary storage carved from the workspace), and the first entry of every run adds the run in list order: C lanes per
 * entry, 256 / c entries side by side, entry k of the run to slot k mod (256 / c), fp64 accumulators, the slots added in order, rounded
 * once.  The work is linear in the number of contributions; no floating-point atomics.  A row's bytes depend on its own list only; rows
 * nothing touches are +0.0f; dF0 [n0, c] and dF1 [n1, c] are written completely.
 *
 * Launches: forward 5 (one fill, table build and index check, search, terms, final pass); backward 4 of this library (two fills, weights,
 * row sums), whatever the sizes, plus those of the one rocPRIM sort, which chooses its passes by the length of the list (8 at 18 432
 * entries: a block sort and merge passes).  Stream-ordered: no synchronisation, no allocation, no
 * environment variable, no floating-point atomics, nothing read back; caller-owned 256-byte aligned workspace, which the backward reads as
 * the forward of the SAME arguments left it.
 * --------------------------------------------------------------------------------------------- */
#define EYOC_TRIPLET_BAD_INDEX 1u
#define EYOC_TRIPLET_MASKED 1u      /* flags: dropped (the negative is a known positive, or there is no candidate) */
#define EYOC_TRIPLET_VALID 2u       /* flags: the term's own indices were in range */
#define EYOC_TRIPLET_ACTIVE 4u      /* flags: kept and (pos + margin) - neg > 0 */

typedef struct eyoc_triplet_record {
  double sum_rand, sum01, sum10;                          /* the kept terms of the three parts */
  double sum_pos_dist, sum_rand_neg, sum_d01, sum_d10;    /* the monitors' sums */
  int32_t n_used, n_rand, k_rand, k01, k10;
  uint32_t status;
  float loss, pos_dist_mean, neg_dist_mean;
  int32_t reserved;
} eyoc_triplet_record;              /* 96 bytes */

/* byte offsets into the workspace: record (eyoc_triplet_record), tstar int32 [2][n_used] (-1: none), dist f32 [2][n_used] (d01, d10),
 * pos_dist f32 [n_used], term f32 [2][n_used], flags uint32 [2][n_used] ([0] is direction 01, [1] direction 10); rand_pos, rand_neg,
 * rand_term f32 [n_rand], rand_flags uint32 [n_rand]; after the backward: contrib_key uint32 [n_contrib], n_contrib = 3 (n_rand + 2 n_used): the
 * destination of each entry as 2 row + matrix + 1 (matrix 0 = dF0, 1 = dF1), 0 = empty */
typedef struct eyoc_triplet_layout {
  int32_t anchors, tile, n_used, n_rand, table_slots, n_contrib;
  uint64_t total, off_record, off_tstar, off_dist, off_pos_dist, off_term, off_flags, off_rand_pos, off_rand_neg, off_rand_term,
      off_rand_flags, off_contrib_key;
} eyoc_triplet_layout;

size_t eyoc_triplet_workspace_bytes(int n_pairs, int n_used, int s0, int s1, int n_rand, int c);
int eyoc_triplet_workspace_layout(int n_pairs, int n_used, int s0, int s1, int n_rand, int c, eyoc_triplet_layout* out);
int eyoc_triplet_forward(eyoc_ctx* ctx, const float* F0_dev, int n0, const float* F1_dev, int n1, int c, const int64_t* pairs_dev,
                         int n_pairs, const int64_t* used_dev, int n_used, const int64_t* sel0_dev, int s0, const int64_t* sel1_dev,
                         int s1, const int64_t* rand_idx_dev, const int64_t* negatives_dev, int n_rand, float margin,
                         eyoc_triplet_record* record_out_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
int eyoc_triplet_backward(eyoc_ctx* ctx, const float* F0_dev, int n0, const float* F1_dev, int n1, int c, const int64_t* pairs_dev,
                          int n_pairs, const int64_t* used_dev, int n_used, const int64_t* sel0_dev, int s0, const int64_t* sel1_dev,
                          int s1, const int64_t* rand_idx_dev, const int64_t* negatives_dev, int n_rand, float margin,
                          const float* g_dev, float* dF0_dev, float* dF1_dev, void* workspace_dev, size_t workspace_bytes,
                          void* stream);

/* ------------------------------------------------------------------------------------------------
 * random-negative contrastive loss of the base trainer (lib/trainer.py:201-221 generate_rand_negative_pairs and :262-286, the loss in
 * _train_epoch) and its gradient.  Added after 111 without a bump, additive only.
 *   F0, F1      f32 [n0, c], [n1, c], c in {16, 32, 64}; n0, n1 <= 2^30
 *   pairs       int64 [n_pairs, 2] on the device: ALL positives, each counted as often as it occurs
 *   neg         int64 [n_neg, 2] on the device: the raw candidate negatives (row of F0, row of F1), before the membership test
 *   n_pairs + n_neg < 2^30, anything else is EYOC_ERR_INVALID
 * Membership: candidate q = (a, b) is dropped (MASKED) exactly when a + b * max(n0, n1) is one of the keys pairs[:,0] + pairs[:,1] *
 * max(n0, n1) of the in-range positives - the table of eyoc_hcloss_* (integer compare-and-swaps: membership does not depend on the
 * order of pairs); since a < max(n0, n1) this is exact pair membership, the reference's np.isin on _hash(., max(N0, N1)).  Nothing is
 * compacted: candidate q keeps its place and gets a flag word; k_neg, the number of kept candidates, is counted on the device.
 * No contraction anywhere:
 *   positive p = (i, j):   pos_d2[p] = f32(sum_c (F0[i]_c - F1[j]_c)^2), the sum in fp64, rounded once
 *   kept candidate (a, b): dist[q] = f32(sqrt(sum_c (F0[a]_c - F1[b]_c)^2 + (double)1e-4f)), sum and root in fp64, rounded once;
 *                          h = neg_thresh - dist in fp32; ACTIVE when h > 0 strictly, then term[q] = h * h in fp32, else term[q] = +0
 *   dropped candidates and candidates with a bad index store dist = term = +0.
 * Sums are fp64 sums of the stored fp32 values in a fixed order: lane -> wave (one workgroup of EYOC_HCLOSS_ANCHORS terms), then the
 * workgroups in order in a final pass.  pos_loss = f32(sum_pos / n_pairs), neg_loss = f32(sum_neg / k_neg); a mean over nothing is NaN
 * (all candidates dropped: neg_loss is NaN, pos_loss is not).  n_pairs == 0: both values are NaN, the gradients exactly +0.0f.  Every
 * index of pairs and neg is checked before a feature is read through it: a bad one is skipped, sets EYOC_CLOSS_BAD_INDEX and makes both
 * values (and, in the backward, every row that receives a contribution) NaN.
 *
 * Backward, g_pos and g_neg f32 device scalars.  Positive p = (i, j): w = f32(2 g_pos / n_pairs); active candidate q = (a, b):
 * w = f32(-2 (g_neg / k_neg) (neg_thresh - dist) / dist), the difference in fp32 as in the forward, the rest in fp64.  A term with rows
 * (r0, r1) contributes w (F0[r0] - F1[r1]) to dF0[r0] and w (F1[r1] - F0[r0]) to dF1[r1].  Terms are numbered positives by p, then
 * candidates by q; term t owns entry 2 t (its dF0 row) and 2 t + 1 (its dF1 row) of ONE contribution list: the entry number is the
 * sequence number.  Dropped, inactive and bad terms leave their entries empty and read nothing.  The list is grouped by destination
 * (row, matrix) with one stable radix sort (rocPRIM, its temporary storage carved from the workspace), and the first entry of every run
 * adds the run in list order exactly as eyoc_triplet_backward does: C lanes per entry, 256 / c entries side by side, entry k of the run to
 * slot k mod (256 / c), fp64 accumulators (factor times difference, both widened), the slots added in order, rounded once.  The work is
 * linear in the number of contributions; no floating-point atomics.  A row's bytes depend on its own entries in list order only; rows
 * nothing touches are +0.0f; dF0 [n0, c] and dF1 [n1, c] are written completely.
 *
 * Launches: forward 4 (one fill, table build and index check of the positives, terms, final pass); backward 4 of this library (two fills,
 * weights, row sums; the two fills alone when n_pairs == 0), whatever the sizes, plus those of the one rocPRIM sort, which chooses its
 * passes by the length of the list.  Stream-ordered: no synchronisation, no allocation, no environment variable, no floating-point
 * atomics, nothing read back; caller-owned 256-byte aligned workspace, which the backward reads as the forward of the SAME arguments
 * left it.
 * --------------------------------------------------------------------------------------------- */
#define EYOC_CLOSS_BAD_INDEX 1u
#define EYOC_CLOSS_MASKED 1u        /* flags: dropped (the candidate is a known positive, or one of its indices is out of range) */
#define EYOC_CLOSS_VALID 2u         /* flags: the candidate's own indices were in range */
#define EYOC_CLOSS_ACTIVE 4u        /* flags: kept and neg_thresh - dist > 0 */

typedef struct eyoc_closs_record {
  double sum_pos, sum_neg;           /* the positives' squared distances; the kept candidates' terms */
  int32_t n_pairs, n_neg, k_neg, n_active;
  uint32_t status;
  float pos_loss, neg_loss;
  int32_t reserved;
} eyoc_closs_record;                /* 48 bytes */

/* byte offsets into the workspace: record (eyoc_closs_record), pos_d2 f32 [n_pairs], dist f32 [n_neg], term f32 [n_neg], flags uint32
 * [n_neg]; after the backward: contrib_key uint32 [n_contrib], n_contrib = 2 (n_pairs + n_neg): the destination of each entry as
 * 2 row + matrix + 1 (matrix 0 = dF0, 1 = dF1), 0 = empty */
typedef struct eyoc_closs_layout {
  int32_t anchors, n_pairs, n_neg, table_slots, n_contrib, reserved;
  uint64_t total, off_record, off_pos_d2, off_dist, off_term, off_flags, off_contrib_key;
} eyoc_closs_layout;

size_t eyoc_closs_workspace_bytes(int n_pairs, int n_neg, int c);
int eyoc_closs_workspace_layout(int n_pairs, int n_neg, int c, eyoc_closs_layout* out);
int eyoc_closs_forward(eyoc_ctx* ctx, const float* F0_dev, int n0, const float* F1_dev, int n1, int c, const int64_t* pairs_dev,
                       int n_pairs, const int64_t* neg_dev, int n_neg, float neg_thresh, eyoc_closs_record* record_out_dev,
                       void* workspace_dev, size_t workspace_bytes, void* stream);
int eyoc_closs_backward(eyoc_ctx* ctx, const float* F0_dev, int n0, const float* F1_dev, int n1, int c, const int64_t* pairs_dev,
                        int n_pairs, const int64_t* neg_dev, int n_neg, float neg_thresh, const float* g_pos_dev,
                        const float* g_neg_dev, float* dF0_dev, float* dF1_dev, void* workspace_dev, size_t workspace_bytes,
                        void* stream);

/* ------------------------------------------------------------------------------------------------
 * device-side draws for the training losses: a counter-based generator and the two draw primitives of the reference's trainers.
 * Added after 111 without a bump, additive only.  The index arrays these calls write are what eyoc_hcloss_*, eyoc_triplet_* and
 * eyoc_closs_* take as sel0 / sel1 / used / rand_idx / negatives / neg.
 *
 * Generator: Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11) - ten rounds, multipliers 0xD2511F53 (word 0) and 0xCD9E8D57 (word 2),
 * Weyl increments 0x9E3779B9 and 0xBB67AE85 of the two key words.  Key and counter of the 128-bit block of element `index` of draw
 * `slot` of call `call` under `seed`:
 *   key     k0 = seed[31:0]    k1 = seed[63:32]
 *   counter c0 = index[31:0]   c1 = index[63:32]   c2 = call[31:0]   c3 = call[59:32] | slot << 28
 * call < 2^60 and slot < 8 (anything else: EYOC_ERR_INVALID).  The block's four output words are x0 .. x3.  Every number is a pure
 * function of (seed, call, slot, index): no device state, no atomics, the same on any grid, stream, device or host - a host program
 * that evaluates Philox4x32-10 on this layout gets the same bits.
 *
 * eyoc_draw_subsets: np.random.choice(n, k, replace=False) as a distribution (lib/trainer.py:445-449, :715-719, :754-760, :946-955):
 * a uniformly random k-subset of [0, n) in uniformly random order, for up to EYOC_DRAW_MAX_SLOTS independent draws in one call.  The
 * position in n[] / k[] IS the slot number.  Element i of slot s gets the 64-bit key
 *   (s << 61) | ((x1 << 32 | x0) >> 3)            x0, x1 of the block (seed, call, s, i)
 * all keys of the call are ordered with ONE stable radix sort (rocPRIM, the wrapper of the map build, all 64 bits) together with
 * their i, and the first k[s] values of slot s's run are its draw, written as int64; k == n is a full permutation.  The outputs lie back
 * to back in out_idx in slot order (slot s starts at k[0] + ... + k[s - 1]).  Two elements of one slot whose 61 generator bits collide
 * are ordered by i (the sort is stable): the outcome is deterministic, and the departure from a uniform permutation is bounded by the
 * collision probability, n^2 / 2^62 - below 1e-8 for a cloud of 2^17 rows.  A slot's result depends on (seed, call, s, n[s], k[s]) only,
 * not on which other slots share the call.  n[] and k[] are HOST arrays of n_slots entries.
 *   k > n, a negative size, n_slots outside [0, EYOC_DRAW_MAX_SLOTS], call >= 2^60, more than 2^31 - 1 elements in one call:
 *   EYOC_ERR_INVALID before any launch, nothing written.  A slot with k == 0 or n == 0 is legal, puts no keys into the sort and writes
 *   nothing; a call whose slots are all empty launches nothing (out_idx and the workspace may be NULL then).
 * Workspace: eyoc_draw_workspace_bytes(total_n), total_n = the sum of n[s] over the slots with k[s] > 0 (0 for total_n <= 0); caller-owned,
 * 256-byte aligned, needed until the call's kernels have run; a smaller one is EYOC_ERR_WORKSPACE, a misaligned one EYOC_ERR_INVALID,
 * both before any launch.
 * Launches: one that writes keys, the rocPRIM sort (which chooses its passes by the length), one that writes out_idx.
 *
 * eyoc_draw_pairs: floor(rand(N, 2) * [n0, n1]) as a distribution (lib/trainer.py:212-218): out int64 [n_rows][2], row-major, in one
 * launch.  Row r: out[r][0] = mulhi64(x1 << 32 | x0, n0), out[r][1] = mulhi64(x3 << 32 | x2, n1) with x0 .. x3 of the block (seed,
 * call, slot, r) and mulhi64(x, n) = floor(x n / 2^64), always < n.  The probability of every index differs from 1 / n by less than
 * 2^-64 (a relative departure of n / 2^64 < 2^-33 for n < 2^31); no floating point anywhere.  n_rows == 0 launches
 * nothing; a negative size, slot outside [0, 8), call >= 2^60, or n_rows > 0 with n0 == 0 or n1 == 0: EYOC_ERR_INVALID before any launch.
 *
 * Both: stream-ordered, no synchronisation, no allocation, no environment variable, no atomics, nothing read back.
 * --------------------------------------------------------------------------------------------- */
#define EYOC_DRAW_MAX_SLOTS 8

size_t eyoc_draw_workspace_bytes(int total_n);
int eyoc_draw_subsets(eyoc_ctx* ctx, uint64_t seed, uint64_t call, int n_slots, const int* n, const int* k, int64_t* out_idx_dev,
                      void* workspace_dev, size_t workspace_bytes, void* stream);
int eyoc_draw_pairs(eyoc_ctx* ctx, uint64_t seed, uint64_t call, int slot, int n_rows, int n0, int n1, int64_t* out_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EYOC_HIP_H */
