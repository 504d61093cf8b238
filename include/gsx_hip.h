/*
 * gsx_hip.h -- C ABI of libgsx_hip.so, the MI355X (gfx950) implementation of the
 * 3dgsconverter point-cloud filtering hot path.
 *
 * The reference (francescofugazzi/3dgsconverter v0.8) is pure Python and has no
 * FFI; its "operator API" for this path is a handful of Python callables.  Each
 * entry point below names the reference interface it replaces (file:line into
 * the reference tree) -- the ctypes stub a maintainer would add is shown in
 * INTEGRATION.md and implemented in 3dgsconverter_amd/_lib.py.
 *
 * Conventions
 *   - plain pointers and sizes only; no torch / numpy types;
 *   - every function returns 0 on success, non-zero on failure; the message is
 *     available from gsx_last_error() (thread-local);
 *   - "host" entry points borrow caller-owned HOST buffers for one call and keep
 *     nothing; "_dev" entry points take DEVICE pointers that are already resident
 *     in HBM and enqueue work on the context's stream (asynchronous unless noted);
 *   - xyz is described by three base pointers and an element stride, so both the
 *     SoA columns and the reference's (N,3) row-major coords
 *     (data_processor.py:139, column_stack) can be passed without a copy
 *     (SoA: stride 1; (N,3): y = x + 1, z = x + 2, stride 3).
 */
#ifndef GSX_HIP_H
#define GSX_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gsx_ctx gsx_ctx;

/* KNN algorithm selector for the SOR entry points */
enum {
    GSX_KNN_AUTO = 0,  /* grid-binned exact KNN, brute force for tiny inputs   */
    GSX_KNN_BRUTE = 1, /* LDS-tiled brute force (BASELINE.json configs[1])     */
    GSX_KNN_GRID = 2,  /* grid-binned exact KNN + exact fallback ring/brute    */
    GSX_KNN_TREE = 3   /* Morton-ordered leaves + exact tree descent: clouds whose density varies by orders of
                          magnitude (csrc/sor_tree.hip); same bits as the other two; k <= 64                      */
};

/* timing slots (HIP-event pairs recorded on the context stream when enabled) */
enum {
    GSX_T_SOR_KNN = 0,    /* dominant kernel: knn_brick / knn_brute             */
    GSX_T_SOR_BIN = 1,    /* bbox + cell histogram + scan + scatter             */
    GSX_T_SOR_FALLBACK = 2,
    GSX_T_SOR_STATS = 3,  /* numpy-exact mean/std/threshold + mask              */
    GSX_T_DENSITY = 4,
    GSX_T_KMEANS_ASSIGN = 5,
    GSX_T_KMEANS_UPDATE = 6,
    GSX_T_QUANTIZE = 7,
    /* multi-GPU slab step (gsx_sor_slab_step_dev), round 5: where a step's time goes besides the KNN slots above */
    GSX_T_SLAB_PREP = 8,   /* this rank's own passes: clear, box, histogram, partition, un-permute            */
    GSX_T_SLAB_ROWS = 9,   /* rows (own + halo) to the slab owners: the grouped send / receive over xGMI     */
    GSX_T_SLAB_MEANS = 10, /* mean distances back to the index owners (+ the < 8192 head elements)            */
    GSX_T_SLAB_COLL = 11,  /* the small collectives: box all-reduce, histogram and piece-sum all-gathers     */
    GSX_T_SLOTS = 12
};

/* diagnostics of one SOR KNN call (all counts are exact) */
typedef struct gsx_sor_info {
    int32_t algo;            /* algorithm actually used                          */
    int32_t grid_dim[3];     /* cells per axis (0 for brute force)               */
    float   cell_size;       /* cell edge h                                      */
    int64_t n_cells;
    int64_t n_bricks;
    int64_t n_fallback;      /* queries re-done by the expanding-ring kernel     */
    int64_t n_exhaustive;    /* of those, queries that needed the whole cloud    */
    int64_t n_deferred_bricks; /* bricks handed to a finer grid (adaptive mode)  */
    int64_t n_refined;       /* points of the sub-cloud that finer grid was built on */
} gsx_sor_info;

/* ---- library / device -------------------------------------------------- */
const char *gsx_version(void);
const char *gsx_last_error(void);
/* replaces the capability probe gpu_ops.py:8-23 (HAS_TAICHI) */
int gsx_device_count(void);
/* the PCI bus id of visible device `device` as text ("0000:c1:00.0"): two processes name the same physical GPU exactly
 * when the strings match, whatever HIP_VISIBLE_DEVICES each of them runs under.  launch.py picks the communicator's
 * transport with it (distinct GPUs -> RCCL, shared ones -> hostwire).  Launcher plumbing, no reference counterpart. */
int gsx_device_uid(int device, char *out, int cap);

/* ---- context ------------------------------------------------------------ */
int  gsx_ctx_create(int device, gsx_ctx **out);
void gsx_ctx_destroy(gsx_ctx *ctx);
/* use an existing hipStream_t (e.g. torch's current stream); NULL = legacy default stream */
int  gsx_ctx_set_stream(gsx_ctx *ctx, void *hip_stream);
/* give the context a non-blocking stream of its own (destroyed with it): several contexts then run concurrently on one
 * GPU -- the independent SOG palette chunks (formats/sog.py:536-552) are dealt out to a few such "lanes" */
int  gsx_ctx_own_stream(gsx_ctx *ctx);
/* GSX_KNN_* of the path the context's last KNN call ended up in (adaptive mode chooses between GRID and TREE); no synchronisation */
int  gsx_ctx_last_knn_algo(gsx_ctx *ctx);
int  gsx_ctx_synchronize(gsx_ctx *ctx);
/* synchronises, then reports (and clears) errors the asynchronous _dev calls detected ON THE DEVICE since the
 * last check: non-finite coordinates given to gsx_sor_knn_dev / gsx_sor_knn_share_dev (their mean_out was
 * filled with NaN, so statistics and masks derived from it are NaN / all-false, never garbage).  The host
 * entry points call it themselves -- the reference's cKDTree raises on such input (data_processor.py:160). */
int  gsx_ctx_check(gsx_ctx *ctx);
int  gsx_ctx_set_timing(gsx_ctx *ctx, int enable);
int  gsx_ctx_reset_timing(gsx_ctx *ctx);
/* synchronises, then returns the number of recorded launches and their summed duration */
int  gsx_ctx_get_timing(gsx_ctx *ctx, int slot, uint64_t *launches, double *total_ms);
/* knobs: "grid_points_per_cell" (0 = auto), "brute_below", "adaptive" (1: a cloud that no single grid
 * resolves -- its coarse histogram is uneven: a scene inside a box inflated by floaters, blobs of very
 * different density -- takes the Morton-tree path, csrc/sor_tree.hip; costs one host synchronisation
 * inside gsx_sor_knn_dev, so it is ON for the host entry point gsx_sor_filter and OFF by default for
 * contexts driven through the asynchronous _dev calls), "tree" (default 1; 0: adaptive mode refines the
 * grid level by level instead, DESIGN.md 5.5 -- kept for A/B and used by the replicated multi-GPU shares),
 * "tree_scale" (0, default: the tree path's density probe stretches the key grid by up to 2x so that the leaves of
 * a cloud with one dominant density are cubes of ~50 points; f > 0: that factor, no probe -- A/B; results are
 * bit-identical for every value), "filter_mfma" (1 = matrix-core phase-1 filter, default), "brick_plan" (1 = knn_brick on planned bricks where the call allows them, default; 0 = the fixed bricks; bit-identical
 * either way), "epilogue_cert" (1 = knn_brick at k = 16 certifies the float32 mean of short float64 roots and
 * recomputes exactly where it cannot, default; 0 = the exact epilogue throughout; bit-identical either way),
 * "timing_mask" (bit s set = slot
 * GSX_T_s records events while timing is enabled; default all -- every event pair costs stream time),
 * "tree_leaf_cap" (0, default: points per leaf of the tree path by k -- 64 up to k = 28, 96 up to 34, 128 above; 64 ... 256: that
 * capacity; results are bit-identical for every value), "tree_cand_limit" (candidates per 64 points of leaf capacity above which
 * a leaf hands its queries to the per-query kernels; 0 = 4096), "tree_near_cell" (0.5, default: knn_tree_near covers a query's
 * ball with cells whose edge is at least this fraction of its radius; values up to 0.05 set the default; small fractions send
 * every query on to the descent, large ones make the cells dense; results are bit-identical for every value), "kmeans_cs_small" (1, default: the K-Means assign kernel uses
 * 4-wave / 2-wave workgroups for K <= 256 / K <= 64), "km_small_wgs" (their workgroups per CU; 0 = 3), "debug_skip" (profiling only) */
int  gsx_ctx_set_param(gsx_ctx *ctx, const char *name, double value);

/* raw device memory for hosts that have no other allocator (bench without torch) */
int gsx_dev_malloc(gsx_ctx *ctx, size_t bytes, void **dptr);
int gsx_dev_free(gsx_ctx *ctx, void *dptr);
/* page-locked host memory (hipHostMalloc) for staging buffers that host routines fill and the device reads at link rate: the lazy
 * DataProcessor gathers `coords` (data_processor.py:38,139) straight into one, once per process */
int gsx_host_pinned_alloc(gsx_ctx *ctx, size_t bytes, void **hptr);
int gsx_host_pinned_free(gsx_ctx *ctx, void *hptr);
int gsx_dev_upload(gsx_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
int gsx_dev_download(gsx_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);
int gsx_dev_copy(gsx_ctx *ctx, void *dst_dev, const void *src_dev, size_t bytes);  /* device to device, asynchronous */
int gsx_dev_upload_async(gsx_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);  /* enqueue only */
int gsx_dev_memset(gsx_ctx *ctx, void *dst_dev, int value, size_t bytes);                    /* enqueue only */
/* bulk copies of PAGEABLE host memory (a numpy array), threaded (csrc/host_rows.hip).  Upload: the caller's pages are pinned IN
 * PLACE, 32 MiB at a time, by a few lanes that run ahead of the DMA (hipHostRegister on the lane's thread -> hipMemcpyAsync on
 * its stream -> hipHostUnregister two chunks later): link rate on the FIRST copy of a buffer, where hipMemcpy of pageable memory
 * pins, copies, pins ... (24-30 GB/s; its pinned-range cache is emptied by any munmap in the process).  A range the driver will
 * not pin, and every transfer below 128 / 256 MiB, goes through lanes that fill / drain one pinned 8 MiB staging buffer while the
 * DMA of their other one is in flight; large downloads pin the DESTINATION in place the same way (touch its pages first:
 * _lib.prefault does that on a helper thread while the device works).  Synchronous; waits for the
 * context's stream first.  What the writers move: the 2.48 GB splat table up, 240 MB of texels down. */
int gsx_dev_upload_staged(gsx_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
int gsx_dev_download_staged(gsx_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);

/* ---- Host-side row operations around every filter -- */
/*
 * out[r*ncols + c] = *(float*)((char*)rows + r*row_bytes + offsets[c]) -- replaces
 * data_processor.py:38,139 (np.column_stack of the x,y,z fields of the structured array).
 * Threaded; rows are opaque bytes.
 */
int gsx_host_gather_f32(const void *rows, int64_t row_bytes, int64_t n, const int64_t *offsets,
                        int ncols, float *out);
/* the same gather with a COLUMN-major result, out[c*n + r]: one contiguous float32 column per field, as the writers upload them
 * (formats/compressed_ply.py:200-241 reads `data[name]` per column; formats/sog.py likewise) */
int gsx_host_gather_columns_f32(const void *rows, int64_t row_bytes, int64_t n, const int64_t *offsets,
                                int ncols, float *out);
/*
 * Stable compaction of the rows with mask[r] != 0 -- replaces data_processor.py:114,149
 * (self.data = vertices[mask]).  out must hold out_rows rows; *n_out = number of survivors
 * (error if it exceeds out_rows).  Threaded.
 */
int gsx_host_compact_rows(const void *rows, int64_t row_bytes, int64_t n, const uint8_t *mask,
                          void *out, int64_t out_rows, int64_t *n_out);
/* the same compaction from the survivor LIST the device chain returns (strictly ascending row indices): out[i] = rows[idx[i]] --
 * `self.data = vertices[mask]` (data_processor.py:114,149) without building the boolean mask first.  Threaded. */
int gsx_host_take_rows(const void *rows, int64_t row_bytes, int64_t n, const uint32_t *idx, int64_t n_idx, void *out);

/*
 * Device-resident filter chain (device half): stable compaction of (n,3) float32 rows by a device
 * mask -- the device-side `vertices[mask]` of data_processor.py:114,149 for the coordinates only.  orig_dev (nullable =
 * identity) / orig_out_dev carry the index into the table the chain started from, so that the host compacts its
 * 248-byte rows once, after the last filter.  *n_out = survivors (one small synchronisation).
 */
int gsx_compact_rows_dev(gsx_ctx *ctx, const float *rows_dev, const uint32_t *orig_dev, const uint8_t *mask_dev, int64_t n,
                         float *rows_out_dev, uint32_t *orig_out_dev, int64_t *n_out);

/*
 * data_processor.py:233-274,316-343 (add_rgb_from_sh / _compute_rgb_from_sh) for ONE colour channel:
 * u8((clip(0.5 + f_dc * C0, 0, 1) ** (1/2.2)) * 255) in numpy's float32 arithmetic.  The power is evaluated in float64 on
 * the device with a rounding certificate (see gsx_sog_positions): uncertain_out[i] = 1 marks the (~1e-4) elements the
 * CALLER evaluates with numpy's own expression.  Byte-identical colours.
 */
int gsx_rgb_from_sh(const float *f_dc, int64_t n, uint8_t *out, uint8_t *uncertain_out);
int gsx_rgb_from_sh_dev(gsx_ctx *ctx, const float *f_dc_dev, int64_t n, uint8_t *out_dev, uint8_t *uncertain_dev);
/* the same colours with the uncertain elements as a LIST of their indices (unordered; `cap` entries, *count keeps counting past
 * cap: the caller then falls back to the flag form) instead of one flag byte per value: for a 10M-splat table the 30 MB of flags
 * cost more to bring back and scan on the host (8 ms) than the colours themselves */
int gsx_rgb_from_sh_list(const float *f_dc, int64_t n, uint8_t *out, uint32_t *list_out, int64_t cap, int64_t *count_out);
int gsx_rgb_from_sh_list_dev(gsx_ctx *ctx, const float *f_dc_dev, int64_t n, uint8_t *out_dev, uint32_t *list_dev, int64_t cap,
                             uint32_t *count_dev);
/*
 * Host row helpers of the two table-shaping methods (threaded, no device code):
 *   gsx_host_zero_columns   -- data_processor.py:276-314 cap_sh_degree: `self.data[f_rest_i] = 0.0` for the columns above the
 *                              kept degree, ONE pass over the rows instead of up to 45 strided column fills;
 *   gsx_host_append_columns -- data_processor.py:262-274: the table widened by (red, green, blue) u1 fields, one pass instead
 *                              of one strided copy per field.  extra: n x extra_bytes row-major.
 */
int gsx_host_zero_columns(void *rows, int64_t row_bytes, int64_t n, const int64_t *offsets, int ncols);
int gsx_host_append_columns(const void *rows, int64_t row_bytes, int64_t n, const uint8_t *extra, int64_t extra_bytes,
                            void *out, int64_t out_row_bytes);
/* both steps at once -- `self.data = vertices[mask]` (data_processor.py:114,149) then the widened copy of add_rgb_from_sh
 * (:262-274), which is what the reference's converter does before every writer that needs colours (converter.py:243-252): output
 * row j = source row idx[j] + the extra_bytes of THAT source row (extra: n x extra_bytes, indexed like the source table; idx strictly
 * ascending).  One pass over the survivors instead of two copies of the table. */
int gsx_host_take_rows_append(const void *rows, int64_t row_bytes, int64_t n, const uint32_t *idx, int64_t n_idx,
                              const uint8_t *extra, int64_t extra_bytes, void *out, int64_t out_row_bytes);
/* ... and cap_sh_degree's column fill (data_processor.py:310-313 `self.data[f_rest_i] = 0.0`) in the same pass: zero_offsets = byte
 * offsets of nzero 4-byte fields to zero in every OUTPUT row; extra may be NULL with extra_bytes 0 (no columns appended).  The lazy
 * class's whole table shaping -- compaction, SH cap, colours -- is one read of the survivors and one write of the new table. */
int gsx_host_take_rows_shape(const void *rows, int64_t row_bytes, int64_t n, const uint32_t *idx, int64_t n_idx,
                             const uint8_t *extra, int64_t extra_bytes, const int64_t *zero_offsets, int nzero, void *out,
                             int64_t out_row_bytes);

/*
 * The O(N) row filters that run before density / SOR (converter.py:196-203), as device masks over the chain's rows --
 * SURVEY.md 8(f) rank 4.  gsx_mask_bbox_dev replaces crop_by_bbox's six comparisons (data_processor.py:217-224);
 * bounds6 = {min_x,min_y,min_z,max_x,max_y,max_z} on the host, compared in f64 (pass float32-rounded values for Python
 * floats, which numpy treats as weak scalars).  gsx_mask_ge_dev replaces apply_alpha_filter's
 * `self.data['opacity'] >= logit_thresh` (:210, an f64 comparison because logit_thresh is a np.float64): vals_dev is
 * the float32 column of the ORIGINAL table, orig_dev (nullable = identity) the chain's survivor list.
 */
int gsx_mask_bbox_dev(gsx_ctx *ctx, const float *rows_dev, int64_t n, const double *bounds6, uint8_t *mask_dev);
int gsx_mask_ge_dev(gsx_ctx *ctx, const float *vals_dev, const uint32_t *orig_dev, int64_t n, double threshold,
                    uint8_t *mask_dev);

/* ---- Statistical Outlier Removal --------------------------------------- */
/*
 * KNN mean distance -- replaces data_processor.py:156-173 (cKDTree build + chunked
 * query(k+1) + row mean) and the Taichi kernel gpu_ops.py:98-176 / its host prep
 * :193-256.  For the queries [q_begin, q_begin+q_count) of the n_ref reference
 * points writes mean_out[i - q_begin] = (float) mean of the k nearest neighbour
 * distances (self excluded), bit-identical to the reference's cKDTree path.
 */
int gsx_sor_knn_dev(gsx_ctx *ctx, const float *x, const float *y, const float *z, int64_t stride,
                    int64_t n_ref, int64_t q_begin, int64_t q_count, int k, int algo,
                    float *mean_out_dev, gsx_sor_info *info /* nullable; forces a sync if given */);
/*
 * Multi-GPU building block: the same KNN over the whole cloud of n points, but
 * only for the queries of share `share` of `nshares`.  The reference already treats queries as
 * independent units -- data_processor.py:167-173 loops over 50 000-query chunks of one tree --
 * here a share is a contiguous range of the grid's bricks, i.e. a spatial slab (an index range
 * for the brute-force algorithm).  mean_out_dev has n entries in ORIGINAL order: the share's
 * queries are written, every other entry is set to +0.0f, so the shares of all ranks combine
 * with one sum all-reduce into exactly what gsx_sor_knn_dev computes for q = [0, n).
 */
int gsx_sor_knn_share_dev(gsx_ctx *ctx, const float *x, const float *y, const float *z, int64_t stride,
                          int64_t n, int k, int algo, int share, int nshares, float *mean_out_dev,
                          gsx_sor_info *info /* nullable; forces a sync if given */);
/* Debug / tests: the brick plan of the context's last grid KNN call (context parameter brick_plan).
 * grid[8] = nx, ny, nz, plan (1: the planned bricks ran), bricks, 0, 0, 0; origin[4] = ox, oy, oz, 1/h;
 * list (nullable, room for cap entries of two words): {bundle of 2x2 query rows, first | last << 16 quarter-cell slab}. */
int gsx_sor_debug_brick_plan(gsx_ctx *ctx, int32_t *grid, float *origin, uint32_t *list, int64_t cap);
/* Debug / tests: the work queues of the context's last grid KNN call, in the order knn_brick, knn_brick (second batches),
 * knn_ring, knn_ring_fast: ctr[4][8] = final tail counters of the eight groups, items[4], blocks[4] = workgroups per launch. */
int gsx_sor_debug_work_queue(gsx_ctx *ctx, uint32_t *ctr, int64_t *items, int32_t *blocks);
/* Debug / tests: which stage of the Morton-tree path (csrc/sor_tree.hip) answered, and the leaves, of the context's last tree
 * run.  counters[16] = n, leaves, fail_count (queries knn_leaf handed to knn_tree_near), fail2_count (... knn_tree_near handed
 * to knn_tree_query), max_leaf (set by adaptive mode's guard only), leaf capacity in force, 0, 0, defer_why[0..7] (knn_tree_near's
 * reasons: 0 more than 512 cover cells, 1 a cell of more than 4096 points, 2 buffer full, 3 / 4 fewer than k points inside the
 * last radius tried / a known bound, 5-7 reason 1 by attempt).  keys / leafstart (nullable, room for cap entries each): the n
 * sorted Morton keys and the leaves + 1 leaf starts.  *n_out, *leaves_out (nullable) are set before cap is checked.  Fails when
 * no tree run has happened on the context or cap is too small.  Synchronises; launches nothing. */
int gsx_sor_debug_tree(gsx_ctx *ctx, uint32_t *counters, uint64_t *keys, uint32_t *leafstart, int64_t cap, int64_t *n_out,
                       int64_t *leaves_out);
/* Diagnostic builds (-DGSX_WAVE_STAMPS) only: per-wave records of knn_brick (kernel 0) and knn_ring_fast (kernel 1) of the
 * context's last grid KNN call, 16 words each (csrc/sor_grid_params.h); tools/wave_stamps.py prints them. */
int gsx_sor_debug_wave_stamps(gsx_ctx *ctx, int kernel, uint64_t *out, int64_t cap, int64_t *count);
/* Tests: the grid's host-side decisions (csrc/grid_policy.h), callable without a GPU (tests/test_grid_policy_host.py).
 * Points per cell for k neighbours and n reference points: tuned = 0 the base rule (what the slab plan estimates its halo
 * with), 1 the rule the grid uses when the context's grid_points_per_cell is 0. */
double gsx_sor_debug_points_per_cell(int k, int64_t n, int tuned);
/* The deferred bricks `bricks[count]` (ids (bz * nby + by) * nbx + bx) rewritten group by group, largest group first;
 * group_sizes[8] and *n_groups receive the groups. */
int gsx_sor_debug_group_bricks(uint32_t *bricks, int64_t count, int nbx, int nby, int nbz, uint32_t *group_sizes, int32_t *n_groups);
/* Sizing of one refinement round: the clip around the group's queries, the density probe's grid and the cell edge its histogram
 * suggests (0 = the box-volume edge h_est stays). */
typedef struct gsx_refine_sizing_in {
    float    qb_lo[3], qb_hi[3];     /* box of the group's queries                                              */
    uint32_t sub_queries, n_sub;     /* queries in the box; points gathered around them                          */
    double   pts_per_cell;
    float    parent_h;               /* cell edge of the level that deferred the bricks                          */
    int32_t  adaptive;               /* the context's adaptive mode: 1 clips and probes                          */
    uint32_t hist[32];               /* the probe's point-weighted histogram of log2(points per bin)             */
    double   bin_vol;                /* volume of one probe bin                                                  */
} gsx_refine_sizing_in;
typedef struct gsx_refine_sizing_out {
    int32_t nd3, probe_g;            /* axes with an extent; probe bins per axis (0: no probe)                   */
    double  h_est, margin, cert;
    float   clip_lo[3], clip_hi[3], r_cert;   /* r_cert = 0: no clipping                                         */
    double  h_hint;                  /* 0 when probe_g is 0: the histogram is not looked at                      */
} gsx_refine_sizing_out;
int gsx_sor_debug_refine_sizing(const gsx_refine_sizing_in *in, gsx_refine_sizing_out *out);
/* Debug / tests: the device functions beneath every mean distance (csrc/knn_common.h), called on the caller's inputs by
 * csrc/knn_probe.hip -- the same inline functions the KNN kernels call, not copies (tests/test_knn_epilogue_gpu.py).
 * Root: out[i] = the float64 square root of in[i] as knn_brick's and knn_anyk's epilogues take it (sqrt_rn_dist2; defined
 * for 0 and [2^-298, 2^260), what a squared distance of float32 coordinates can be) or as every other epilogue and the
 * SPZ / compressed-PLY readers take it (__dsqrt_rn). */
enum { GSX_PROBE_ROOT_DIST2 = 0, GSX_PROBE_ROOT_DSQRT = 1 };
int gsx_knn_probe_root_dev(gsx_ctx *ctx, const double *in_dev, int64_t n, int mode, double *out_dev);
/* The short root of knn_brick's certified epilogue (sqrt_short_dist2: no residual correction; same domain) or its seed alone:
 * out[i] = v_rsq_f64(max(in[i], 1e-300)), whose relative error against 1 / sqrt decides the short root's. */
enum { GSX_PROBE_SHORT_ROOT = 0, GSX_PROBE_SHORT_SEED = 1 };
int gsx_knn_probe_root_short_dev(gsx_ctx *ctx, const double *in_dev, int64_t n, int mode, double *out_dev);
/* Mean: d2_dev holds m rows of `stride` >= k ascending squared distances of a query's neighbours (the query itself is not
 * in the row); out_dev[r] = (float)(sum of the roots of row r's first k entries / k), summed the way `form` does:
 *   NET    mean_from_net<cap>: cap = a list length of knn_brick / knn_leaf (8, 12, 16, ... 56, 64), k <= cap; row entries
 *          k .. cap-1 are loaded into the list as the further neighbours they are in the kernels (+inf past the row);
 *   LIST   mean_from_list<cap>: cap = a capacity of knn_brick's bubble-insert variant / knn_brute (9, 17, 26, 33, 51, 65),
 *          k <= cap - 1; entry 0 of the list is the query (squared distance 0);
 *   LE128  __dsqrt_rn of an LDS list, then pairwise_sum_le128 by one lane (knn_ring, knn_ring_fast, the tree's fallbacks), k <= 128;
 *   NP     sqrt_rn_dist2 of an LDS list, then pairwise_sum_np<5> (knn_anyk), k <= 1000;  cap is ignored by LE128 and NP.
 * A form or capacity that no kernel instantiates is refused. */
enum { GSX_PROBE_MEAN_NET = 0, GSX_PROBE_MEAN_LIST = 1, GSX_PROBE_MEAN_LE128 = 2, GSX_PROBE_MEAN_NP = 3 };
int gsx_knn_probe_mean_dev(gsx_ctx *ctx, const double *d2_dev, int64_t m, int64_t stride, int k, int form, int cap,
                           float *out_dev);
/*
 * np.mean / np.std / threshold -- replaces data_processor.py:176-178 and
 * gpu_ops.py:259-261 with numpy's exact float32 arithmetic (8192-element buffered
 * pairwise sums, float64 division).  stats_dev[0..2] = mean, std, threshold.
 */
int gsx_sor_stats_dev(gsx_ctx *ctx, const float *mean_dists_dev, int64_t n, double threshold_factor,
                      float *stats_dev);
/* mask = mean_dists < threshold (strict) -- data_processor.py:180, gpu_ops.py:263 */
int gsx_sor_mask_dev(gsx_ctx *ctx, const float *mean_dists_dev, int64_t n, const float *threshold_dev,
                     uint8_t *mask_out_dev);

/* ---- multi-GPU SOR on one node: RCCL + the slab exchange ----
 * The reference has no distributed path: its queries are independent units over one reference set
 * (data_processor.py:167-173, 50 000-query chunks of one cKDTree) and its threshold is numpy's f32
 * mean/std over the whole mean-distance array (:176-178).  One process per GPU, splats sharded by index; the
 * host (3dgsconverter_amd/dist.py: slab_sor) drives these entry points; DESIGN.md section 7 has the protocol.
 *
 * gsx_comm_*: the collectives of the data path, on the context's stream.  Two transports behind the same calls
 * (csrc/comm.hip): "rccl" -- librccl dlopen'ed at first use, plain ncclAllReduce / ncclAllGather / grouped ncclSend +
 * ncclRecv over xGMI, one rank per GPU (the product) -- and "hostwire" -- POSIX shared-memory outboxes for ranks that SHARE
 * a GPU, which RCCL refuses (the full N-rank choreography on a one-GPU box: tests, `bench.py --gpus N` there).  The unique
 * id is created on rank 0 (under GSX_COMM_TRANSPORT=hostwire it names the shared-memory job) and handed to the other
 * ranks by the launcher (128 bytes; 3dgsconverter_amd/launch.py: a file next to the job). */
enum { GSX_COMM_F32_MAX = 0, GSX_COMM_F32_SUM = 1, GSX_COMM_I64_SUM = 2, GSX_COMM_F64_MAX = 3, GSX_COMM_I64_MIN = 4 };
int gsx_comm_unique_id(void *out128);
int gsx_comm_init(gsx_ctx *ctx, int rank, int world, const void *id128);
int gsx_comm_destroy(gsx_ctx *ctx);
int gsx_comm_abort(gsx_ctx *ctx);                 /* this rank gives up: peers waiting on it fail at once (hostwire) */
int gsx_comm_transport(gsx_ctx *ctx);             /* 0 = no communicator, 1 = rccl, 2 = hostwire */
int gsx_comm_rank(gsx_ctx *ctx, int *rank_out, int *world_out);   /* (0, 1) without a communicator */
int gsx_comm_barrier(gsx_ctx *ctx);               /* all stream work of every rank up to here has completed */
/* in place on device memory; kind: GSX_COMM_* above */
int gsx_comm_all_reduce(gsx_ctx *ctx, void *buf_dev, int64_t count, int kind);
int gsx_comm_all_gather(gsx_ctx *ctx, const void *send_dev, void *recv_dev, int64_t bytes_per_rank);
/* grouped ncclSend/ncclRecv: offsets and counts (host arrays, one entry per peer) in elements of elem_bytes
 * (1, 4, 8 or 12 = a row of three floats) */
int gsx_comm_all_to_all_v(gsx_ctx *ctx, const void *send_dev, const int64_t *send_off, const int64_t *send_cnt,
                          void *recv_dev, const int64_t *recv_off, const int64_t *recv_cnt, int elem_bytes);
/* nseg <= 2 such exchanges in ONE group (own rows and halo rows of the slab partition): entry [s * world + p] of the four
 * arrays = segment s to / from peer p */
int gsx_comm_all_to_all_segs(gsx_ctx *ctx, const void *send_dev, void *recv_dev, int nseg, const int64_t *send_off,
                             const int64_t *send_cnt, const int64_t *recv_off, const int64_t *recv_cnt, int elem_bytes);

/* ---- the slab step as ONE call (what bench.py --gpus N and dist_slab.LibSlab drive) ----
 * Why a rank may decline a step (status != 0; decided from all-gathered data, so every rank declines together and the
 * caller's replicated exchange -- dist.replicated_sor, exact for any cloud -- takes over): */
enum { GSX_SLAB_OK = 0, GSX_SLAB_EMPTY = 1, GSX_SLAB_NONFINITE = 2, GSX_SLAB_SMALL_SHARD = 3, GSX_SLAB_NO_STRUCTURE = 4 };
typedef struct gsx_slab_plan_t {
    int32_t status, world, rank, axis, halo_bins;
    float   lo, hi;                  /* binned range of the partition axis (the all-reduced box words)          */
    float   plane_lo, plane_hi;      /* this rank holds EVERY point of the cloud between these (+-inf at the ends) */
    int32_t cut[17];                 /* slab s owns the bins [cut[s], cut[s+1]) of 4096                          */
    int64_t n_local, n_total, n_own, n_halo, n_send, halo_total;
    int64_t sizes[16];               /* index-shard size of every rank                                           */
    int64_t own_cnt[16], halo_cnt[16], own_off[16], halo_off[16];       /* rows this rank sends slab s ...        */
    int64_t in_own[16], in_halo[16], r_own_off[16], r_halo_off[16];     /* ... and receives from source q         */
} gsx_slab_plan_t;
typedef struct gsx_slab_step_t {
    int32_t status;                  /* = plan.status                                                            */
    gsx_slab_plan_t plan;
    const uint8_t *mask_dev;         /* u8[n_local]: survivor mask of the local index range                      */
    const float   *mean_dists_dev;   /* f32[n_local], index order (context workspace: valid until the next step) */
    const float   *stats_dev;        /* mean, std, threshold: numpy's bits for the WHOLE cloud                    */
    const int64_t *uncertain_dev;    /* all-reduced number of queries the slabs could not certify: read it (one
                                        synchronisation) before trusting the buffers; non-zero = use the fallback */
} gsx_slab_step_t;
/* host-only: the plan from the step's gathered words (box words [0,7), histograms from word 8) */
int gsx_slab_plan(const uint32_t *words, int world, int rank, int64_t n_local, int k, double halo_cells, gsx_slab_plan_t *out);
/* rows_dev: this rank's (n_local,3) float32 index shard; replaces data_processor.py:156-180 across ranks */
int gsx_sor_slab_step_dev(gsx_ctx *ctx, const float *rows_dev, int64_t n_local, int k, double threshold_factor,
                          double halo_cells, uint8_t *mask_out_dev /* nullable */, gsx_slab_step_t *out);

/* out7_dev = max over the points of (-x,-y,-z,x,y,z) and a non-finite flag: ONE float32 max all-reduce gives the
 * global bounding box (the per-rank half of gpu_ops.py:203-206) */
int gsx_slab_bbox_dev(gsx_ctx *ctx, const float *x, const float *y, const float *z, int64_t stride, int64_t n,
                      float *out7_dev);
/* 4096-bin histogram (uint32) of the partition coordinate = the longest axis of the box in bbox7_dev (read ON THE DEVICE:
 * no host round trip after the bbox all-reduce).  All-gathered, the histograms give every rank the equal-count slab
 * cuts AND every (source, destination) row count, since slab membership is decided by bin index. */
int gsx_slab_hist_dev(gsx_ctx *ctx, const float *x, const float *y, const float *z, int64_t stride, int64_t n,
                      const float *bbox7_dev, uint32_t *hist4096_dev);
/* Slab s OWNS the bins [cut[s], cut[s+1]) of the axis range [lo, hi] and also receives, as REFERENCE-ONLY rows, the
 * bins within halo_bins of them.  Rows (3 floats) are written to send_dev starting at start_off[2*world] (HOST array:
 * first row of slot 2s = rows owned by slab s, slot 2s+1 = halo copies for slab s; cursor_dev[2*world] is device scratch,
 * zeroed by the call), send_src_dev[row] = local index of each own row.  planes_out (host, 2*world floats, nullable):
 * coordinates between which slab s holds EVERY point of the cloud. */
int gsx_slab_partition_dev(gsx_ctx *ctx, const float *x, const float *y, const float *z, int64_t stride, int64_t n,
                           int world, int axis, float lo, float hi, const int32_t *cut, int halo_bins,
                           const uint32_t *start_off, uint32_t *cursor_dev, float *send_dev, uint32_t *send_src_dev,
                           float *planes_out);
/* exact KNN mean distance of the first n_own rows against all n_own + n_halo rows (the halo rows are never
 * queries); kth_d2_dev[i] = squared distance of query i's (k+1)-th neighbour INCLUDING itself, i.e. its k-th other */
int gsx_sor_knn_slab_dev(gsx_ctx *ctx, const float *rows_dev, int64_t n_own, int64_t n_halo, int k,
                         float *mean_out_dev, double *kth_d2_dev);
/* *n_uncertain_dev = number of queries whose k-th neighbour is not provably among the rows this rank holds:
 * kth_d2 > min(coord - open_lo, open_hi - coord)^2 (open_* = the slab's planes_out entries, +-inf at the cloud's ends).
 * The counter is 8 bytes (uint32 count + a zeroed upper word, so that it can be all-reduced as an int64); set by the call */
int gsx_slab_certify_dev(gsx_ctx *ctx, const float *coord, int64_t stride, int64_t n_own, const double *kth_d2_dev,
                         float open_lo, float open_hi, uint32_t *n_uncertain_dev);
/* out_dev[send_src_dev[p]] = recv_dev[p]: mean distances come back in the order the rows were sent */
int gsx_slab_unpermute_dev(gsx_ctx *ctx, const float *recv_dev, const uint32_t *send_src_dev, int64_t n, float *out_dev);
/* numpy's float32 reduction (data_processor.py:176-177) is "pairwise inside 8192-element pieces, pieces added
 * sequentially": piece sums of a piece-aligned sub-range can be computed where the data lives ... */
int gsx_sor_piece_sums_dev(gsx_ctx *ctx, const float *a_dev, int64_t n, const float *mean_dev /* NULL: plain sum,
                           else sum of (a - *mean)^2 */, float *piece_out_dev);
/* ... and combined anywhere: mode 0: stats[0] = mean; mode 1: stats[1] = std, stats[2] = mean + factor * std */
int gsx_sor_stats_from_pieces_dev(gsx_ctx *ctx, const float *pieces_dev, int64_t npieces, int64_t n_total, int mode,
                                  double threshold_factor, float *stats_dev);

/* host buffers, one GPU: the whole of filter_sor_gpu (gpu_ops.py:193-263).
 * mean_out (n floats) and stats_out (3 floats) may be NULL. */
int gsx_sor_filter(const float *x, const float *y, const float *z, int64_t stride, int64_t n,
                   int k, double threshold_factor, int algo, uint8_t *mask_out, float *mean_out,
                   float *stats_out, gsx_sor_info *info);

/* ---- voxel-density filter ---------------------------------------------- */
/*
 * Voxel occupancy -- replaces data_processor.py:38-52 (floor(xyz / voxel) keys,
 * np.unique(axis=0) counts, dense = count >= min_points).  Returns the number of
 * occupied voxels and the dense voxels (lexicographically sorted like np.unique)
 * in dense_keys_out (3 x int64 each) / dense_counts_out, at most dense_cap.
 */
int gsx_density_voxels(const float *x, const float *y, const float *z, int64_t stride, int64_t n,
                       double voxel_size, int64_t min_points, int64_t dense_cap,
                       int64_t *n_unique_out, int64_t *n_dense_out, int64_t *dense_keys_out,
                       int64_t *dense_counts_out);
/*
 * Per-point membership -- replaces data_processor.py:111-114: mask[i] = voxel(i) in kept set.
 * kept_keys: n_kept x 3 int64.
 */
int gsx_density_mask(const float *x, const float *y, const float *z, int64_t stride, int64_t n,
                     double voxel_size, const int64_t *kept_keys, int64_t n_kept, uint8_t *mask_out);

/* device-resident variants (dense_* outputs are HOST arrays; the kept set is a HOST array) */
int gsx_density_voxels_dev(gsx_ctx *ctx, const float *x, const float *y, const float *z, int64_t stride,
                           int64_t n, double voxel_size, int64_t min_points, int64_t dense_cap,
                           int64_t *n_unique_out, int64_t *n_dense_out, int64_t *dense_keys_out,
                           int64_t *dense_counts_out);
/*
 * Multi-GPU density filter (the reference is single-process): rank r counts the voxels of ITS index
 * shard and exports every occupied voxel as an absolute int64 key triple + int64 count into DEVICE buffers
 * (gsx_density_hist_dev; cap entries each, arbitrary order; *n_unique_out = entries written), the lists are all-gathered
 * (gsx_comm_*), and gsx_density_merge_dev adds the counts of equal keys of the m gathered entries in a hash table and
 * returns what gsx_density_voxels would have returned for the whole cloud: data_processor.py:43-52 with
 * min_points = int(N_global * thr / 100) (:48).  The host BFS (:59-108) and gsx_density_mask_dev on the local rows follow.
 */
int gsx_density_hist_dev(gsx_ctx *ctx, const float *x, const float *y, const float *z, int64_t stride, int64_t n,
                         double voxel_size, int64_t cap, int64_t *n_unique_out, int64_t *keys3_dev, int64_t *counts_dev);
int gsx_density_merge_dev(gsx_ctx *ctx, const int64_t *keys3_dev, const int64_t *counts_dev, int64_t m, int64_t min_points,
                          int64_t dense_cap, int64_t *n_unique_out, int64_t *n_dense_out, int64_t *dense_keys_out,
                          int64_t *dense_counts_out);
/* The whole filter on device-resident rows in ONE call (data_processor.py:38-114): occupancy, dense voxels, their
 * 6-connected clusters (one workgroup: at most n / min_points <= ~1000 voxels are dense), the keep rule (:95-106) and the
 * membership mask -- one synchronisation, at the end.  box6 (host, nullable): minima then maxima of a superset of the rows
 * (saves the box pass and its synchronisation).  info->status: GSX_DENSITY_OK (mask_out_dev holds the mask),
 * GSX_DENSITY_EMPTY (no dense voxel: the filter removes everything, :54-57), GSX_DENSITY_HOST (more than 1024 dense voxels,
 * or two clusters tie for the largest without keep_multicluster -- which one survives is the reference's python-set
 * iteration order).  On GSX_DENSITY_HOST nothing was applied: gsx_density_filter_large_dev below takes any number of dense
 * voxels and answers GSX_DENSITY_HOST for the tie alone, which gsx_density_voxels_dev + processing/clusters.py +
 * gsx_density_mask_dev then decide. */
enum { GSX_DENSITY_OK = 0, GSX_DENSITY_EMPTY = 1, GSX_DENSITY_HOST = 2 };
typedef struct gsx_density_info {
    int32_t status;
    int64_t n_unique, n_dense, n_kept_voxels, kept_clusters, largest;
} gsx_density_info;
int gsx_density_filter_dev(gsx_ctx *ctx, const float *x, const float *y, const float *z, int64_t stride, int64_t n,
                           double voxel_size, int64_t min_points, int keep_multicluster, const float *box6,
                           uint8_t *mask_out_dev, gsx_density_info *info);
int gsx_density_mask_dev(gsx_ctx *ctx, const float *x, const float *y, const float *z, int64_t stride,
                         int64_t n, double voxel_size, const int64_t *kept_keys, int64_t n_kept,
                         uint8_t *mask_out_dev);
/* The same call with no cap on the number of dense voxels -- replaces data_processor.py:57-112 (the set of dense voxels, the
 * BFS over their six face neighbours, the keep rule, the per-point membership) for any size: the 6-connected components are
 * found on the voxel hash table itself by a lock-free union-find (a fixed number of launches, whatever a cluster's diameter).
 * Same contract as gsx_density_filter_dev (box6, one synchronisation); GSX_DENSITY_HOST only for a tie for the largest cluster
 * without keep_multicluster. */
int gsx_density_filter_large_dev(gsx_ctx *ctx, const float *x, const float *y, const float *z, int64_t stride, int64_t n,
                                 double voxel_size, int64_t min_points, int keep_multicluster, const float *box6,
                                 uint8_t *mask_out_dev, gsx_density_info *info);
/* Clusters of a HOST list of m distinct absolute voxel keys (3 x int64 each) -- of data_processor.py:57-112 the part that
 * needs no rows, :57-108 (dense_set, BFS, sort by size, keep rule): keep_out[i] = 1 when key i belongs to a kept cluster, in
 * input order; info->kept_clusters, largest, n_kept_voxels and status as above (GSX_DENSITY_HOST: a tie without
 * keep_multicluster, keep_out is undefined).  The keys may span at most 2^31 - 1 voxels on an axis. */
int gsx_voxel_clusters(const int64_t *keys3, int64_t m, int keep_multicluster, uint8_t *keep_out, gsx_density_info *info);
int gsx_voxel_clusters_dev(gsx_ctx *ctx, const int64_t *keys3, int64_t m, int keep_multicluster, uint8_t *keep_out,
                           gsx_density_info *info);
/* Stage clocks (ms) of the context's last gsx_density_filter_large_dev / gsx_voxel_clusters_dev call, recorded while
 * gsx_ctx_set_timing is on: table fill, init, hook, flatten + sizes, reduce, membership. */
#define GSX_DENSITY_STAGES 6
int gsx_density_stage_clocks(gsx_ctx *ctx, double *ms_out);

/* ---- K-Means codebook (SOG writer) ------------------------------------- */
/*
 * Lloyd iterations with an injected initialisation -- replaces _kmeans_taichi
 * (gpu_ops.py:178-191) and its kernels k_means_assign (:57-73) / k_means_update
 * (:75-96): exactly max_iter x (assign, update), empty cluster -> 0, returned
 * labels are one step older than the returned centroids.  data: n x d row-major.
 */
int gsx_kmeans_lloyd(const float *data, int64_t n, int d, int k, int max_iter,
                     const float *init_centroids, float *centroids_out, int32_t *labels_out);
/* nearest entry of a sorted codebook -- replaces quantize_to_codebook, formats/sog.py:408-419 */
int gsx_quantize_sorted_codebook(const float *vals, int64_t n, const float *codebook, int kcb,
                                 uint8_t *idx_out);

/*
 * Scalar (D = 1) K-Means codebook -- replaces the two places where the reference fits a 1-D codebook with scikit-learn's
 * k-means++-seeded MiniBatchKMeans: formats/sog.py:561 (MiniBatchKMeans(n_clusters=256, n_init='auto') over the flattened
 * SH palette, hard-wired) and processing/gpu_ops.py:48-52 (_kmeans_sklearn, what gpu_ops.kmeans runs for
 * formats/sog.py:402,443 when Taichi is absent or use_gpu=False).  Both are unseeded in the reference: the contract is
 * quality (inertia <= sklearn's on the same data), not bits.  Deterministic: sort + float64 prefix sums + `iters` Lloyd
 * steps on run boundaries from two companded starts (csrc/kmeans1d.hip).  centroids_out: k floats, ASCENDING;
 * labels_out (may be NULL): nearest centroid per value, ties to the lower index (gpu_ops.py:66-70);
 * inertia3_out (may be NULL): {chosen, uniform-bin start, equal-count-bin start}.  1 <= k <= 1024, values finite.
 */
int gsx_kmeans1d(const float *vals, int64_t n, int k, int iters, float *centroids_out, int32_t *labels_out,
                 double *inertia3_out);
/* start_mask: bit 0 = uniform-bin start, bit 1 = equal-count-bin start (0 = both); inertia3_host is a HOST array.
 * The slot of a start that start_mask leaves out is 0.0 (cleared on every call); with both starts the first wins unless
 * the second's inertia is strictly smaller. */
int gsx_kmeans1d_dev(gsx_ctx *ctx, const float *vals_dev, int64_t n, int k, int iters, int start_mask,
                     float *centroids_dev, int32_t *labels_dev, double *inertia3_host);

/*
 * Greedy k-means++ seeding (D^2 sampling, n_local_trials candidates per centroid, the one that lowers the potential most
 * wins) -- the initialisation of the reference's CPU path, scikit-learn's MiniBatchKMeans (processing/gpu_ops.py:48-52;
 * sklearn uses n_local_trials = 2 + int(ln k)).  The host draws the 1 + (k-1) * n_local_trials uniform numbers in [0,1)
 * (numpy's global stream, like sklearn); the device does the O(n d) passes (csrc/kmeans_pp.hip).  Follow with gsx_kmeans_lloyd.
 */
int gsx_kmeans_pp(const float *data, int64_t n, int d, int k, const double *uniforms, int n_local_trials, float *centroids_out);
int gsx_kmeans_pp_dev(gsx_ctx *ctx, const float *data_dev, int64_t n, int d, int k, const double *uniforms_host,
                      int n_local_trials, float *centroids_dev);

/* device-resident variants: centroids_dev holds the init on entry and the result on exit */
int gsx_kmeans_lloyd_dev(gsx_ctx *ctx, const float *data_dev, int64_t n, int d, int k, int max_iter,
                         float *centroids_dev, int32_t *labels_dev);
/*
 * nprob INDEPENDENT Lloyd problems of the same d and k in one call -- the SH palette of the SOG writer is 64 such problems
 * (formats/sog.py:536-552: `for i in range(num_chunks): ... kmeans(chunk, k_per_chunk, max_iter=10)`).  Rows concatenated:
 * problem p = rows [row_off[p], row_off[p+1]) of data_dev / labels_dev (row_off: HOST array of nprob + 1 offsets, row_off[0]
 * = 0), its k x d centroids at centroids_dev + p*k*d (init on entry, result on exit), labels local to the problem (0..k-1,
 * as gpu_ops.kmeans returns them; the writer adds the chunk's offset, sog.py:546-552).  Per problem the same kernels,
 * launch order and arithmetic as gsx_kmeans_lloyd_dev; for the matrix-core shapes (d in {9, 24, 45}, k >= 64) every
 * iteration of ALL problems is one set of launches (the problem is a grid dimension) instead of nprob x 6.
 */
int gsx_kmeans_lloyd_batch_dev(gsx_ctx *ctx, const float *data_dev, const int64_t *row_off, int nprob, int d, int k,
                               int max_iter, float *centroids_dev, int32_t *labels_dev);
int gsx_quantize_sorted_codebook_dev(gsx_ctx *ctx, const float *vals_dev, int64_t n,
                                     const float *codebook_dev, int kcb, uint8_t *idx_out_dev);

/* ---- SOG writer numeric core next to the codebooks ---- */
/* perm = np.lexsort((k0, k1, k2)): k2 is the primary key -- formats/sog.py:264 lexsort((z, y, x)).  Three stable radix
 * passes; -0.0 == +0.0 and NaNs last, like numpy.  perm_out: n uint32 */
int gsx_lexsort3(const float *k0, const float *k1, const float *k2, int64_t n, uint32_t *perm_out);
int gsx_lexsort3_dev(gsx_ctx *ctx, const float *k0, const float *k1, const float *k2, int64_t stride, int64_t n,
                     uint32_t *perm_out_dev);
/*
 * formats/sog.py:279-309 for ONE axis: v -> sign(v) log(|v| + 1) -> (l - log_min) / (log_max - log_min) * 65535 -> clip ->
 * uint16, and formats/sog.py:457-459: 255 / (1 + exp(-opacity)) -> clip -> uint8.  The reference evaluates log / exp with
 * numpy's float32 SIMD routines (not correctly rounded), so the device computes them in float64, brackets numpy's possible
 * float32 result (+-5 ulp for log, +-4 for exp) and emits the texel only when both ends of the bracket quantise to the same integer through
 * numpy's exact float32 sequence; uncertain_out[i] = 1 marks the (~1 %) elements the CALLER must evaluate with numpy's
 * own expression.  log_min / log_max: numpy's np.min / np.max of the transformed axis (the host obtains them from the few
 * values next to the extremes of v: the transform is monotone).  Result: byte-identical textures.
 */
int gsx_sog_positions(const float *v, int64_t n, float log_min, float log_max, uint16_t *out, uint8_t *uncertain_out);
int gsx_sog_positions_dev(gsx_ctx *ctx, const float *v_dev, int64_t n, float log_min, float log_max, uint16_t *out_dev,
                          uint8_t *uncertain_dev);
int gsx_sog_alpha(const float *opacity, int64_t n, uint8_t *out, uint8_t *uncertain_out);
int gsx_sog_alpha_dev(gsx_ctx *ctx, const float *opacity_dev, int64_t n, uint8_t *out_dev, uint8_t *uncertain_dev);

/* formats/sog.py:315-386: normalise the (n,4) float32 quaternion rows, flip to the positive hemisphere of the largest
 * component, scale by sqrt(2), quantise the three others to bytes; out4[i] = (c0, c1, c2, 252 + argmax), byte-exact */
int gsx_sog_quats(const float *rot_rows, int64_t n, uint8_t *out4);
int gsx_sog_quats_dev(gsx_ctx *ctx, const float *rot_rows_dev, int64_t n, uint8_t *out4_dev);

/* ---- the SOG writer on a DEVICE-RESIDENT splat table (csrc/sog_table.hip) ----
 * formats/sog.py:249-600 between the structured table and the RGBA texel arrays of its WebP images, without the host copies
 * the reference makes (`data_s = data[indices]` :265, the quaternion / SH `column_stack`s :315,:499-503, `np.concatenate` of
 * the 3N scalars :391,:434): the raw rows are uploaded once (gsx_dev_upload), every stage reads and writes HBM, only texels
 * (4 bytes per splat and image) and short lists of texels for the host's numpy come back.  Call order:
 * scan -> extremes -> order -> gather -> *_texels (+ gsx_kmeans1d_dev / gsx_kmeans_lloyd_batch_dev for the codebooks). */
#define GSX_SOG_FIELDS 59
typedef struct gsx_sog_layout {
    int64_t row_bytes;                 /* itemsize of the structured dtype: at most 512; ANY size up to 500 (the table widened by the
                                          three u1 colour fields of data_processor.py:262-274 has 251-byte rows: the kernels then
                                          assemble every field from two words of their LDS tile, and read up to 3 bytes past the
                                          last row -- rows_dev must be readable up to the next 4-byte boundary) */
    int32_t n_rest;                    /* f_rest columns present (0, 9, 24 or 45: sog.py:468-474) */
    int32_t offset[GSX_SOG_FIELDS];    /* byte offset of the float32 fields x y z | rot_0..3 | scale_0..2 | f_dc_0..2 | opacity |
                                          f_rest_0..44 inside a row (any offset; entries beyond 14 + n_rest are ignored) */
} gsx_sog_layout;
typedef struct gsx_sog_scan {
    float    vmin[3], vmax[3];         /* np.min / np.max of x, y, z (a -0.0 is reported as +0.0) */
    uint32_t nonfinite;                /* bit a: axis a holds a NaN or an infinity */
    uint32_t reserved;
    uint64_t rest_nonzero;             /* bit i: np.any(data['f_rest_i'] != 0) -- the band detection of sog.py:476-486 */
} gsx_sog_scan;
/* one pass over the n rows in table order: keys3_dev[a * n + i] = the uint32 whose unsigned order is numpy's sort order of
 * axis a's float32 value (-0.0 == +0.0, NaN last); *out (HOST) after one small synchronisation */
int gsx_sog_scan_dev(gsx_ctx *ctx, const void *rows_dev, const gsx_sog_layout *layout, int64_t n, uint32_t *keys3_dev,
                     gsx_sog_scan *out);
/* the values v <= lo3[a] (list 2a) and v >= hi3[a] (list 2a + 1) of every axis, from the key columns: the candidates for
 * np.min / np.max of the log-transformed axis (sog.py:287-288; numpy's float32 log is monotone only up to a few ulp, so the
 * host evaluates its own expression on the values within a small window of the extremes).  vals_out: HOST float[6][cap],
 * counts6_out: HOST, the true list lengths (entries beyond cap are dropped).  Synchronises. */
int gsx_sog_extremes_dev(gsx_ctx *ctx, const uint32_t *keys3_dev, int64_t n, const float *lo3, const float *hi3, int cap,
                         float *vals_out, int64_t *counts6_out);
/* perm = np.lexsort((z, y, x)) (sog.py:264) from the key columns: three stable radix passes */
int gsx_sog_order_dev(gsx_ctx *ctx, const uint32_t *keys3_dev, int64_t n, uint32_t *perm_out_dev);
/* `data_s = data[indices]` (sog.py:265) for the columns the writer reads, one pass: pos_dev f32[3][n] (x, y, z columns),
 * rot_dev f32[n][4] (the column_stack of :315), scale_dev / dc_dev f32[3][n] (= the np.concatenate of :391 / :434),
 * opacity_dev f32[n], sh_dev f32[n][d_sh] (the column_stack of :499-503; d_sh = 0, 9, 24 or 45; nullable for 0) */
int gsx_sog_gather_dev(gsx_ctx *ctx, const void *rows_dev, const gsx_sog_layout *layout, const uint32_t *perm_dev, int64_t n,
                       int d_sh, float *pos_dev, float *rot_dev, float *scale_dev, float *dc_dev, float *opacity_dev,
                       float *sh_dev);
/* Texel writers: out = `texels` x 4 bytes, the flat RGBA array the reference hands to write_webp (texels = width * height
 * >= n; the padding texels get the reference's fill value).  Lists: `cap` entries of two uint32 (texel index * 4 + channel,
 * the bits of the float32 input value) for the values whose float32 log / exp bracket straddles a rounding boundary -- the
 * caller evaluates numpy's own expression for those (see gsx_sog_positions) and patches the texel; *count_dev (uint32,
 * zeroed by the call) keeps counting past cap.
 *   means:  sog.py:279-312 -> means_l (low bytes of the u16 x, y, z, 255) and means_u (high bytes, 255); padding 255.
 *           log_min3 / log_max3 = numpy's np.min / np.max of the transformed axes (gsx_sog_extremes_dev), arg_min3 / arg_max3
 *           = a coordinate value per axis whose transform numpy evaluated to exactly that minimum / maximum (texels 0 / 65535
 *           for every copy of it without consulting the bracket)
 *   quats:  sog.py:315-386 -> (c0, c1, c2, 252 + argmax); padding 255
 *   codes:  sog.py:408-431 / :446-459 -> (codebook index of the three columns, 255 or -- opacity_dev given -- the sigmoid of
 *           the opacity as a byte); padding 0.  cols3_dev = f32[3][n], codebook_dev = kcb <= 256 ascending float32
 *   labels: sog.py:546-552,:600-606 -> palette label = labels_dev[i] + (i / chunk_rows) * k as (low byte, high byte, 0, 255) */
int gsx_sog_means_texels_dev(gsx_ctx *ctx, const float *pos_dev, int64_t n, int64_t texels, const float *log_min3,
                             const float *log_max3, const float *arg_min3 /* nullable */, const float *arg_max3 /* nullable */,
                             uint8_t *means_l_dev, uint8_t *means_u_dev, uint32_t *list_dev,
                             int64_t cap, uint32_t *count_dev);
int gsx_sog_quats_texels_dev(gsx_ctx *ctx, const float *rot_rows_dev, int64_t n, int64_t texels, uint8_t *out_dev);
int gsx_sog_codes_texels_dev(gsx_ctx *ctx, const float *cols3_dev, int64_t n, int64_t texels, const float *codebook_dev, int kcb,
                             const float *opacity_dev /* nullable */, uint8_t *out_dev, uint32_t *list_dev, int64_t cap,
                             uint32_t *count_dev);
int gsx_sog_labels_texels_dev(gsx_ctx *ctx, const int32_t *labels_dev, int64_t n, int64_t texels, int64_t chunk_rows, int k,
                              uint8_t *out_dev);
/* dst row i = src row idx_dev[i] (rows of row_floats float32): `s_data[idx]` of the codebooks' 50 000-sample (sog.py:397-400,
 * row_floats = 1) and the palette's initial centroids `data[np.random.choice(N, k)]` (gpu_ops.py:182) */
int gsx_gather_rows_dev(gsx_ctx *ctx, const float *src_dev, int row_floats, const int64_t *idx_dev, int64_t m, float *dst_dev);

/* ---- compressed-PLY writer numeric core ---- */
/*
 * formats/compressed_ply.py:245-291 _sort_morton_order: 10-bit-per-axis Morton codes inside the bounding box, groups of
 * equal code with more than 256 members re-sorted inside their own box, recursively.  order_out_dev: n uint32, the
 * `indices` array the reference sorts in place.  The sequence of codes is the reference's; splats with EQUAL code keep
 * ascending input index here, while np.argsort (not stable) leaves them in a build-dependent order.  *levels_out
 * (nullable) = recursion depth reached.  Coordinates must be finite.
 */
int gsx_morton_order_dev(gsx_ctx *ctx, const float *x_dev, const float *y_dev, const float *z_dev, int64_t stride, int64_t n,
                         uint32_t *order_out_dev, int *levels_out);
/*
 * compressed_ply.py:205-234 (chunk loop) with :293-341 (_normalize_and_pack_11_10_11, _normalize_and_pack_8888,
 * _pack_quaternions): one workgroup per 256-splat chunk.  cols14_dev: HOST array of 14 device columns of the ORIGINAL
 * table (float32, contiguous): x y z, scale_0..2, f_dc_0..2, alpha = sigmoid(opacity) as numpy computed it (:200-203),
 * rot_0..3.  order_dev (nullable = identity): the Morton order.  chunk_out_dev: ceil(n/256) x 18 float32 in the field
 * order of the reference's chunk record (:167-174); vertex_out_dev: n x 4 uint32 (packed_position, packed_rotation,
 * packed_scale, packed_color), 16-byte aligned.  Bit-exact given the same order.
 */
int gsx_cply_pack_dev(gsx_ctx *ctx, const float *const *cols14_dev, const uint32_t *order_dev, int64_t n,
                      float *chunk_out_dev, uint32_t *vertex_out_dev);
/* compressed_ply.py:236-241: out[i, c] = uint8(clip((col_c[order[i]] / 8.0 + 0.5) * 256, 0, 255)); cols_dev = m columns
 * of col_stride floats each (m <= 45), out_dev = (n, m) bytes = the reference's `sh` element */
int gsx_cply_sh_dev(gsx_ctx *ctx, const float *cols_dev, int m, int64_t col_stride, const uint32_t *order_dev, int64_t n,
                    uint8_t *out_dev);
/* Round 6: the same two packers on RAW ROWS resident in HBM (the table uploaded once, no column gather on the host): column a of
 * splat s is cols14_dev[a][s * strides14[a]] (strides14: HOST array, 1 = a contiguous column such as the numpy-computed alpha,
 * row_bytes / 4 = a field inside the rows; NULL = all 1); coefficient c of splat s is cols_dev[c * col_stride + s * elem_stride]
 * (the consecutive f_rest fields of a row: col_stride 1, elem_stride = row_bytes / 4).  gsx_morton_order_dev takes its stride
 * argument the same way.  out_dev of the SH packer must be 4-byte aligned. */
int gsx_cply_pack_strided_dev(gsx_ctx *ctx, const float *const *cols14_dev, const int64_t *strides14, const uint32_t *order_dev,
                              int64_t n, float *chunk_out_dev, uint32_t *vertex_out_dev);
int gsx_cply_sh_strided_dev(gsx_ctx *ctx, const float *cols_dev, int m, int64_t col_stride, int64_t elem_stride,
                            const uint32_t *order_dev, int64_t n, uint8_t *out_dev);
/* compressed_ply.py:139-150 `np.any(data[f"f_rest_{i}"] != 0)` from 44 downwards (and sog.py:476-486, the same loop), for m <= 64
 * CONSECUTIVE float32 fields of rows resident in HBM: bit c of *mask_out (HOST word) is set iff field c -- first_field_dev[s * row_stride
 * + c], s < n -- holds a value != 0 (NaN counts, -0.0 does not, as in numpy).  One pass over the rows (10M x 45 fields: < 1 ms) where
 * the reference's loop costs ~0.1 s per strided column.  Synchronises the context's stream. */
int gsx_fields_nonzero_dev(gsx_ctx *ctx, const float *first_field_dev, int64_t row_stride, int64_t n, int m, uint64_t *mask_out);
/* rows of any size -> rows of out_pitch bytes (a multiple of 4 >= row_bytes; the padding bytes are zero), both resident in HBM: the
 * table the reference's converter widens by three u1 colour fields (data_processor.py:262-274, 251-byte rows) becomes one whose
 * float32 fields at 4-byte offsets can be read by the strided packers above.  rows_dev must be readable up to 8 bytes past the
 * last row (a device allocation's slack). */
int gsx_rows_repack_dev(gsx_ctx *ctx, const void *rows_dev, int64_t row_bytes, int64_t n, void *out_dev, int64_t out_pitch);
/* ... with column 9 = the OPACITY itself (compressed_ply.py:200-203 `1.0 / (1.0 + np.exp(-x))`, then :312 floor(a * 255 + 0.5)): the
 * alpha byte comes from a float64 exp + the rounding certificate of gsx_sog_alpha; list_dev receives `cap` entries of two uint32
 * (position in the NEW order, bits of the opacity) for the ~1e-4 splats whose byte the caller patches with numpy's own expression
 * (`vertex[pos, 3] = vertex[pos, 3] & ~0xff | byte`); *count_dev (zeroed by the call) keeps counting past cap */
int gsx_cply_pack_opacity_dev(gsx_ctx *ctx, const float *const *cols14_dev, const int64_t *strides14, const uint32_t *order_dev,
                              int64_t n, float *chunk_out_dev, uint32_t *vertex_out_dev, uint32_t *list_dev, int64_t cap,
                              uint32_t *count_dev);


/* ---- the SPZ v3 writer's body on a DEVICE-RESIDENT splat table (csrc/spz.hip) ----
 * gsconverter/formats/spz.py:49-173 and :298-343.  The raw rows are uploaded once; the body the reference assembles in
 * `_pack_v3` -- positions 9n | alpha n | colours 3n | scales 3n | rotations 4n | SH 3*sh_dim*n bytes, sh_dim = 0, 3, 8, 15 for
 * degree 0..3 -- is written to one device buffer, byte for byte. */
typedef struct gsx_spz_layout {
    int64_t row_bytes;                 /* itemsize of the structured dtype: 1 ... 512, any size (251: the table widened by the three
                                          u1 colour fields of data_processor.py:262-274).  rows_dev must be 16-byte aligned and
                                          readable up to 15 bytes past the last row */
    int32_t offset[GSX_SOG_FIELDS];    /* byte offset of the float32 (little-endian) fields x y z | rot_0..3 | scale_0..2 | f_dc_0..2 |
                                          opacity | f_rest_0..44 inside a row (gsx_sog_layout's order; any offset); -1 = the field
                                          is absent (allowed for f_dc_*, opacity and f_rest_*) */
} gsx_spz_layout;
/* spz.py:60-77 `np.any(data[f'f_rest_{i}'] != 0)`, the loop of the SH-degree refinement: bit i of *mask_out (HOST word) is set iff
 * some row holds f_rest_i != 0 (NaN counts, -0.0 does not), for the f_rest fields whose bit is set in `fields` (all present).
 * One pass over the rows for every field at once.  Synchronises the context's stream. */
int gsx_spz_rest_nonzero_dev(gsx_ctx *ctx, const void *rows_dev, const gsx_spz_layout *layout, int64_t n, uint64_t fields,
                             uint64_t *mask_out);
/* spz.py:111-170 (`_pack_v3`) and :298-343 (`_pack_rot_v3`): the whole body, (20 + 3 * sh_dim) * n bytes at body_dev (16-byte
 * aligned), for the given SH degree (f_rest_i, f_rest_{i+15}, f_rest_{i+30} must be present for i < sh_dim: spz.py:152-154).
 * list_dev receives `cap` entries of two uint32 (row, kind) for the bytes the caller fills with numpy's own expression: kind 0 =
 * the alpha byte (spz.py:121: NaN, or numpy's float32 exp within the certificate's bracket of a byte boundary), kind 1 = the
 * rotation word (a non-largest component is NaN: numpy's float32 -> uint32 cast of a NaN depends on its position in the array);
 * *count_dev (zeroed by the call) keeps counting past cap.  Asynchronous. */
int gsx_spz_pack_dev(gsx_ctx *ctx, const void *rows_dev, const gsx_spz_layout *layout, int64_t n, int sh_degree, uint8_t *body_dev,
                     uint32_t *list_dev, int64_t cap, uint32_t *count_dev);


/* ---- the .ksplat writer's payload on a DEVICE-RESIDENT splat table (csrc/ksplat.hip) ----
 * gsconverter/formats/ksplat.py:319-544 (KSplatFormat.write).  The payload behind the 4096 + 1024 header bytes is
 * [u32 N % bucket_size] | [bucket_count x 3 f32 centres, levels >= 1] | N interleaved rows; the host writes the headers and the
 * first word, these calls the rest.  The rows use gsx_spz_layout (x y z, rot_0..3, scale_0..2, f_dc_0..2 and opacity required).
 * Both pack calls APPEND (index, kind) entries to list_dev and count on in *count_dev (zero it first: gsx_dev_memset); kind 0 =
 * row `index`, whose bytes the caller fills with numpy's own expressions (a NaN reaches a float -> u8 / u16 / f16 cast), kind 2 =
 * bucket `index`, whose centre and rows the caller takes from numpy (a NaN centre, or an axis of zeros of both signs, where
 * numpy's reduction order picks the sign).  Asynchronous. */
/* ksplat.py:426-450: the centre (min + max) / 2.0 per axis of every bucket of `bucket_size` consecutive rows (the last one may be
 * partial; any bucket_size >= 1), written as n_buckets x 3 float32 at centres_dev (4-byte aligned: its payload slot). */
int gsx_ksplat_centres_dev(gsx_ctx *ctx, const void *rows_dev, const gsx_spz_layout *layout, int64_t n, int64_t bucket_size,
                           float *centres_dev, uint32_t *list_dev, int64_t cap, uint32_t *count_dev);
/* ksplat.py:452-536: every interleaved row -- level 0: 3 f32 position, 3 f32 np.exp(scale), 4 f32 rotation, 4 u8 colour, sh_count
 * f32; level 1: 3 u16 quantised position (sf_inv = float32(32767 / (block_size / 2.0)), against centres_dev), 3 f16, 4 f16, 4 u8,
 * sh_count f16; level 2: the same with sh_count u8 clip((v + 2) / 4 * 255, 0, 255); level 3 (every level >= 3): sh_count u8
 * astype(np.uint8) of the values themselves (ksplat.py:527-533 quantise at level 2 only).  sh_count = 0, 9 or 24:
 * f_rest_0 .. f_rest_{sh_count-1} in index order (ksplat.py:488).  Rows land at payload_dev + row_base (payload_dev 16-byte aligned). */
int gsx_ksplat_pack_dev(gsx_ctx *ctx, const void *rows_dev, const gsx_spz_layout *layout, int64_t n, int level, int sh_count,
                        int64_t bucket_size, float sf_inv, const float *centres_dev, uint8_t *payload_dev, int64_t row_base,
                        uint32_t *list_dev, int64_t cap, uint32_t *count_dev);
/* ksplat.py:464 and :482 np.exp, ksplat.py:468 astype(np.float16): numpy's float32 exp (csrc/np_exp.h) and the device's
 * float32 -> float16 cast of every x_dev[i], as bits.  Synchronises the context's stream (the proofs of tests/devtools). */
int gsx_ksplat_math_dev(gsx_ctx *ctx, const float *x_dev, int64_t n, uint32_t *exp_out_dev, uint16_t *half_out_dev);
/* ksplat.py:464 np.exp on the HOST: the twin of the device's exp (csrc/np_exp.h), for the writer's runtime probe against this
 * process's numpy.  HOST pointers. */
int gsx_np_expf_host(const float *x, float *out, int64_t n);


/* ---- the .splat writer on a DEVICE-RESIDENT splat table (csrc/splat.hip) ----
 * gsconverter/formats/splat.py:82-166 (SplatFormat.write).  The file is n records of 32 bytes -- 3 f32 position, 3 f32
 * np.exp(scale), 4 u8 colour (r g b alpha), 4 u8 rotation -- in the order np.argsort(-metric, kind="stable") (the reference's
 * sort is numpy's unstable default; equal keys keep input order here).  The rows use gsx_spz_layout: x y z, rot_0..3,
 * scale_0..2 and opacity required, f_dc_0..2 too unless the colour comes from u1 fields.  All calls are asynchronous. */
/* splat.py:92-94 and :104-161: for every row, the sort key of -metric (metric = np.exp((s0 + s1) + s2) * (1 / (1 + np.exp(-opacity))),
 * float32; -0 keyed as +0, every NaN as 0xffffffff) and the row's record.  red_off / green_off / blue_off: byte offsets of the u1
 * fields red, green, blue (splat.py:140-143), or all -1 for the colour of :134-138 from f_dc_0..2.
 *   order_dev NULL, keys_dev and recs_dev set: rows in input order, tiles staged in LDS -> keys_dev[i], recs_dev + 32 i;
 *   order_dev NULL, recs_dev NULL: keys only;
 *   order_dev set, keys_dev NULL: the record of row order_dev[i] at recs_dev + 32 i (the sort-first variant).
 * rows_dev and recs_dev 16-byte aligned; rows_dev readable up to 15 bytes past the last row. */
int gsx_splat_pack_dev(gsx_ctx *ctx, const void *rows_dev, const gsx_spz_layout *layout, int red_off, int green_off, int blue_off, int64_t n,
                       const uint32_t *order_dev, uint32_t *keys_dev, uint8_t *recs_dev);
/* splat.py:93-98 from a given float32 metric: keys_dev[i] = the sort key of -metric_dev[i], as gsx_splat_pack_dev keys it. */
int gsx_splat_keys_dev(gsx_ctx *ctx, const float *metric_dev, int64_t n, uint32_t *keys_dev);
/* splat.py:98 `np.argsort(-metric)`, made stable: order_dev = the row indices sorted by key, equal keys in ascending index order
 * (a stable radix sort of (key, index) pairs; n < 2^32).  keys_dev is left as it is. */
int gsx_splat_order_dev(gsx_ctx *ctx, const uint32_t *keys_dev, int64_t n, uint32_t *order_dev);
/* splat.py:101 `data[sorted_indices]` on the records: out_dev + 32 i = recs_dev + 32 order_dev[i] (both 16-byte aligned). */
int gsx_splat_permute_dev(gsx_ctx *ctx, const uint8_t *recs_dev, const uint32_t *order_dev, int64_t n, uint8_t *out_dev);


/* ---- the compressed-PLY reader (csrc/cply_read.hip) ----
 * gsconverter/formats/compressed_ply.py:14-124 (CompressedPlyFormat.read) with :342-378 (_unpack_and_denormalize_11_10_11,
 * _unpack_and_denormalize_8888, _unpack_quaternions): the elements `chunk`, `vertex` and `sh` as they lie in a binary
 * little-endian file -> the reference's rows, x y z nx ny nz f_dc_0..2 opacity scale_0..2 rot_0..3 and the sh properties in
 * file order, all float32, bit for bit (NaN bits included: x86's). */
#define GSX_CPLY_READ_MAX_SH 256
typedef struct gsx_cply_read_layout {
    int64_t chunk_stride;               /* bytes per row of each element */
    int64_t vertex_stride;
    int64_t sh_stride;
    int32_t chunk_offset[18];           /* byte offsets of the float32 chunk properties min_x min_y min_z max_x max_y max_z
                                           min_scale_x..z max_scale_x..z min_r min_g min_b max_r max_g max_b (any alignment) */
    int32_t vertex_offset[4];           /* ... of the uint32 packed_position packed_rotation packed_scale packed_color */
    int32_t n_sh;                       /* uint8 sh properties (0 ... GSX_CPLY_READ_MAX_SH) and their byte offsets */
    int32_t sh_offset[GSX_CPLY_READ_MAX_SH];
} gsx_cply_read_layout;
/* the host-built tables (numpy's own results), one buffer: float64 nv / 2047 [2048] | nv / 1023 [1024] | n / 255.0 [256] |
 * (v / 1023.0 - 0.5) / 0.7071067811865476 [1024], then float32 opacity logit of byte na [256] | (u8 / 256.0 - 0.5) * 8.0 [256] */
#define GSX_CPLY_TAB_Q2047 0
#define GSX_CPLY_TAB_Q1023 2048
#define GSX_CPLY_TAB_Q255 3072
#define GSX_CPLY_TAB_DQ 3328
#define GSX_CPLY_TAB_DOUBLES 4352
#define GSX_CPLY_TAB_OPA 0
#define GSX_CPLY_TAB_SH 256
#define GSX_CPLY_TAB_BYTES (8 * 4352 + 4 * 512)
/* The first min(n_vertices, 256 n_chunks) rows -> out_dev (68 + 4 n_sh bytes per row, 16-byte aligned); the rows after them
 * are the caller's (the reference leaves them zero).  Row i of the sh element belongs to vertex i (the sh element must have at
 * least that many rows).  chunk_dev, vertex_dev and sh_dev (16-byte aligned) readable up to 16 bytes past their last row.
 * Asynchronous. */
int gsx_cply_unpack_dev(gsx_ctx *ctx, const void *chunk_dev, int64_t n_chunks, const void *vertex_dev, int64_t n_vertices, const void *sh_dev,
                        const gsx_cply_read_layout *layout, const void *tables_dev, float *out_dev);


/* ---- the .ksplat reader (csrc/ksplat_read.hip) ----
 * gsconverter/formats/ksplat.py:29-317 (KSplatFormat.read) with :24-27 (_linear_u8_to_logit): the per-row decode of :148-156
 * (row -> bucket), :197-261 (position, scale, rotation, colour, opacity, sh at compression level 0, 1 and >= 2) and the
 * consolidation of :266-315 -- the sections' interleaved rows as they lie in the file -> the reference's rows in
 * GaussianStruct.define_dtype's order, x y z nx ny nz f_dc_0..2 f_rest_0..n_coeffs-1 opacity scale_0..2 rot_0..3, all
 * float32, bit for bit (NaN bits included: x86's).  The headers are parsed and checked by the caller
 * (formats/ksplat_reader.py). */
typedef struct gsx_ksplat_read_section {
    int64_t rows_offset;     /* byte offset inside body_dev of the section's first splat row (any alignment) */
    int64_t centres_offset;  /* ... of its bucket centres, 3 float32 each (any alignment; level >= 1) */
    int64_t n_rows;          /* rows to decode (< 2^32) */
    int64_t out_row;         /* where its first row goes in the output */
    int64_t full_rows;       /* rows of the full buckets, min(fullBucketCount x bucketSize, n_rows): row i < full_rows lies in
                                bucket i / bucket_size (level >= 1) */
    int64_t prefix_offset;   /* first of its n_partial entries in prefix_dev: entry j = the section's rows up to and including
                                partially filled bucket j (capped at 2^32 - 1); row i >= full_rows lies in bucket n_full + the
                                first j whose entry is > i.  The entries must cover n_rows. */
    uint32_t bucket_size, n_full, n_partial, n_buckets;   /* every bucket index the rows reach must be < n_buckets */
    int32_t sh_count;        /* f_rest values per row in the file: 0, 9 or 24, <= n_coeffs; float32 at level 0, float16 at
                                level 1, uint8 at level >= 2 */
    float scale_range;       /* float32(compressionScaleRange) (ksplat.py:207) */
    float scale_factor;      /* float32((bucketBlockSize / 2.0) / compressionScaleRange), the quotient in float64 (:206) */
} gsx_ksplat_read_section;
/* tables_dev: float32 (b / 255 - 0.5) / 0.28209479177387814 [256] | the opacity logit of byte b [256], numpy's own results.
 * body_dev: the file from its first payload byte, 16-byte aligned and readable up to 16 bytes past body_bytes.  out_dev:
 * out_rows rows of 68 + 4 n_coeffs bytes (n_coeffs = 0, 9, 24, 45), 16-byte aligned; the sections' rows must tile it (every
 * row is written by exactly one section, whole).  One launch per section with rows.  Asynchronous. */
int gsx_ksplat_unpack_dev(gsx_ctx *ctx, const void *body_dev, int64_t body_bytes, int level, const gsx_ksplat_read_section *sections,
                          int n_sections, const uint32_t *prefix_dev, int64_t n_prefix, const float *tables_dev, int n_coeffs,
                          float *out_dev, int64_t out_rows);


/* ---- the SPZ reader (csrc/spz_read.hip) ----
 * gsconverter/formats/spz.py:175-251 (SpzFormat._read_body) with :253-262 (_unpack_rot_legacy), :267-296 (_unpack_rot_v3) and
 * :345-348 (_linear_u8_to_logit): the six planar sections of an inflated body -- positions (6 bytes a row at version 1, else
 * 9), alpha (1), colour (3), scale (3), rotation (3 below version 3, else 4), sh (3 x 0/3/8/15 for degree 0..3), each
 * following the other at any byte -- -> the reference's rows in GaussianStruct.define_dtype(has_rgb=True)'s order, x y z nx ny
 * nz f_dc_0..2 f_rest_0.. opacity scale_0..2 rot_0..3 as float32, then red green blue as bytes, packed (71, 107, 167 or 251
 * bytes a row), bit for bit.  The header is parsed and checked by the caller (formats/spz_reader.py).
 * tables_dev: the host-built tables (numpy's own results), 32-bit words: float32 opacity logit of byte b [256] | float32 f_dc
 * of byte b [256] | the red/green/blue byte the reference derives from that f_dc, as uint32 [256] | float32 scale [256] |
 * float32 sh [256] | float32 legacy rotation component b / 127.5 - 1 [256] | float32 signed version-3 rotation component of
 * the 10-bit code c [1024].  (Scale and sh are exact in float32 and the kernel computes them; their tables are the host's.) */
#define GSX_SPZ_TAB_OPA 0
#define GSX_SPZ_TAB_DC 256
#define GSX_SPZ_TAB_RGB 512
#define GSX_SPZ_TAB_SCALE 768
#define GSX_SPZ_TAB_SH 1024
#define GSX_SPZ_TAB_ROTL 1280
#define GSX_SPZ_TAB_ROT3 1536
#define GSX_SPZ_TAB_WORDS 2560
/* body_dev: the inflated file from byte 16 on, 16-byte aligned and readable up to 16 bytes past body_bytes, which must hold
 * the six sections of n rows (n < 2^32).  out_dev: n packed rows, 16-byte aligned.  version 1 ... 3, sh_degree 0 ... 3,
 * fractional_bits 0 ... 255 (the divisor is float32(1 << fractional_bits): inf from 128 on).  One launch.  Asynchronous. */
int gsx_spz_unpack_dev(gsx_ctx *ctx, const void *body_dev, int64_t body_bytes, int version, int sh_degree, int fractional_bits,
                       const void *tables_dev, void *out_dev, int64_t n);


/* ---- the SOG reader (csrc/sog_read.hip) ----
 * gsconverter/formats/sog.py:23-247 (SogFormat.read) from the textures' decoded RGBA texels: positions (:67-86), scales
 * (:92-102), rotation (:106-142), f_dc and opacity (:147-158), the shN palette (:183-225) -> the reference's rows in
 * GaussianStruct.define_dtype(has_scal=False, has_rgb=False)'s order, x y z nx ny nz f_dc_0..2 f_rest_0.. opacity scale_0..2
 * rot_0..3 as float32, packed (68, 104, 164 or 248 bytes a row for 0 ... 3 bands), bit for bit.  The bundle is opened, checked
 * and decoded to texels by the caller (formats/sog_reader.py).
 * tables_dev: the host-built tables (numpy's own results), float32 as 32-bit words: the scales codebook [256] | the sh0
 * codebook [256] | the shN codebook [256] | the opacity logit of alpha byte b [256] | the rotation component (b / 255 - 0.5) * 2
 * [256] | the position of u16 code c on axis a [3][65536].  A shorter codebook is padded: the caller has checked its indices. */
#define GSX_SOG_TAB_SCALE 0
#define GSX_SOG_TAB_SH0 256
#define GSX_SOG_TAB_SHN 512
#define GSX_SOG_TAB_OPA 768
#define GSX_SOG_TAB_QUAT 1024
#define GSX_SOG_TAB_POS 1280
#define GSX_SOG_TAB_WORDS (1280 + 3 * 65536)
/* texels_dev: 16-byte aligned; offsets[7]: the byte offsets (multiples of 4) inside it of the first n RGBA texels of means_l,
 * means_u, scales, quats, sh0 and shN_labels, and of the centroid pixels -- the first 64 C pixels of every centroid image row
 * of 64 * 3 C, C = 3 / 8 / 15 coefficients per channel, row after row, so that pixel (label, j) is number label * C + j;
 * palette * C of them must be there.  The last two are ignored at 0 bands.  palette 1 ... 65536: a label at or above it sets
 * *flag_dev (which the caller has zeroed) and reads nothing; that row's f_rest are then unspecified.  out_dev: n packed rows,
 * 16-byte aligned; n < 2^32.  One launch.  Asynchronous. */
int gsx_sog_unpack_dev(gsx_ctx *ctx, const void *texels_dev, int64_t texels_bytes, const int64_t *offsets, int bands, int64_t palette,
                       const void *tables_dev, void *out_dev, int64_t n, uint32_t *flag_dev);


/* ---- the .splat reader (csrc/splat_read.hip) ----
 * gsconverter/formats/splat.py:9-80 (SplatFormat.read): the file's 32-byte records -- 3 f32 position, 3 f32 linear scale, 4 u8
 * colour (r g b alpha), 4 u8 rotation -- -> the reference's rows in GaussianStruct.define_dtype(has_scal=False, has_rgb=True,
 * sh_degree=0)'s order, x y z nx ny nz f_dc_0..2 opacity scale_0..2 rot_0..3 as float32, then red green blue as bytes, packed
 * (71 bytes a row), bit for bit: positions moved as bits (:38-40), np.log(np.maximum(scale, 1e-6)) with numpy's own float32 log
 * (:43-48, csrc/np_log.h), the renormalised rotation (:52-63), nx ny nz red green blue zero (:36: never assigned).
 * tables_dev: the host-built tables (numpy's own results), float32: f_dc of colour byte b [256] (:75-77) | the opacity logit of
 * alpha byte b [256] (:67-69). */
#define GSX_SPLAT_TAB_DC 0
#define GSX_SPLAT_TAB_OPA 256
#define GSX_SPLAT_TAB_WORDS 512
/* recs_dev: n records, 16-byte aligned (nothing behind them is read).  out_dev: n packed rows, 16-byte aligned; n < 2^32.  One
 * launch.  Asynchronous. */
int gsx_splat_unpack_dev(gsx_ctx *ctx, const void *recs_dev, int64_t n, const float *tables_dev, void *out_dev);
/* splat.py:46-48 np.log: numpy's float32 log (csrc/np_log.h) of every x_dev[i], as bits.  Synchronises the context's stream
 * (the proof of tests/devtools/check_np_log.py). */
int gsx_np_log_math_dev(gsx_ctx *ctx, const float *x_dev, int64_t n, uint32_t *out_bits_dev);
/* splat.py:46-48 np.log on the HOST: the twin of the device's log (csrc/np_log.h), for the reader's runtime probe against this
 * process's numpy.  HOST pointers. */
int gsx_np_logf_host(const float *x, float *out, int64_t n);


/* ---- the 3DGS / CloudCompare PLY readers (csrc/ply_read.hip) ----
 * gsconverter/formats/ply_3dgs.py:8-60 (Ply3DGSFormat.read) and gsconverter/formats/ply_cc.py:8-62 (PlyCCFormat.read): the
 * zeroed table of :45 and the mapping loop of ply_3dgs.py:48-58 / ply_cc.py:48-60 (`converted_data[target] = vertices[source]`,
 * numpy's cast by value) as one pass over the vertex element's rows -> the reference's packed rows, bit for bit.  Which source
 * a target takes is decided on the host (formats/ply_reader.py); a field is described by
 *   src_offset   byte offset inside an input row, -1 = no source: the field stays zero
 *   src_type     GSX_PLY_T_I1 ... GSX_PLY_T_F8: convert that PLY scalar to float32 by value (dst_bytes 4; f4 moves its bits, f8
 *                rounds as x86 does, NaN payload kept and quieted); GSX_PLY_T_RAW: copy dst_bytes bytes as they are
 *   dst_offset   byte offset inside an output row
 *   dst_bytes    1, 2, 4 or 8
 * The output fields must tile the output row.  big_endian: every converted field is byte-swapped as it is read (a raw copy of
 * more than one byte is then refused). */
#define GSX_PLY_READ_MAX_FIELDS 128
#define GSX_PLY_T_I1 0
#define GSX_PLY_T_U1 1
#define GSX_PLY_T_I2 2
#define GSX_PLY_T_U2 3
#define GSX_PLY_T_I4 4
#define GSX_PLY_T_U4 5
#define GSX_PLY_T_F4 6
#define GSX_PLY_T_F8 7
#define GSX_PLY_T_RAW 8
typedef struct gsx_ply_read_layout {
    int32_t in_stride;                  /* bytes per row of the file's vertex element, 1 ... 512 */
    int32_t out_stride;                 /* bytes per output row, 1 ... 512 */
    int32_t n_fields;                   /* output fields, 1 ... GSX_PLY_READ_MAX_FIELDS */
    int32_t big_endian;                 /* 0 or 1 */
    int32_t src_offset[GSX_PLY_READ_MAX_FIELDS];
    int32_t src_type[GSX_PLY_READ_MAX_FIELDS];
    int32_t dst_offset[GSX_PLY_READ_MAX_FIELDS];
    int32_t dst_bytes[GSX_PLY_READ_MAX_FIELDS];
} gsx_ply_read_layout;
/* body_dev: 16-byte aligned, row 0 at its byte first_byte (0 ... 15), readable up to 16 bytes past the last row.  out_dev: n
 * rows of out_stride bytes, 16-byte aligned.  One launch.  Asynchronous. */
int gsx_ply_unpack_dev(gsx_ctx *ctx, const void *body_dev, int64_t first_byte, int64_t n, const gsx_ply_read_layout *layout, void *out_dev);
/* the same transcode on the HOST, field by field with the kernel's own conversion code (the host tests hold it against numpy).
 * HOST pointers; body readable up to 4 bytes past the last row. */
int gsx_ply_unpack_host(const void *body, int64_t n, const gsx_ply_read_layout *layout, void *out);

/* ---- ASCII bodies of the 3DGS / CloudCompare PLY readers (csrc/ply_text.hip, csrc/dec_to_f64.h) ----
 * gsconverter/formats/ply_3dgs.py:10 and gsconverter/formats/ply_cc.py:10 (`PlyData.read`) on a file of `format ascii 1.0`: the
 * element's text -> its rows in binary little-endian form, in the declared property types -- what plyfile hands the mapping loops
 * of ply_3dgs.py:45-58 / ply_cc.py:45-60, which gsx_ply_unpack_dev then runs as it does for a binary body.  Lines end at \n;
 * tokens are separated by runs of 0x20 0x09 0x0b 0x0c 0x0d; every line holds one token per property; float and double tokens are
 * [+-]?(D+(\.D*)?|\.D+)([eE][+-]?D+)? or [+-]?(nan|inf|infinity), rounded correctly to a double (a `float` is that double cast to
 * float32); integer tokens are [+-]?D+ within the type's range.  A chunk of text starts at a line start and ends with a newline. */
#define GSX_PLY_TEXT_MAX_PROPS 512
typedef struct gsx_ply_text_layout {
    int32_t n_props;                    /* properties of the element = tokens of a line, 1 ... GSX_PLY_TEXT_MAX_PROPS */
    int32_t in_stride;                  /* bytes of a binary row, 1 ... 512 */
    int32_t offset[GSX_PLY_TEXT_MAX_PROPS];   /* byte offset of the property inside a row */
    int32_t type[GSX_PLY_TEXT_MAX_PROPS];     /* GSX_PLY_T_I1 ... GSX_PLY_T_F8 */
} gsx_ply_text_layout;
/* result words of gsx_ply_text_parse_dev and gsx_ply_text_host */
#define GSX_PLY_TEXT_TOKENS 0           /* tokens of the chunk */
#define GSX_PLY_TEXT_LINES 1            /* newlines of the chunk */
#define GSX_PLY_TEXT_ROWS 2             /* rows taken from it: min(rows_left, lines) */
#define GSX_PLY_TEXT_BAD_LINE 3         /* the first of those lines (0-based) that does not hold n_props tokens, or -1 */
#define GSX_PLY_TEXT_FLAGGED 4          /* tokens left to the host (all of them, beyond list_cap too) */
#define GSX_PLY_TEXT_END 5              /* byte offset just past the last of those lines */
#define GSX_PLY_TEXT_RESULT_WORDS 6
/* bytes the text buffer must hold for a chunk of text_len bytes (the bytes from text_len on filled with \n), and bytes of `work` */
int64_t gsx_ply_text_padded_bytes(int64_t text_len);
int64_t gsx_ply_text_work_bytes(int64_t text_len);
/* token starts and newlines per tile of text, their exclusive scan: text_dev 16-byte aligned, the chunk from its byte 0,
 * 1 ... 2^30 bytes.  Asynchronous. */
int gsx_ply_text_scan_dev(gsx_ctx *ctx, const void *text_dev, int64_t text_len, void *work_dev, int64_t work_bytes);
/* after gsx_ply_text_scan_dev on the same chunk: its first min(rows_left, lines) lines -> rows of in_stride bytes from rows_dev on
 * (rows_left rows of room).  list_dev: list_cap entries of four uint32 (token of the chunk, its byte offset, its length or 0
 * beyond 63 bytes, 0) for the tokens the device does not settle, whose bytes are zero in the rows: not of the grammar, out of
 * range, a rounding it cannot certify, a subnormal double.  result: GSX_PLY_TEXT_RESULT_WORDS HOST words.  Synchronises. */
int gsx_ply_text_parse_dev(gsx_ctx *ctx, const void *text_dev, int64_t text_len, int64_t rows_left, const gsx_ply_text_layout *layout,
                           void *rows_dev, void *work_dev, int64_t work_bytes, void *list_dev, int64_t list_cap, int64_t *result);
/* the same tokeniser and number code on the HOST (the host tests hold it against Python; it converts a chunk whose list
 * overflowed).  HOST pointers. */
int gsx_ply_text_host(const void *text, int64_t text_len, int64_t rows_left, const gsx_ply_text_layout *layout, void *rows, uint32_t *list,
                      int64_t list_cap, int64_t *result);
/* one float token of n bytes -> the float64 bits of Python's float(token): 0, or GSX_DEC_FLAGGED when the code leaves it to the host */
#define GSX_DEC_FLAGGED 2
int gsx_dec_to_f64(const void *token, int32_t n, uint64_t *bits);
/* entry q (-342 ... 308) of the certificate's table: floor(5^q normalised to 128 bits) and exp2 with 5^q in [m, m + 1) * 2^exp2 */
int gsx_dec_pow5_entry(int32_t q, uint64_t *hi, uint64_t *lo, int32_t *exp2);


/* ---- the 3DGS / CloudCompare PLY writers (csrc/ply_write.hip) ----
 * gsconverter/formats/ply_3dgs.py:62-121 (Ply3DGSFormat.write) and gsconverter/formats/ply_cc.py:64-132 (PlyCCFormat.write): the
 * zeroed table of ply_3dgs.py:104 / ply_cc.py:112 and the copy loop of ply_3dgs.py:107-109 / ply_cc.py:115-116
 * (`output_data[name] = data[name]`, never a cast: the file keeps the table's types) as one pass over the table's rows -> the
 * rows of the file's vertex element, byte for byte.  Which fields the file holds and in what order is decided on the host
 * (formats/ply_writer.py), which merges fields adjacent in the table and in the file into runs:
 *   src_offset   byte offset inside a row of the table, -1 = no source: the run is zero (a padded nx ny nz or f_rest_*)
 *   dst_offset   byte offset inside a row of the file
 *   bytes        1 ... 512
 * The runs must tile the output row. */
#define GSX_PLY_WRITE_MAX_RUNS 128
typedef struct gsx_ply_write_layout {
    int32_t in_stride;                  /* bytes per row of the table (its itemsize: holes included), 1 ... 512 */
    int32_t out_stride;                 /* bytes per row of the file, 1 ... 512 */
    int32_t n_runs;                     /* 1 ... GSX_PLY_WRITE_MAX_RUNS */
    int32_t reserved;
    int32_t src_offset[GSX_PLY_WRITE_MAX_RUNS];
    int32_t dst_offset[GSX_PLY_WRITE_MAX_RUNS];
    int32_t bytes[GSX_PLY_WRITE_MAX_RUNS];
} gsx_ply_write_layout;
/* ply_3dgs.py:104-109 / ply_cc.py:112-116.  rows_dev: n rows of in_stride bytes, 16-byte aligned, readable up to 16 bytes past
 * the last row.  out_dev: n rows of out_stride bytes, 16-byte aligned.  One launch.  Asynchronous. */
int gsx_ply_pack_dev(gsx_ctx *ctx, const void *rows_dev, int64_t n, const gsx_ply_write_layout *layout, void *out_dev);
/* the same pack on the HOST, tile by tile and unit by unit with the kernel's own run code (the host tests hold it against
 * numpy).  HOST pointers; nothing outside the rows is read. */
int gsx_ply_pack_host(const void *rows, int64_t n, const gsx_ply_write_layout *layout, void *out);
/* ply_3dgs.py:70-76 `np.any(data[f'f_rest_{i}'] != 0)` / ply_cc.py:70-76 `np.any(data[f'f_rest_{i}'])`, the loop behind crop_sh:
 * bit i of *mask_out (HOST word) is set iff some row holds a little-endian float32 != 0 at byte offsets[i] (NaN and denormals
 * count, -0.0 does not), for the i whose bit is set in present_mask -- the result word of gsx_spz_rest_nonzero_dev, for a table
 * that need not hold the fields gsx_spz_layout requires.  offsets: 45 HOST values, read where present.  rows_dev as above; rows
 * of 1 ... 512 bytes.  One pass over the rows for every field at once.  Synchronises the context's stream. */
int gsx_ply_rest_nonzero_dev(gsx_ctx *ctx, const void *rows_dev, int64_t stride, int64_t n, const int32_t *offsets, uint64_t present_mask,
                             uint64_t *mask_out);


/* ---- the Parquet reader and writer (csrc/parquet.hip) ----
 * gsconverter/formats/parquet.py (ParquetFormat).  pyarrow keeps the file's pages, snappy, dictionaries and Thrift on both sides;
 * the device does the transposes between Arrow's columns and the table's rows, with the casts and the validity bitmaps. */
#define GSX_PARQUET_MAX_FIELDS 128
/* source types of the reader beyond GSX_PLY_T_I1 ... GSX_PLY_T_F8 (and GSX_PLY_T_RAW = 8: copy dst_bytes bytes) */
#define GSX_PARQUET_T_I8 9
#define GSX_PARQUET_T_U8 10
#define GSX_PARQUET_T_F2 11
/* The reader, parquet.py:51-55: the loop `converted_data[name] = df_renamed[name].values` (one strided, casting column copy per
 * output field) with the null -> NaN pass pandas runs ahead of it, as one pass.  Per output field:
 *   col_offset    byte offset of the source column's n values inside cols_dev (a multiple of 16), -1 = none: the field is zero
 *   valid_offset  byte offset of its Arrow validity bitmap there (bit r = row r, LSB first, (n + 63) / 64 * 8 bytes, a multiple
 *                 of 8), -1 = every row is valid.  A row whose bit is cleared reads 0x7fc00000 whatever its value slot holds
 *                 (0x7fffe000 from a float16 column: to_pandas' half NaN 0x7fff, cast).
 *                 Converted fields only.
 *   src_type      GSX_PLY_T_I1 ... GSX_PLY_T_F8, GSX_PARQUET_T_I8 / _U8 / _F2: numpy's cast of that type to float32, bit for bit
 *                 (dst_bytes 4); GSX_PLY_T_RAW: a copy of dst_bytes bytes (1, 2, 4 or 8: red green blue from a uint8 column)
 *   dst_offset, dst_bytes   where the field lies in an output row.  The fields must tile the output row. */
typedef struct gsx_parquet_rows_layout {
    int32_t out_stride;                 /* bytes per output row, 1 ... 512 */
    int32_t n_fields;                   /* output fields, 1 ... GSX_PARQUET_MAX_FIELDS */
    int32_t src_type[GSX_PARQUET_MAX_FIELDS];
    int32_t dst_offset[GSX_PARQUET_MAX_FIELDS];
    int32_t dst_bytes[GSX_PARQUET_MAX_FIELDS];
    int64_t col_offset[GSX_PARQUET_MAX_FIELDS];
    int64_t valid_offset[GSX_PARQUET_MAX_FIELDS];
} gsx_parquet_rows_layout;
/* cols_dev: cols_bytes bytes, 16-byte aligned; every column and bitmap is checked to lie inside it.  out_dev: n rows of
 * out_stride bytes, 16-byte aligned.  One launch.  Asynchronous. */
int gsx_parquet_rows_dev(gsx_ctx *ctx, const void *cols_dev, int64_t cols_bytes, int64_t n, const gsx_parquet_rows_layout *layout, void *out_dev);
/* the same on the HOST with the kernel's own cast code (the host tests hold it against numpy).  HOST pointers. */
int gsx_parquet_rows_host(const void *cols, int64_t cols_bytes, int64_t n, const gsx_parquet_rows_layout *layout, void *out);
/* The writer, parquet.py:94-108: `pd.DataFrame(data)`, the rename and the reorder -- a strided copy of every field into a column
 * of its own -- and the NaN scan `pa.Table.from_pandas` runs over every float column for its validity bitmap and null count, as
 * one pass over the rows.  Per field (= output column):
 *   src_offset, bytes   where the field lies in a row of the table; 1, 2, 4 or 8 bytes, any byte offset.  A bit copy.
 *   kind          0: no bitmap; 1: float32, 2: float64 -- bit r of the bitmap is !isnan(row r)
 *   col_offset    byte offset of the column's n values inside out_dev (a multiple of 16)
 *   valid_offset  byte offset of the bitmap there (kind 1, 2; a multiple of 8): (n + 63) / 64 * 8 bytes, every one of them
 *                 written, LSB first, the bits past n zero */
typedef struct gsx_parquet_columns_layout {
    int32_t in_stride;                  /* bytes per row of the table (its itemsize: holes included), 1 ... 512 */
    int32_t n_fields;                   /* 1 ... GSX_PARQUET_MAX_FIELDS */
    int32_t src_offset[GSX_PARQUET_MAX_FIELDS];
    int32_t bytes[GSX_PARQUET_MAX_FIELDS];
    int32_t kind[GSX_PARQUET_MAX_FIELDS];
    int64_t col_offset[GSX_PARQUET_MAX_FIELDS];
    int64_t valid_offset[GSX_PARQUET_MAX_FIELDS];
} gsx_parquet_columns_layout;
/* rows_dev: n rows of in_stride bytes, 16-byte aligned, readable up to 16 bytes past the last row.  out_dev: out_bytes bytes,
 * 16-byte aligned; every column and bitmap is checked to lie inside it.  null_counts_dev: GSX_PARQUET_MAX_FIELDS device words,
 * zeroed here; word f receives the NaN count of field f (kind 1, 2).  One launch.  Asynchronous. */
int gsx_parquet_columns_dev(gsx_ctx *ctx, const void *rows_dev, int64_t n, const gsx_parquet_columns_layout *layout, void *out_dev,
                            int64_t out_bytes, uint64_t *null_counts_dev);
/* the same on the HOST (the host tests hold it against numpy).  HOST pointers; nothing outside the rows is read. */
int gsx_parquet_columns_host(const void *rows, int64_t n, const gsx_parquet_columns_layout *layout, void *out, int64_t out_bytes,
                             uint64_t *null_counts);


/* ---- the table profile: what the orchestrator and `--info` ask of a decoded table, in one pass (csrc/table_profile.hip) ----
 * converter.py:121-146 finds the source SH degree with `np.any(self.data[f'f_rest_{i}'] != 0)` on one strided column at a time
 * and main.py:109-114,190-209 takes six strided min / max reductions and up to 45 more `np.any` scans for the info block.  All of
 * them are reductions over rows a reader holds decoded in HBM just before its download: one pass there, or one threaded pass over
 * a host table (csrc/host_rows.hip). */
typedef struct {
    int64_t row_bytes;                 /* 1 ... 512 */
    int32_t xyz_offset[3];             /* byte offsets of the float32 (little-endian) fields x y z inside a row, -1 = absent */
    int32_t rest_offset[45];           /* ... of f_rest_0..44, -1 = absent */
} gsx_profile_layout;
typedef struct {
    uint64_t rest_nonzero;             /* bit i: some row has (bits(f_rest_i) & 0x7fffffff) != 0 -- np.any(col != 0) and np.any(col):
                                          NaN and denormals count, -0.0 does not.  An absent field leaves its bit clear */
    float    lo[3], hi[3];             /* np.min / np.max of x y z by value (the sign of a zero extreme is unspecified; +-inf pass
                                          through).  An absent axis: lo = +inf, hi = -inf */
    uint32_t nan_axes;                 /* bit a: axis a holds a NaN; its lo and hi are then unspecified */
    int64_t  n;
} gsx_table_profile;
/* rows_dev: 16-byte aligned, row 0 at byte first_byte (0 ... 15), n >= 1 rows, readable up to 15 bytes past the last row.  Every
 * present field lies inside a row (any byte offset).  *out is a HOST struct.  One launch; synchronises the context's stream. */
int gsx_table_profile_dev(gsx_ctx *ctx, const void *rows_dev, int64_t first_byte, int64_t n, const gsx_profile_layout *layout,
                          gsx_table_profile *out);
/* the same on the HOST, threaded (threads <= 0: by the table's size); nothing outside the rows is read.  The model the host tests
 * hold against numpy, and the product path for a table that is not resident. */
int gsx_table_profile_host(const void *rows, int64_t n, const gsx_profile_layout *layout, int threads, gsx_table_profile *out);


/* ---- a reader's decoded rows, kept in HBM for the filters and a writer (csrc/resident_rows.hip) ----
 * rows_dev as gsx_table_profile_dev takes it: 16-byte aligned, row 0 at byte first_byte (0 ... 15), rows of 1 ... 512 bytes, readable
 * up to 15 bytes past the last row; fields at any byte offset.  Every value is a bit copy (NaN payloads, -0.0).
 *
 * m (1 ... 4) 4-byte fields of every row -> out_dev (16-byte aligned): a dense (n, m) array of 32-bit words -- the coordinates of
 * data_processor.py:38,139, the opacity column of :210, the f_dc of :316-343.  One launch.  Asynchronous. */
int gsx_rows_columns_f32_dev(gsx_ctx *ctx, const void *rows_dev, int64_t first_byte, int64_t stride, int64_t n, const int32_t *offsets,
                             int m, void *out_dev);
/* gsx_host_take_rows_shape on the device: out row j = source row idx_dev[j] (strictly ascending uint32 in HBM; NULL = row j), the
 * n_zero 4-byte fields at zero_offsets (host array) zeroed, then e (0 ... 4) bytes of extra_dev[idx[j]] ((n_in, e) u8 in HBM)
 * appended; stride_out = stride_in + e.  out_dev: 16-byte aligned, n_out * stride_out bytes (nothing behind them is written).
 * A list that leaves [0, n_in) or does not ascend is refused after the launch (no row outside the table is read).  One launch;
 * synchronises the context's stream. */
int gsx_rows_take_dev(gsx_ctx *ctx, const void *rows_dev, int64_t first_byte, int64_t stride_in, int64_t n_in, const uint32_t *idx_dev,
                      int64_t n_out, const int32_t *zero_offsets, int n_zero, const uint8_t *extra_dev, int e, void *out_dev,
                      int64_t stride_out);
/* dst_dev[idx[i]] = val[i] for cnt entries of HOST arrays (every idx[i] < dst_len, checked): numpy's own bytes for the elements
 * gsx_rgb_from_sh_list_dev lists, so that the colours stay in HBM.  Synchronises the context's stream. */
int gsx_dev_patch_u8(gsx_ctx *ctx, uint8_t *dst_dev, int64_t dst_len, const uint32_t *idx, const uint8_t *val, int64_t cnt);


/* ---- the rows of one table re-laid into another table's row layout (csrc/rows_remap.hip): the merge of several scenes ----
 * Rows [dst_row0, dst_row0 + n) of the destination (dst_rows rows of dst_stride bytes) become the n source rows: run k of `runs`
 * (HOST array, n_runs x 3 int32, 1 ... 128 runs) copies runs[3k+2] bytes from byte runs[3k] of a source row (-1: zero fill) to
 * byte runs[3k+1] of its destination row.  Every run lies inside its rows and every byte of a destination row belongs to exactly
 * one run, or the call is refused.  Source and destination as gsx_rows_take_dev takes its rows (16-byte aligned base, row 0 at
 * byte *_first_byte = 0 ... 15, 15 readable bytes past the last row, rows of 1 ... 512 bytes); they must not overlap.  Every value
 * is a bit copy; no byte outside the n destination rows is written, so remaps into neighbouring row ranges may run back to back.
 * n, dst_rows in [0, 2^32); n = 0 launches nothing.  A single run of the whole row is a device-to-device copy on the context's
 * stream, everything else one launch.  Asynchronous. */
int gsx_rows_remap_dev(gsx_ctx *ctx, const void *src_dev, int64_t src_first_byte, int64_t src_stride, int64_t n, const int32_t *runs,
                       int n_runs, void *dst_dev, int64_t dst_first_byte, int64_t dst_stride, int64_t dst_row0, int64_t dst_rows);
/* the same on HOST pointers, with the same refusals, threaded; nothing outside the rows is read or written. */
int gsx_rows_remap_host(const void *src, int64_t src_first_byte, int64_t src_stride, int64_t n, const int32_t *runs, int n_runs, void *dst,
                        int64_t dst_first_byte, int64_t dst_stride, int64_t dst_row0, int64_t dst_rows);


/* ---- a similarity transform p' = s R p + t of a whole table (csrc/transform.hip) ----
 * R a proper rotation, s > 0, t a translation.  Four parts of a splat depend on the frame: the position, the log-scales, the
 * orientation quaternion and every spherical-harmonic band above DC (and the normals of a table that has them).  Every product
 * and sum is float64, rounded once per operation, left to right, the result cast to float32; the log-scales take one float32
 * add.  A part whose bit is clear, and every other byte of a row, is a bit copy.  The caller computes the numbers (the Python
 * package: transform.plan_transform); nothing here checks that R is a rotation or that the D matrices belong to it. */
enum { GSX_TF_POSITION = 1, GSX_TF_NORMALS = 2, GSX_TF_SCALES = 4, GSX_TF_ROTATION = 8, GSX_TF_SH1 = 16, GSX_TF_SH2 = 32, GSX_TF_SH3 = 64,
       GSX_TF_ALL = 127 };
typedef struct {
    uint32_t parts;                    /* GSX_TF_* bits: the parts that are rewritten */
    int32_t  rest_m;                   /* f_rest coefficients per colour channel: 3, 8 or 15 when an SH bit is set */
    int32_t  xyz_offset[3];            /* byte offsets of the float32 (little-endian) fields inside a row; read for set bits only */
    int32_t  normal_offset[3];
    int32_t  scale_offset[3];
    int32_t  rot_offset[4];            /* rot_0..3 = (w, x, y, z) */
    int32_t  rest_offset[45];          /* f_rest_i; channel c, coefficient k is f_rest_(c * rest_m + k), band l starts at k = l*l - 1 */
    float    log_scale;                /* float32(log(s)): scale_i' = scale_i + log_scale */
    double   M[9];                     /* s R, row-major: x' = f32(((M00 x + M01 y) + M02 z) + t0) */
    double   R[9];                     /* the normals: the same without the translation */
    double   t[3];
    double   q[4];                     /* q_R = (w, x, y, z): rot' = q_R (x) rot (Hamilton product), the norm is kept */
    double   D1[9], D2[25], D3[49];    /* band l of every channel: c'_j = f32((...(D[j][0] c_0 + D[j][1] c_1) + ...)), row-major */
} gsx_transform_layout;
/* rows_dev as gsx_rows_take_dev takes it; out_dev (16-byte aligned, row 0 at byte first_byte too) may be rows_dev: in place.
 * Only the n * stride bytes of the rows are written.  A field of a set part outside a row, or two written fields that share a
 * byte, are refused.  n = 0 launches nothing.  One launch.  Asynchronous. */
int gsx_rows_transform_dev(gsx_ctx *ctx, const void *rows_dev, int64_t first_byte, int64_t stride, int64_t n,
                           const gsx_transform_layout *layout, void *out_dev);
/* the same on the HOST, from the same per-row functions (the host tests hold it against the definition, bit for bit).  HOST
 * pointers, rows at any address, out may be rows; nothing outside the rows is read or written. */
int gsx_rows_transform_host(const void *rows, int64_t stride, int64_t n, const gsx_transform_layout *layout, void *out);


/* ---- the splat budget: keep the N most visible rows (csrc/limit.hip) ----
 * The metric of a row is the .splat writer's (formats/splat.py:92-94): m = E((s0 + s1) + s2) * (1 / (1 + E(-opacity))), every
 * operation float32 in this order, E the float32 exp of csrc/np_exp.h (on the host: gsx_np_expf_host) whatever numpy the process
 * runs.  Its key is the writer's sort key of -m: an order-preserving map of float32 to uint32 after -0 -> +0, every NaN ->
 * 0xffffffff (removed first), an infinite metric 0x007fffff (kept first).  The kept rows are the first N entries of the stable
 * ascending order of the keys: among equal keys the lower row index wins.
 *
 * cols_dev (16-byte aligned): n0 rows of four float32 -- scale_0, scale_1, scale_2, opacity --, the (n0, 4) array that
 * gsx_rows_columns_f32_dev writes for those four fields (and gsx_host_gather_f32 on the host) -> keys_dev[n0].  One launch.
 * Asynchronous. */
int gsx_limit_keys_dev(gsx_ctx *ctx, const float *cols_dev, int64_t n0, uint32_t *keys_dev);
/* Row j of the n rows a chain currently has carries the key keys_dev[orig_dev ? orig_dev[j] : j] (gsx_mask_ge_dev's convention).
 * mask_dev[j] (n bytes, nothing behind them is written) = 1 for exactly min(max_count, n) rows, the definition's, else 0.
 * info_out (HOST, three words): the threshold key T -- the min(max_count, n)-th smallest --, how many of the rows with key == T
 * are kept (>= 1; the first ones in row order), and min(max_count, n); all 0 when n = 0.  A radix select, 8 bits per pass, most
 * significant digit first: four histogram passes over the keys, the digit walk on the device between them, then per-tile tie
 * counts, one scan and the mask pass -- no sort, no host round trip between passes, n / 2048 + 1032 words of workspace.
 * max_count < 1, n < 0, n >= 2^32 and null pointers are refused.  Synchronises the context's stream (the copy of info_out). */
int gsx_limit_select_dev(gsx_ctx *ctx, const uint32_t *keys_dev, const uint32_t *orig_dev, int64_t n, int64_t max_count, uint8_t *mask_dev,
                         uint32_t *info_out);
/* the same on the HOST, from the same digit walk and tie rule (csrc/limit_select.h); HOST pointers, serial. */
int gsx_limit_select_host(const uint32_t *keys, const uint32_t *orig, int64_t n, int64_t max_count, uint8_t *mask, uint32_t *info_out);


/* ---- voxel decimation: one moment-matched splat per occupied voxel (csrc/decimate.hip) ----
 * No reference counterpart: the definition is this project's own (tests/decimate_numpy.py) and the device
 * reproduces it bit for bit.  The rows of one cell of side voxel_size (the density filter's cell, (int)floorf(v / (float)h) per
 * axis) that are mergeable -- finite position, finite visibility weight > 0 (csrc/splat_metric.h's float32 expression), a
 * quaternion of finite norm > 0 -- become ONE row: the Gaussian with their combined weight, mean and covariance.  Every other
 * row, and a cell's only row, is a bit copy.  Groups leave in the order of their first member's row; members are summed in row
 * order, in blocks of 256 (float64, every operation rounded once).
 *
 * The layout names the float32 ('<f4') fields of a row by byte offset: the eleven geometry fields, up to GSX_DECIMATE_MAX_MEAN
 * fields that become the weighted mean of the members (f_dc_*, f_rest_*, nx ny nz), up to three uint8 colour fields (weighted
 * mean, rounded to nearest even, clipped) and the 4-byte fields zeroed in every output row.  Every other byte of an output row
 * is the first member's. */
enum { GSX_DECIMATE_MAX_MEAN = 51, GSX_DECIMATE_MAX_ZERO = 128, GSX_DECIMATE_STAGES = 5, GSX_DECIMATE_INFO_WORDS = 5 };
enum { GSX_DECIMATE_OK = 0, GSX_DECIMATE_CELL_RANGE = 1, GSX_DECIMATE_BAD_LIST = 2 };
typedef struct {
    double  voxel_size;                /* finite, > 0 */
    int32_t xyz_offset[3];
    int32_t scale_offset[3];
    int32_t rot_offset[4];             /* rot_0..3 = (w, x, y, z) */
    int32_t opacity_offset;
    int32_t n_mean;                    /* 0 ... GSX_DECIMATE_MAX_MEAN */
    int32_t mean_offset[GSX_DECIMATE_MAX_MEAN];
    int32_t n_u8;                      /* 0 or 3 */
    int32_t u8_offset[3];
    int32_t n_zero;                    /* 0 ... GSX_DECIMATE_MAX_ZERO; none of them a geometry field */
    int32_t zero_offset[GSX_DECIMATE_MAX_ZERO];
} gsx_decimate_layout;
/* bytes of device workspace that the two calls below need for n rows -> *bytes_out (HOST).  Launches nothing. */
int gsx_rows_decimate_work_dev(gsx_ctx *ctx, int64_t n, int64_t *bytes_out);
/* Keys, stable order, group heads and output slots of the n rows idx_dev[0 .. n) (strictly ascending uint32 in HBM; NULL: rows
 * 0 .. n - 1, and n = n_in) of the n_in resident rows at rows_dev (as gsx_rows_take_dev takes them).  work_dev: 16-byte aligned,
 * work_bytes >= gsx_rows_decimate_work_dev(n); it carries the plan to gsx_rows_decimate_write_dev and must not be touched in
 * between.  info_out (HOST, GSX_DECIMATE_INFO_WORDS int64): status (GSX_DECIMATE_*), groups (the output's row count), groups of
 * more than one row, 256-member blocks of those groups, groups of one row.  A status other than GSX_DECIMATE_OK -- a mergeable
 * row whose cell leaves [-2^20, 2^20) on an axis, a list that leaves [0, n_in) or does not ascend -- returns 0 with the status
 * set: the caller refuses, and nothing may be written.  stage_ms (HOST, GSX_DECIMATE_STAGES floats, or NULL): the stream clocks
 * of keys, order and heads are ADDED to entries 0, 1, 2.  Synchronises the context's stream (the one readback of the step). */
int gsx_rows_decimate_plan_dev(gsx_ctx *ctx, const void *rows_dev, int64_t first_byte, int64_t stride, int64_t n_in, const uint32_t *idx_dev,
                               int64_t n, const gsx_decimate_layout *layout, void *work_dev, int64_t work_bytes, int64_t *info_out,
                               float *stage_ms);
/* The n_out = info_out[1] output rows of a plan with status GSX_DECIMATE_OK -> out_dev (16-byte aligned, row 0 at byte
 * out_first_byte = 0 ... 15, rows of `stride` bytes; it must not overlap the source).  The same rows, list, layout and workspace
 * as the plan call.  No byte outside the n_out rows is written.  stage_ms: the clocks of the block sums and of the finish
 * (partials of groups above 256 rows, eigen-solve, single rows' copies) are ADDED to entries 3, 4.  Synchronises the context's
 * stream when stage_ms is given, else asynchronous. */
int gsx_rows_decimate_write_dev(gsx_ctx *ctx, const void *rows_dev, int64_t first_byte, int64_t stride, int64_t n_in, const uint32_t *idx_dev,
                                int64_t n, const gsx_decimate_layout *layout, void *work_dev, int64_t work_bytes, void *out_dev,
                                int64_t out_first_byte, int64_t n_out, float *stage_ms);


/* ---- the preview image: a tile-based forward rasteriser of the splats (csrc/render.hip) ----
 * No reference counterpart: the definition is this project's own (tests/render_numpy.py) and the device reproduces
 * it bit for bit.  A pinhole camera (x right, y down, z forward; pixel samples at integer coordinates, row 0 the top) projects
 * every row in float64 to a record; the image is blended per pixel in float32, front to back in the order of (float32 depth,
 * row), over the records whose pixel rectangle holds the pixel -- so it depends on the rows and the camera alone, never on the
 * tile size, the launch geometry or the sort.
 *
 * The layout names the float32 ('<f4') fields of a row by byte offset.  Colour: f_dc (dc_offset) with the SH bands up to `degree`
 * from rest_offset (channel c, coefficient k is f_rest_(c * rest_m + k)), or, with dc_offset[0] = -1, three uint8 at rgb_offset. */
enum { GSX_RENDER_STAGES = 6, GSX_RENDER_INFO_WORDS = 4, GSX_RENDER_RECORD_WORDS = 16, GSX_RENDER_TILE = 16, GSX_RENDER_MAX_SIDE = 8192 };
enum { GSX_RENDER_OK = 0, GSX_RENDER_TOO_MANY = 1 };
typedef struct {
    int32_t xyz_offset[3];
    int32_t scale_offset[3];
    int32_t rot_offset[4];             /* rot_0..3 = (w, x, y, z) */
    int32_t opacity_offset;
    int32_t dc_offset[3];              /* f_dc_0..2, or -1: the colour bytes */
    int32_t rgb_offset[3];             /* red green blue (uint8); read when dc_offset[0] < 0 */
    int32_t degree;                    /* SH degree that is evaluated, 0 ... 3 */
    int32_t rest_m;                    /* f_rest coefficients per colour channel: 0, 3, 8 or 15, >= (degree + 1)^2 - 1 */
    int32_t rest_offset[45];
    int32_t width, height;             /* 1 ... GSX_RENDER_MAX_SIDE */
    double  view[12];                  /* 3 x 4 row-major: p_cam = V (p, 1) */
    double  eye[3];                    /* the camera's position: SH is evaluated along normalize(p - eye) */
    double  fx, fy, cx, cy;            /* u = fx x / z + cx */
    double  tan_fovx, tan_fovy;
    double  near;                      /* > 0: a row with z_cam <= near is not drawn */
    float   background[3];
} gsx_render_layout;
/* bytes of the fixed device workspace for n rows and a width x height image -> *bytes_out (HOST).  Launches nothing. */
int gsx_rows_render_work_dev(gsx_ctx *ctx, int64_t n, int32_t width, int32_t height, int64_t *bytes_out);
/* Projects the n resident rows at rows_dev (as gsx_rows_take_dev takes them), one lane per row, counts the 16 x 16 tiles every
 * pixel rectangle touches and scans the counts.  work_dev: 16-byte aligned, work_bytes >= gsx_rows_render_work_dev; it carries
 * the plan to gsx_rows_render_draw_dev and must not be touched in between.  Its first n * 64 bytes are the records, one per row,
 * GSX_RENDER_RECORD_WORDS 32-bit words each: float32 u, v (the centre in pixels), a, b, c (the conic), opacity, red, green, blue,
 * depth; int32 x0, x1, y0, y1 (the rectangle, inclusive, clipped to the image); uint32 visible; one zero word.  An invisible
 * row's record is all zero.  info_out (HOST, GSX_RENDER_INFO_WORDS int64): status (GSX_RENDER_*), visible rows, instances
 * (tile, row pairs), bytes of instance workspace the draw call needs.  GSX_RENDER_TOO_MANY -- 2^31 instances or more -- returns 0
 * with the status set: the caller refuses.  stage_ms (HOST, GSX_RENDER_STAGES floats, or NULL): the stream clocks of project
 * and of count + scan are ADDED to entries 0, 1.  n = 0 launches nothing.  Synchronises the context's stream (the one readback). */
int gsx_rows_render_plan_dev(gsx_ctx *ctx, const void *rows_dev, int64_t first_byte, int64_t stride, int64_t n,
                             const gsx_render_layout *layout, void *work_dev, int64_t work_bytes, int64_t *info_out, float *stage_ms);
/* The image of a plan with status GSX_RENDER_OK -> image_dev (height * width * 3 bytes, RGB, row 0 the top; no byte outside them
 * is written).  The same n, layout and workspace as the plan call; inst_dev: 16-byte aligned, inst_bytes >= the plan's
 * info_out[3] (NULL and 0 when there are no instances: no sort is launched, the image is the background).  Emits
 * (tile << 32 | depth bits, row) in row order, orders them by a stable radix sort of the keys -- ties fall to the lower row --,
 * finds the tiles' ranges and blends: one workgroup of 256 lanes per tile, one pixel per lane, the tile's records staged in LDS
 * in batches of 256.  stage_ms: the clocks of emit, sort, ranges and blend are ADDED to entries 2 ... 5.  Synchronises the
 * context's stream. */
int gsx_rows_render_draw_dev(gsx_ctx *ctx, int64_t n, const gsx_render_layout *layout, void *work_dev, int64_t work_bytes, void *inst_dev,
                             int64_t inst_bytes, void *image_dev, float *stage_ms);

/* ---- view scores: what every row contributed to the pixels of a view (csrc/render.hip) ----
 * The definition is tests/view_scores_numpy.py, a twin of the image's loop: for every (pixel, splat) pair the blend adds, the
 * float32 weight wgt = alpha * T the colour sum uses.  peak[row] = max(peak[row], wgt) as float32 bits (non-negative floats order
 * as their bit patterns), total[row] += (uint64)(wgt * 2^24) -- an exact truncation to an integer below 2^24.  Integer atomics
 * only: the two arrays are the definition's bits on every run, whatever the order the tiles arrive in.
 *
 * Runs after gsx_rows_render_plan_dev, in place of the draw call and with its arguments: the same emit, stable sort and tile
 * ranges, then the score kernel -- one workgroup per tile, one pixel per lane, the blend's tests and early exits; the weights of
 * a record are reduced inside each wave, combined per batch in LDS, and leave as at most one atomicMax and one atomicAdd per
 * (tile, record).  ADDS into peak_dev (n uint32) and total_dev (n uint64, 8-byte aligned): the caller zeroes both before the
 * first view, and after the last they hold the maximum and the sum over the views.  No image is written; a plan without
 * instances launches nothing.  A layout whose dc_offset[0] and rgb_offset[0] are both -1 reads no colour (the records' are 0).
 * stage_ms: the clocks of emit, sort, ranges and score are ADDED to entries 2 ... 5.  Synchronises the context's stream. */
int gsx_rows_render_score_dev(gsx_ctx *ctx, int64_t n, const gsx_render_layout *layout, void *work_dev, int64_t work_bytes, void *inst_dev,
                              int64_t inst_bytes, uint32_t *peak_dev, uint64_t *total_dev, float *stage_ms);
/* The ranking key of a summed contribution for gsx_limit_select_*: keys[i] = 0xffffffff - fbits(total[i]), fbits the bit pattern
 * of total converted to float32 rounding toward zero, computed in integers (csrc/view_key.h): 0 for 0, else with
 * e = bit_length(total) - 1 and m = total >> (e - 23) (e >= 23) or total << (23 - e): ((e + 127) << 23) | (m & 0x7fffff).  The most
 * visible row has the smallest key, a row no view blended 0xffffffff.  One launch.  Asynchronous. */
int gsx_view_keys_dev(gsx_ctx *ctx, const uint64_t *total_dev, int64_t n, uint32_t *keys_dev);
/* the same on the HOST, from the same function; HOST pointers, serial. */
int gsx_view_keys_host(const uint64_t *total, int64_t n, uint32_t *keys);


/* ---- fidelity: two rendered images compared in integers (csrc/fidelity.hip; --fidelity) ----
 * No reference counterpart: the definition is this project's own (tests/fidelity_numpy.py) and the device
 * reproduces it bit for bit.  A and B are height x width x 3 uint8 images (RGB, row 0 the top, rows packed).  Nine words:
 *   out_words[0..2]  sse[c]: the sum over all pixels of (A - B)^2 in channel c (< 2^43)
 *   out_words[3]     windows: (height - 7) * (width - 7) when both sides are at least 8, else 0 -- every 8 x 8 box at stride 1
 *   out_words[4..6]  ssim[c]: the sum over the windows of q = floor(r1 * r2 * 2^32), a signed 32.32 fixed-point SSIM.  With the
 *                    window's integer sums Sa, Sb, Saa, Sbb, Sab over its N = 64 pixels, c1 = 26634 and c2 = 239708:
 *                    r1 = f64(2 Sa Sb + c1) / f64(Sa^2 + Sb^2 + c1), r2 = f64(2 (N Sab - Sa Sb) + c2) / f64((N Saa - Sa^2) +
 *                    (N Sbb - Sb^2) + c2): four integers below 2^31, two correctly rounded divisions, one product, no fma
 *   out_words[7..8]  0
 * The addends are integers, so the words do not depend on the order of summation. */
enum { GSX_FIDELITY_WORDS = 9, GSX_FIDELITY_TILE = 32, GSX_FIDELITY_MAX_SIDE = 8192 };
/* a_dev, b_dev: the images in HBM (any alignment; only their height * width * 3 bytes are read).  One launch over tiles of
 * GSX_FIDELITY_TILE x GSX_FIDELITY_TILE pixels and window origins: both images' (T + 7) x (T + 7) x 3 bytes staged in LDS, the
 * window sums built separably, the six sums reduced in the wave, then in LDS, then by one 64-bit integer atomicAdd per workgroup
 * and quantity.  Tiles over the right and bottom edge and images narrower or shorter than 8 (windows = 0) are the kernel's to
 * handle.  out_words: HOST, GSX_FIDELITY_WORDS int64.  stage_ms (HOST, one float, or NULL): the stream clock of the launch is
 * ADDED to it.  width, height in 1 ... GSX_FIDELITY_MAX_SIDE.  Synchronises the context's stream (the one readback). */
int gsx_image_compare_dev(gsx_ctx *ctx, const void *a_dev, const void *b_dev, int32_t width, int32_t height, int64_t *out_words,
                          float *stage_ms);
/* the same on the HOST, from the same per-window function; HOST pointers, serial, only the images' bytes are read. */
int gsx_image_compare_host(const void *a, const void *b, int32_t width, int32_t height, int64_t *out_words);

#ifdef __cplusplus
}
#endif
#endif /* GSX_HIP_H */
