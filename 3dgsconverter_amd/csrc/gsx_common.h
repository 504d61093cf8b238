// gsx_common.h -- context, error plumbing, workspace arena and timing for libgsx_hip.so.
// gfx950 only: wave64 is hard-coded throughout.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/gsx_hip.h"
#include "dev_carve.h"

namespace gsx {

constexpr int WAVE = 64;

void set_error(const char *fmt, ...);

#define GSX_HIP(call)                                                                         \
    do {                                                                                      \
        hipError_t e__ = (call);                                                              \
        if (e__ != hipSuccess) {                                                              \
            gsx::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), __FILE__,  \
                           __LINE__);                                                         \
            return 1;                                                                         \
        }                                                                                     \
    } while (0)

#define GSX_CHECK(expr)            \
    do {                           \
        int r__ = (expr);          \
        if (r__ != 0) return r__;  \
    } while (0)

#define GSX_FAIL(...)                \
    do {                             \
        gsx::set_error(__VA_ARGS__); \
        return 1;                    \
    } while (0)

// A grow-only device buffer owned by the context (no hipMalloc inside a timed step once warm).  It frees its memory when it
// dies, so a buffer added to a struct below needs no second mention anywhere; it cannot be copied (one owner).
// reserve() frees and re-allocates on growth: every pointer into the buffer is dead after it.  A buffer of several regions is
// therefore sized and placed by ONE carve() (dev_carve.h), never by a reserve followed by offsets.
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    int reserve(size_t bytes);
    void release();
    template <class T>
    T *as() const { return reinterpret_cast<T *>(p); }
};

// DevBuf's pinned-host twin (exact size: no headroom)
struct PinnedBuf {
    void *p = nullptr;
    size_t cap = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf &) = delete;
    PinnedBuf &operator=(const PinnedBuf &) = delete;
    ~PinnedBuf() { release(); }
    int reserve(size_t bytes);
    void release();
};

// Buffers of one grid-binned KNN run (sor_grid.hip).  Refinement levels > 0 re-run the pipeline on the
// sub-cloud around the cells a uniform grid cannot resolve; each level owns a full set.
constexpr int KNN_MAX_LEVELS = 5;
struct KnnWs {
    DevBuf packed;      // float4[n_ref]  (brute: original order; grid: cell-sorted refs)
    DevBuf qsorted;     // float4[q_count] cell-sorted queries when q != all refs
    DevBuf bucketpts;   // float4[n_ref] points grouped by bucket (between the two sort levels)
    DevBuf bkcnt;       // u32 bucket sizes | starts: a block of fixed size, carved once (level_reserve) into ...
    unsigned *bk_size = nullptr, *bk_start = nullptr;   // ... u32[MAX_BUCKETS] | u32[MAX_BUCKETS + 1]
    DevBuf tilecnt;     // u16[slot][bucket]: points of each coarse-pass tile in each bucket
    DevBuf tileoff;     // u32[slot][bucket]: where each tile's run starts inside its bucket
    DevBuf cellstart;   // u32[cap+1]
    DevBuf qcellstart;
    DevBuf gridparams;  // GridParams + work counters
    DevBuf bboxpart;    // float[7 * blocks]
    DevBuf faillist;    // u32[q_count] queries knn_brick could not certify | u32[q_count] knn_ring_fast's leftovers
    DevBuf extraitems;  // uint2[q_count/64 + 64]: (brick, first query) of every batch beyond a brick's first
    DevBuf finestart;   // u32[4 * cap + 1]: cell_start at quarter-cell steps along x (planned bricks only)
    DevBuf bricklist;   // uint2[n / 16 + 4096]: (bundle, first | last << 16 quarter) of every planned brick
    DevBuf bundleoff;   // u32[2 * bundles]: planned bricks per bundle of 2x2 query rows | their exclusive scan
    DevBuf wavestamps;  // -DGSX_WAVE_STAMPS builds only: one record per wave of knn_brick and knn_ring_fast
    // adaptive refinement (level L -> L+1)
    DevBuf deferred;    // u32[nbricks]: bricks whose neighbourhood is too populated for this level's cells
    DevBuf cellflag;    // u8[ncells]: 1 = cell belongs to the sub-cloud, 2 = ... of a deferred brick (its points are queries)
    DevBuf subxyz;      // float[3 * n_sub] SoA sub-cloud
    DevBuf submap;      // u32[2 * n_sub]: original index | this level's sorted index (bit 31 of the first: is a query)
    DevBuf submean;     // float[n_sub] mean distances computed at the next level
    DevBuf subkth;      // double[n_sub] (k+1)-th squared distance computed at the next level
    DevBuf heavylist;   // u32[q_count] sorted indices of the knn_ring queries handed to knn_heavy
    DevBuf heavypart;   // double[batch * chunks * KCAP] per-chunk partial top lists
    DevBuf probe;       // u32[G^3 + 32]: density probe of a sub-cloud (counts of a coarse grid, point-weighted histogram of them)
    uint64_t refined_total = 0;  // host-side: points gathered into sub-clouds by the current call
};

constexpr int GSX_TREE_UNSUITABLE = 2;   // launch_knn_tree(guard = true): the cloud exhausts the key resolution, nothing was computed

// Buffers of the Morton-tree KNN (sor_tree.hip)
struct TreeWs {
    DevBuf keys[2];     // u64[n]: Morton keys (unsorted | sorted)
    DevBuf vals[2];     // u32[n]: original indices (identity | key order)
    DevBuf refs;        // float4[n] points in key order
    DevBuf samples;     // u64[n/32 + 1]: the last key of every 32-key block
    DevBuf blockboxes;  // float4[2 * (n/64 + 1)]: tight box (minima, maxima) of every 64 consecutive points of the key order
    DevBuf flags;       // u8[n]: leaf bit level | 0x80 on a leaf's first point
    DevBuf tilecnt, tileoff;   // u32[tiles]: leaves starting in a tile, exclusive scan
    DevBuf leafstart;   // u32[leaves + 1]
    DevBuf leafbl;      // u8[leaves]
    DevBuf faillist;    // u32[n] sorted indices of the queries knn_leaf could not certify
    DevBuf failbound;   // double[n]: their k-th distance bound (>= 0) or minus the squared radius to start with
    DevBuf bboxpart;    // float[7 * blocks]
    DevBuf params;      // TreeParams
    DevBuf temp;        // rocprim temporary storage
};

// Buffers of one multi-GPU slab step (dist_slab.hip: gsx_sor_slab_step_dev); grow-only like the rest
struct SlabWs {
    DevBuf plan_in;    // 8 words (global box) + 4096 u32 per rank (all-gathered histograms)
    DevBuf hist;       // u32[4096]: this rank's histogram (send side of the all-gather)
    DevBuf small;      // u32 cursor[32] | u32 uncertain[2] | u32 uncertain_total[2] (one int64 each) | f32 stats[4]
    DevBuf send;       // float[3 * n_send]: rows grouped by destination slab (own rows, then halo copies)
    DevBuf send_src;   // u32[n_local]: local index of every own row of the send buffer
    DevBuf slab;       // float[3 * (n_own + n_halo)]: what this rank received
    DevBuf md_slab;    // f32[n_own]
    DevBuf kth;        // f64[n_own]
    DevBuf ret;        // f32[n_local]: mean distances in send order
    DevBuf md;         // f32[n_local + 8192 + 4]: ... in index order (+ the right neighbour's head elements)
    DevBuf md_stats;   // aligned copy for piece sums when the first own piece starts off a 16-byte boundary
    DevBuf pieces, allpieces, packed;   // numpy's 8192-element piece sums: mine | all-gathered (padded) | packed
    DevBuf mask;       // u8[n_local] when the caller brings no buffer
    PinnedBuf host;    // pinned staging of plan_in (the step's one host synchronisation)
};

struct TimingSlot {
    std::vector<hipEvent_t> ev;  // pairs: start, stop
    size_t used = 0;
    uint64_t launches = 0;       // resolved so far
    double total_ms = 0.0;
};

}  // namespace gsx

struct gsx_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t owned_stream = nullptr;   // gsx_ctx_own_stream: a non-blocking stream created for (and destroyed with) the context
    bool timing = false;
    unsigned timing_mask = 0xffffffffu;  // slots that record events when timing is on (an event pair costs ~8 us of stream time)
    gsx::TimingSlot slots[GSX_T_SLOTS];
    int num_cu = 256;
    void *comm = nullptr;  // gsx_comm (RCCL communicator, dist_slab.hip) or null

    // tunables
    double grid_points_per_cell = 0.0;  // 0 = auto: grid_policy.h, grid_pts_per_cell
    int64_t brute_below = 2048;
    int debug_skip = 0;  // profiling ablations of knn_brick (never set by the product path)
    int adaptive = 0;    // 1: bricks too populated for the grid are re-run on a finer grid (one host sync per call)
    int defer_words = 64;
    int last_knn_algo = 0;   // algorithm the last KNN call of this context ended up in (GSX_KNN_*)
    int tree = 1;        // adaptive mode: 1 = the Morton-tree path (sor_tree.hip, no host round trips), 0 = level-by-level grid refinement
    int kmeans_mfma = 1;  // K-Means assign for D in {9,24,45}, K >= 64: 1 = matrix-core filter + exact certificate, 0 = packed-f32 VALU scan
    int tree_leaf_cap = 0;         // points per leaf of the Morton-tree path: 0 = by k (sor_tree.hip: tree_leaf_cap_for), else 64 ... 256 (A/B)
    int tree_cand_limit = 0;       // candidates per 64 points of leaf capacity above which a leaf's queries go to the per-query kernels (0 = 4096; A/B)
    double tree_near_cell = 0.5;   // knn_tree_near: edge of the cover's cells as a fraction of the ball's radius (A/B)
    int tree_last_leaf_cap = 0;    // leaf capacity the last tree run of this context built its leaves with (gsx_sor_debug_tree)
    double tree_scale = 0.0;   // > 0: the Morton tree's fine cell edge is (extent / 2^21) x this (A/B of the leaf-shape rule); 0 = chosen by the density probe
    int km_exact_blocks = 4;   // workgroups per CU of kmeans_assign_exact_list (one uncertified point per workgroup and round: A/B)
    int km_seg_rows = 32;   // rows of the label-sorted permutation one wave of kmeans_segment_sum takes (64 / 32 / 16: A/B)
    int km_group_mb = 0;   // gsx_kmeans_lloyd_batch_dev: problems are run in groups whose rows fit this many MB (0: all at once) -- a group's
                           // rows then stay in the 256 MB Infinity Cache across its iterations (round 5, A/B)
    int km_small_wgs = 0;      // workgroups per CU of those shapes (0: 3 resp. 5; A/B)
    int kmeans_cs_small = 1;   // ... with 4-wave / 2-wave workgroups for K <= 256 / K <= 64 (0: the 16-wave shape for every K; A/B)
    int kmeans_cs = 1;   // centroid-stationary matrix-core assign for K <= 1024 (0: the streaming kernel; A/B)
    int ring_fast = 1;   // knn_ring_fast before knn_ring (0: A/B only)
    int phase2_net = 1;  // knn_brick phase 2: 1 = sorting-network block selection (TopNet), 0 = per-candidate bubble insert (A/B only)
    int brick_plan = 1;  // knn_brick on planned bricks (runs of quarter-cell slabs holding at most 64 queries) where the call allows it: the plain
                         // single-cloud call, k <= 16, MFMA filter + network selection (0: the fixed 2x2x2-cell bricks everywhere; A/B)
    int epilogue_cert = 1;   // knn_brick, k = 16 on the network list: certify the float32 mean of short roots, re-sort and round exactly only
                             // where the certificate fails (0: full merge and mean_from_net throughout; A/B and tests)
    int ws_cap = 0;      // -DGSX_WAVE_STAMPS builds: record slots per kernel of the last grid KNN call
    int wq_grid[4] = {0, 0, 0, 0};   // workgroups of the last knn_brick, knn_brick (second batches), knn_ring and knn_ring_fast launches (debug)
    int filter_mfma = 1; // knn_brick phase 1: 1 = bf16-split MFMA filter for batches whose mask words fit LDS, 0 = scalar-load f32 VALU filter only

    // SOR workspace: one KnnWs per refinement level of the KNN grid (level 0 = the whole cloud)
    gsx::KnnWs ws[gsx::KNN_MAX_LEVELS];
    gsx::TreeWs tree_ws;     // Morton-tree KNN workspace
    gsx::SlabWs slab_ws;     // multi-GPU slab step
    gsx::DevBuf commscratch; // gsx_comm_barrier's word
    gsx::DevBuf devflags;    // u32[16]: device-side error word (bit 0: non-finite coordinates), read by gsx_ctx_check
    float density_stage_ms[GSX_DENSITY_STAGES] = {0, 0, 0, 0, 0, 0};   // gsx_density_stage_clocks (density.hip: CcClock)
    gsx::DevBuf vox_ids;     // u16[n]: dense voxel index of every point between the two passes of the density filter (density.hip)
    gsx::DevBuf nzmask;      // one 64-bit word: gsx_fields_nonzero_dev's result before it is copied out (cply.hip)
    gsx::DevBuf statspart;   // float chunk sums
    // Staging and work buffers, named by the tier of the call chain that may take them.  Two rules: the stage_* buffers are
    // touched in api.hip only, and no function takes a buffer that a function it calls (directly or not) also takes.
    //   buffer     taken by
    //   stage_in   api.hip: Staging (every host-pointer entry point's uploaded inputs: xyz, data, values, keys, rows)
    //   stage_aux  api.hip: Staging (the second device array: centroids / codebook in and out, gsx_sor_filter's distances + stats)
    //   stage_out  api.hip: Staging (downloaded results: masks, labels, permutations, texels + uncertain bytes + lists)
    //   work       the implementation an entry point dispatches to: kmeans_lloyd_dev, lloyd_batch_mfma (kmeans.hip),
    //              gsx_kmeans_pp_dev, kmeans1d_dev, lexsort3_dev (sog.hip), gsx_sog_scan_dev, gsx_sog_extremes_dev,
    //              gsx_sog_order_dev (sog_table.hip), morton_order_dev (cply.hip), gsx_rows_transform_dev, gsx_dev_patch_u8
    //              (resident_rows.hip), gsx_image_compare_dev (fidelity.hip: its six sums), and density.hip's density_voxels_dev, density_hist_dev, density_merge_dev,
    //              density_mask_dev, density_filter_dev, density_filter_large_dev, voxel_clusters_dev (the last three end in a
    //              retry of themselves at most once, as a tail call: nothing of the first attempt is used after it)
    //   work_sub   helpers of those, sized by what their caller computed into `work` first: launch_assign_mfma_t (kmeans.hip),
    //              alloc_table (density.hip: the voxel table), density_mask_dev's key list (sized after the frame came back)
    //   work_leaf  cc_components (density.hip: parent | size of a table in work_sub)
    // The named buffers around them belong to leaf functions that call nothing which takes a buffer:
    //   commscratch  gsx_comm_barrier (comm.hip)
    //   devflags     written by the pack / KNN kernels (sor_brute.hip, sor_grid.hip, sor_tree.hip) and launch_sor_stats' ticket,
    //                read and cleared by gsx_ctx_check
    //   vox_ids      density_filter_dev
    //   nzmask       nzmask_word (row_tile.h), gsx_table_profile_dev, gsx_rows_take_dev
    //   statspart    launch_sor_stats, gsx_limit_select_dev, gsx_compact_rows_dev
    //   ksplat_keys  gsx_ksplat_centres_dev
    //   splat_sort   gsx_splat_order_dev
    // The KNN paths keep their own structs above (ws[], tree_ws, slab_ws); compute_frame (density.hip) borrows ws[0].bboxpart.
    gsx::DevBuf stage_in;
    gsx::DevBuf stage_aux;
    gsx::DevBuf stage_out;
    gsx::DevBuf work;
    gsx::DevBuf work_sub;
    gsx::DevBuf work_leaf;
    gsx::DevBuf ksplat_keys; // u32[7 * tiles]: the straddling buckets' min / max keys and NaN flags (ksplat.hip)
    gsx::DevBuf splat_sort;  // u32[n] sorted keys + rocprim temporary storage (splat.hip)
};

namespace gsx {

// RAII-less timing helper: call begin/end around a group of launches on ctx->stream.
int timing_begin(gsx_ctx *ctx, int slot);
int timing_end(gsx_ctx *ctx, int slot);

inline int div_up(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

}  // namespace gsx
