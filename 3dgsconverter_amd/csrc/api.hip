// api.hip -- C-ABI entry points of libgsx_hip.so (see include/gsx_hip.h).
#include <algorithm>
#include <mutex>

#include "grid_policy.h"
#include "gsx_common.h"
#include "gsx_internal.h"
#include "sor_grid_params.h"

namespace gsx {

static thread_local std::string g_err;

void set_error(const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
}

int DevBuf::reserve(size_t bytes)
{
    if (bytes <= cap) return 0;
    if (p) {
        GSX_HIP(hipFree(p));
        p = nullptr;
        cap = 0;
    }
    size_t want = bytes + bytes / 8 + 256;  // a little headroom: fewer re-allocations when N drifts
    GSX_HIP(hipMalloc(&p, want));
    cap = want;
    return 0;
}

void DevBuf::release()
{
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
}

int PinnedBuf::reserve(size_t bytes)
{
    if (bytes <= cap) return 0;
    release();
    GSX_HIP(hipHostMalloc(&p, bytes, hipHostMallocDefault));
    cap = bytes;
    return 0;
}

void PinnedBuf::release()
{
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
}

int timing_begin(gsx_ctx *ctx, int slot)
{
    if (!ctx->timing || !((ctx->timing_mask >> slot) & 1u)) return 0;
    TimingSlot &s = ctx->slots[slot];
    if (s.used + 2 > s.ev.size()) {
        for (int i = 0; i < 64; ++i) {
            hipEvent_t e;
            GSX_HIP(hipEventCreate(&e));
            s.ev.push_back(e);
        }
    }
    GSX_HIP(hipEventRecord(s.ev[s.used], ctx->stream));
    return 0;
}

int timing_end(gsx_ctx *ctx, int slot)
{
    if (!ctx->timing || !((ctx->timing_mask >> slot) & 1u)) return 0;
    TimingSlot &s = ctx->slots[slot];
    GSX_HIP(hipEventRecord(s.ev[s.used + 1], ctx->stream));
    s.used += 2;
    return 0;
}

static int timing_resolve(gsx_ctx *ctx, int slot)
{
    TimingSlot &s = ctx->slots[slot];
    for (size_t i = 0; i + 1 < s.used; i += 2) {
        float ms = 0.f;
        GSX_HIP(hipEventElapsedTime(&ms, s.ev[i], s.ev[i + 1]));
        s.total_ms += ms;
        s.launches += 1;
    }
    s.used = 0;
    return 0;
}

}  // namespace gsx

using namespace gsx;

extern "C" {

const char *gsx_version(void) { return "gsx-hip 0.1 (gfx950)"; }
const char *gsx_last_error(void) { return g_err.c_str(); }

int gsx_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

int gsx_device_uid(int device, char *out, int cap)
{
    if (!out || cap < 16) GSX_FAIL("gsx_device_uid: need a buffer of at least 16 bytes");
    if (hipDeviceGetPCIBusId(out, cap, device) != hipSuccess) {
        (void)hipGetLastError();
        GSX_FAIL("gsx_device_uid: no such device");
    }
    return 0;
}

int gsx_ctx_create(int device, gsx_ctx **out)
{
    if (!out) GSX_FAIL("gsx_ctx_create: null out");
    int n = gsx_device_count();
    if (n <= 0) GSX_FAIL("gsx_ctx_create: no HIP device visible");
    if (device < 0 || device >= n) GSX_FAIL("gsx_ctx_create: device %d out of range (%d visible)", device, n);
    GSX_HIP(hipSetDevice(device));
    gsx_ctx *c = new gsx_ctx();
    c->device = device;
    hipDeviceProp_t prop;
    GSX_HIP(hipGetDeviceProperties(&prop, device));
    c->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        delete c;
        GSX_FAIL("gsx_ctx_create: device %d is %s; this library is built for gfx950 (MI355X) only", device,
                 prop.gcnArchName);
    }
    if (c->devflags.reserve(64) != 0 || hipMemset(c->devflags.p, 0, 64) != hipSuccess) {
        delete c;
        GSX_FAIL("gsx_ctx_create: cannot allocate the device error word");
    }
    *out = c;
    return 0;
}

int gsx_ctx_check(gsx_ctx *c)
{
    if (!c) GSX_FAIL("null ctx");
    GSX_HIP(hipSetDevice(c->device));
    unsigned flags = 0;
    GSX_HIP(hipMemcpyAsync(&flags, c->devflags.p, sizeof(flags), hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(hipStreamSynchronize(c->stream));
    if (flags) {
        GSX_HIP(hipMemsetAsync(c->devflags.p, 0, 64, c->stream));
        if (flags & 1u) GSX_FAIL("sor: coordinates are not finite (NaN/inf): results were set to NaN");
        GSX_FAIL("device-side error flags 0x%x", flags);
    }
    return 0;
}

void gsx_ctx_destroy(gsx_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)gsx_comm_destroy(c);
    (void)hipStreamSynchronize(c->stream);
    for (auto &s : c->slots)
        for (auto e : s.ev) (void)hipEventDestroy(e);
    const hipStream_t owned = c->owned_stream;
    delete c;   // every DevBuf / PinnedBuf frees itself: the buffers go before the stream, as they always did
    if (owned) (void)hipStreamDestroy(owned);
}

int gsx_ctx_set_stream(gsx_ctx *c, void *s)
{
    if (!c) GSX_FAIL("null ctx");
    c->stream = reinterpret_cast<hipStream_t>(s);
    return 0;
}

int gsx_ctx_last_knn_algo(gsx_ctx *c) { return c ? c->last_knn_algo : -1; }

int gsx_ctx_own_stream(gsx_ctx *c)
{
    if (!c) GSX_FAIL("null ctx");
    GSX_HIP(hipSetDevice(c->device));
    if (!c->owned_stream) GSX_HIP(hipStreamCreateWithFlags(&c->owned_stream, hipStreamNonBlocking));
    c->stream = c->owned_stream;
    return 0;
}

int gsx_ctx_synchronize(gsx_ctx *c)
{
    if (!c) GSX_FAIL("null ctx");
    GSX_HIP(hipSetDevice(c->device));
    GSX_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

int gsx_ctx_set_timing(gsx_ctx *c, int enable)
{
    if (!c) GSX_FAIL("null ctx");
    c->timing = enable != 0;
    return 0;
}

int gsx_ctx_reset_timing(gsx_ctx *c)
{
    if (!c) GSX_FAIL("null ctx");
    GSX_HIP(hipStreamSynchronize(c->stream));
    for (auto &s : c->slots) {
        s.used = 0;
        s.launches = 0;
        s.total_ms = 0.0;
    }
    return 0;
}

int gsx_ctx_get_timing(gsx_ctx *c, int slot, uint64_t *launches, double *total_ms)
{
    if (!c || slot < 0 || slot >= GSX_T_SLOTS) GSX_FAIL("gsx_ctx_get_timing: bad arguments");
    GSX_HIP(hipStreamSynchronize(c->stream));
    GSX_CHECK(timing_resolve(c, slot));
    if (launches) *launches = c->slots[slot].launches;
    if (total_ms) *total_ms = c->slots[slot].total_ms;
    return 0;
}

int gsx_ctx_set_param(gsx_ctx *c, const char *name, double value)
{
    if (!c || !name) GSX_FAIL("gsx_ctx_set_param: bad arguments");
    if (!strcmp(name, "grid_points_per_cell")) {
        if (value != 0.0 && !(value >= 1.0 && value <= 512.0)) GSX_FAIL("grid_points_per_cell must be 0 (auto) or in [1,512]");
        c->grid_points_per_cell = value;
    } else if (!strcmp(name, "brute_below")) {
        c->brute_below = (int64_t)value;
    } else if (!strcmp(name, "debug_skip")) {
#ifdef GSX_ABLATE
        c->debug_skip = (int)value;
#else
        if (value != 0.0) GSX_FAIL("debug_skip needs a profiling build of the library (-DGSX_ABLATE); this one computes exact results only");
#endif
    } else if (!strcmp(name, "kmeans_mfma")) {
        c->kmeans_mfma = value != 0.0;
    } else if (!strcmp(name, "km_exact_blocks")) {
        c->km_exact_blocks = value < 1 ? 1 : (value > 32 ? 32 : (int)value);
    } else if (!strcmp(name, "km_seg_rows")) {
        c->km_seg_rows = value >= 64 ? 64 : (value >= 32 ? 32 : 16);
    } else if (!strcmp(name, "km_group_mb")) {
        c->km_group_mb = value < 0 ? 0 : (int)value;
    } else if (!strcmp(name, "kmeans_cs")) {
        c->kmeans_cs = value != 0.0;
    } else if (!strcmp(name, "km_small_wgs")) {
        c->km_small_wgs = (int)value;
    } else if (!strcmp(name, "kmeans_cs_small")) {
        c->kmeans_cs_small = value != 0.0;
    } else if (!strcmp(name, "ring_fast")) {
        c->ring_fast = value != 0.0;
    } else if (!strcmp(name, "phase2_net")) {
        c->phase2_net = value != 0.0;
    } else if (!strcmp(name, "timing_mask")) {
        c->timing_mask = (unsigned)value;
    } else if (!strcmp(name, "adaptive")) {
        c->adaptive = (int)value;
    } else if (!strcmp(name, "tree")) {
        c->tree = (int)value;
    } else if (!strcmp(name, "tree_leaf_cap")) {
        c->tree_leaf_cap = (int)value;
    } else if (!strcmp(name, "tree_cand_limit")) {
        c->tree_cand_limit = (int)value;
    } else if (!strcmp(name, "tree_near_cell")) {
        c->tree_near_cell = value > 0.05 ? value : 0.5;
    } else if (!strcmp(name, "tree_scale")) {
        c->tree_scale = value;
    } else if (!strcmp(name, "defer_words")) {
        c->defer_words = (int)value;
    } else if (!strcmp(name, "brick_plan")) {
        c->brick_plan = value != 0.0;
    } else if (!strcmp(name, "epilogue_cert")) {
        c->epilogue_cert = value != 0.0;
    } else if (!strcmp(name, "filter_mfma")) {
        c->filter_mfma = value != 0.0;
    } else {
        GSX_FAIL("gsx_ctx_set_param: unknown parameter '%s'", name);
    }
    return 0;
}

int gsx_dev_malloc(gsx_ctx *c, size_t bytes, void **dptr)
{
    if (!c || !dptr) GSX_FAIL("gsx_dev_malloc: bad arguments");
    GSX_HIP(hipSetDevice(c->device));
    GSX_HIP(hipMalloc(dptr, bytes ? bytes : 1));
    return 0;
}

// page-locked host memory the DMA engines read at link rate (a staging buffer a host routine fills, e.g. gsx_host_gather_f32 writing
// the (n, 3) coordinates of a table straight into it: no page faults of a fresh allocation, no munmap afterwards)
int gsx_host_pinned_alloc(gsx_ctx *c, size_t bytes, void **hptr)
{
    if (!c || !hptr) GSX_FAIL("gsx_host_pinned_alloc: bad arguments");
    GSX_HIP(hipSetDevice(c->device));
    GSX_HIP(hipHostMalloc(hptr, bytes ? bytes : 1, hipHostMallocDefault));
    return 0;
}

int gsx_host_pinned_free(gsx_ctx *c, void *hptr)
{
    if (!c) GSX_FAIL("null ctx");
    if (hptr) GSX_HIP(hipHostFree(hptr));
    return 0;
}

int gsx_dev_free(gsx_ctx *c, void *dptr)
{
    if (!c) GSX_FAIL("null ctx");
    if (dptr) GSX_HIP(hipFree(dptr));
    return 0;
}

int gsx_dev_upload(gsx_ctx *c, void *dst, const void *src, size_t bytes)
{
    if (!c) GSX_FAIL("null ctx");
    GSX_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    GSX_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

int gsx_dev_download(gsx_ctx *c, void *dst, const void *src, size_t bytes)
{
    if (!c) GSX_FAIL("null ctx");
    GSX_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

// ------------------------------------------------------------------ SOR
int gsx_sor_knn_dev(gsx_ctx *c, const float *x, const float *y, const float *z, int64_t stride, int64_t n_ref,
                    int64_t q_begin, int64_t q_count, int k, int algo, float *mean_out, gsx_sor_info *info)
{
    if (!c || !x || !y || !z || !mean_out) GSX_FAIL("gsx_sor_knn_dev: null argument");
    if (n_ref <= 0 || n_ref >= (1LL << 31) - 1024) GSX_FAIL("gsx_sor_knn_dev: n_ref=%lld out of range", (long long)n_ref);
    if (q_begin < 0 || q_count < 0 || q_begin + q_count > n_ref) GSX_FAIL("gsx_sor_knn_dev: query range out of bounds");
    if (k < 1 || k > 2047) GSX_FAIL("gsx_sor_knn_dev: k=%d not supported (1 <= k <= 2047)", k);
    if (stride < 1) GSX_FAIL("gsx_sor_knn_dev: bad stride");
    GSX_HIP(hipSetDevice(c->device));
    if (q_count == 0) return 0;
    if (algo == GSX_KNN_AUTO) algo = n_ref < c->brute_below ? GSX_KNN_BRUTE : GSX_KNN_GRID;
    if (k > 64) algo = GSX_KNN_GRID;   // the list-free any-k kernel lives on the grid path (csrc/sor_grid.hip: knn_anyk_kernel)
    if (algo == GSX_KNN_BRUTE) {
        GSX_CHECK(c->ws[0].packed.reserve(sizeof(float4) * (size_t)n_ref));
        GSX_CHECK(timing_begin(c, GSX_T_SOR_BIN));
        GSX_CHECK(launch_pack_points(c, x, y, z, stride, n_ref, c->ws[0].packed.as<float4>()));
        GSX_CHECK(timing_end(c, GSX_T_SOR_BIN));
        GSX_CHECK(timing_begin(c, GSX_T_SOR_KNN));
        GSX_CHECK(launch_knn_brute(c, c->ws[0].packed.as<float4>(), n_ref, q_begin, q_count, nullptr, nullptr, 0, k, mean_out));
        GSX_CHECK(timing_end(c, GSX_T_SOR_KNN));
        if (info) {
            memset(info, 0, sizeof(*info));
            info->algo = GSX_KNN_BRUTE;
            GSX_HIP(hipStreamSynchronize(c->stream));
        }
        return 0;
    }
    // (adaptive mode: launch_knn_grid itself hands clouds its grid cannot resolve to the tree path, csrc/sor_tree.hip)
    if (algo == GSX_KNN_GRID) return launch_knn_grid(c, x, y, z, stride, n_ref, q_begin, q_count, k, mean_out, info);
    if (algo == GSX_KNN_TREE) return launch_knn_tree(c, x, y, z, stride, n_ref, q_begin, q_count, k, mean_out, nullptr, info, INT32_MAX, 0, 1, false);
    GSX_FAIL("gsx_sor_knn_dev: unknown algo %d", algo);
}

// Debug / test download of the brick plan the context's last grid KNN call ran on.  grid[8] = nx, ny, nz, plan (1: the list
// was used), bricks, 0, 0, 0; origin[4] = ox, oy, oz, inv_h; list (nullable) receives min(bricks, cap) entries
// {bundle = bz * ceil(ny / 2) + by, first quarter | last quarter << 16}.  Synchronises.
int gsx_sor_debug_brick_plan(gsx_ctx *c, int32_t *grid, float *origin, uint32_t *list, int64_t cap)
{
    if (!c || !grid || !origin) GSX_FAIL("gsx_sor_debug_brick_plan: null argument");
    gsx::KnnWs &w = c->ws[0];
    if (!w.gridparams.p) GSX_FAIL("gsx_sor_debug_brick_plan: no grid KNN call has run on this context");
    GSX_HIP(hipSetDevice(c->device));
    gsx::GridParams h;
    GSX_HIP(hipMemcpyAsync(&h, w.gridparams.p, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(hipStreamSynchronize(c->stream));
    const int32_t g[8] = {h.nx, h.ny, h.nz, h.plan, h.nbricks, 0, 0, 0};
    memcpy(grid, g, sizeof(g));
    const float o[4] = {h.ox, h.oy, h.oz, h.inv_h};
    memcpy(origin, o, sizeof(o));
    if (h.plan && list && w.bricklist.p) {
        const int64_t m = std::min<int64_t>(h.nbricks, cap);
        if (m > 0) GSX_HIP(hipMemcpy(list, w.bricklist.p, sizeof(uint32_t) * 2 * (size_t)m, hipMemcpyDeviceToHost));
    }
    return 0;
}

// Debug / test download of the work queues of the context's last grid KNN call (level 0), in the order knn_brick, knn_brick
// (second batches), knn_ring, knn_ring_fast: ctr[4][8] = the final tail counters of the eight groups, items[4] = the items
// of each queue, blocks[4] = the workgroups of each launch (four waves each).  Synchronises.
int gsx_sor_debug_work_queue(gsx_ctx *c, uint32_t *ctr, int64_t *items, int32_t *blocks)
{
    if (!c || !ctr || !items || !blocks) GSX_FAIL("gsx_sor_debug_work_queue: null argument");
    gsx::KnnWs &w = c->ws[0];
    if (!w.gridparams.p) GSX_FAIL("gsx_sor_debug_work_queue: no grid KNN call has run on this context");
    GSX_HIP(hipSetDevice(c->device));
    gsx::GridParams h;
    GSX_HIP(hipMemcpyAsync(&h, w.gridparams.p, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(hipStreamSynchronize(c->stream));
    const unsigned *src[4] = {h.brick_ctr, h.extra_ctr, h.ring_ctr, h.ringf_ctr};
    for (int q = 0; q < 4; ++q)
        for (int y = 0; y < 8; ++y) ctr[q * 8 + y] = src[q][y * 32];
    items[0] = h.part_hi - h.part_lo;
    items[1] = h.extra_count;
    items[2] = c->ring_fast ? h.ring2_count : h.fail_count;
    items[3] = c->ring_fast ? h.fail_count : 0;
    for (int q = 0; q < 4; ++q) blocks[q] = c->wq_grid[q];
    return 0;
}

// Debug / test download of the stage counters and the leaf partition of the context's last Morton-tree run (csrc/sor_tree.hip:
// knn_tree_debug; the layout of counters[16] is in include/gsx_hip.h).  Synchronises; launches nothing.
int gsx_sor_debug_tree(gsx_ctx *c, uint32_t *counters, uint64_t *keys, uint32_t *leafstart, int64_t cap, int64_t *n_out, int64_t *leaves_out)
{
    if (!c || !counters) GSX_FAIL("gsx_sor_debug_tree: null argument");
    GSX_HIP(hipSetDevice(c->device));
    return gsx::knn_tree_debug(c, counters, keys, leafstart, cap, n_out, leaves_out);
}

// Diagnostic builds (-DGSX_WAVE_STAMPS) only: the wave records of the context's last grid KNN call.  kernel 0 = knn_brick (first
// launch), 1 = knn_ring_fast; out receives at most cap records of 16 words (layout: WS_WORDS in csrc/sor_grid_params.h), *count
// the number of record slots (records of waves that did not run stay zero).  Synchronises.
int gsx_sor_debug_wave_stamps(gsx_ctx *c, int kernel, uint64_t *out, int64_t cap, int64_t *count)
{
    if (!c || !out || !count || kernel < 0 || kernel > 1) GSX_FAIL("gsx_sor_debug_wave_stamps: bad arguments");
#ifdef GSX_WAVE_STAMPS
    gsx::KnnWs &w = c->ws[0];
    if (!w.wavestamps.p) GSX_FAIL("gsx_sor_debug_wave_stamps: no grid KNN call has run on this context");
    GSX_HIP(hipSetDevice(c->device));
    GSX_HIP(hipStreamSynchronize(c->stream));
    const int64_t slots = c->ws_cap;
    const int64_t m = std::min<int64_t>(slots, cap);
    if (m > 0)
        GSX_HIP(hipMemcpy(out, (const uint64_t *)w.wavestamps.p + (size_t)kernel * slots * gsx::WS_WORDS,
                          sizeof(uint64_t) * gsx::WS_WORDS * (size_t)m, hipMemcpyDeviceToHost));
    *count = slots;
    return 0;
#else
    (void)cap;
    GSX_FAIL("gsx_sor_debug_wave_stamps needs a diagnostic build of the library (-DGSX_WAVE_STAMPS)");
#endif
}

// Tests: the host-side decisions of the grid (grid_policy.h), the very functions knn_grid_level calls.  No device is touched.
double gsx_sor_debug_points_per_cell(int k, int64_t n, int tuned)
{
    return tuned ? gsx::grid_pts_per_cell(k, n) : gsx::grid_pts_per_cell_base(k, n);
}

int gsx_sor_debug_group_bricks(uint32_t *bricks, int64_t count, int nbx, int nby, int nbz, uint32_t *group_sizes, int32_t *n_groups)
{
    if (!bricks || !group_sizes || !n_groups || count < 0 || count > UINT32_MAX || nbx < 1 || nby < 1 || nbz < 1)
        GSX_FAIL("gsx_sor_debug_group_bricks: bad arguments");
    for (int64_t i = 0; i < count; ++i)
        if ((uint64_t)bricks[i] >= (uint64_t)nbx * nby * nbz) GSX_FAIL("gsx_sor_debug_group_bricks: brick %u outside the grid", bricks[i]);
    const std::vector<unsigned> sizes = gsx::group_deferred_bricks(bricks, (unsigned)count, nbx, nby, nbz);
    for (int g = 0; g < gsx::GRID_MAX_GROUPS; ++g) group_sizes[g] = g < (int)sizes.size() ? sizes[g] : 0u;
    *n_groups = (int32_t)sizes.size();
    return 0;
}

int gsx_sor_debug_refine_sizing(const gsx_refine_sizing_in *in, gsx_refine_sizing_out *out)
{
    if (!in || !out) GSX_FAIL("gsx_sor_debug_refine_sizing: null argument");
    const gsx::RefineClip r = gsx::refine_clip(in->qb_lo, in->qb_hi, in->sub_queries, in->pts_per_cell, in->parent_h, in->adaptive);
    *out = gsx_refine_sizing_out{r.nd3, r.probe_g, r.h_est, r.M, r.cert, {r.lo[0], r.lo[1], r.lo[2]}, {r.hi[0], r.hi[1], r.hi[2]}, r.r_cert,
                                 r.probe_g ? gsx::refine_probe_edge(in->hist, in->bin_vol, in->qb_lo, in->qb_hi, r.r_cert, in->n_sub,
                                                                    r.h_est, in->pts_per_cell)
                                           : 0.0};
    return 0;
}

int gsx_sor_knn_share_dev(gsx_ctx *c, const float *x, const float *y, const float *z, int64_t stride, int64_t n,
                          int k, int algo, int share, int nshares, float *mean_out, gsx_sor_info *info)
{
    if (!c || !x || !y || !z || !mean_out) GSX_FAIL("gsx_sor_knn_share_dev: null argument");
    if (nshares < 1 || share < 0 || share >= nshares) GSX_FAIL("gsx_sor_knn_share_dev: share %d of %d", share, nshares);
    if (n <= 0 || n >= (1LL << 31) - 1024) GSX_FAIL("gsx_sor_knn_share_dev: n=%lld out of range", (long long)n);
    if (k < 1 || k > 64) GSX_FAIL("gsx_sor_knn_share_dev: k=%d not supported (1 <= k <= 64)", k);
    if (stride < 1) GSX_FAIL("gsx_sor_knn_share_dev: bad stride");
    GSX_HIP(hipSetDevice(c->device));
    // every query belongs to exactly one share; the other shares' entries stay +0.0f so that the
    // shares combine by a plain sum (x + 0 = x exactly)
    GSX_HIP(hipMemsetAsync(mean_out, 0, sizeof(float) * (size_t)n, c->stream));
    if (algo == GSX_KNN_AUTO) algo = n < c->brute_below ? GSX_KNN_BRUTE : GSX_KNN_GRID;
    if (algo == GSX_KNN_BRUTE) {  // no spatial structure: the share is an index range
        const int64_t q0 = n * share / nshares, q1 = n * (share + 1) / nshares;
        if (q1 == q0) return 0;
        return gsx_sor_knn_dev(c, x, y, z, stride, n, q0, q1 - q0, k, GSX_KNN_BRUTE, mean_out + q0, info);
    }
    if (algo == GSX_KNN_GRID) return launch_knn_grid(c, x, y, z, stride, n, 0, n, k, mean_out, info, share, nshares);
    if (algo == GSX_KNN_TREE) return launch_knn_tree(c, x, y, z, stride, n, 0, n, k, mean_out, nullptr, info, INT32_MAX, share, nshares, false);
    GSX_FAIL("gsx_sor_knn_share_dev: unknown algo %d", algo);
}

int gsx_sor_stats_dev(gsx_ctx *c, const float *md, int64_t n, double factor, float *stats_dev)
{
    if (!c || !md || !stats_dev) GSX_FAIL("gsx_sor_stats_dev: null argument");
    if (reinterpret_cast<uintptr_t>(md) & 15) GSX_FAIL("gsx_sor_stats_dev: mean_dists must be 16-byte aligned");
    GSX_HIP(hipSetDevice(c->device));
    GSX_CHECK(timing_begin(c, GSX_T_SOR_STATS));
    GSX_CHECK(launch_sor_stats(c, md, n, factor, stats_dev));
    GSX_CHECK(timing_end(c, GSX_T_SOR_STATS));
    return 0;
}

int gsx_sor_mask_dev(gsx_ctx *c, const float *md, int64_t n, const float *thr_dev, uint8_t *mask)
{
    if (!c || !md || !thr_dev || !mask) GSX_FAIL("gsx_sor_mask_dev: null argument");
    GSX_HIP(hipSetDevice(c->device));
    GSX_CHECK(timing_begin(c, GSX_T_SOR_STATS));
    GSX_CHECK(launch_sor_mask(c, md, n, thr_dev, mask));
    GSX_CHECK(timing_end(c, GSX_T_SOR_STATS));
    return 0;
}

// one cached context per process for the host-buffer entry points (callers are single-threaded,
// SURVEY.md 8(b)); guarded anyway
static std::mutex g_host_mu;
static gsx_ctx *g_host_ctx = nullptr;

static int host_ctx(gsx_ctx **out)
{
    if (!g_host_ctx) {
        GSX_CHECK(gsx_ctx_create(0, &g_host_ctx));
        g_host_ctx->adaptive = 1;  // the host entry points are synchronous anyway
    }
    GSX_HIP(hipSetDevice(g_host_ctx->device));
    *out = g_host_ctx;
    return 0;
}

}  // extern "C"

// One call of a host-pointer entry point: the process-wide lock for its whole length, the cached context, inputs staged into
// the context's stage_* buffers, outputs queued for download, one synchronise.  (The stage_* buffers are touched here only.)
struct HostCall {
    std::lock_guard<std::mutex> lk{g_host_mu};
    gsx_ctx *c = nullptr;

    int open() { return host_ctx(&c); }
    // room for `count` elements (+ `slack` bytes behind them) at the start of `buf`
    template <class T>
    int room(DevBuf &buf, size_t count, T **dev, size_t slack = 0)
    {
        GSX_CHECK(buf.reserve(sizeof(T) * count + slack));
        *dev = buf.as<T>();
        return 0;
    }
    template <class T>
    int put(T *dev, const T *src, size_t count)
    {
        GSX_HIP(hipMemcpyAsync(dev, src, sizeof(T) * count, hipMemcpyHostToDevice, c->stream));
        return 0;
    }
    template <class T>
    int up(DevBuf &buf, const T *src, size_t count, T **dev)
    {
        GSX_CHECK(room(buf, count, dev));
        return put(*dev, src, count);
    }
    template <class T>
    int down(T *dst, const T *dev, size_t count)
    {
        GSX_HIP(hipMemcpyAsync(dst, dev, sizeof(T) * count, hipMemcpyDeviceToHost, c->stream));
        return 0;
    }
    int sync()
    {
        GSX_HIP(hipStreamSynchronize(c->stream));
        return 0;
    }
    // strided host xyz as three device columns (SoA in HBM) of stage_in
    int up_xyz(const float *x, const float *y, const float *z, int64_t stride, int64_t n, float **dx, float **dy, float **dz, int64_t *dstride)
    {
        float *base;
        if (stride == 1) {
            GSX_CHECK(room(c->stage_in, 3 * (size_t)n, &base));
            GSX_CHECK(put(base, x, (size_t)n));
            GSX_CHECK(put(base + n, y, (size_t)n));
            GSX_CHECK(put(base + 2 * n, z, (size_t)n));
            *dx = base; *dy = base + n; *dz = base + 2 * n; *dstride = 1;
            return 0;
        }
        if (stride == 3 && y == x + 1 && z == x + 2) {  // the reference's (N,3) coords: one contiguous copy
            GSX_CHECK(up(c->stage_in, x, 3 * (size_t)n, &base));
            *dx = base; *dy = base + 1; *dz = base + 2; *dstride = 3;
            return 0;
        }
        GSX_FAIL("xyz layout not supported by the host entry points (use three contiguous columns or (N,3) rows)");
    }
};

// Bytes the byte-wide outputs have always had behind them.  None of the kernels that fill them (sor_mask_kernel,
// voxel_mask_kernel, quantize_kernel, the SOG texel kernels) was found to touch the tail; it is kept all the same.
constexpr size_t MASK_TAIL = 4, TEXEL_TAIL = 16;

extern "C" {

int gsx_sor_filter(const float *x, const float *y, const float *z, int64_t stride, int64_t n, int k, double factor,
                   int algo, uint8_t *mask_out, float *mean_out, float *stats_out, gsx_sor_info *info)
{
    HostCall h;
    if (!x || !y || !z || !mask_out) GSX_FAIL("gsx_sor_filter: null argument");
    if (n <= 0) GSX_FAIL("gsx_sor_filter: empty cloud");
    GSX_CHECK(h.open());
    gsx_ctx *c = h.c;
    float *dx, *dy, *dz, *dmd = nullptr, *dstats = nullptr;
    int64_t ds;
    uint8_t *dmask;
    GSX_CHECK(h.up_xyz(x, y, z, stride, n, &dx, &dy, &dz, &ds));
    GSX_CHECK(carve(c->stage_aux, [&](Carve &a) {
        dmd = a.take<float>((size_t)n);   // (16-byte aligned: gsx_sor_stats_dev)
        dstats = a.take<float>(4);        // mean, std, threshold
    }));
    GSX_CHECK(h.room(c->stage_out, (size_t)n, &dmask, MASK_TAIL));
    GSX_CHECK(gsx_sor_knn_dev(c, dx, dy, dz, ds, n, 0, n, k, algo, dmd, nullptr));
    GSX_CHECK(gsx_sor_stats_dev(c, dmd, n, factor, dstats));
    GSX_CHECK(gsx_sor_mask_dev(c, dmd, n, dstats + 2, dmask));
    GSX_CHECK(h.down(mask_out, dmask, (size_t)n));
    if (mean_out) GSX_CHECK(h.down(mean_out, dmd, (size_t)n));
    if (stats_out) GSX_CHECK(h.down(stats_out, dstats, 3));
    GSX_CHECK(gsx_ctx_check(c));  // synchronises; non-finite coordinates (either algorithm) are an error, like cKDTree's
    int used = k > 64 ? GSX_KNN_GRID : (algo == GSX_KNN_AUTO ? (n < c->brute_below ? GSX_KNN_BRUTE : GSX_KNN_GRID) : algo);
    if (used == GSX_KNN_GRID && c->last_knn_algo == GSX_KNN_TREE) used = GSX_KNN_TREE;   // adaptive mode chose the tree path
    if (info) {
        // re-query diagnostics without recomputing: only the grid path has device-side counters
        memset(info, 0, sizeof(*info));
        info->algo = used;
        if (used == GSX_KNN_GRID) {
            GridParams hgp;
            GSX_HIP(hipMemcpy(&hgp, c->ws[0].gridparams.p, sizeof(hgp), hipMemcpyDeviceToHost));
            info->grid_dim[0] = hgp.nx; info->grid_dim[1] = hgp.ny; info->grid_dim[2] = hgp.nz;
            info->cell_size = hgp.h;
            info->n_cells = hgp.ncells;
            info->n_bricks = hgp.nbricks;
            info->n_fallback = hgp.fail_count;
            info->n_exhaustive = hgp.exhaustive_count;
            info->n_deferred_bricks = hgp.deferred_count;
            info->n_refined = (int64_t)c->ws[0].refined_total;
        }
        if (used == GSX_KNN_TREE) GSX_CHECK(knn_tree_info(c, info));
    }
    return 0;
}

// ------------------------------------------------------------------ density
int gsx_density_voxels_dev(gsx_ctx *c, const float *x, const float *y, const float *z, int64_t stride, int64_t n,
                           double voxel_size, int64_t min_points, int64_t dense_cap, int64_t *n_unique_out,
                           int64_t *n_dense_out, int64_t *dense_keys_out, int64_t *dense_counts_out)
{
    if (!c || !x || !y || !z || !n_unique_out || !n_dense_out || !dense_keys_out || !dense_counts_out)
        GSX_FAIL("gsx_density_voxels_dev: null argument");
    if (n <= 0) GSX_FAIL("gsx_density_voxels_dev: empty cloud");
    GSX_HIP(hipSetDevice(c->device));
    return density_voxels_dev(c, x, y, z, stride, n, voxel_size, min_points, dense_cap, n_unique_out, n_dense_out,
                              dense_keys_out, dense_counts_out);
}

int gsx_density_hist_dev(gsx_ctx *c, const float *x, const float *y, const float *z, int64_t stride, int64_t n, double voxel_size,
                         int64_t cap, int64_t *n_unique_out, int64_t *keys3_dev, int64_t *counts_dev)
{
    if (!c || !x || !y || !z || !n_unique_out || !keys3_dev || !counts_dev) GSX_FAIL("gsx_density_hist_dev: null argument");
    if (n <= 0) GSX_FAIL("gsx_density_hist_dev: empty cloud");
    GSX_HIP(hipSetDevice(c->device));
    return density_hist_dev(c, x, y, z, stride, n, voxel_size, cap, n_unique_out, keys3_dev, counts_dev);
}

int gsx_density_merge_dev(gsx_ctx *c, const int64_t *keys3_dev, const int64_t *counts_dev, int64_t m, int64_t min_points,
                          int64_t dense_cap, int64_t *n_unique_out, int64_t *n_dense_out, int64_t *dense_keys_out,
                          int64_t *dense_counts_out)
{
    if (!c || !n_unique_out || !n_dense_out || !dense_keys_out || !dense_counts_out || (m > 0 && (!keys3_dev || !counts_dev)))
        GSX_FAIL("gsx_density_merge_dev: null argument");
    GSX_HIP(hipSetDevice(c->device));
    return density_merge_dev(c, keys3_dev, counts_dev, m, min_points, dense_cap, n_unique_out, n_dense_out, dense_keys_out,
                             dense_counts_out);
}

int gsx_density_filter_dev(gsx_ctx *c, const float *x, const float *y, const float *z, int64_t stride, int64_t n, double voxel_size,
                           int64_t min_points, int keep_multicluster, const float *box6, uint8_t *mask_out_dev, gsx_density_info *info)
{
    if (!c || !x || !y || !z || !mask_out_dev || !info) GSX_FAIL("gsx_density_filter_dev: null argument");
    if (n <= 0) GSX_FAIL("gsx_density_filter_dev: empty cloud");
    GSX_HIP(hipSetDevice(c->device));
    return density_filter_dev(c, x, y, z, stride, n, voxel_size, min_points, keep_multicluster, box6, mask_out_dev, info);
}

int gsx_density_filter_large_dev(gsx_ctx *c, const float *x, const float *y, const float *z, int64_t stride, int64_t n, double voxel_size,
                                 int64_t min_points, int keep_multicluster, const float *box6, uint8_t *mask_out_dev, gsx_density_info *info)
{
    if (!c || !x || !y || !z || !mask_out_dev || !info) GSX_FAIL("gsx_density_filter_large_dev: null argument");
    if (n <= 0) GSX_FAIL("gsx_density_filter_large_dev: empty cloud");
    GSX_HIP(hipSetDevice(c->device));
    return density_filter_large_dev(c, x, y, z, stride, n, voxel_size, min_points, keep_multicluster, box6, mask_out_dev, info);
}

int gsx_voxel_clusters_dev(gsx_ctx *c, const int64_t *keys3, int64_t m, int keep_multicluster, uint8_t *keep_out, gsx_density_info *info)
{
    if (!c || !info || m < 0 || (m > 0 && (!keys3 || !keep_out))) GSX_FAIL("gsx_voxel_clusters_dev: null argument");
    if (m > (1ll << 30)) GSX_FAIL("gsx_voxel_clusters_dev: too many keys for the voxel table");
    if (m == 0) {
        *info = gsx_density_info{};
        info->status = GSX_DENSITY_EMPTY;
        return 0;
    }
    GSX_HIP(hipSetDevice(c->device));
    return voxel_clusters_dev(c, keys3, m, keep_multicluster, keep_out, info);
}

int gsx_voxel_clusters(const int64_t *keys3, int64_t m, int keep_multicluster, uint8_t *keep_out, gsx_density_info *info)
{
    HostCall h;
    GSX_CHECK(h.open());
    return gsx_voxel_clusters_dev(h.c, keys3, m, keep_multicluster, keep_out, info);
}

int gsx_density_stage_clocks(gsx_ctx *c, double *ms_out)
{
    if (!c || !ms_out) GSX_FAIL("gsx_density_stage_clocks: null argument");
    for (int i = 0; i < GSX_DENSITY_STAGES; ++i) ms_out[i] = c->density_stage_ms[i];
    return 0;
}

int gsx_density_mask_dev(gsx_ctx *c, const float *x, const float *y, const float *z, int64_t stride, int64_t n,
                         double voxel_size, const int64_t *kept_keys, int64_t n_kept, uint8_t *mask_out_dev)
{
    if (!c || !x || !y || !z || !mask_out_dev || (n_kept > 0 && !kept_keys)) GSX_FAIL("gsx_density_mask_dev: null argument");
    if (n <= 0) return 0;
    GSX_HIP(hipSetDevice(c->device));
    return density_mask_dev(c, x, y, z, stride, n, voxel_size, kept_keys, n_kept, mask_out_dev);
}

int gsx_density_voxels(const float *x, const float *y, const float *z, int64_t stride, int64_t n, double voxel_size,
                       int64_t min_points, int64_t dense_cap, int64_t *n_unique_out, int64_t *n_dense_out,
                       int64_t *dense_keys_out, int64_t *dense_counts_out)
{
    HostCall h;
    if (!x || !y || !z) GSX_FAIL("gsx_density_voxels: null argument");
    if (n <= 0) GSX_FAIL("gsx_density_voxels: empty cloud");
    GSX_CHECK(h.open());
    float *dx, *dy, *dz;
    int64_t ds;
    GSX_CHECK(h.up_xyz(x, y, z, stride, n, &dx, &dy, &dz, &ds));
    return gsx_density_voxels_dev(h.c, dx, dy, dz, ds, n, voxel_size, min_points, dense_cap, n_unique_out, n_dense_out,
                                  dense_keys_out, dense_counts_out);
}

int gsx_density_mask(const float *x, const float *y, const float *z, int64_t stride, int64_t n, double voxel_size,
                     const int64_t *kept_keys, int64_t n_kept, uint8_t *mask_out)
{
    HostCall h;
    if (!x || !y || !z || !mask_out) GSX_FAIL("gsx_density_mask: null argument");
    if (n <= 0) return 0;
    GSX_CHECK(h.open());
    float *dx, *dy, *dz;
    int64_t ds;
    uint8_t *dmask;
    GSX_CHECK(h.up_xyz(x, y, z, stride, n, &dx, &dy, &dz, &ds));
    GSX_CHECK(h.room(h.c->stage_out, (size_t)n, &dmask, MASK_TAIL));
    GSX_CHECK(gsx_density_mask_dev(h.c, dx, dy, dz, ds, n, voxel_size, kept_keys, n_kept, dmask));
    GSX_CHECK(h.down(mask_out, dmask, (size_t)n));
    return h.sync();
}

// ------------------------------------------------------------------ K-Means
int gsx_kmeans_lloyd_dev(gsx_ctx *c, const float *data_dev, int64_t n, int d, int k, int max_iter,
                         float *centroids_dev, int32_t *labels_dev)
{
    if (!c || !data_dev || !centroids_dev || !labels_dev) GSX_FAIL("gsx_kmeans_lloyd_dev: null argument");
    if (max_iter < 0) GSX_FAIL("gsx_kmeans_lloyd_dev: negative max_iter");
    GSX_HIP(hipSetDevice(c->device));
    return kmeans_lloyd_dev(c, data_dev, n, d, k, max_iter, centroids_dev, labels_dev);
}

int gsx_kmeans_lloyd_batch_dev(gsx_ctx *c, const float *data_dev, const int64_t *row_off, int nprob, int d, int k, int max_iter,
                               float *centroids_dev, int32_t *labels_dev)
{
    if (!c || !data_dev || !row_off || !centroids_dev || !labels_dev) GSX_FAIL("gsx_kmeans_lloyd_batch_dev: null argument");
    if (max_iter < 0) GSX_FAIL("gsx_kmeans_lloyd_batch_dev: negative max_iter");
    GSX_HIP(hipSetDevice(c->device));
    return kmeans_lloyd_batch_dev(c, data_dev, row_off, nprob, d, k, max_iter, centroids_dev, labels_dev);
}

int gsx_kmeans_lloyd(const float *data, int64_t n, int d, int k, int max_iter, const float *init_centroids,
                     float *centroids_out, int32_t *labels_out)
{
    HostCall h;
    if (!data || !init_centroids || !centroids_out || !labels_out) GSX_FAIL("gsx_kmeans_lloyd: null argument");
    if (n <= 0 || d <= 0 || k <= 0) GSX_FAIL("gsx_kmeans_lloyd: bad shape");
    GSX_CHECK(h.open());
    const size_t nd = (size_t)n * d, kd = (size_t)k * d;
    float *d_data, *d_cent;
    int32_t *d_labels;
    GSX_CHECK(h.up(h.c->stage_in, data, nd, &d_data));
    GSX_CHECK(h.up(h.c->stage_aux, init_centroids, kd, &d_cent));
    GSX_CHECK(h.room(h.c->stage_out, (size_t)n, &d_labels));
    GSX_HIP(hipMemsetAsync(d_labels, 0, sizeof(int32_t) * (size_t)n, h.c->stream));  // max_iter == 0: labels stay 0 (gpu_ops.py:183)
    GSX_CHECK(gsx_kmeans_lloyd_dev(h.c, d_data, n, d, k, max_iter, d_cent, d_labels));
    GSX_CHECK(h.down(centroids_out, d_cent, kd));
    GSX_CHECK(h.down(labels_out, d_labels, (size_t)n));
    return h.sync();
}

int gsx_kmeans_pp(const float *data, int64_t n, int d, int k, const double *uniforms, int n_local_trials, float *centroids_out)
{
    HostCall h;
    if (!data || !uniforms || !centroids_out) GSX_FAIL("gsx_kmeans_pp: null argument");
    if (n <= 0 || d <= 0 || k <= 0) GSX_FAIL("gsx_kmeans_pp: bad shape");
    GSX_CHECK(h.open());
    const size_t nd = (size_t)n * d, kd = (size_t)k * d;
    float *d_data, *d_cent;
    GSX_CHECK(h.up(h.c->stage_in, data, nd, &d_data));
    GSX_CHECK(h.room(h.c->stage_aux, kd, &d_cent));
    GSX_CHECK(gsx_kmeans_pp_dev(h.c, d_data, n, d, k, uniforms, n_local_trials, d_cent));
    GSX_CHECK(h.down(centroids_out, d_cent, kd));
    return h.sync();
}

int gsx_kmeans1d(const float *vals, int64_t n, int k, int iters, float *centroids_out, int32_t *labels_out, double *inertia3_out)
{
    HostCall h;
    if (!vals || !centroids_out) GSX_FAIL("gsx_kmeans1d: null argument");
    if (n <= 0 || k <= 0) GSX_FAIL("gsx_kmeans1d: bad shape");
    GSX_CHECK(h.open());
    float *d_vals, *d_cent;
    int32_t *d_labels = nullptr;
    GSX_CHECK(h.up(h.c->stage_in, vals, (size_t)n, &d_vals));
    GSX_CHECK(h.room(h.c->stage_aux, (size_t)k, &d_cent));
    if (labels_out) GSX_CHECK(h.room(h.c->stage_out, (size_t)n, &d_labels));
    GSX_CHECK(gsx_kmeans1d_dev(h.c, d_vals, n, k, iters, 3, d_cent, d_labels, inertia3_out));
    GSX_CHECK(h.down(centroids_out, d_cent, (size_t)k));
    if (labels_out) GSX_CHECK(h.down(labels_out, d_labels, (size_t)n));
    return h.sync();
}

int gsx_quantize_sorted_codebook_dev(gsx_ctx *c, const float *vals_dev, int64_t n, const float *codebook_dev, int kcb,
                                     uint8_t *idx_out_dev)
{
    if (!c || !vals_dev || !codebook_dev || !idx_out_dev) GSX_FAIL("gsx_quantize_sorted_codebook_dev: null argument");
    GSX_HIP(hipSetDevice(c->device));
    return quantize_dev(c, vals_dev, n, codebook_dev, kcb, idx_out_dev);
}

int gsx_quantize_sorted_codebook(const float *vals, int64_t n, const float *codebook, int kcb, uint8_t *idx_out)
{
    HostCall h;
    if (!vals || !codebook || !idx_out) GSX_FAIL("gsx_quantize_sorted_codebook: null argument");
    if (n <= 0) return 0;
    GSX_CHECK(h.open());
    float *d_vals, *d_cb;
    uint8_t *d_idx;
    GSX_CHECK(h.up(h.c->stage_in, vals, (size_t)n, &d_vals));
    GSX_CHECK(h.room(h.c->stage_aux, 256, &d_cb));
    GSX_CHECK(h.room(h.c->stage_out, (size_t)n, &d_idx, MASK_TAIL));
    GSX_CHECK(h.put(d_cb, codebook, (size_t)(kcb > 0 && kcb <= 256 ? kcb : 0)));
    GSX_CHECK(gsx_quantize_sorted_codebook_dev(h.c, d_vals, n, d_cb, kcb, d_idx));
    GSX_CHECK(h.down(idx_out, d_idx, (size_t)n));
    return h.sync();
}

// ------------------------------------------------------------------ SOG writer numeric core (host buffers)
int gsx_lexsort3(const float *k0, const float *k1, const float *k2, int64_t n, uint32_t *perm_out)
{
    HostCall h;
    if (!k0 || !k1 || !k2 || !perm_out) GSX_FAIL("gsx_lexsort3: null argument");
    if (n <= 0) return 0;
    GSX_CHECK(h.open());
    float *base;
    uint32_t *d_perm;
    GSX_CHECK(h.room(h.c->stage_in, 3 * (size_t)n, &base));
    GSX_CHECK(h.room(h.c->stage_out, (size_t)n, &d_perm));
    const float *src[3] = {k0, k1, k2};
    for (int a = 0; a < 3; ++a) GSX_CHECK(h.put(base + (size_t)a * n, src[a], (size_t)n));
    GSX_CHECK(gsx_lexsort3_dev(h.c, base, base + n, base + 2 * (size_t)n, 1, n, d_perm));
    GSX_CHECK(h.down(perm_out, d_perm, (size_t)n));
    return h.sync();
}

}  // extern "C"

// a texel column and its uncertain bytes behind it: the outputs of gsx_rgb_from_sh, gsx_sog_positions and gsx_sog_alpha
template <class T>
static int texel_room(HostCall &h, size_t n, T **d_out, uint8_t **d_unc)
{
    return carve(h.c->stage_out, [&](Carve &a) {
        *d_out = a.take<T>(n);
        *d_unc = a.take<uint8_t>(n, 1);
        a.take<uint8_t>(TEXEL_TAIL, 1);
    });
}

extern "C" {

int gsx_rgb_from_sh(const float *f_dc, int64_t n, uint8_t *out, uint8_t *uncertain_out)
{
    HostCall h;
    if (!f_dc || !out || !uncertain_out) GSX_FAIL("gsx_rgb_from_sh: null argument");
    if (n <= 0) return 0;
    GSX_CHECK(h.open());
    float *d_in;
    uint8_t *d_out = nullptr, *d_unc = nullptr;
    GSX_CHECK(h.up(h.c->stage_in, f_dc, (size_t)n, &d_in));
    GSX_CHECK(texel_room(h, (size_t)n, &d_out, &d_unc));
    GSX_CHECK(gsx_rgb_from_sh_dev(h.c, d_in, n, d_out, d_unc));
    GSX_CHECK(h.down(out, d_out, (size_t)n));
    GSX_CHECK(h.down(uncertain_out, d_unc, (size_t)n));
    return h.sync();
}

int gsx_rgb_from_sh_list(const float *f_dc, int64_t n, uint8_t *out, uint32_t *list_out, int64_t cap, int64_t *count_out)
{
    HostCall h;
    if (!f_dc || !out || !count_out || (cap > 0 && !list_out)) GSX_FAIL("gsx_rgb_from_sh_list: null argument");
    *count_out = 0;
    if (n <= 0) return 0;
    GSX_CHECK(h.open());
    float *d_in;
    uint8_t *d_out = nullptr;
    uint32_t *d_cnt = nullptr, *d_list = nullptr;
    GSX_CHECK(h.up(h.c->stage_in, f_dc, (size_t)n, &d_in));
    GSX_CHECK(carve(h.c->stage_out, [&](Carve &a) {
        d_out = a.take<uint8_t>((size_t)n);
        d_cnt = a.take<uint32_t>(4, 16);   // the count word, on a 16-byte boundary
        d_list = a.take<uint32_t>((size_t)cap, 4);
        a.take<uint8_t>(TEXEL_TAIL, 1);
    }));
    GSX_CHECK(gsx_rgb_from_sh_list_dev(h.c, d_in, n, d_out, d_list, cap, d_cnt));
    uint32_t hc = 0;
    GSX_CHECK(h.down(out, d_out, (size_t)n));
    GSX_CHECK(h.down(&hc, d_cnt, 1));
    GSX_CHECK(h.sync());
    *count_out = hc;
    const size_t m = std::min<size_t>(hc, (size_t)cap);
    if (m) {
        GSX_CHECK(h.down(list_out, d_list, m));
        GSX_CHECK(h.sync());
    }
    return 0;
}

int gsx_sog_positions(const float *v, int64_t n, float log_min, float log_max, uint16_t *out, uint8_t *uncertain_out)
{
    HostCall h;
    if (!v || !out || !uncertain_out) GSX_FAIL("gsx_sog_positions: null argument");
    if (n <= 0) return 0;
    GSX_CHECK(h.open());
    float *d_in;
    uint16_t *d_out = nullptr;
    uint8_t *d_unc = nullptr;
    GSX_CHECK(h.up(h.c->stage_in, v, (size_t)n, &d_in));
    GSX_CHECK(texel_room(h, (size_t)n, &d_out, &d_unc));
    GSX_CHECK(gsx_sog_positions_dev(h.c, d_in, n, log_min, log_max, d_out, d_unc));
    GSX_CHECK(h.down(out, d_out, (size_t)n));
    GSX_CHECK(h.down(uncertain_out, d_unc, (size_t)n));
    return h.sync();
}

int gsx_sog_alpha(const float *opacity, int64_t n, uint8_t *out, uint8_t *uncertain_out)
{
    HostCall h;
    if (!opacity || !out || !uncertain_out) GSX_FAIL("gsx_sog_alpha: null argument");
    if (n <= 0) return 0;
    GSX_CHECK(h.open());
    float *d_in;
    uint8_t *d_out = nullptr, *d_unc = nullptr;
    GSX_CHECK(h.up(h.c->stage_in, opacity, (size_t)n, &d_in));
    GSX_CHECK(texel_room(h, (size_t)n, &d_out, &d_unc));
    GSX_CHECK(gsx_sog_alpha_dev(h.c, d_in, n, d_out, d_unc));
    GSX_CHECK(h.down(out, d_out, (size_t)n));
    GSX_CHECK(h.down(uncertain_out, d_unc, (size_t)n));
    return h.sync();
}

int gsx_sog_quats(const float *rot_rows, int64_t n, uint8_t *out4)
{
    HostCall h;
    if (!rot_rows || !out4) GSX_FAIL("gsx_sog_quats: null argument");
    if (n <= 0) return 0;
    GSX_CHECK(h.open());
    float *d_in;
    uint8_t *d_out;
    GSX_CHECK(h.up(h.c->stage_in, rot_rows, 4 * (size_t)n, &d_in));
    GSX_CHECK(h.room(h.c->stage_out, 4 * (size_t)n, &d_out));
    GSX_CHECK(gsx_sog_quats_dev(h.c, d_in, n, d_out));
    GSX_CHECK(h.down(out4, d_out, 4 * (size_t)n));
    return h.sync();
}

}  // extern "C"
