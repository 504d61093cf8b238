// sor_grid.hip -- grid-binned EXACT k-nearest-neighbour mean distance.
//
// Replaces the hot loop of data_processor.py:160-173 (cKDTree build + query(k+1) + row
// mean) and supersedes the reference's approximate Taichi kernel gpu_ops.py:98-176 and
// its numpy hash-grid prep gpu_ops.py:203-237 (27 cells, K<=50, hash collisions; SURVEY
// F4/F5).  Results are bit-identical to the cKDTree path.
//
// Pipeline (all on one stream, no host round trip):
//   bbox_partial -> grid_params            per-axis min/max, cell edge h for ~m pts/cell
//   bucket_hist / bucket_offsets / bucket_scatter / bucket_sort
//                                          two-level counting sort into float4 {x,y,z,orig}: every
//                                          per-point atomic is an LDS atomic (see the kernels)
//   brick_plan (x2)                        plain single-cloud call, k <= 16: the bricks become runs of quarter-cell slabs along x
//                                          holding <= 64 queries (see "brick plan" below); every other call keeps the fixed bricks
//   knn_brick                              one WAVE per brick: 2x2x2 cells (~54 queries) or a planned run (~59)
//   knn_ring                               expanding-ring exact fallback for the few queries
//                                          whose (k+1)-th neighbour is farther than one cell
//
// knn_brick: the 64 lanes of a wave are 64 queries of one brick (2x2x2 cells for k <= 16, fewer
// cells for larger k).  The brick's neighbourhood (brick + 1 cell each way, 4x4x4 cells) is 16
// x-rows, each a CONTIGUOUS range of the sorted array, which the wave walks in lock step.
// Phase 1 only FILTERS: it builds a per-lane bit mask of the candidates
// whose squared distance is below r_safe^2 (32 candidates per word, words parked in LDS) -- for a
// batch whose words all fit the park with one v_mfma_f32_32x32x16_bf16 per 32 candidates x 32
// queries on bf16-split coordinates (see "MFMA phase-1 filter" below), otherwise with 6 f32 ops per
// candidate on scalar-cache loads and a sign-bit shift-in.  Phase 2 walks each lane's set bits
// (~4.19*m of ~512) with a private cursor, recomputes those distances in float64 exactly as
// cKDTree does and keeps the k+1 smallest in a register-resident sorted list.  A query is exact
// iff its (k+1)-th distance is <= r_safe = h*(1-1e-3): every point outside the searched cells is
// farther.
//
// Clouds the uniform grid cannot resolve (bounding box inflated by far outliers, clusters far
// denser than a cell) are handled by knn_grid_level's adaptive refinement: bricks that would be
// too expensive are deferred to a finer grid built on their neighbourhood, exactly.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "grid_policy.h"
#include "gsx_common.h"
#include "gsx_internal.h"
#include "knn_common.h"
#include "knn_mfma.h"
#include "sor_grid_params.h"

namespace gsx {


constexpr int MAX_DIM = 1024;       // cells per axis (keeps the cell-index rounding bound, see r_safe)
// (MAX_BUCKETS and MAX_BUCKET_CELLS, the two-level sort's limits: grid_policy.h, where they also bound a level's cells)
#ifndef GSX_BUCKET_POINTS
#define GSX_BUCKET_POINTS 4096
#endif
constexpr int BUCKET_POINTS = GSX_BUCKET_POINTS;   // target points per bucket (tuning builds: -DGSX_BUCKET_POINTS, with GSX_SORT_THREADS)
#ifndef GSX_BIN_TILE
#define GSX_BIN_TILE 8192
#endif
constexpr int BIN_TILE = GSX_BIN_TILE;    // points per workgroup tile in the coarse pass (4096 / 16384: no better)
constexpr int BRICK_THREADS = 256;  // 4 independent waves per workgroup
constexpr int HEAVY_RING_CANDIDATES = 1 << 16;
constexpr int HEAVY_CHUNK = 32768;  // points of the sorted array one wave of knn_heavy_scan covers (512 per lane: the
                                    // per-lane top list stops changing after the first few dozen, and the wave merge amortises)
#ifndef GSX_WCAP_BIG   // mask words parked per wave for the lists of more than 32 entries (round 5: 32 -- these kernels run two or three
#define GSX_WCAP_BIG 32   // waves per SIMD, LDS is not what limits them; a brick of more words is filtered by the float32 loop: k = 57 11.2 -> 7.8 ms)
#endif
#ifndef GSX_WCAP_MID   // ... and for 17 ... 32 entries (four waves per SIMD)
#define GSX_WCAP_MID 24
#endif
constexpr int WCAP = 24;            // mask words parked in LDS per wave between drains (6 KiB/wave)

// ---------------------------------------------------------------- bbox + grid params
struct GridParamArgs {   // what grid_params needs besides the partial boxes
    int n;
    double pts_per_cell;
    int cell_cap, debug_skip, share, nshares, defer_words;
    float parent_h;
    GridParams *gp;
    unsigned *devflags;
    double h_hint;   // > 0: cell edge suggested by the density probe of the parent level (never above the bbox-volume edge)
    // multi-GPU slab step (launch_knn_slab): the certificate's planes and counter (axis < 0: off) ...
    int cert_axis;
    float cert_lo, cert_hi;
    unsigned *cert_count;
    int plan_req = 0, plan_cap = 0;   // planned bricks asked for (the call allows them), entries the brick list has room for
#ifdef GSX_WAVE_STAMPS
    unsigned long long *stamps = nullptr;
    int stamps_cap = 0;
#endif
};
__device__ void grid_params_body(const float *part, int nparts, const GridParamArgs &a);

// The LAST workgroup to arrive (ticket in GridParams) turns the partial boxes into the grid parameters: a separate
// one-wave launch cost ~9 us per step -- 2.5 % of the 1M-splat step.
__global__ __launch_bounds__(256) void bbox_partial_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                           const float *__restrict__ z, int64_t stride, int n,
                                                           float *__restrict__ part, GridParamArgs gpa)
{
    __shared__ float red[7][4];
    float mn[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
    float mx[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    float bad = 0.0f;  // fminf/fmaxf drop NaNs silently, so non-finite input is tracked separately
    const int step = gridDim.x * blockDim.x;
    for (int64_t i0 = blockIdx.x * blockDim.x + threadIdx.x; i0 < n; i0 += 4 * (int64_t)step) {   // 12 loads in flight per lane
        float v[4][3];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t i = (int64_t)(i0 + u * step < n ? i0 + u * step : i0) * stride;   // (a repeated point changes no extremum)
            v[u][0] = x[i];
            v[u][1] = y[i];
            v[u][2] = z[i];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                mn[a] = fminf(mn[a], v[u][a]);
                mx[a] = fmaxf(mx[a], v[u][a]);
                bad = (fabsf(v[u][a]) < __builtin_inff()) ? bad : 1.0f;
            }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            mn[a] = fminf(mn[a], __shfl_xor(mn[a], off));
            mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], off));
        }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) bad = fmaxf(bad, __shfl_xor(bad, off));
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            red[a][w] = mn[a];
            red[3 + a][w] = mx[a];
        }
        red[6][w] = bad;
    }
    __syncthreads();
    if (threadIdx.x < 7) {
        float v = red[threadIdx.x][0];
        for (int i = 1; i < 4; ++i) v = threadIdx.x < 3 ? fminf(v, red[threadIdx.x][i]) : fmaxf(v, red[threadIdx.x][i]);
        __hip_atomic_store(&part[blockIdx.x * 7 + threadIdx.x], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // write-through
    }
    __shared__ unsigned s_last;
    __builtin_amdgcn_s_waitcnt(0);   // the write-through stores above have completed before the ticket (no L2 write-back needed)
    __syncthreads();
    if (threadIdx.x == 0) s_last = atomicAdd(&gpa.gp->ticket_bbox, 1u) == gridDim.x - 1 ? 1u : 0u;
    __syncthreads();
    if (!s_last) return;
    if (threadIdx.x == 0) gpa.gp->ticket_bbox = 0;
    if (threadIdx.x < 64) grid_params_body(part, (int)gridDim.x, gpa);
}

__device__ void grid_params_body(const float *part, int nparts, const GridParamArgs &a)
{
    const int n = a.n, cell_cap = a.cell_cap, debug_skip = a.debug_skip, share = a.share, nshares = a.nshares,
              defer_words = a.defer_words;
    const double pts_per_cell = a.pts_per_cell;
    const float parent_h = a.parent_h;
    GridParams *gp = a.gp;
    unsigned *devflags = a.devflags;
    const int lane = threadIdx.x;
    // all 7 x ceil(nparts/64) loads are independent: issue them together (reducing one value at a time
    // serialised 7 round trips and made this one-wave kernel 9 us, 2 % of the 1M-splat step)
    float v[7] = {__builtin_inff(), __builtin_inff(), __builtin_inff(), -__builtin_inff(), -__builtin_inff(),
                  -__builtin_inff(), -__builtin_inff()};
    // (written by other workgroups: device-scope loads, which the compiler keeps in program order -- so eight
    // partial boxes are requested back to back before the first one is consumed: 2 round trips for 1024 parts, not 16)
    for (int i0 = lane; i0 < nparts; i0 += 64 * 8) {
        float t[8][7];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = i0 + 64 * u < nparts ? i0 + 64 * u : i0;
#pragma unroll
            for (int a = 0; a < 7; ++a) t[u][a] = __hip_atomic_load(&part[i * 7 + a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
            for (int a = 0; a < 7; ++a) v[a] = a < 3 ? fminf(v[a], t[u][a]) : fmaxf(v[a], t[u][a]);
    }
#pragma unroll
    for (int a = 0; a < 7; ++a)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float o = __shfl_xor(v[a], off);
            v[a] = a < 3 ? fminf(v[a], o) : fmaxf(v[a], o);
        }
    if (lane != 0) return;
    double e[3] = {(double)v[3] - (double)v[0], (double)v[4] - (double)v[1], (double)v[5] - (double)v[2]};
    double vol = 1.0, emax = 0.0;
    int nd = 0;
    for (int a = 0; a < 3; ++a) {
        if (e[a] > 0.0) { vol *= e[a]; ++nd; }
        emax = e[a] > emax ? e[a] : emax;
    }
    double h;
    if (nd == 0 || !(emax < 1e300)) {
        h = 1.0;
    } else {
        double per = vol * pts_per_cell / (double)(n > 0 ? n : 1);
        h = nd == 3 ? cbrt(per) : (nd == 2 ? sqrt(per) : per);
        if (a.h_hint > 0.0 && a.h_hint < h) h = a.h_hint;   // any edge is valid (exactness does not depend on it): section 5.5
        double hmin = emax / (double)(MAX_DIM - 1);
        if (!(h > hmin)) h = hmin;
    }
    int nx, ny, nz;
    int bg = 1, bny = 1, bnz = 1;
    long long padded = 0;
    float inv_h;
    for (int it = 0; it < 256; ++it) {
        inv_h = (float)(1.0 / h);
        // dims from the SAME f32 arithmetic the kernels use, so no point ever indexes past the grid
        nx = (int)((v[3] - v[0]) * inv_h) + 1;
        ny = (int)((v[4] - v[1]) * inv_h) + 1;
        nz = (int)((v[5] - v[2]) * inv_h) + 1;
        bool ok = nx <= MAX_DIM && ny <= MAX_DIM && nz <= MAX_DIM && nx > 0 && ny > 0 && nz > 0;
        if (ok) {
            // bucket = bg x bg x-rows, ~BUCKET_POINTS points; at most MAX_BUCKETS buckets, MAX_BUCKET_CELLS cells each
            double per_row = (double)nx * pts_per_cell;
            bg = (int)(sqrt((double)BUCKET_POINTS / (per_row > 1.0 ? per_row : 1.0)) + 0.5);
            if (bg < 1) bg = 1;
            if (bg > (ny > nz ? ny : nz)) bg = ny > nz ? ny : nz;  // never wider than the grid itself
            while (bg > 1 && (long long)bg * bg * nx > MAX_BUCKET_CELLS) --bg;
            for (;;) {
                bny = (ny + bg - 1) / bg;
                bnz = (nz + bg - 1) / bg;
                if ((long long)bny * bnz <= MAX_BUCKETS) break;
                ++bg;
            }
            padded = (long long)bny * bnz * bg * bg * nx;
            ok = (long long)bg * bg * nx <= MAX_BUCKET_CELLS && padded <= (long long)cell_cap;
        }
        if (ok) break;
        h *= 1.1;
    }
    bool bad = v[6] > 0.0f;  // NaN or inf anywhere in the cloud
    for (int a = 0; a < 6; ++a) bad |= !(fabsf(v[a]) < 3.0e38f);
    if (bad || !(nx > 0 && ny > 0 && nz > 0) || padded <= 0 || padded > (long long)cell_cap ||
        (long long)bg * bg * nx > MAX_BUCKET_CELLS) {
        // no grid can be built; an exhaustive search would be O(N^2): refuse instead (host raises)
        bad = true;
        nx = ny = nz = 1;
        bg = bny = bnz = 1;
        inv_h = 0.0f;
    }
    gp->ox = v[0]; gp->oy = v[1]; gp->oz = v[2];
    gp->inv_h = inv_h;
    gp->h = (float)h;
    gp->nx = nx; gp->ny = ny; gp->nz = nz;
    gp->bk_g = bg; gp->bk_ny = bny; gp->bk_nz = bnz;
    gp->bk_count = bny * bnz;
    gp->bk_cells = bg * bg * nx;
    gp->ncells = gp->bk_count * gp->bk_cells;
    // brick = the cells one wave owns.  Its ~pts_per_cell * cells queries should fill 64 lanes in ONE
    // batch (a second batch repeats the whole neighbourhood scan): 2x2x2 cells up to ~8 pts/cell
    // (k <= 16), then 2x2x1, 2x1x1, 1x1x1 as k -- hence the cell population -- grows.
    int bdx = 2, bdy = 2, bdz = 2;
    if (pts_per_cell * 8.0 > 66.0) bdz = 1;
    if (pts_per_cell * 4.0 > 66.0) bdy = 1;
    if (pts_per_cell * 2.0 > 66.0) bdx = 1;
    gp->bdx = bdx; gp->bdy = bdy; gp->bdz = bdz;
    gp->nbx = (nx + bdx - 1) / bdx; gp->nby = (ny + bdy - 1) / bdy; gp->nbz = (nz + bdz - 1) / bdz;
    gp->nbricks = bad ? 0 : gp->nbx * gp->nby * gp->nbz;
    // planned bricks: the quarter index floor(fl(fl(x-o) * 4 inv_h)) has 4 nx values, and its rounding bound (see r_safe
    // below) is the cell index's with dim = 4 nx -- so 4 nx <= MAX_DIM.  Larger grids keep the fixed bricks.
    gp->plan = (a.plan_req && !bad && bdx == 2 && bdy == 2 && bdz == 2 && 4 * nx <= MAX_DIM) ? 1 : 0;
    gp->plan_cap = a.plan_cap;
    // bricks are numbered z-major, so a contiguous share is a slab of the cloud
    gp->part_lo = (int)(((long long)gp->nbricks * share) / nshares);
    gp->part_hi = (int)(((long long)gp->nbricks * (share + 1)) / nshares);
    gp->bad_input = bad ? 1u : 0u;
    if (bad) atomicOr(devflags, 1u);  // reported by gsx_ctx_check; knn_ring fills the output with NaN
    gp->debug_skip = debug_skip;
    // r_safe: |p-q| <= H*h'*(1-1e-3) implies the cell coordinates differ by <= H per axis: the
    // f32 cell index floor(fl(fl(x-o)*inv_h)) is monotone and off by < dim*2^-22 <= 2.5e-4 cells.
    double hp = inv_h > 0.0f ? 1.0 / (double)inv_h : 0.0;
    double r1 = hp * (1.0 - 1e-3);
    gp->hprime = hp;
    gp->r1sq = r1 * r1;
    gp->tau1 = bound_from(r1 * r1);
    // refinement only pays while the cells keep shrinking (a cloud of identical points never would)
    gp->defer_words = (parent_h > 0.0f && !((float)h < 0.8f * parent_h)) ? 0 : defer_words;
    gp->fail_count = 0;
    gp->exhaustive_count = 0;
    gp->extra_count = 0;
    gp->heavy_limit = defer_words > 0 ? HEAVY_RING_CANDIDATES : 0;  // both need the host in the loop
    gp->heavy_count = 0;
    gp->ring2_count = 0;
    for (int a = 0; a < 3; ++a) {
        gp->qb_lo[a] = __builtin_inff();
        gp->qb_hi[a] = -__builtin_inff();
    }
    gp->deferred_count = 0;
    gp->sub_count = 0;
    gp->sub_queries = 0;
    gp->refined_count = 0;
    gp->cert_axis = a.cert_axis;
    gp->cert_lo = a.cert_lo;
    gp->cert_hi = a.cert_hi;
    gp->cert_count = a.cert_count;
#ifdef GSX_WAVE_STAMPS
    gp->stamps = a.stamps;
    gp->stamps_cap = a.stamps_cap;
#endif
    for (int i = 0; i < 8; ++i) {
        gp->brick_ctr[i * 32] = 0;
        gp->extra_ctr[i * 32] = 0;
        gp->ring_ctr[i * 32] = 0;
        gp->ringf_ctr[i * 32] = 0;
    }

}

// The box is known (multi-GPU slab step: the all-reduced global box, cut to the slab's bins along the partition axis):
// no pass over the rows, one wave writes the grid parameters.
__global__ __launch_bounds__(64) void grid_params_known_box_kernel(KnownBox kb, float *__restrict__ part, GridParamArgs gpa)
{
    if (threadIdx.x < 7) {
        const int a = threadIdx.x;
        float v = a < 3 ? -kb.b7[a] : kb.b7[a];          // minima | maxima | non-finite flag
        if (a == kb.axis) v = fmaxf(v, kb.lo);
        if (a == 3 + kb.axis) v = fminf(v, kb.hi);
        __hip_atomic_store(&part[a], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
    grid_params_body(part, 1, gpa);
}

__device__ __forceinline__ int cell_coord(float v, float o, float inv_h, int dim)
{
    int c = (int)((v - o) * inv_h);
    return min(max(c, 0), dim - 1);
}

// Cell index space is BUCKET-MAJOR: all cells of bucket (by, bz) are contiguous, inside a bucket the
// x-rows follow each other, inside a row the cells run along x.  Every x-row of cells is therefore
// still one contiguous range of the sorted array (what knn_brick / knn_ring walk), and a bucket's
// cells can be laid out by the workgroup that sorts the bucket without any global scan.
__device__ __forceinline__ int row_base(const GridParams &g, int cy, int cz)
{
    const int by = cy / g.bk_g, bz = cz / g.bk_g;
    return (bz * g.bk_ny + by) * g.bk_cells + ((cz - bz * g.bk_g) * g.bk_g + (cy - by * g.bk_g)) * g.nx;
}

__device__ __forceinline__ int bucket_of(const GridParams &g, int cy, int cz)
{
    return (cz / g.bk_g) * g.bk_ny + cy / g.bk_g;
}

// ---------------------------------------------------------------- two-level counting sort by cell
// The points arrive in arbitrary order.  A one-level counting sort needs one returning device-scope
// atomic and one random 16-byte write per point (measured 0.69 ms per 10M points: the L2 atomic
// units, not HBM, are the limit).  Two levels keep every per-point atomic in LDS:
//   A1 bucket_hist    one BIN_TILE-point tile per workgroup -> LDS histogram over <= 4096 buckets ->
//                     the tile's row of u16 counts in tile_cnt[slot][bucket] (plain stores, no atomics)
//   A2 bucket_offsets one workgroup per strip of 16 buckets: exclusive scan down each bucket's column of
//                     tile counts -> tile_off[slot][bucket] and the bucket's size; the last workgroup
//                     scans the sizes into bk_start
//   A3 bucket_scatter same tiles: rank inside the (tile, bucket) run with LDS atomics, stage the float4
//                     {x,y,z,orig} records in LDS in bucket order, write them to bk_start[b] +
//                     tile_off[slot][b] + rank run by run -- no global atomic
//   B  bucket_sort    one workgroup per bucket: LDS histogram over the bucket's cells, LDS scan ->
//                     cell_start (bucket base + local prefix, no global scan), LDS cursors -> final
//                     position; reads are contiguous, writes stay inside the bucket's ~64 KiB window.
// Inside a bucket the runs of the tiles are laid out in SLOT order: the tiles of one XCD (workgroup i runs on XCD i % 8)
// first, in tile order.  A run is ~2.5 points (40 B), so a 128-B line of the bucket-grouped array holds the runs of
// ~3 tiles; in slot order these tiles run on the same XCD at about the same time and their partial lines merge in that
// XCD's L2 before they are written back (runs reserved by device atomics, in arrival order, left L2 as 32-B pieces:
// 2.2x the payload; plain tile order costs ~35 us per 10M points, profiles/r08_binning_ab.txt).  The order only decides
// where a point lands inside its bucket; bucket_sort re-sorts the bucket.
#ifndef GSX_BIN_XCDS
#define GSX_BIN_XCDS 8
#endif
constexpr int BIN_XCDS = GSX_BIN_XCDS;   // (1: the runs in plain tile order)

// the ONE partition of [0, n) into tiles that bucket_hist, bucket_offsets and bucket_scatter share: tile t = workgroup t
// covers [t * BIN_TILE, min(n, (t + 1) * BIN_TILE)) and owns row slot(t) of tile_cnt / tile_off
struct BinTiles {
    int ntiles, per_xcd;   // slots = BIN_XCDS * per_xcd >= ntiles; the slots past the last tile hold no tile
    __host__ __device__ static BinTiles of(int n)
    {
        const int nt = (n + BIN_TILE - 1) / BIN_TILE;
        return BinTiles{nt, (nt + BIN_XCDS - 1) / BIN_XCDS};
    }
    __host__ __device__ int slots() const { return BIN_XCDS * per_xcd; }
    __host__ __device__ int slot(int t) const { return (t % BIN_XCDS) * per_xcd + t / BIN_XCDS; }
    __host__ __device__ int tile(int s) const { return (s % per_xcd) * BIN_XCDS + s / per_xcd; }   // >= ntiles: empty slot
};

__global__ __launch_bounds__(256) void bucket_hist_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                          const float *__restrict__ z, int64_t stride, int first, int n,
                                                          const GridParams *__restrict__ gp, unsigned short *__restrict__ tile_cnt)
{
    __shared__ unsigned hist[MAX_BUCKETS];
    const GridParams g = *gp;
    if (g.bad_input) return;
    const BinTiles bt = BinTiles::of(n);
    const int t = blockIdx.x;
    if (t >= bt.ntiles) return;
    for (int i = threadIdx.x; i < g.bk_count; i += 256) hist[i] = 0;
    __syncthreads();
    const int lo = t * BIN_TILE, hi = min(n, lo + BIN_TILE);
    for (int i0 = lo + threadIdx.x; i0 < hi; i0 += 2048) {   // 16 independent loads in flight per lane
        float py[8], pz[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = min(i0 + 256 * u, hi - 1);
            const int64_t s = (int64_t)(first + i) * stride;
            py[u] = y[s];
            pz[u] = z[s];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (i0 + 256 * u < hi)
                atomicAdd(&hist[bucket_of(g, cell_coord(py[u], g.oy, g.inv_h, g.ny), cell_coord(pz[u], g.oz, g.inv_h, g.nz))], 1u);
    }
    __syncthreads();
    static_assert(BIN_TILE <= 65535, "a tile's per-bucket count is stored as u16");
    unsigned short *row = tile_cnt + (size_t)bt.slot(t) * g.bk_count;
    for (int i = threadIdx.x; i < g.bk_count; i += 256) row[i] = (unsigned short)hist[i];
}

__device__ __forceinline__ unsigned block_exclusive_scan_256(unsigned v, unsigned *total, unsigned *wsum /*[4]*/)
{
    // inclusive scan inside the wave
    unsigned inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        unsigned o = __shfl_up(inc, off);
        if ((int)(threadIdx.x & 63) >= off) inc += o;
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 63) wsum[w] = inc;
    __syncthreads();
    unsigned base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        unsigned s = wsum[i];
        if (i < w) base += s;
        tot += s;
    }
    *total = tot;
    __syncthreads();
    return base + inc - v;
}

constexpr int OFFSETS_THREADS = 1024;
constexpr int OFFSETS_BUCKETS = 16;                                       // buckets of one workgroup (a strip of the tables)
constexpr int OFFSETS_CHUNKS = OFFSETS_THREADS / OFFSETS_BUCKETS;         // slot ranges of a strip, one per lane of a bucket

// bk_start[0..bk_count] = exclusive scan of bk_size.
// Run by the OFFSETS_THREADS threads of bucket_offsets' last workgroup; bk_size was written with agent-scope (write-through) stores.
__device__ void bucket_scan_body(int nb, const unsigned *bk_size, unsigned *bk_start)
{
    constexpr int T = OFFSETS_THREADS, W = T / 64, PER = MAX_BUCKETS / T;
    static_assert(PER * T == MAX_BUCKETS, "bucket_scan_body preloads MAX_BUCKETS / T values per thread");
    __shared__ unsigned wsum[W];
    unsigned vals[PER];   // every bucket size requested before the first scan round (one round trip)
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const int i = T * u + (int)threadIdx.x;
        vals[u] = i < nb ? __hip_atomic_load(&bk_size[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
    }
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    unsigned carry = 0;
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        if (T * u >= nb) break;   // block-uniform
        const unsigned v = vals[u];
        unsigned inc = v;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned o = __shfl_up(inc, off);
            if (lane >= off) inc += o;
        }
        if (lane == 63) wsum[w] = inc;
        __syncthreads();
        unsigned base = 0, tot = 0;
#pragma unroll
        for (int i = 0; i < W; ++i) {
            const unsigned x = wsum[i];
            if (i < w) base += x;
            tot += x;
        }
        __syncthreads();
        const int i = T * u + (int)threadIdx.x;
        if (i < nb) bk_start[i] = carry + base + inc - v;
        carry += tot;
    }
    if (threadIdx.x == 0) bk_start[nb] = carry;
}

constexpr int OFFSETS_UNROLL = 24;   // table loads in flight per lane

// One workgroup per strip of OFFSETS_BUCKETS buckets: lane (chunk c, bucket j) sums tile_cnt[s][b0 + j] over its
// contiguous range of slots (16 lanes read 32 contiguous bytes of a row), the chunk sums are scanned in LDS, and a second
// sweep over the same rows (now L2 hits) writes the running sums to tile_off[s][b0 + j] (64 contiguous bytes per row).
// Workgroup i runs on XCD i % 8: the strips are dealt so that each XCD owns one contiguous range of buckets.  The last
// workgroup to arrive (ticket in GridParams) turns the bucket sizes into bk_start.
__global__ __launch_bounds__(OFFSETS_THREADS) void bucket_offsets_kernel(int n, GridParams *__restrict__ gp,
                                                                         const unsigned short *__restrict__ tile_cnt,
                                                                         unsigned *__restrict__ tile_off, unsigned *__restrict__ bk_size,
                                                                         unsigned *__restrict__ bk_start)
{
    __shared__ unsigned part[OFFSETS_CHUNKS][OFFSETS_BUCKETS];
    const GridParams g = *gp;
    if (g.bad_input) return;
    const int nb = g.bk_count;
    const BinTiles bt = BinTiles::of(n);
    const int strips = (nb + OFFSETS_BUCKETS - 1) / OFFSETS_BUCKETS;
    const int per_xcd = (strips + BIN_XCDS - 1) / BIN_XCDS;   // (the grid has room for all: MAX_BUCKETS / OFFSETS_BUCKETS)
    const int strip = (int)(blockIdx.x % BIN_XCDS) * per_xcd + (int)(blockIdx.x / BIN_XCDS);
    const int j = threadIdx.x % OFFSETS_BUCKETS, c = threadIdx.x / OFFSETS_BUCKETS;
    const int b = strip * OFFSETS_BUCKETS + j;
    const bool active = (int)(blockIdx.x / BIN_XCDS) < per_xcd && strip < strips;   // block-uniform
    if (active) {
        const bool own = b < nb;
        const int slots = bt.slots(), per_chunk = (slots + OFFSETS_CHUNKS - 1) / OFFSETS_CHUNKS;
        const int s_lo = min(slots, c * per_chunk), s_hi = min(slots, s_lo + per_chunk);
        auto count = [&](int s) -> unsigned {
            return own && s < s_hi && bt.tile(s) < bt.ntiles ? (unsigned)tile_cnt[(size_t)s * nb + b] : 0u;
        };
        // a chunk of at most OFFSETS_UNROLL slots (10M points: 20) is loaded once and kept in registers for the second sweep
        const bool held = per_chunk <= OFFSETS_UNROLL;   // block-uniform
        unsigned hv[OFFSETS_UNROLL];
        unsigned sum = 0;
        for (int s0 = s_lo; s0 < s_hi; s0 += OFFSETS_UNROLL) {
#pragma unroll
            for (int u = 0; u < OFFSETS_UNROLL; ++u) hv[u] = count(s0 + u);
#pragma unroll
            for (int u = 0; u < OFFSETS_UNROLL; ++u) sum += hv[u];
        }
        part[c][j] = sum;
        __syncthreads();
        if (threadIdx.x < 64 * OFFSETS_BUCKETS) {   // wave jj scans the OFFSETS_CHUNKS (= 64) chunk sums of bucket jj
            static_assert(OFFSETS_CHUNKS == 64, "one wave scans the chunk sums of one bucket");
            const int jj = threadIdx.x >> 6, lane = threadIdx.x & 63;
            const unsigned v = part[lane][jj];
            unsigned inc = v;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned o = __shfl_up(inc, off);
                if (lane >= off) inc += o;
            }
            part[lane][jj] = inc - v;
            const int bb = strip * OFFSETS_BUCKETS + jj;
            if (lane == 63 && bb < nb) __hip_atomic_store(&bk_size[bb], inc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // write-through
        }
        __syncthreads();
        unsigned run = part[c][j];
        for (int s0 = s_lo; s0 < s_hi; s0 += OFFSETS_UNROLL) {
            unsigned v[OFFSETS_UNROLL];
#pragma unroll
            for (int u = 0; u < OFFSETS_UNROLL; ++u) v[u] = held ? hv[u] : count(s0 + u);
#pragma unroll
            for (int u = 0; u < OFFSETS_UNROLL; ++u) {
                const int s = s0 + u;
                if (own && s < s_hi && bt.tile(s) < bt.ntiles) tile_off[(size_t)s * nb + b] = run;
                run += v[u];
            }
        }
    }
    if (!active) return;   // (only the workgroups that own a strip take a ticket: one returning atomic each on one word)
    __shared__ unsigned s_last;
    __builtin_amdgcn_s_waitcnt(0);   // the write-through stores above have completed before the ticket (no L2 write-back needed)
    __syncthreads();
    if (threadIdx.x == 0) s_last = atomicAdd(&gp->ticket_hist, 1u) == (unsigned)strips - 1 ? 1u : 0u;
    __syncthreads();
    if (!s_last) return;
    if (threadIdx.x == 0) gp->ticket_hist = 0;
    bucket_scan_body(nb, bk_size, bk_start);
}

#ifndef GSX_SCATTER_THREADS
#define GSX_SCATTER_THREADS 1024
#endif
constexpr int SCATTER_THREADS = GSX_SCATTER_THREADS;
constexpr int SCATTER_PPT = BIN_TILE / SCATTER_THREADS;  // points per thread, kept in registers
static_assert(SCATTER_PPT * SCATTER_THREADS == BIN_TILE, "a scatter workgroup covers exactly one tile");

// One BIN_TILE-point tile per workgroup of 1024 threads, every point read ONCE: coordinates, bucket and the rank the
// returning LDS atomic hands out stay in registers across the count.  The base of every run of the tile,
// bk_start[b] + tile_off[slot][b], is loaded with the points: nothing waits on another workgroup.  The records are then
// staged in LDS in bucket order (local prefix of the tile's histogram + rank) and streamed out in that order: the lanes of
// one store instruction write whole runs, one L1 -> L2 request per run and line instead of one per record (a run is
// ~2.5 records).  (Round 1 swept the tile twice with 256 threads: 0.21 ms per 10M points.)
__global__ __launch_bounds__(SCATTER_THREADS) void bucket_scatter_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                             const float *__restrict__ z, int64_t stride, int first, int n,
                                                             const GridParams *__restrict__ gp, const unsigned *__restrict__ bk_start,
                                                             const unsigned *__restrict__ tile_off, float4 *__restrict__ out,
                                                             int ref_only_from)
{
    constexpr int BPT = MAX_BUCKETS / SCATTER_THREADS;   // buckets per thread
    static_assert(BIN_TILE * sizeof(float4) + MAX_BUCKETS * sizeof(unsigned) <= 160 * 1024, "the stage and the table fit the LDS");
    static_assert(BPT * SCATTER_THREADS == MAX_BUCKETS, "every thread owns the same number of buckets");
    __shared__ float4 stage[BIN_TILE];        // the tile's records in bucket order
    __shared__ unsigned tab[MAX_BUCKETS];     // count -> local start -> global start minus local start, per bucket
    unsigned *wsum = reinterpret_cast<unsigned *>(stage);   // scan scratch: the stage is written after the scan
    const GridParams g = *gp;
    if (g.bad_input) return;
    const int nb = g.bk_count;
    const BinTiles bt = BinTiles::of(n);
    const int t = blockIdx.x;
    if (t >= bt.ntiles) return;
    const unsigned *off = tile_off + (size_t)bt.slot(t) * nb;
    unsigned gb[BPT];
#pragma unroll
    for (int u = 0; u < BPT; ++u) {
        const int i = u * SCATTER_THREADS + (int)threadIdx.x;
        gb[u] = i < nb ? bk_start[i] + off[i] : 0u;
        if (i < nb) tab[i] = 0;
    }
    const int lo = t * BIN_TILE, hi = min(n, lo + BIN_TILE);
    float px[SCATTER_PPT], py[SCATTER_PPT], pz[SCATTER_PPT];
    int bk[SCATTER_PPT];
    unsigned rk[SCATTER_PPT];
#pragma unroll
    for (int u = 0; u < SCATTER_PPT; ++u) {   // all loads of the tile in flight
        const int i = min(lo + u * SCATTER_THREADS + (int)threadIdx.x, hi - 1);
        const int64_t sidx = (int64_t)(first + i) * stride;
        px[u] = x[sidx];
        py[u] = y[sidx];
        pz[u] = z[sidx];
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < SCATTER_PPT; ++u) {
        bk[u] = bucket_of(g, cell_coord(py[u], g.oy, g.inv_h, g.ny), cell_coord(pz[u], g.oz, g.inv_h, g.nz));
        rk[u] = lo + u * SCATTER_THREADS + (int)threadIdx.x < hi ? atomicAdd(&tab[bk[u]], 1u) : 0u;
    }
    __syncthreads();
    // exclusive scan of the tile's histogram in place (each entry is read and rewritten by the thread that owns it)
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    unsigned carry = 0;
#pragma unroll
    for (int u = 0; u < BPT; ++u) {
        if (u * SCATTER_THREADS >= nb) break;   // block-uniform
        const int i = u * SCATTER_THREADS + (int)threadIdx.x;
        const unsigned v = i < nb ? tab[i] : 0u;
        unsigned inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned up = __shfl_up(inc, o);
            if (lane >= o) inc += up;
        }
        if (lane == 63) wsum[w] = inc;
        __syncthreads();
        unsigned base = 0, tot = 0;
#pragma unroll
        for (int k = 0; k < SCATTER_THREADS / 64; ++k) {
            const unsigned q = wsum[k];
            if (k < w) base += q;
            tot += q;
        }
        __syncthreads();
        const unsigned ex = carry + base + inc - v;
        if (i < nb) tab[i] = ex;
        gb[u] -= ex;   // record j of the stage goes to gb + j
        carry += tot;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < SCATTER_PPT; ++u) {
        const int i = lo + u * SCATTER_THREADS + (int)threadIdx.x;
        if (i < hi)
            // points from ref_only_from on are REFERENCE-ONLY (the halo of a multi-GPU slab): bit 31 of
            // the index word keeps their lanes dead in knn_brick
            stage[tab[bk[u]] + rk[u]] = make_float4(px[u], py[u], pz[u],
                                                    __uint_as_float((unsigned)(first + i) | (i >= ref_only_from ? 0x80000000u : 0u)));
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < BPT; ++u) {
        const int i = u * SCATTER_THREADS + (int)threadIdx.x;
        if (i < nb) tab[i] = gb[u];
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < SCATTER_PPT; ++u) {
        const int j = u * SCATTER_THREADS + (int)threadIdx.x;
        if (j < hi - lo) {
            const float4 r = stage[j];
            out[tab[bucket_of(g, cell_coord(r.y, g.oy, g.inv_h, g.ny), cell_coord(r.z, g.oz, g.inv_h, g.nz))] + j] = r;
        }
    }
}

#ifndef GSX_SORT_THREADS
#define GSX_SORT_THREADS 512
#endif
#ifndef GSX_SORT_PPT
#define GSX_SORT_PPT 16
#endif
constexpr int SORT_THREADS = GSX_SORT_THREADS;
constexpr int SORT_PPT = GSX_SORT_PPT;                // points per thread kept in registers
constexpr unsigned SORT_CAP = SORT_THREADS * SORT_PPT;  // buckets up to 8192 points are read ONCE

// Quarter index along x: q4 >> 2 IS cell_coord(x) -- multiplying inv_h by 4 is exact in f32, so (x - o) * (4 inv_h) is exactly
// four times the product cell_coord truncates, and floor(4t) >> 2 = floor(t) for t >= 0; the clamps agree as well.
__device__ __forceinline__ int quarter_coord(float v, float o, float inv_h, int dim)
{
    int c = (int)((v - o) * (4.0f * inv_h));
    return min(max(c, 0), 4 * dim - 1);
}

// FINE (planned bricks): the bins are the quarter-cell slabs along x, four per cell, in cell order -- the points of a cell
// stay one contiguous range and cell_start keeps its meaning (every fourth bin start); fine_start[4 c + j] is where quarter j
// of cell c begins.  4 x MAX_BUCKET_CELLS counters are 64 KiB of LDS: two workgroups per CU, as the registers allow anyway.
template <bool FINE>
__global__ __launch_bounds__(SORT_THREADS) void bucket_sort_kernel(const GridParams *__restrict__ gp,
                                                          const unsigned *__restrict__ bk_start,
                                                          const float4 *__restrict__ in, float4 *__restrict__ out,
                                                          unsigned *__restrict__ cell_start, unsigned big_limit,
                                                          unsigned *__restrict__ fine_start)
{
    constexpr int SUB = FINE ? 4 : 1;
    __shared__ unsigned cnt[SUB * MAX_BUCKET_CELLS];
    __shared__ unsigned wsum[SORT_THREADS / 64];
    const GridParams g = *gp;
    const int b = blockIdx.x;
    if (g.bad_input || b >= g.bk_count) return;
    const int ncell = g.bk_cells;
    const int cells = SUB * ncell;   // bins of this bucket
    const unsigned s0 = bk_start[b], s1 = bk_start[b + 1];
    if (b == g.bk_count - 1 && threadIdx.x == 0) {
        cell_start[(size_t)g.bk_count * ncell] = s1;
        if (FINE) fine_start[(size_t)g.bk_count * cells] = s1;
    }
    if (s1 - s0 > big_limit) return;  // sorted by the multi-workgroup path below
    const int by = b % g.bk_ny, bz = b / g.bk_ny;
    for (int i = threadIdx.x; i < cells; i += SORT_THREADS) cnt[i] = 0;
    __syncthreads();
    auto local_cell = [&](const float4 p) {
        const int cx = FINE ? quarter_coord(p.x, g.ox, g.inv_h, g.nx) : cell_coord(p.x, g.ox, g.inv_h, g.nx);
        const int cy = cell_coord(p.y, g.oy, g.inv_h, g.ny);
        const int cz = cell_coord(p.z, g.oz, g.inv_h, g.nz);
        return ((cz - bz * g.bk_g) * g.bk_g + (cy - by * g.bk_g)) * (SUB * g.nx) + cx;
    };
    const bool fits = s1 - s0 <= SORT_CAP;  // block-uniform: the bucket's points, cells and ranks stay in registers
    float4 p[SORT_PPT];
    int cell[SORT_PPT];
    unsigned rk[SORT_PPT];
    if (fits) {
#pragma unroll
        for (int u = 0; u < SORT_PPT; ++u) p[u] = in[min(s0 + u * SORT_THREADS + threadIdx.x, s1 - 1)];
#pragma unroll
        for (int u = 0; u < SORT_PPT; ++u) {
            cell[u] = local_cell(p[u]);
            rk[u] = s0 + u * SORT_THREADS + threadIdx.x < s1 ? atomicAdd(&cnt[cell[u]], 1u) : 0u;
        }
    } else {
        for (unsigned i = s0 + threadIdx.x; i < s1; i += SORT_THREADS) atomicAdd(&cnt[local_cell(in[i])], 1u);
    }
    __syncthreads();
    // exclusive scan over the bucket's cells: each thread owns a contiguous segment
    const int seg = (cells + SORT_THREADS - 1) / SORT_THREADS;
    const int c0 = min(cells, (int)threadIdx.x * seg), c1 = min(cells, c0 + seg);
    unsigned sum = 0;
    for (int c = c0; c < c1; ++c) sum += cnt[c];
    // inclusive scan inside the wave, then across the SORT_THREADS / 64 waves
    unsigned inc = sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        unsigned o = __shfl_up(inc, off);
        if ((int)(threadIdx.x & 63) >= off) inc += o;
    }
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 63) wsum[wv] = inc;
    __syncthreads();
    unsigned run = inc - sum;
    for (int i = 0; i < wv; ++i) run += wsum[i];
    __syncthreads();
    for (int c = c0; c < c1; ++c) {
        const unsigned v = cnt[c];
        cnt[c] = run;   // becomes the start (fits) / the cursor (two-pass) of the cell
        run += v;
    }
    __syncthreads();
    unsigned *cs = cell_start + (size_t)b * ncell;
    for (int i = threadIdx.x; i < ncell; i += SORT_THREADS) cs[i] = s0 + cnt[SUB * i];
    if (FINE) {
        unsigned *fs = fine_start + (size_t)b * cells;
        for (int i = threadIdx.x; i < cells; i += SORT_THREADS) fs[i] = s0 + cnt[i];
    }
    if (fits) {
#pragma unroll
        for (int u = 0; u < SORT_PPT; ++u)
            if (s0 + u * SORT_THREADS + threadIdx.x < s1) out[s0 + cnt[cell[u]] + rk[u]] = p[u];
    } else {
        __syncthreads();
        for (unsigned i = s0 + threadIdx.x; i < s1; i += SORT_THREADS) {
            const float4 q = in[i];
            out[s0 + atomicAdd(&cnt[local_cell(q)], 1u)] = q;
        }
    }
}

// ---- oversized buckets (adaptive mode only) -------------------------------------------------------
// bucket_sort is one workgroup per bucket, sized for ~4096 points.  When far outliers inflate the
// bounding box the whole scene lands in a handful of cells, i.e. ONE bucket holds millions of points
// and that workgroup alone took 4.5 of the 7.5 ms of a refined 1M-splat run (40 of 53 ms at 10M).
// Buckets above BIG_BUCKET points are instead sorted by all workgroups: every 8192-point chunk of the
// bucket-grouped array counts its points per cell into the (zeroed) cell_start entries of the
// bucket, one workgroup per big bucket turns the counts into cell starts + global cursors, and the
// chunks scatter into runs reserved with one returning atomic per (chunk, non-empty cell).
constexpr unsigned BIG_BUCKET = 32768;
constexpr int BIG_CHUNK = 8192;

// first bucket whose range contains position pos: largest b with bk_start[b] <= pos
__device__ __forceinline__ int bucket_containing(const unsigned *bk_start, int nb, unsigned pos)
{
    int lo = 0, hi = nb;  // bk_start[nb] = n
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (bk_start[mid] <= pos) lo = mid; else hi = mid;
    }
    return lo;
}

template <bool SCATTER>
__global__ __launch_bounds__(256) void big_bucket_kernel(const GridParams *__restrict__ gp, const unsigned *__restrict__ bk_start,
                                                         int n, const float4 *__restrict__ in, float4 *__restrict__ out,
                                                         unsigned *cell_start /* counts (pass 1) */,
                                                         unsigned *cursor /* global cursors (pass 2) */)
{
    __shared__ unsigned cnt[MAX_BUCKET_CELLS];
    __shared__ unsigned base[SCATTER ? MAX_BUCKET_CELLS : 1];
    const GridParams g = *gp;
    if (g.bad_input) return;
    const unsigned lo = (unsigned)blockIdx.x * BIG_CHUNK;
    if (lo >= (unsigned)n) return;
    const unsigned hi = min((unsigned)n, lo + BIG_CHUNK);
    const int cells = g.bk_cells;
    for (int b = bucket_containing(bk_start, g.bk_count, lo); b < g.bk_count; ++b) {  // block-uniform
        const unsigned s0 = bk_start[b], s1 = bk_start[b + 1];
        if (s0 >= hi) break;
        if (s1 - s0 <= BIG_BUCKET) continue;
        const unsigned p0 = max(lo, s0), p1 = min(hi, s1);
        const int by = b % g.bk_ny, bz = b / g.bk_ny;
        auto local_cell = [&](const float4 p) {
            const int cx = cell_coord(p.x, g.ox, g.inv_h, g.nx);
            const int cy = cell_coord(p.y, g.oy, g.inv_h, g.ny);
            const int cz = cell_coord(p.z, g.oz, g.inv_h, g.nz);
            return ((cz - bz * g.bk_g) * g.bk_g + (cy - by * g.bk_g)) * g.nx + cx;
        };
        for (int i = threadIdx.x; i < cells; i += 256) cnt[i] = 0;
        __syncthreads();
        for (unsigned i = p0 + threadIdx.x; i < p1; i += 256) atomicAdd(&cnt[local_cell(in[i])], 1u);
        __syncthreads();
        unsigned *gc = (SCATTER ? cursor : cell_start) + (size_t)b * cells;
        for (int i = threadIdx.x; i < cells; i += 256) {
            const unsigned c = cnt[i];
            if (c) {
                const unsigned r = atomicAdd(&gc[i], c);
                if (SCATTER) base[i] = r;
            }
            if (SCATTER) cnt[i] = 0;
        }
        __syncthreads();
        if (SCATTER) {
            for (unsigned i = p0 + threadIdx.x; i < p1; i += 256) {
                const float4 p = in[i];
                const int c = local_cell(p);
                out[base[c] + atomicAdd(&cnt[c], 1u)] = p;
            }
            __syncthreads();
        }
    }
}

// one workgroup per big bucket: counts in cell_start -> cell starts; cursors = copies
__global__ __launch_bounds__(256) void big_bucket_scan_kernel(const GridParams *__restrict__ gp,
                                                              const unsigned *__restrict__ bk_start,
                                                              unsigned *cell_start, unsigned *cursor)
{
    __shared__ unsigned wsum[4];
    const GridParams g = *gp;
    const int b = blockIdx.x;
    if (g.bad_input || b >= g.bk_count) return;
    const unsigned s0 = bk_start[b], s1 = bk_start[b + 1];
    if (s1 - s0 <= BIG_BUCKET) return;
    const int cells = g.bk_cells;
    unsigned *cs = cell_start + (size_t)b * cells, *cu = cursor + (size_t)b * cells;
    const int seg = (cells + 255) / 256;
    const int c0 = min(cells, (int)threadIdx.x * seg), c1 = min(cells, c0 + seg);
    unsigned sum = 0;
    for (int c = c0; c < c1; ++c) sum += cs[c];
    unsigned tot;
    unsigned run = s0 + block_exclusive_scan_256(sum, &tot, wsum);
    for (int c = c0; c < c1; ++c) {
        const unsigned v = cs[c];
        cs[c] = run;
        cu[c] = run;
        run += v;
    }
}

// ---------------------------------------------------------------- brick plan
// Planned bricks (the plain single-cloud call, 2x2x2-cell bricks, k <= 16): a fixed brick holds 54 +- 7.3 queries of a
// uniform cloud, so ten of a batch's 64 lanes idle and one brick in thirteen pays a second batch for a handful of
// queries.  A BUNDLE is the 2x2 query rows of the bricks (., by, bz); its points are ordered by quarter-cell slab along x
// (bucket_sort<true>, fine_start).  One wave per bundle cuts the bundle's 4 nx quarter-slabs into greedy runs: a run grows
// while it holds at most PLAN_MAXQ queries and PLAN_MAXRUN quarters; a single quarter with more queries is a run of its
// own (knn_brick's multi-batch / extra path).  The runs of all bundles, in bundle-then-x order, are knn_brick's work items.
// Pass 1 counts the runs of every bundle, its last workgroup scans the counts (no atomics hand out slots: the list is the
// same for the same cloud); pass 2 cuts the same runs again and writes them.  4 nx <= MAX_DIM (grid_params), so a bundle's
// counts fit the LDS arrays below.
constexpr int PLAN_MAXQ = 64;
constexpr int PLAN_MAXRUN = 10;   // quarters: 2.5 cells -- with one cell either side |u| <= 2.25 in the MFMA frame (knn_mfma.h)
constexpr int PLAN_WAVES = 4;

template <bool WRITE>
__global__ __launch_bounds__(64 * PLAN_WAVES) void brick_plan_kernel(GridParams *__restrict__ gp, const unsigned *__restrict__ fine_start,
                                                                     unsigned *__restrict__ bundle_cnt, unsigned *__restrict__ bundle_off,
                                                                     uint2 *__restrict__ list)
{
    // Both passes are a few dependent round trips per wave (3 bundles per SIMD at 10M points), so every load of a step is
    // independent of the others: the first version (a load pair per quarter and row inside a rolled loop, a serial walk per
    // run start, one load after the other in the scan) took 39 + 23 us per 10M points.
    __shared__ unsigned s_sum[PLAN_WAVES][MAX_DIM + 1];
    __shared__ unsigned short s_nxt[PLAN_WAVES][MAX_DIM];
    __shared__ unsigned wsum[4];
    __shared__ unsigned s_last;
    const GridParams g = *gp;
    if (g.bad_input || !g.plan) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    unsigned *S = s_sum[wv];
    unsigned short *nxt = s_nxt[wv];
    const int nq4 = 4 * g.nx, nbund = g.nby * g.nbz;
    const unsigned cap = (unsigned)g.plan_cap;
    constexpr int QPL = MAX_DIM / 64 + 1;   // quarter boundaries per lane: 4 nx + 1 <= 1025
    for (int bundle = (int)blockIdx.x * PLAN_WAVES + wv; bundle < nbund; bundle += (int)gridDim.x * PLAN_WAVES) {   // wave-uniform
        const int bz = bundle / g.nby, by = bundle - bz * g.nby;
        int rb[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int yy = 2 * by + (r & 1), zz = 2 * bz + (r >> 1);
            rb[r] = yy < g.ny && zz < g.nz ? 4 * row_base(g, yy, zz) : -1;
        }
        // S[q] = sum over the bundle's rows of fine_start[row + q], q = 0 .. 4 nx: the queries of the quarters [a, b) are
        // S[b] - S[a] (mod 2^32: the differences are exact)
        unsigned v[QPL][4];
#pragma unroll
        for (int u = 0; u < QPL; ++u) {
            const int q = lane + 64 * u;
#pragma unroll
            for (int r = 0; r < 4; ++r) v[u][r] = (q <= nq4 && rb[r] >= 0) ? fine_start[rb[r] + q] : 0u;
        }
#pragma unroll
        for (int u = 0; u < QPL; ++u) {
            const int q = lane + 64 * u;
            if (q <= nq4) S[q] = v[u][0] + v[u][1] + v[u][2] + v[u][3];
        }
        wave_sync();
        for (int s = lane; s < nq4; s += 64) {   // where the run that starts at quarter s ends (exclusive): S is monotone
            const unsigned s0 = S[s];
            int e = s + 1;
#pragma unroll
            for (int j = 2; j <= PLAN_MAXRUN; ++j) e += (s + j <= nq4 && S[min(s + j, nq4)] - s0 <= (unsigned)PLAN_MAXQ) ? 1 : 0;
            nxt[s] = (unsigned short)e;
        }
        wave_sync();
        if (lane == 0) {
            const unsigned base = WRITE ? bundle_off[bundle] : 0u;
            unsigned n = 0;
            for (int s = 0; s < nq4; ++n) {
                const int e = nxt[s];
                if (WRITE && base + n < cap) list[base + n] = make_uint2((unsigned)bundle, (unsigned)s | ((unsigned)(e - 1) << 16));
                s = e;
            }
            if (!WRITE) __hip_atomic_store(&bundle_cnt[bundle], n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // write-through
        }
        wave_sync();   // the arrays are rewritten for the wave's next bundle
    }
    if (WRITE) return;
    __builtin_amdgcn_s_waitcnt(0);   // the write-through stores above have completed before the ticket
    __syncthreads();
    if (threadIdx.x == 0) s_last = atomicAdd(&gp->ticket_plan, 1u) == gridDim.x - 1 ? 1u : 0u;
    __syncthreads();
    if (!s_last) return;
    // the last workgroup: exclusive scan of the bundles' run counts, each thread a contiguous segment (held in registers
    // when it is short: 13 entries at 10M points)
    constexpr int HOLD = 16;
    const int seg = (nbund + 255) / 256;
    const int c0 = min(nbund, (int)threadIdx.x * seg), c1 = min(nbund, c0 + seg);
    const bool held = seg <= HOLD;   // block-uniform
    unsigned hv[HOLD];
    unsigned sum = 0;
    for (int c = c0; c < c1; c += HOLD) {
#pragma unroll
        for (int u = 0; u < HOLD; ++u) hv[u] = c + u < c1 ? __hip_atomic_load(&bundle_cnt[c + u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
#pragma unroll
        for (int u = 0; u < HOLD; ++u) sum += hv[u];
    }
    unsigned tot;
    unsigned run = block_exclusive_scan_256(sum, &tot, wsum);
    for (int c = c0; c < c1; c += HOLD) {
        unsigned w[HOLD];
#pragma unroll
        for (int u = 0; u < HOLD; ++u)
            w[u] = held ? hv[u] : (c + u < c1 ? __hip_atomic_load(&bundle_cnt[c + u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u);
#pragma unroll
        for (int u = 0; u < HOLD; ++u) {
            if (c + u < c1) bundle_off[c + u] = run;
            run += w[u];
        }
    }
    if (threadIdx.x == 0) {
        gp->ticket_plan = 0;
        if (tot > cap) {
            gp->plan = 0;   // (a cloud of long empty stretches: more runs than the list holds) -- the fixed bricks, numbered as ever
        } else {
            gp->nbricks = (int)tot;   // knn_brick's items are list positions now
            gp->part_lo = 0;
            gp->part_hi = (int)tot;
        }
    }
}

// ---------------------------------------------------------------- knn_brick
// One wave per brick.  refs/rstart: cell-sorted reference points and cell starts;
// qpts/qstart: cell-sorted QUERY points (same arrays when every reference is a query).
// Work item = (brick, batch of 64 queries).  EXTRA == false: one item per brick, its first batch; any
// further batch (a brick holding more than 64 queries: ~15-45 % of bricks on uniform data, thousands
// of batches for one brick inside a dense cluster) is APPENDED to a list instead of being looped over
// by the same wave.  EXTRA == true (second launch) spreads those items over the whole chip.
// waves per SIMD the register allocator must leave room for (the top-k list is 2*KCAP VGPRs)
// Round 3 (profiles/r03_variants.txt): phase 2 takes the candidates in blocks of 8 (TopNet::BS) -- the list, one block and
// four gathers in flight then need ~95 VGPRs and five waves per SIMD are resident for k <= 16 (four for k <= 32: round 4, -3 % at k = 25 / 32; five spill into the loops: +70 %).  The
// kernel is bound by latency as much as by issue: 3 -> 5 waves took knn_brick from 1.92 to 1.68 ms at 10M splats, the
// setup code's spills (outside the loops) notwithstanding; six waves push spills into the loops (2.39 ms).
// (tuning builds override these constants with -D; tools/build_variants.sh)
#ifndef GSX_NET_WAVES17
#define GSX_NET_WAVES17 5
#endif
#ifndef GSX_BRICK_UNROLL3   // phase 1's word pipeline with rotating names (round 5, A/B)
#define GSX_BRICK_UNROLL3 0
#endif
#ifndef GSX_NET_WAVES33
#define GSX_NET_WAVES33 4
#endif
#ifndef GSX_NET_HB
#define GSX_NET_HB 4
#endif
#ifndef GSX_NET_WAVES25
#define GSX_NET_WAVES25 4
#endif
#ifndef GSX_NET_WAVES49
#define GSX_NET_WAVES49 3
#endif
constexpr int NET_WAVES9 = 5, NET_WAVES17 = GSX_NET_WAVES17, NET_WAVES25 = GSX_NET_WAVES25, NET_WAVES33 = GSX_NET_WAVES33,
              NET_WAVES49 = GSX_NET_WAVES49;
constexpr int NET_HB = GSX_NET_HB;   // candidate gathers in flight per lane (8: no change)
constexpr int brick_min_waves(int kcap, bool mf, bool net)
{
    (void)mf;  // the MFMA filter's registers are not live together with the top-k list (single-drain path)
    // NET: list of KCAP-1 doubles + a 16-candidate block + 8 gathers in flight
    if (net) return kcap <= 9 ? NET_WAVES9 : (kcap <= 17 ? NET_WAVES17 : (kcap <= 25 ? NET_WAVES25 : (kcap <= 33 ? NET_WAVES33 : (kcap <= 49 ? NET_WAVES49 : 2))));   // (41 -> like 49, 57 -> like 65)
    return kcap <= 17 ? 5 : (kcap <= 26 ? 4 : (kcap <= 33 ? 3 : 2));
}

// NET: phase 2 selects with TopNet<KCAP-1> (sorting-network blocks, the query excluded by index) instead
// of the per-candidate bubble insert of TopList<KCAP>; needs KCAP-1 to be a power of two.
// PLAN: the work items are planned bricks (brick_plan_kernel): quarter-slabs [qf, ql] of the bundle (by, bz), rows taken from
// fine_start (passed as rstart; queries and references are the same table).  The 16 candidate rows are the quarters
// [qf - 4, ql + 4]: |p - q| <= r_safe = h'(1 - 1e-3) is 4 - 4e-3 quarter units, and the f32 quarter index
// floor(fl(fl(x-o) * 4 inv_h)) is monotone and off by < 4 nx * 2^-22 <= 2.5e-4 quarters (4 nx <= MAX_DIM, grid_params), so the
// quarter indices of p and q differ by at most 4 -- the cell argument of r_safe with dim = 4 nx.  Where brick_plan withdrew
// the plan (gp->plan == 0) the same kernel takes the fixed bricks as the aligned runs [8 bx, 8 bx + 7]: fine_start[4 c] is
// cell_start[c], the rows are the fixed brick's.
// CERT (k = 16 on the 16-entry network list, no kth_out; the context's epilogue_cert): the wave's last block of a batch is
// merged without the re-sort (TopNet::merge_block_last) and the epilogue certifies the float32 mean of short roots
// (mean_from_net_cert, knn_mean_cert.h), recomputing exactly in the same wave where it cannot.  Acceptance sees the same k-th
// distance, so the fail list is the same.
template <int KCAP, bool EXTRA, bool MF, bool NET, bool PLAN = false, bool CERT = false>
__global__ __launch_bounds__(BRICK_THREADS, brick_min_waves(KCAP, MF, NET)) void knn_brick_kernel(
    GridParams *__restrict__ gp, const float4 *__restrict__ refs, const unsigned *__restrict__ rstart,
    const float4 *__restrict__ qpts, const unsigned *__restrict__ qstart, int k, int q_begin,
    float *__restrict__ mean_out, unsigned *__restrict__ faillist, uint2 *__restrict__ extra,
    unsigned *__restrict__ deferred, double *__restrict__ kth_out, const uint2 *__restrict__ plist)
{
    static_assert(!CERT || (NET && KCAP == 17), "the certified epilogue is derived for the 16-entry network list");
    constexpr int WCAP = KCAP > 33 ? GSX_WCAP_BIG : (KCAP > 17 ? GSX_WCAP_MID : gsx::WCAP);
    __shared__ unsigned s_mask[BRICK_THREADS / 64][WCAP][64];
    // per mask word: first candidate (index into refs); (c1, b2 - c1): candidates of the first row segment and the
    // offset of the second (MFMA words may span two rows).  Two narrow arrays: one 16-byte entry per word read
    // with per-lane indices cost 0.14 ms at 10M splats (LDS bank conflicts)
    __shared__ unsigned s_wbase[BRICK_THREADS / 64][WCAP];
    __shared__ uint2 s_wseg[MF ? BRICK_THREADS / 64 : 1][MF ? WCAP : 1];

    if (EXTRA && gp->extra_count == 0) return;  // the usual case: no brick shed a batch (an empty pass still cost 6.6 us)
    const int lane = lane_id();
    const int wv = uniform((int)(threadIdx.x >> 6));
    unsigned(*mask)[64] = s_mask[wv];
    unsigned *wbase = s_wbase[wv];
    uint2 *wseg = s_wseg[MF ? wv : 0];

    // Every field of *gp read here, and below every argument, becomes a scalar of its own (own_scalar, knn_common.h): the
    // kernel needs more scalars than there are SGPRs, and what the allocator parks in vector lanes it parks and fetches by
    // the group the value arrived in -- eight dwords to read one pointer.  The fields are read through a
    // constant-address-space view: none of them is written while this kernel runs (the counters are, and stay with gp), and
    // a load that follows an asm statement would otherwise count as clobbered and become a vector load.
    // NET kernels only (the default form and its fixed-brick twin): the bubble-insert kernels do not park enough to gain, and
    // stay as they were.
    const auto *gk = (const __attribute__((address_space(4))) GridParams *)gp;
#define GSX_OWN_FIELD(f) (NET ? own_scalar(gk->f) : gp->f)
    const int nx = GSX_OWN_FIELD(nx), ny = GSX_OWN_FIELD(ny), nz = GSX_OWN_FIELD(nz);
    const int nbx = GSX_OWN_FIELD(nbx), nby = GSX_OWN_FIELD(nby);
    const int bdx = GSX_OWN_FIELD(bdx), bdy = GSX_OWN_FIELD(bdy), bdz = GSX_OWN_FIELD(bdz);
    const int cry = bdy + 2;                  // candidate rows per z-slab
    const int ncrows = cry * (bdz + 2);       // <= 16 candidate x-rows
    const int nqrows = bdy * bdz;             // <= 4 query x-rows
    const double r1sq = GSX_OWN_FIELD(r1sq);
    const double hp = GSX_OWN_FIELD(hprime);
    const float tau1 = GSX_OWN_FIELD(tau1);
    const float g_ox = GSX_OWN_FIELD(ox), g_oy = GSX_OWN_FIELD(oy), g_oz = GSX_OWN_FIELD(oz), g_inv_h = GSX_OWN_FIELD(inv_h);
    const int bk_g = GSX_OWN_FIELD(bk_g), bk_ny = GSX_OWN_FIELD(bk_ny), bk_cells = GSX_OWN_FIELD(bk_cells);
    auto row_base_g = [&](int cy, int cz) {  // bucket-major cell index of cell (0, cy, cz); cy, cz >= 0 wherever the result is used
        // (unsigned: a signed division by a run-time divisor also keeps the divisor's sign and its absolute value for the kernel's length)
        const int by_ = NET ? (int)((unsigned)cy / (unsigned)bk_g) : cy / bk_g, bz_ = NET ? (int)((unsigned)cz / (unsigned)bk_g) : cz / bk_g;
        return (bz_ * bk_ny + by_) * bk_cells + ((cz - bz_ * bk_g) * bk_g + (cy - by_ * bk_g)) * nx;
    };
#ifdef GSX_ABLATE  // profiling build only (results become wrong): -DGSX_ABLATE + gsx_ctx_set_param("debug_skip")
    const int dbg = gp->debug_skip;
#else
    constexpr int dbg = 0;
#endif
    const int kk = k + 1;
    const int kq = NET ? k : kk;  // position of the acceptance distance in the list (NET lists do not hold the query)

    WorkQueue wq;
    const int part_lo = GSX_OWN_FIELD(part_lo);
    const int nq4 = 4 * nx;
    const bool planned = PLAN && (NET ? gk->plan : gp->plan) != 0;   // kernel-uniform
    const int dw = EXTRA ? 0 : GSX_OWN_FIELD(defer_words);  // loaded once: gp is written by atomics, the compiler would reload it per brick
#ifdef GSX_WAVE_STAMPS
    const unsigned long long ws_t0 = ws_realtime();
#endif
    wq_init(wq, EXTRA ? gp->extra_ctr : gp->brick_ctr, EXTRA ? (int)gp->extra_count : (NET ? gk->part_hi : gp->part_hi) - part_lo,
            BRICK_THREADS / 64);
#undef GSX_OWN_FIELD
    // (the arguments: after the last plain load through gp)
    if constexpr (NET) {
        refs = own_table(refs), rstart = own_table(rstart), qpts = own_table(qpts), qstart = own_table(qstart), plist = own_table(plist);
        k = own_scalar(k), q_begin = own_scalar(q_begin);
        mean_out = own_output(mean_out), faillist = own_output(faillist), extra = own_output(extra), deferred = own_output(deferred);
        kth_out = own_output(kth_out);
    }
    for (;;) {
        const int item = uniform(wq_next(wq));
        if (item < 0) break;
        int b = item + part_lo, qb = 0;
        if (EXTRA) {
            const uint2 it = extra[item];
            b = uniform((int)it.x);
            qb = uniform((int)it.y);
        }
        int bx, by, bz;
        int qf = 0, ql = 0;   // PLAN: first and last quarter-slab of the brick
        if constexpr (PLAN) {
            int bundle;
            if (planned) {
                const uint2 e = plist[b];
                bundle = uniform((int)e.x);
                qf = uniform((int)(e.y & 0xffffu));
                ql = uniform((int)(e.y >> 16));
            } else {
                // (the withdrawn plan only: its divisor is pinned in here, so that the division's reciprocal is made in this
                //  branch and not kept, with the divisor, from the kernel's entry on)
                const int nbx_h = pinned_here_s(nbx);
                bundle = (int)((unsigned)b / (unsigned)nbx_h);
                qf = 8 * (b - bundle * nbx_h);
                ql = min(qf + 7, nq4 - 1);
            }
            bz = (int)((unsigned)bundle / (unsigned)nby);   // (b, bundle >= 0: unsigned, see row_base_g)
            by = bundle - bz * nby;
            bx = 0;
        } else {
            bz = b / (nbx * nby);
            const int brem = b - bz * nbx * nby;
            by = brem / nbx;
            bx = brem - by * nbx;
        }

        // lane r < 16: candidate row r (bdx+2 cells along x); lanes 16..19: query rows (bdx cells)
        int v_start = 0, v_len = 0;
        {
            // (recomputed per brick from a pinned lane id: as loop invariants these five values, the division magic behind
            //  them and a dozen more were kept in scratch across the whole kernel.  bdy is 1 or 2, cry = bdy + 2 is 3 or 4)
            const int ln = pinned_here(lane);
            const bool isq = ln >= 16;
            const int r = isq ? ln - 16 : ln;
            const int r_mod_bdy = bdy == 2 ? (r & 1) : 0, r_div_bdy = bdy == 2 ? (r >> 1) : r;
            const int r_div_cry = cry == 4 ? (r >> 2) : (r * 11) >> 5;       // r < 16
            const int r_mod_cry = r - r_div_cry * cry;
            const int yy = isq ? by * bdy + r_mod_bdy : by * bdy - 1 + r_mod_cry;
            const int zz = isq ? bz * bdz + r_div_bdy : bz * bdz - 1 + r_div_cry;
            // (PLAN: quarters, an index into fine_start = 4 x the row's first cell + the quarter)
            const int xa = PLAN ? (isq ? qf : max(qf - 4, 0)) : (isq ? bx * bdx : max(bx * bdx - 1, 0));
            const int xb = PLAN ? (isq ? ql : min(ql + 4, nq4 - 1))
                                : (isq ? min(bx * bdx + bdx - 1, nx - 1) : min(bx * bdx + bdx, nx - 1));
            const bool valid = (isq ? (lane < 20 && r < nqrows) : r < ncrows) && yy >= 0 && yy < ny && zz >= 0 && zz < nz;
            if (valid) {
                const unsigned *st = isq ? qstart : rstart;
                const int row = PLAN ? 4 * row_base_g(yy, zz) : row_base_g(yy, zz);
                unsigned s = st[row + xa], e = st[row + xb + 1];
                v_start = (int)s;
                v_len = (int)(e - s);
            }
        }
        if (dbg & 16) continue;  // queue + row-table loads only
        int qoff[5];
        qoff[0] = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) qoff[r + 1] = qoff[r] + __builtin_amdgcn_readlane(v_len, 16 + r);
        const int nq = qoff[4];
        if (!EXTRA) {
            // Adaptive refinement: the cost of this brick is batches x candidate words.  A uniform grid
            // gives ~1.5 x 15; a brick inside (or next to) a cluster much denser than the cell size can
            // reach millions.  Such a brick is not searched here: it goes on the deferred list, and the
            // host re-runs the whole pipeline on the points of the deferred neighbourhoods with a grid
            // sized for THEM (launch_knn_grid, refine_level).
            if (dw > 0 && nq > 0) {
                int ncand = 0;
#pragma unroll
                for (int r = 0; r < 16; ++r) ncand += __builtin_amdgcn_readlane(v_len, r);
                const int words = (ncand + 31) >> 5, batches = (nq + 63) >> 6;
                if (words > dw || (long long)words * batches > 2LL * dw) {
                    if (lane == 0) deferred[atomicAdd(&gp->deferred_count, 1u)] = (unsigned)b;
                    continue;
                }
            }
        }
        // A wave loops over up to LOCAL_BATCHES batches of its brick itself (the neighbourhood is hot in
        // the scalar cache / L2 then); the batches beyond that -- a brick inside a dense cluster can
        // hold thousands -- become items of the second launch.
        constexpr int LOCAL_MAX = 3;
        const int LOCAL_BATCHES = nq > 64 * LOCAL_MAX ? 1 : LOCAL_MAX;  // heavy brick: keep one, spread the rest
        if (!EXTRA && nq > 64 * LOCAL_BATCHES) {
            const int nextra = (nq - 1) / 64 + 1 - LOCAL_BATCHES;
            unsigned slot = 0;
            if (lane == 0) slot = atomicAdd(&gp->extra_count, (unsigned)nextra);
            slot = (unsigned)uniform((int)slot);
            for (int e = lane; e < nextra; e += 64)
                extra[slot + e] = make_uint2((unsigned)b, (unsigned)(64 * (e + LOCAL_BATCHES)));
        }
        const int qb_end = EXTRA ? min(nq, qb + 64) : min(nq, 64 * LOCAL_BATCHES);

        for (; qb < qb_end; qb += 64) {
            // ---- this lane's query
            const int f = qb + lane;
            const bool live = f < nq;
            int qidx = 0;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                int s = __builtin_amdgcn_readlane(v_start, 16 + r);
                if (f >= qoff[r] && f < qoff[r + 1]) qidx = s + (f - qoff[r]);
            }
            const float4 qp = qpts[live ? qidx : 0];
            const float qx = qp.x, qy = qp.y, qz = qp.z;
            const bool is_query = live && !(__float_as_uint(qp.w) >> 31);  // reference-only points (slab halo) are never queries
            if (!__any(is_query)) continue;  // a batch of halo points only
            float tau = is_query ? tau1 : -1.0f;
            double racc_sq = r1sq;  // this lane's acceptance radius^2 (== the exact value its filter bound comes from)
            // Queries next to the cloud's bounding box see only part of their neighbourhood ball, so
            // their (k+1)-th neighbour is farther than one cell and they would all go to knn_ring.  But
            // where the brick's neighbourhood is cut by the GRID boundary nothing exists beyond that
            // face, so it does not limit the guaranteed radius: r_safe(q) = distance to the nearest
            // face of the searched box that has cells behind it (>= h').  The filter radius is widened
            // only as far as the missing ball volume requires (so phase 2 sees the usual ~30 candidates).
            {
                const int ulo[3] = {bx * bdx - 1, by * bdy - 1, bz * bdz - 1};
                const int uhi[3] = {bx * bdx + bdx, by * bdy + bdy, bz * bdz + bdz};
                const int dim[3] = {nx, ny, nz};
                const bool boundary = (PLAN ? qf - 4 <= 0 || ql + 4 >= nq4 - 1 : ulo[0] <= 0 || uhi[0] >= nx - 1) || ulo[1] <= 0 ||
                                      ulo[2] <= 0 || uhi[1] >= ny - 1 || uhi[2] >= nz - 1;
                // Only for a brick's FIRST batch: the later ones scan a sub-box of the neighbourhood (below) that reaches exactly one
                // cell beyond their queries' cells -- a radius above h' would certify against points that were never looked at.
                // (Found by the randomised sweep, round 3: a planar cloud, k = 64, two queries at the rim wrong in ~15 % of the
                // runs -- which queries land in a later batch depends on the order the binning's atomics leave in a cell.)
                if (boundary && qb == 0) {  // wave-uniform
                    // f32 is enough: the 1e-3*h' margin dwarfs its rounding (<= dims * 2^-23 * h' ~ 1e-4 h')
                    // (pinned: 8 % of the bricks get here; hoisted, its per-brick operands were computed and parked in
                    //  scratch for every brick)
                    const float hf = pinned_here((float)hp);
                    // (the faces again, from pinned brick coordinates: their float conversions stay in here too)
                    const int pbx = pinned_here_s(bx), pby = pinned_here_s(by), pbz = pinned_here_s(bz);
                    const int ulo[3] = {pbx * bdx - 1, pby * bdy - 1, pbz * bdz - 1};
                    const int uhi[3] = {pbx * bdx + bdx, pby * bdy + bdy, pbz * bdz + bdz};
                    const float rel[3] = {qx - g_ox, qy - g_oy, qz - g_oz};
                    const float r1 = hf * (1.0f - 1e-3f);
                    float rsafe = 3.0e38f, frac = 1.0f;
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        // faces of the searched box with cells behind them (margin as in grid_params_kernel)
                        if (PLAN && a == 0) {
                            // along x the searched box is the quarters [qf - 4, ql + 4]: its faces sit at (qf - 4) / 4 and
                            // (ql + 5) / 4 cells (exact in f32).  A point left out has a quarter index <= qf - 5 or >= ql + 5, so
                            // it lies beyond the face but for the index's rounding, 2.5e-4 quarters -- the same 2e-3 h' margin covers it
                            const int pqf = pinned_here_s(qf), pql = pinned_here_s(ql);
                            if (pqf - 4 > 0) rsafe = fminf(rsafe, rel[0] - (float)(pqf - 4) * 0.25f * hf - 2e-3f * hf);
                            if (pql + 4 < nq4 - 1) rsafe = fminf(rsafe, (float)(pql + 5) * 0.25f * hf - rel[0] - 2e-3f * hf);
                        } else {
                        if (ulo[a] > 0) rsafe = fminf(rsafe, rel[a] - (float)ulo[a] * hf - 2e-3f * hf);
                        if (uhi[a] < dim[a] - 1) rsafe = fminf(rsafe, (float)(uhi[a] + 1) * hf - rel[a] - 2e-3f * hf);
                        }
                        // part of [q - r1, q + r1] that lies inside the grid along this axis
                        const float tl = fminf(fmaxf(rel[a], 0.0f), r1);
                        const float th = fminf(fmaxf((float)dim[a] * hf - rel[a], 0.0f), r1);
                        frac *= (tl + th) / (2.0f * r1);
                    }
                    float rq = r1 * cbrtf(1.0f / fmaxf(frac, 0.125f));
                    rq = fminf(rq, rsafe);
                    if (rq > r1 && is_query) {
                        racc_sq = (double)rq * (double)rq;
                        tau = bound_from(racc_sq);
                    }
                }
            }

            // Batches after a brick's first hold the LAST queries of the brick (typically its last cell
            // or two): their neighbourhood is a sub-box of the brick's, so only the rows / cells within
            // one cell of the batch's bounding box are scanned (still a superset of every live query's
            // 3x3x3 cells, so r_safe is unchanged).
            int rs_start = v_start, rs_len = v_len;
            if (qb > 0) {
                int lo[3], hi[3];
                const int c3[3] = {cell_coord(qx, g_ox, g_inv_h, nx), cell_coord(qy, g_oy, g_inv_h, ny),
                                   cell_coord(qz, g_oz, g_inv_h, nz)};
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    lo[a] = is_query ? c3[a] : 0x7fffffff;
                    hi[a] = is_query ? c3[a] : -1;
#pragma unroll
                    for (int off = 32; off > 0; off >>= 1) {
                        lo[a] = min(lo[a], __shfl_xor(lo[a], off));
                        hi[a] = max(hi[a], __shfl_xor(hi[a], off));
                    }
                    lo[a] = uniform(lo[a]);
                    hi[a] = uniform(hi[a]);
                }
                rs_start = 0;
                rs_len = 0;
                if (lane < ncrows) {
                    const int ln = pinned_here(lane);
                    const int l_div_cry = cry == 4 ? (ln >> 2) : (ln * 11) >> 5;     // ln < 16
                    const int yy = by * bdy - 1 + (ln - l_div_cry * cry);
                    const int zz = bz * bdz - 1 + l_div_cry;
                    // (PLAN: the brick's quarters cut to the CELLS within one of the batch's -- both are supersets of what r_safe
                    //  needs, the quarters by the argument at the top of the kernel, the cells by r_safe's own)
                    const int xa = PLAN ? max(max(qf - 4, 0), 4 * (lo[0] - 1)) : max(max(bx * bdx - 1, 0), lo[0] - 1);
                    const int xb = PLAN ? min(min(ql + 4, nq4 - 1), 4 * (hi[0] + 1) + 3) : min(min(bx * bdx + bdx, nx - 1), hi[0] + 1);
                    const bool need = yy >= max(lo[1] - 1, 0) && yy <= min(hi[1] + 1, ny - 1) &&
                                      zz >= max(lo[2] - 1, 0) && zz <= min(hi[2] + 1, nz - 1) && xa <= xb;
                    if (need) {
                        const int row = PLAN ? 4 * row_base_g(yy, zz) : row_base_g(yy, zz);
                        const unsigned s0 = rstart[row + xa], e0 = rstart[row + xb + 1];
                        rs_start = (int)s0;
                        rs_len = (int)(e0 - s0);
                    }
                }
            }
            // initialised where phase 1 needs it live (see the MFMA single-drain path)
            typename std::conditional<NET, TopNet<NET ? KCAP - 1 : 8>, TopList<KCAP>>::type lst;
            bool lst_empty = true;  // wave-uniform: no block merged yet (NET)

            int widx = 0;
            unsigned nzw = 0;

            // ---- phase 2: walk this lane's set bits, exact f64 distance, sorted insert
            // (final_drain: std::true_type for the batch's last call -- CERT leaves the list as a set there)
            auto drain = [&](auto final_drain) __attribute__((always_inline)) {
                constexpr bool SET_FORM = CERT && decltype(final_drain)::value;
                // widened here, not before phase 1: six registers that the filter loop does not have to carry
                const double qxd = (double)qx, qyd = (double)qy, qzd = (double)qz;
                wave_sync();  // wbase[] written by lane 0 is visible to every lane
                if (dbg & 32) nzw = 0;  // profiling: masks are built but never walked
                unsigned m = 0;
                int base = 0, c1 = 32, base2 = 0;
                if constexpr (NET) {
                    // Blocks of BS candidates per lane: the lane's next BS set bits are gathered (HB loads in
                    // flight), their exact distances fill a register block (+inf where the lane has run out, and
                    // for the query's own point), one sorting network orders the block and a bitonic merge folds
                    // it into the list.  The wave repeats while any lane has bits left.
                    using Net = TopNet<NET ? KCAP - 1 : 8>;
                    constexpr int BS = Net::BS, HB = NET_HB < BS ? NET_HB : BS;
                    const unsigned self_w = __float_as_uint(qp.w);
                    for (;;) {
                        double blk[BS];
#pragma unroll
                        for (int h0 = 0; h0 < BS; h0 += HB) {
                            float4 pt[HB];
                            bool ok[HB];
#pragma unroll
                            for (int j = 0; j < HB; ++j) {
                                if (m == 0 && nzw != 0) {
                                    const int w = __builtin_ctz(nzw);
                                    nzw &= nzw - 1;
                                    m = mask[w][lane];
                                    base = (int)wbase[w];
                                    if constexpr (MF) {
                                        const uint2 sg = wseg[w];
                                        c1 = (int)sg.x;
                                        base2 = (int)sg.y;
                                    }
                                }
                                ok[j] = m != 0;
                                // branch-free: a lane that has run out (m == 0) re-reads candidate 0 of its last
                                // word (a valid, cached address) and the result is discarded below
                                const int i = ok[j] ? __builtin_clz(m) : 0;
                                m &= ~(0x80000000u >> i);  // m == 0 stays 0
                                const int idx = (MF && i >= c1 ? base2 : base) + i;
                                // MF + NET kernels: a 32-bit byte offset from the kernel-argument base (one v_add_lshl_u32 and a
                                // global_load with saddr, instead of a sign extension and a 64-bit shift-add per candidate);
                                // dispatch_bricks runs them only for clouds of fewer than 2^28 points
                                if constexpr (MF && NET) pt[j] = *(const float4 *)((const char *)refs + ((unsigned)idx << 4));
                                else pt[j] = refs[idx];
                            }
#pragma unroll
                            for (int j = 0; j < HB; ++j) {
                                double d = dist2_f64(qxd, qyd, qzd, pt[j].x, pt[j].y, pt[j].z);
                                blk[h0 + j] = (ok[j] && __float_as_uint(pt[j].w) != self_w) ? d : __builtin_inf();
                            }
                        }
                        if constexpr (SET_FORM) {
                            // merge_block in its two halves, the loop's exit between them: the wave's last block leaves
                            // the list as a set
                            const bool first = uniform((int)lst_empty);
                            if (first) lst.assign_block(blk); else lst.merge_block_last(blk);
                            lst_empty = false;
                            if (!__any(m != 0 || nzw != 0)) break;
                            if (!first) lst.sort_set();
                        } else {
                        if (uniform((int)lst_empty)) lst.assign_block(blk); else lst.merge_block(blk);
                        lst_empty = false;
                        if (!__any(m != 0 || nzw != 0)) break;
                        }
                    }
                } else {
                // software pipeline: the gather of candidate n+1 is in flight while candidate n goes
                // through the float64 distance + the 2*KCAP-op sorted insert
                bool have_cur = false;
                float4 pc = make_float4(0.f, 0.f, 0.f, 0.f);
                for (;;) {
                    if (m == 0 && nzw != 0) {
                        const int w = __builtin_ctz(nzw);
                        nzw &= nzw - 1;
                        m = mask[w][lane];
                        base = (int)wbase[w];
                        if constexpr (MF) {
                            const uint2 sg = wseg[w];
                            c1 = (int)sg.x;
                            base2 = (int)sg.y;
                        }
                    }
                    const bool have_next = m != 0;
                    float4 pn = pc;
                    if (have_next) {
                        const int i = __builtin_clz(m);
                        m &= ~(0x80000000u >> i);
                        pn = refs[(MF && i >= c1 ? base2 : base) + i];
                    }
                    if (have_cur && !(dbg & 1)) lst.insert(dist2_f64(qxd, qyd, qzd, pc.x, pc.y, pc.z));
                    if (!__any(have_next)) break;
                    pc = pn;
                    have_cur = have_next;
                }
                }
                if constexpr (!SET_FORM) tau = fminf(tau, bound_from(lst.kth(kq)));   // (nothing filters after the final drain)
                widx = 0;
                nzw = 0;
                wave_sync();  // all reads of mask/wbase done before they are overwritten
            };

            // ---- phase 1: lock-step filter over the 16 candidate rows
            // MFMA variant: only when ALL mask words of the batch fit the LDS park (the usual case).  Then
            // phase 2 runs exactly once, after phase 1, and the 2*KCAP registers of the top-k list are not
            // live while the 16 accumulators and the operands are: both phases fit 5 waves/SIMD without
            // spills (carrying the list through the MFMA loop cost 41-46 spilled dwords and made
            // phase 2 40 % slower).  A batch with more words takes the scalar filter.
            bool mf_done = false;
            if constexpr (MF) {
                // number of words the cutting below will produce (same rule: a word holds at most two row segments)
                int nwords = 0;
                {
                    int fill = 0, segs = 0;
                    for (int r = 0; r < ncrows; ++r) {
                        int len = __builtin_amdgcn_readlane(rs_len, r & 15);
                        while (len > 0) {
                            if (fill == 32 || segs == 2) {
                                ++nwords;
                                fill = 0;
                                segs = 0;
                            }
                            const int take = min(len, 32 - fill);
                            fill += take;
                            len -= take;
                            ++segs;
                        }
                    }
                    nwords += fill > 0;
                }
                if (nwords <= WCAP && !(dbg & 2)) {
                mf_done = true;
                // cell-unit coordinates relative to the brick centre; see the MFMA notes at the top
                // (pinned: computed here, per batch -- nine instructions -- instead of per brick with a round trip through scratch)
                const float hf = pinned_here((float)hp);
                // (PLAN: the middle of the run [qf, ql + 1) quarters -- a run of at most PLAN_MAXRUN = 10 quarters and one cell
                //  either side keep |u_x| <= 2.25, knn_mfma.h)
                const float ccx = PLAN ? g_ox + ((float)(qf + ql + 1) * 0.125f) * hf : g_ox + ((float)(bx * bdx) + 0.5f * (float)bdx) * hf;
                const float ccy = g_oy + ((float)(by * bdy) + 0.5f * (float)bdy) * hf;
                const float ccz = g_oz + ((float)(bz * bdz) + 0.5f * (float)bdz) * hf;
                const float uqx = (qx - ccx) * g_inv_h, uqy = (qy - ccy) * g_inv_h, uqz = (qz - ccz) * g_inv_h;
                const float nq2 = __builtin_fmaf(uqz, uqz, __builtin_fmaf(uqy, uqy, uqx * uqx));
                const bool upper = lane >= 32;
                // what the word loop multiplies and fills in per word, held in vector registers for the batch: as scalars the
                // allocator parked 1/h in a lane of a spill register and fetched it back (v_readlane) for every word
                const float inv_h_v = pinned_here(g_inv_h);
                const unsigned kconst = mf_candidate_const(upper);
                // (tau * inv_h) * inv_h: no overflow for tiny cells; dead lanes (tau = -1) never pass
                const float s_q = tau >= 0.0f ? nq2 - ((tau * g_inv_h) * g_inv_h * (1.0f + 1e-6f) + MF_SLACK) : 1.0e30f;
                bf16x8 opa, opb;
                mf_query_operands(uqx, uqy, uqz, s_q, opa, opb);
                // The candidate rows are walked as ONE flat sequence cut into 32-candidate words; a word may
                // continue into the next non-empty row (two segments at most), otherwise the ~25 % of rows
                // with 33..40 candidates would each cost a second, almost empty, MFMA pair.  The points of
                // words n+1 and n+2 are requested before word n is processed (a per-lane 16-B load takes
                // ~1-2k cycles from L2/HBM, one word is ~400 cycles of work).
                const int nrows = ncrows;
                struct Word { int b1, c1, b2, c2, r, off; };  // wave-uniform; r/off = where the NEXT word starts
                auto next_word = [&](int r, int off) __attribute__((always_inline)) {
                    Word o{0, 0, 0, 0, r, off};
                    int len = r < nrows ? __builtin_amdgcn_readlane(rs_len, r & 15) : 0;
                    while (r < nrows && off >= len) {  // skip exhausted / empty rows
                        ++r;
                        off = 0;
                        len = r < nrows ? __builtin_amdgcn_readlane(rs_len, r & 15) : 0;
                    }
                    if (r < nrows) {
                        o.b1 = __builtin_amdgcn_readlane(rs_start, r & 15) + off;
                        o.c1 = min(32, len - off);
                        off += o.c1;
                        if (o.c1 < 32) {  // row finished inside the word: continue with the next non-empty row
                            do {
                                ++r;
                                off = 0;
                                len = r < nrows ? __builtin_amdgcn_readlane(rs_len, r & 15) : 0;
                            } while (r < nrows && len == 0);
                            if (r < nrows) {
                                o.b2 = __builtin_amdgcn_readlane(rs_start, r & 15);
                                o.c2 = min(32 - o.c1, len);
                                off = o.c2;
                            }
                        }
                    }
                    o.r = r;
                    o.off = off;
                    return o;
                };
                // (from a lane id made here, per batch: computed from the kernel's it is hoisted to the entry and, with the loop's
                //  registers taken, parked in scratch and reloaded per batch)
                const int my_cand = mf_cand_of_row(fresh_lane_id() & 31);
                const int my_cand16 = my_cand << 4;
                auto fetch = [&](const Word &w) __attribute__((always_inline)) {
                    const int c = w.c1 + w.c2;
                    if (c == 0) return make_float4(0.f, 0.f, 0.f, 0.f);
                    if constexpr (NET) {
                        // a 32-bit byte offset (as phase 2), built in bytes from the start: slots past the end repeat the last
                        // candidate (masked out below), the second segment is one conditional add of a wave-uniform delta
                        // (the sum with the delta is pinned: left alone, the select is moved in front of the adds, where it
                        //  chooses between two scalars and costs two v_mov on top)
                        const int t16 = min(my_cand16, (c - 1) << 4);
                        const unsigned off1 = (unsigned)t16 + ((unsigned)w.b1 << 4);
                        const unsigned off2 = (unsigned)pinned_here((int)(off1 + ((unsigned)(w.b2 - w.c1 - w.b1) << 4)));
                        return *(const float4 *)((const char *)refs + (t16 >= (w.c1 << 4) ? off2 : off1));
                    } else {
                        const int t = min(my_cand, c - 1);
                        const int idx = t < w.c1 ? w.b1 + t : w.b2 + (t - w.c1);
                        return refs[idx];
                    }
                };
                // The word metadata phase 2 reads (first candidate; candidates of the first segment, offset of the second) is
                // collected in lane widx of three registers and stored once after the loop: no per-word stores by lane 0
                unsigned meta_b1 = 0, meta_c1 = 0, meta_d = 0;
                auto process = [&](const Word &w_cur, const float4 &p_cur) __attribute__((always_inline)) {
                    const bf16x8 cand = mf_candidate_operand((p_cur.x - ccx) * inv_h_v, (p_cur.y - ccy) * inv_h_v,
                                                             (p_cur.z - ccz) * inv_h_v, kconst);
                    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                    // lane l: tile a = rows-set (l>>5) of query l&31, tile b = of query 32 + (l&31)
                    const unsigned ma = mf_sign_bits(__builtin_amdgcn_mfma_f32_32x32x16_bf16(cand, opa, zero, 0, 0, 0));
                    const unsigned mb = mf_sign_bits(__builtin_amdgcn_mfma_f32_32x32x16_bf16(cand, opb, zero, 0, 0, 0));
                    auto sw = __builtin_amdgcn_permlane32_swap(ma, mb, false, false);
                    // now sw[0] = rows-set 0, sw[1] = rows-set 1 of THIS lane's query (16 bits each: mf_sign_bits starts
                    // from 0); drop the bits of the clamped duplicates past the end of a partial word
                    const unsigned m = ((sw[0] << 16) | sw[1]) & (0xffffffffu << (32 - (w_cur.c1 + w_cur.c2)));
                    if (dbg & 64) atomicAdd(&gp->exhaustive_count, (unsigned)__builtin_popcount(m));  // profiling: candidates passed
                    mask[widx][lane] = m;
                    write_lane3(meta_b1, meta_c1, meta_d, w_cur.b1, w_cur.c1, w_cur.b2 - w_cur.c1, widx);
                    nzw |= nonzero01(m) << widx;
                    ++widx;
                };
#if GSX_BRICK_UNROLL3
                // the three-deep word pipeline with ROTATING names instead of register moves (the rolled loop spends 4 of its 79
                // vector instructions per word on moves of the two prefetched points; unrolled the count is 78.3 per word at
                // three times the code -- not the default.  Names alternating over two words, or one point in flight loaded in
                // place, make the compiler wait for the newest load in the middle of a word: tools/asm_count.py)
                Word w0 = next_word(0, 0);
                Word w1 = next_word(w0.r, w0.off), w2;
                float4 p0 = fetch(w0), p1 = fetch(w1), p2;
                for (;;) {
                    if (!(w0.c1 > 0)) break;
                    w2 = next_word(w1.r, w1.off);
                    p2 = fetch(w2);
                    process(w0, p0);
                    if (!(w1.c1 > 0)) break;
                    w0 = next_word(w2.r, w2.off);
                    p0 = fetch(w0);
                    process(w1, p1);
                    if (!(w2.c1 > 0)) break;
                    w1 = next_word(w0.r, w0.off);
                    p1 = fetch(w1);
                    process(w2, p2);
                }
#else
                Word w_cur = next_word(0, 0);
                Word w_n1 = next_word(w_cur.r, w_cur.off);
                float4 p_cur = fetch(w_cur), p_n1 = fetch(w_n1);
                while (w_cur.c1 > 0) {
                    const Word w_n2 = next_word(w_n1.r, w_n1.off);
                    const float4 p_n2 = fetch(w_n2);
                    process(w_cur, p_cur);
                    w_cur = w_n1;
                    p_cur = p_n1;
                    w_n1 = w_n2;
                    p_n1 = p_n2;
                }
#endif
                // (drain()'s wave_sync orders these stores before phase 2 reads them)
                {
                    const int ln = fresh_lane_id();  // (not the kernel's lane id: that one is live, or spilled, across everything)
                    if (ln < widx) {
                        wbase[ln] = meta_b1;
                        wseg[ln] = make_uint2(meta_c1, meta_d);
                    }
                }
                lst.init();
                }
            }
            if (!mf_done) {
            lst.init();
            for (int r = 0; r < ((dbg & 2) ? 0 : ncrows); ++r) {
                const int gs = __builtin_amdgcn_readlane(rs_start, r);
                const int len = __builtin_amdgcn_readlane(rs_len, r);
                for (int w0 = 0; w0 < len; w0 += 32) {
                    if (widx == WCAP) drain(std::false_type{});
                    const int c = min(32, len - w0);
                    const float4 *__restrict__ p = refs + gs + w0;
                    const float neg_tau = -tau;  // dead lanes: tau = -1 => t > 0 => bit 0
                    unsigned m = 0;
                    int i = 0;
                    // 4 candidates per scalar load (s_load_dwordx16), 8 in flight
                    struct Quad { float4 v[4]; };
                    const Quad *__restrict__ pq = reinterpret_cast<const Quad *>(p);
                    for (; i + 8 <= c; i += 8) {
                        const Quad a = pq[i / 4], b = pq[i / 4 + 1];  // wave-uniform addresses
#pragma unroll
                        for (int u = 0; u < 4; ++u) m = shift_in_lt(m, qx, qy, qz, a.v[u].x, a.v[u].y, a.v[u].z, neg_tau);
#pragma unroll
                        for (int u = 0; u < 4; ++u) m = shift_in_lt(m, qx, qy, qz, b.v[u].x, b.v[u].y, b.v[u].z, neg_tau);
                    }
                    for (; i < c; ++i) {
                        float4 P = p[i];
                        m = shift_in_lt(m, qx, qy, qz, P.x, P.y, P.z, neg_tau);
                    }
                    m <<= (32 - c);  // candidate i of this word <-> bit 31-i
                    if (dbg & 64) atomicAdd(&gp->exhaustive_count, (unsigned)__builtin_popcount(m));  // profiling: candidates passed
                    mask[widx][lane] = m;
                    if (lane == 0) {
                        wbase[widx] = (unsigned)(gs + w0);
                        if constexpr (MF) wseg[widx] = make_uint2(32u, 0u);
                    }
                    nzw |= (m != 0 ? 1u : 0u) << widx;
                    ++widx;
                }
            }
            }
            drain(std::true_type{});

            // ---- exact iff the (k+1)-th distance lies inside the searched cells
            if (is_query) {
                double kth_d2;
                if constexpr (CERT) kth_d2 = lst.kth_of_set();   // k = 16 = the list's length: its largest entry, sorted or not
                else kth_d2 = lst.kth(kq);
                if (dbg & 8) {
                    if (kth_d2 == 12345.0) mean_out[0] = 1.0f;  // keeps the list live, writes nothing
                } else if (dbg & 4) {
                    mean_out[(int)__float_as_uint(qp.w) - q_begin] = (float)kth_d2;
                } else if (kth_d2 <= racc_sq) {
                    if constexpr (CERT) {   // (kth_out is null here: dispatch_bricks)
                        bool exact;
                        mean_out[(int)__float_as_uint(qp.w) - q_begin] = mean_from_net_cert(lst, exact);
#ifdef GSX_ABLATE
                        if ((dbg & 128) && exact && lane == __builtin_ctzll(__ballot(1))) atomicAdd(&gp->exhaustive_count, 1u);   // profiling: batches on the exact branch
#endif
                        (void)exact;
                    } else {
                    kth_emit<NET>(gp, kth_out, (int)__float_as_uint(qp.w) - q_begin, kth_d2, qx, qy, qz);
                    if constexpr (NET) mean_out[(int)__float_as_uint(qp.w) - q_begin] = mean_from_net(lst, k);
                    else mean_out[(int)__float_as_uint(qp.w) - q_begin] = mean_from_list<KCAP>(lst, k);
                    }
                } else {
                    unsigned slot = atomicAdd(&gp->fail_count, 1u);
                    faillist[slot] = (unsigned)qidx;
                }
            }
        }
    }
#ifdef GSX_WAVE_STAMPS
    if constexpr (!EXTRA) ws_write(gp, 0, wq, ws_t0, nullptr);
#endif
}

// ---------------------------------------------------------------- knn_ring (fallback)
// One wave per failed query: search the (2H+1)^3 cells around the query's cell, H = 2,4,8..;
// lanes split every row, keep private sorted lists, then the wave merges the 64 lists by
// repeated min-extraction.  Exact once the (k+1)-th distance <= H*r_safe or the ring covers
// the whole grid.
__device__ __forceinline__ double wave_min_f64(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        double o = __shfl_xor(v, off);
        v = o < v ? o : v;
    }
    return v;
}

constexpr int RING_ROWS = 320;  // rows whose bounds are prefetched in parallel (covers H <= 8: 17x17)

template <int KCAP>
__global__ __launch_bounds__(BRICK_THREADS) void knn_ring_kernel(
    GridParams *__restrict__ gp, const float4 *__restrict__ refs, const unsigned *__restrict__ rstart,
    const float4 *__restrict__ qpts, const unsigned *__restrict__ faillist, int k, int q_begin,
    float *__restrict__ mean_out, double *__restrict__ kth_out, unsigned *__restrict__ heavylist, int out_count, int after_fast)
{
    __shared__ double s_out[BRICK_THREADS / 64][KCAP];
    __shared__ int s_rs[BRICK_THREADS / 64][RING_ROWS];       // first point of each row
    __shared__ int s_ro[BRICK_THREADS / 64][RING_ROWS + 1];   // flat offset of each row
    const int lane = lane_id();
    const int wv = uniform((int)(threadIdx.x >> 6));
    double *out = s_out[wv];
    int *rs = s_rs[wv], *ro = s_ro[wv];
    const GridParams g = *gp;
    if (g.bad_input) {  // non-finite coordinates: no kernel searched anything -- the whole output becomes NaN
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < out_count; i += gridDim.x * blockDim.x)
            mean_out[i] = __builtin_nanf("");
        return;
    }
    const int nfail = (int)(after_fast ? g.ring2_count : g.fail_count);   // after_fast: what knn_ring_fast could not finish
    if (nfail == 0) return;
    const int kk = k + 1;

    WorkQueue wq;
    wq_init(wq, gp->ring_ctr, nfail, BRICK_THREADS / 64);
    for (;;) {
        const int t = uniform(wq_next(wq));
        if (t < 0) break;
        const unsigned fq = faillist[t];
        const float4 qp = qpts[fq];
        const double qxd = (double)qp.x, qyd = (double)qp.y, qzd = (double)qp.z;
        const int cx = cell_coord(qp.x, g.ox, g.inv_h, g.nx);
        const int cy = cell_coord(qp.y, g.oy, g.inv_h, g.ny);
        const int cz = cell_coord(qp.z, g.oz, g.inv_h, g.nz);

        for (int H = 2;; H *= 2) {
            double a[KCAP];  // ascending, +inf padded: a[0] is this lane's smallest
#pragma unroll
            for (int i = 0; i < KCAP; ++i) a[i] = __builtin_inf();
            auto consider = [&](const float4 p) __attribute__((always_inline)) {
                double d = dist2_f64(qxd, qyd, qzd, p.x, p.y, p.z);
                if (d < a[KCAP - 1]) {
#pragma unroll
                    for (int i = 0; i < KCAP; ++i) {
                        double lo, hi;
                        asm("v_min_f64 %0, %1, %2" : "=v"(lo) : "v"(a[i]), "v"(d));
                        asm("v_max_f64 %0, %1, %2" : "=v"(hi) : "v"(a[i]), "v"(d));
                        a[i] = lo;
                        d = hi;
                    }
                }
            };
            const int x0 = max(cx - H, 0), x1 = min(cx + H, g.nx - 1);
            const int y0 = max(cy - H, 0), y1 = min(cy + H, g.ny - 1);
            const int z0 = max(cz - H, 0), z1 = min(cz + H, g.nz - 1);
            const int nyr = y1 - y0 + 1;
            const int nrows = nyr * (z1 - z0 + 1);
            if (nrows <= RING_ROWS) {
                // all row bounds in parallel (one lane per row), wave scan -> flat offsets in LDS
                int carry = 0;
                for (int r0 = 0; r0 < nrows; r0 += 64) {
                    const int r = r0 + lane;
                    int s = 0, len = 0;
                    if (r < nrows) {
                        const int zz = z0 + r / nyr, yy = y0 + r % nyr;
                        const int row = row_base(g, yy, zz);
                        s = (int)rstart[row + x0];
                        len = (int)rstart[row + x1 + 1] - s;
                    }
                    int inc = len;
#pragma unroll
                    for (int off = 1; off < 64; off <<= 1) {
                        int o = __shfl_up(inc, off);
                        if (lane >= off) inc += o;
                    }
                    if (r < nrows) {
                        rs[r] = s;
                        ro[r] = carry + inc - len;
                    }
                    carry += __shfl(inc, 63);
                }
                const int total = carry;
                if (g.heavy_limit > 0 && total > g.heavy_limit) {  // wave-uniform
                    if (lane == 0) heavylist[atomicAdd(&gp->heavy_count, 1u)] = fq;
                    break;
                }
                if (lane == 0) ro[nrows] = total;
                wave_sync();
                // every lane walks the flat candidate range with stride 64, 4 independent loads in flight
                int row = 0;
                for (int f0 = lane; f0 < total; f0 += 256) {
                    float4 p[4];
                    bool ok[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int f = f0 + 64 * u;
                        ok[u] = f < total;
                        if (ok[u]) {
                            while (f >= ro[row + 1]) ++row;
                            p[u] = refs[rs[row] + (f - ro[row])];
                        }
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (ok[u]) consider(p[u]);
                }
            } else {
                if (g.heavy_limit > 0) {
                    int total = 0;
                    for (int r = lane; r < nrows; r += 64) {
                        const int row = row_base(g, y0 + r % nyr, z0 + r / nyr);
                        total += (int)(rstart[row + x1 + 1] - rstart[row + x0]);
                    }
#pragma unroll
                    for (int off = 32; off > 0; off >>= 1) total += __shfl_xor(total, off);
                    if (uniform(total) > g.heavy_limit) {
                        if (lane == 0) heavylist[atomicAdd(&gp->heavy_count, 1u)] = fq;
                        break;
                    }
                }
                for (int zz = z0; zz <= z1; ++zz)
                    for (int yy = y0; yy <= y1; ++yy) {
                        const int row = row_base(g, yy, zz);
                        const int s = (int)rstart[row + x0], e = (int)rstart[row + x1 + 1];
                        for (int j = s + lane; j < e; j += 64) consider(refs[j]);
                    }
            }
            // merge: kk rounds of wave-min over the list heads
            for (int r = 0; r < kk; ++r) {
                const double mn = wave_min_f64(a[0]);
                const unsigned long long eq = __ballot(a[0] == mn);
                const int win = (int)__builtin_ctzll(eq);
                if (lane == 0) out[r] = mn;
                if (lane == win) {
#pragma unroll
                    for (int i = 0; i + 1 < KCAP; ++i) a[i] = a[i + 1];
                    a[KCAP - 1] = __builtin_inf();
                }
            }
            wave_sync();
            const bool covers = x0 == 0 && y0 == 0 && z0 == 0 && x1 == g.nx - 1 && y1 == g.ny - 1 && z1 == g.nz - 1;
            const double rH = (double)H * g.hprime * (1.0 - 1e-3);
            const double kth = out[kk - 1];
            if (covers || kth <= rH * rH) {
                // sqrt of the k+1 winners in parallel (one lane each), then lane 0 sums in numpy order
                for (int i = lane; i < kk; i += 64) out[i] = __dsqrt_rn(out[i]);
                wave_sync();
                if (lane == 0) {
                    if (covers && !(kth <= rH * rH)) atomicAdd(&gp->exhaustive_count, 1u);
                    double sum = pairwise_sum_le128([&](int i) { return out[1 + i]; }, k);
                    mean_out[(int)__float_as_uint(qp.w) - q_begin] = mean_finish(sum, k);
                    kth_emit(gp, kth_out, (int)__float_as_uint(qp.w) - q_begin, kth, qp.x, qp.y, qp.z);
                }
                wave_sync();
                break;
            }
            wave_sync();
        }
    }
}

// ---------------------------------------------------------------- knn_anyk (k > 64)
// The reference's cKDTree path takes any k (data_processor.py:171; the CLI's hidden --sor_k, main.py:278); the
// register-resident lists of the kernels above stop at k = 64.  Larger k takes this exact, list-free path: one wave per
// query; the (2H+1)^3 cells around the query's cell are walked as contiguous x-rows; the (k+1)-th smallest squared
// distance is found by an 8-pass radix SELECT on the float64 bit pattern (non-negative doubles order like their bits): a
// 256-bin LDS histogram per pass over the candidates that match the prefix so far, distances recomputed each pass -- no
// per-query storage that grows with the candidate count.  Exact iff that distance is within the guaranteed radius
// H h' (1 - 1e-3) (section 4.2's argument) or the block covers the grid; otherwise H grows.  The k+1 winners (ties at the
// k-th value are equal numbers: which one is taken does not matter) are then collected, sorted in LDS by a wave-wide
// bitonic network and summed by one lane in numpy's pairwise order (loops_utils.h.src: 8 accumulators up to 128
// elements, halves rounded down to a multiple of 8 above).  k + 1 <= 2048.  Slow (9 distance evaluations per candidate)
// and rare: nothing in the CLI's documented flags reaches it (--sor_intensity maps to k <= 50).
constexpr int ANYK_MAX = 2048;

__global__ __launch_bounds__(BRICK_THREADS) void knn_anyk_kernel(GridParams *__restrict__ gp, const float4 *__restrict__ refs,
                                                                 const unsigned *__restrict__ rstart, const float4 *__restrict__ qpts,
                                                                 int nq, int k, int q_begin, float *__restrict__ mean_out,
                                                                 double *__restrict__ kth_out)
{
    __shared__ unsigned s_hist[BRICK_THREADS / 64][256];
    __shared__ double s_sel[BRICK_THREADS / 64][ANYK_MAX];
    __shared__ unsigned s_cnt[BRICK_THREADS / 64];
    const int lane = lane_id();
    const int wv = uniform((int)(threadIdx.x >> 6));
    unsigned *hist = s_hist[wv];
    double *sel = s_sel[wv];
    const GridParams g = *gp;
    const int kk = k + 1;
    const int nwaves = gridDim.x * (BRICK_THREADS / 64);
    if (g.bad_input) {
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nq; i += gridDim.x * blockDim.x) mean_out[i] = __builtin_nanf("");
        return;
    }
    for (int t = blockIdx.x * (BRICK_THREADS / 64) + wv; t < nq; t += nwaves) {
        const float4 qp = qpts[t];
        if (__float_as_uint(qp.w) >> 31) continue;   // reference-only point
        const double qxd = (double)qp.x, qyd = (double)qp.y, qzd = (double)qp.z;
        const int cx = cell_coord(qp.x, g.ox, g.inv_h, g.nx);
        const int cy = cell_coord(qp.y, g.oy, g.inv_h, g.ny);
        const int cz = cell_coord(qp.z, g.oz, g.inv_h, g.nz);
        for (int H = 1;; ++H) {
            const int x0 = max(cx - H, 0), x1 = min(cx + H, g.nx - 1);
            const int y0 = max(cy - H, 0), y1 = min(cy + H, g.ny - 1);
            const int z0 = max(cz - H, 0), z1 = min(cz + H, g.nz - 1);
            const bool covers = x0 == 0 && y0 == 0 && z0 == 0 && x1 == g.nx - 1 && y1 == g.ny - 1 && z1 == g.nz - 1;
            // f(d2 bits) for every candidate of the block
            auto for_each = [&](auto f) __attribute__((always_inline)) {
                for (int zz = z0; zz <= z1; ++zz)
                    for (int yy = y0; yy <= y1; ++yy) {
                        const int row = row_base(g, yy, zz);
                        const int sb = (int)rstart[row + x0], se = (int)rstart[row + x1 + 1];
                        for (int j = sb + lane; j < se; j += 64) {
                            const float4 p = refs[j];
                            f((unsigned long long)__double_as_longlong(dist2_f64(qxd, qyd, qzd, p.x, p.y, p.z)));
                        }
                    }
            };
            // ---- radix select of the kk-th smallest
            unsigned long long prefix = 0ull, pmask = 0ull;
            int remaining = kk;
            bool enough = true;
            for (int pass = 0; pass < 8 && enough; ++pass) {
                const int shift = 56 - 8 * pass;
                for (int i = lane; i < 256; i += 64) hist[i] = 0u;
                wave_sync();
                for_each([&](unsigned long long b) {
                    if ((b & pmask) == prefix) atomicAdd(&hist[(unsigned)(b >> shift) & 255u], 1u);
                });
                wave_sync();
                // lane l owns bins 4l .. 4l+3
                const unsigned c0 = hist[4 * lane], c1 = hist[4 * lane + 1], c2 = hist[4 * lane + 2], c3 = hist[4 * lane + 3];
                unsigned inc = c0 + c1 + c2 + c3;
                const unsigned mine = inc;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const unsigned o = __shfl_up(inc, off);
                    if (lane >= off) inc += o;
                }
                const unsigned total = __shfl(inc, 63);
                if (pass == 0 && (int)total < kk) {   // fewer than k+1 points in the block
                    enough = false;
                    break;
                }
                const unsigned before = inc - mine;
                const bool here = (int)before < remaining && remaining <= (int)(before + mine);
                const int owner = (int)__builtin_ctzll(__ballot(here));
                unsigned bin = 0, skip = 0;
                if (lane == owner) {
                    const unsigned c[4] = {c0, c1, c2, c3};
                    unsigned run = before;
                    for (int j = 0; j < 4; ++j) {
                        if ((int)(run + c[j]) >= remaining) {
                            bin = 4u * (unsigned)lane + (unsigned)j;
                            skip = run;
                            break;
                        }
                        run += c[j];
                    }
                }
                bin = (unsigned)__shfl((int)bin, owner);
                skip = (unsigned)__shfl((int)skip, owner);
                remaining -= (int)skip;
                prefix |= (unsigned long long)bin << shift;
                pmask |= 0xffull << shift;
                wave_sync();
            }
            if (!enough) {
                if (covers) {   // N < k + 1: cKDTree pads with inf -> the mean is inf
                    if (lane == 0) {
                        mean_out[(int)__float_as_uint(qp.w) - q_begin] = __builtin_inff();
                        kth_emit(gp, kth_out, (int)__float_as_uint(qp.w) - q_begin, __builtin_inf(), qp.x, qp.y, qp.z);
                    }
                    break;
                }
                continue;
            }
            const double kth = __longlong_as_double((long long)prefix);
            const double rH = (double)H * g.hprime * (1.0 - 1e-3);
            if (!(covers || kth <= rH * rH)) continue;
            // ---- collect the values strictly below the kk-th, fill up with the kk-th itself, sort, sum
            if (lane == 0) s_cnt[wv] = 0u;
            wave_sync();
            for_each([&](unsigned long long b) {
                if (b < prefix) sel[atomicAdd(&s_cnt[wv], 1u)] = __longlong_as_double((long long)b);
            });
            wave_sync();
            const int nlt = (int)s_cnt[wv];   // < kk by the definition of the kk-th smallest
            int P = 64;
            while (P < kk) P <<= 1;
            for (int i = nlt + lane; i < P; i += 64) sel[i] = i < kk ? kth : __builtin_inf();
            wave_sync();
            for (int size = 2; size <= P; size <<= 1)
                for (int stride = size >> 1; stride > 0; stride >>= 1) {
                    for (int i = lane; i < P / 2; i += 64) {
                        const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                        const bool up = (lo & size) == 0;
                        const double a = sel[lo], b = sel[hi];
                        if ((a > b) == up) {
                            sel[lo] = b;
                            sel[hi] = a;
                        }
                    }
                    wave_sync();
                }
            for (int i = lane; i < kk; i += 64) sel[i] = sqrt_rn_dist2(sel[i]);
            wave_sync();
            if (lane == 0) {
                const double sum = pairwise_sum_np<5>([&](int i) { return sel[1 + i]; }, 0, k);   // entry 0 is the query itself
                mean_out[(int)__float_as_uint(qp.w) - q_begin] = mean_finish(sum, k);
                kth_emit(gp, kth_out, (int)__float_as_uint(qp.w) - q_begin, kth, qp.x, qp.y, qp.z);   // (slab mode: the certificate is counted here)
                if (covers && !(kth <= rH * rH)) atomicAdd(&gp->exhaustive_count, 1u);
            }
            wave_sync();
            break;
        }
    }
}

// ---------------------------------------------------------------- knn_heavy (ring queries next to a huge cell)
// A far "floater" whose ring reaches a cell holding most of the cloud would make ONE wave scan
// millions of candidates (measured: 11 ms for 9 such queries at 1M splats).  knn_ring hands these
// queries over; here every wave takes (query, 32768-point chunk of the WHOLE sorted array), keeps
// the k+1 smallest squared distances of its chunk, and a second kernel merges the chunks of a
// query -- exhaustive, hence exact, and spread over the chip.
template <int KCAP>
struct LaneTop {
    double a[KCAP];  // ascending, +inf padded
    __device__ __forceinline__ void init()
    {
#pragma unroll
        for (int i = 0; i < KCAP; ++i) a[i] = __builtin_inf();
    }
    __device__ __forceinline__ void consider(double d)
    {
        if (d < a[KCAP - 1]) {
#pragma unroll
            for (int i = 0; i < KCAP; ++i) {
                double lo, hi;
                asm("v_min_f64 %0, %1, %2" : "=v"(lo) : "v"(a[i]), "v"(d));
                asm("v_max_f64 %0, %1, %2" : "=v"(hi) : "v"(a[i]), "v"(d));
                a[i] = lo;
                d = hi;
            }
        }
    }
    // the kk smallest over the whole wave -> out[0..kk) (written by lane 0)
    __device__ __forceinline__ void wave_merge(int kk, int lane, double *out)
    {
        for (int r = 0; r < kk; ++r) {
            const double mn = wave_min_f64(a[0]);
            const unsigned long long eq = __ballot(a[0] == mn);
            const int win = (int)__builtin_ctzll(eq);
            if (lane == 0) out[r] = mn;
            if (lane == win) {
#pragma unroll
                for (int i = 0; i + 1 < KCAP; ++i) a[i] = a[i + 1];
                a[KCAP - 1] = __builtin_inf();
            }
        }
    }
};

template <int KCAP>
__global__ __launch_bounds__(BRICK_THREADS) void knn_heavy_scan_kernel(const float4 *__restrict__ refs, int n,
                                                                       const float4 *__restrict__ qpts,
                                                                       const unsigned *__restrict__ heavylist, int first,
                                                                       int count, int k, double *__restrict__ part)
{
    const int lane = lane_id();
    const int kk = k + 1;
    const int nchunks = (n + HEAVY_CHUNK - 1) / HEAVY_CHUNK;
    const long long items = (long long)count * nchunks;
    const long long wave0 = (long long)blockIdx.x * (BRICK_THREADS / 64) + (threadIdx.x >> 6);
    const long long nwaves = (long long)gridDim.x * (BRICK_THREADS / 64);
    for (long long it = wave0; it < items; it += nwaves) {
        const int qi = (int)(it / nchunks), c = (int)(it - (long long)qi * nchunks);
        const float4 qp = qpts[heavylist[first + qi]];
        const double qxd = (double)qp.x, qyd = (double)qp.y, qzd = (double)qp.z;
        LaneTop<KCAP> top;
        top.init();
        const int j0 = c * HEAVY_CHUNK, j1 = min(n, j0 + HEAVY_CHUNK);
        for (int j = j0 + lane; j < j1; j += 256) {
            float4 p[4];
            bool ok[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                ok[u] = j + 64 * u < j1;
                if (ok[u]) p[u] = refs[j + 64 * u];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (ok[u]) top.consider(dist2_f64(qxd, qyd, qzd, p[u].x, p[u].y, p[u].z));
        }
        top.wave_merge(kk, lane, part + (size_t)it * KCAP);
    }
}

template <int KCAP>
__global__ __launch_bounds__(BRICK_THREADS) void knn_heavy_merge_kernel(GridParams *__restrict__ gp, int n,
                                                                        const float4 *__restrict__ qpts,
                                                                        const unsigned *__restrict__ heavylist, int first,
                                                                        int count, int k, int q_begin,
                                                                        const double *__restrict__ part,
                                                                        float *__restrict__ mean_out,
                                                                        double *__restrict__ kth_out)
{
    __shared__ double s_out[BRICK_THREADS / 64][KCAP];
    const int lane = lane_id();
    const int wv = uniform((int)(threadIdx.x >> 6));
    double *out = s_out[wv];
    const int kk = k + 1;
    const int nchunks = (n + HEAVY_CHUNK - 1) / HEAVY_CHUNK;
    const int qi = blockIdx.x * (BRICK_THREADS / 64) + wv;
    if (qi >= count) return;
    LaneTop<KCAP> top;
    top.init();
    const double *mine = part + (size_t)qi * nchunks * KCAP;
    for (int e = lane; e < nchunks * KCAP; e += 64)
        if (e % KCAP < kk) top.consider(mine[e]);
    top.wave_merge(kk, lane, out);
    wave_sync();
    const double kth = out[kk - 1];
    for (int i = lane; i < kk; i += 64) out[i] = __dsqrt_rn(out[i]);
    wave_sync();
    if (lane == 0) {
        const float4 qp = qpts[heavylist[first + qi]];
        atomicAdd(&gp->exhaustive_count, 1u);
        double sum = pairwise_sum_le128([&](int i) { return out[1 + i]; }, k);
        mean_out[(int)__float_as_uint(qp.w) - q_begin] = mean_finish(sum, k);
        kth_emit(gp, kth_out, (int)__float_as_uint(qp.w) - q_begin, kth, qp.x, qp.y, qp.z);   // (slab mode: the certificate is counted here)
    }
}

// ---------------------------------------------------------------- host side
static int grid_blocks(const gsx_ctx *ctx, int64_t n, int per_thread = 1)
{
    int64_t want = (n + 256LL * per_thread - 1) / (256LL * per_thread);
    int64_t cap = (int64_t)ctx->num_cu * 16;
    return (int)std::max<int64_t>(1, std::min(want, cap));
}

// ---------------------------------------------------------------- adaptive refinement (level L -> L+1)
// Bucket-major index of cell (cx, cy, cz) -- the same mapping as row_base_g in knn_brick.
__device__ __forceinline__ int cell_index_of(const GridParams *gp, int cx, int cy, int cz)
{
    const int g = gp->bk_g;
    const int by_ = cy / g, bz_ = cz / g;
    return (bz_ * gp->bk_ny + by_) * gp->bk_cells + ((cz - bz_ * g) * g + (cy - by_ * g)) * gp->nx + cx;
}

// per component of deferred bricks: fresh counters and an empty query box
__global__ void reset_refine_kernel(GridParams *gp)
{
    gp->sub_count = 0;
    gp->sub_queries = 0;
    for (int a = 0; a < 3; ++a) {
        gp->qb_lo[a] = __builtin_inff();
        gp->qb_hi[a] = -__builtin_inff();
    }
}

// one 64-thread block per deferred brick: flag the cells of its neighbourhood (pass 0: value 1) and its
// own cells (pass 1: value 3 -- their points are the queries of the finer level)
__global__ __launch_bounds__(64) void mark_cells_kernel(const GridParams *__restrict__ gp, const unsigned *__restrict__ bricks,
                                                        unsigned count, uint8_t *__restrict__ cellflag, int own_pass)
{
    if (blockIdx.x >= count) return;
    const int b = (int)bricks[blockIdx.x];
    const int nbx = gp->nbx, nby = gp->nby;
    const int bz = b / (nbx * nby), brem = b - bz * nbx * nby, by = brem / nbx, bx = brem - by * nbx;
    const int t = threadIdx.x;
    const int dx = t & 3, dy = (t >> 2) & 3, dz = t >> 4;
    if (dx >= gp->bdx + 2 || dy >= gp->bdy + 2 || dz >= gp->bdz + 2) return;
    const int cx = bx * gp->bdx - 1 + dx, cy = by * gp->bdy - 1 + dy, cz = bz * gp->bdz - 1 + dz;
    if (cx < 0 || cy < 0 || cz < 0 || cx >= gp->nx || cy >= gp->ny || cz >= gp->nz) return;
    const bool own = dx >= 1 && dx <= gp->bdx && dy >= 1 && dy <= gp->bdy && dz >= 1 && dz <= gp->bdz;
    if (own_pass ? own : true) cellflag[cell_index_of(gp, cx, cy, cz)] = own_pass ? 3 : 1;
}

__device__ __forceinline__ void atomic_min_f32(float *addr, float v)  // finite v; *addr starts at +inf
{
    if (v >= 0.0f) atomicMin(reinterpret_cast<int *>(addr), __float_as_int(v));
    else atomicMax(reinterpret_cast<unsigned *>(addr), __float_as_uint(v));
}
__device__ __forceinline__ void atomic_max_f32(float *addr, float v)  // finite v; *addr starts at -inf
{
    if (v >= 0.0f) atomicMax(reinterpret_cast<int *>(addr), __float_as_int(v));
    else atomicMin(reinterpret_cast<unsigned *>(addr), __float_as_uint(v));
}

// bounding box and number of the finer level's queries (points of the cells flagged 3).  Grid-stride,
// reduced per workgroup first: one set of same-address atomics per WAVE serialised in L2 and took
// 12 ms at 10M splats.
__global__ __launch_bounds__(256) void query_bbox_kernel(GridParams *__restrict__ gp, const float4 *__restrict__ refs, int n,
                                                         const uint8_t *__restrict__ cellflag)
{
    __shared__ float s_red[4][6];
    __shared__ unsigned s_cnt[4];
    float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
    float hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    unsigned cnt = 0;
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
        const float4 P = refs[j];
        const int cx = cell_coord(P.x, gp->ox, gp->inv_h, gp->nx), cy = cell_coord(P.y, gp->oy, gp->inv_h, gp->ny),
                  cz = cell_coord(P.z, gp->oz, gp->inv_h, gp->nz);
        if (cellflag[cell_index_of(gp, cx, cy, cz)] == 3) {
            lo[0] = fminf(lo[0], P.x); lo[1] = fminf(lo[1], P.y); lo[2] = fminf(lo[2], P.z);
            hi[0] = fmaxf(hi[0], P.x); hi[1] = fmaxf(hi[1], P.y); hi[2] = fmaxf(hi[2], P.z);
            ++cnt;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = fminf(lo[a], __shfl_xor(lo[a], off));
            hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], off));
        }
        cnt += __shfl_xor(cnt, off);
    }
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            s_red[wv][a] = lo[a];
            s_red[wv][3 + a] = hi[a];
        }
        s_cnt[wv] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned c = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        if (c) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                atomic_min_f32(&gp->qb_lo[a], fminf(fminf(s_red[0][a], s_red[1][a]), fminf(s_red[2][a], s_red[3][a])));
                atomic_max_f32(&gp->qb_hi[a], fmaxf(fmaxf(s_red[0][3 + a], s_red[1][3 + a]), fmaxf(s_red[2][3 + a], s_red[3][3 + a])));
            }
            atomicAdd(&gp->sub_queries, c);
        }
    }
}

struct ClipBox {
    float lo[3], hi[3];  // reference points outside are not gathered
    float r_cert;        // every such point is farther than this from every query (0 = no clipping)
};

// gather the points of the flagged cells into a SoA sub-cloud.  One workgroup per 8192-point chunk:
// count, reserve the chunk's run with ONE atomic, then append in order (a returning atomic per wave
// on the same counter cost 1.8 ms at 10M splats).
constexpr int GATHER_CHUNK = 8192;
__global__ __launch_bounds__(256) void gather_sub_kernel(GridParams *__restrict__ gp, const float4 *__restrict__ refs, int n,
                                                         const uint8_t *__restrict__ cellflag, ClipBox clip,
                                                         float *__restrict__ sub, unsigned *__restrict__ sub_orig,
                                                         unsigned *__restrict__ sub_sorted)
{
    __shared__ unsigned s_wave[4];
    __shared__ unsigned s_base;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int j0 = blockIdx.x * GATHER_CHUNK, j1 = min(n, j0 + GATHER_CHUNK);
    auto flag_of = [&](int j, float4 &P) -> unsigned {
        P = refs[j];
        const int cx = cell_coord(P.x, gp->ox, gp->inv_h, gp->nx), cy = cell_coord(P.y, gp->oy, gp->inv_h, gp->ny),
                  cz = cell_coord(P.z, gp->oz, gp->inv_h, gp->nz);
        unsigned flag = cellflag[cell_index_of(gp, cx, cy, cz)];
        if (flag == 1 && clip.r_cert > 0.0f &&
            !(P.x >= clip.lo[0] && P.x <= clip.hi[0] && P.y >= clip.lo[1] && P.y <= clip.hi[1] && P.z >= clip.lo[2] &&
              P.z <= clip.hi[2]))
            flag = 0;  // a reference point farther than r_cert from the box of the queries
        return flag;
    };
    // pass 1: how many points of this chunk are taken, per wave (each wave owns a contiguous quarter)
    const int q = (j1 - j0 + 3) / 4;
    const int w0 = j0 + wv * q, w1 = min(j1, w0 + q);
    unsigned mine = 0;
    for (int j = w0 + lane; j < w1; j += 64) {
        float4 P;
        mine += flag_of(j, P) != 0;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off);
    if (lane == 0) s_wave[wv] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned tot = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        s_base = tot ? atomicAdd(&gp->sub_count, tot) : 0u;
    }
    __syncthreads();
    unsigned pos = s_base;
    for (int i = 0; i < wv; ++i) pos += s_wave[i];
    // pass 2: append
    for (int jb = w0; jb < w1; jb += 64) {
        const int j = jb + lane;
        float4 P = make_float4(0.f, 0.f, 0.f, 0.f);
        const unsigned flag = j < w1 ? flag_of(j, P) : 0u;
        const unsigned long long take = __ballot(flag != 0);
        if (flag != 0) {
            const unsigned at = pos + (unsigned)__builtin_popcountll(take & ((1ull << lane) - 1ull));
            sub[at] = P.x;
            sub[(size_t)n + at] = P.y;
            sub[2 * (size_t)n + at] = P.z;
            sub_orig[at] = __float_as_uint(P.w) | (flag == 3 ? 0x80000000u : 0u);
            sub_sorted[at] = (unsigned)j;
        }
        pos += (unsigned)__builtin_popcountll(take);
    }
}

// Density probe of a gathered sub-cloud (round 3).  The finer level used to size its cells from the sub-cloud's bounding-box
// VOLUME; a Gaussian blob's core is ~30x denser than its box average, so every level only peeled a shell (3-4 levels per
// blob).  Here: counts of a coarse G^3 grid over the box of the group's queries, then the point-weighted histogram of
// log2(count) -- the host reads 32 numbers and sizes the cells for the density that 85 % of the points do not exceed,
// divided by the factor a brick may be over-full before it is deferred again.  Affects speed only: any cell edge is exact.
struct ProbeBox {
    float lo[3], inv[3];   // bin = (int)((p - lo) * inv), inv = G / extent
    int g;
};
__global__ __launch_bounds__(256) void probe_count_kernel(const float *__restrict__ sub, int n_stride, const unsigned *__restrict__ n_sub_p,
                                                          ProbeBox pb, unsigned *__restrict__ counts)
{
    const int n_sub = (int)*n_sub_p;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n_sub; i += gridDim.x * 256) {
        const float p[3] = {sub[i], sub[(size_t)n_stride + i], sub[2 * (size_t)n_stride + i]};
        int b[3];
        bool in = true;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float t = (p[a] - pb.lo[a]) * pb.inv[a];
            in = in && t >= 0.0f && t < (float)pb.g + 1.0f;
            b[a] = min(pb.g - 1, max(0, (int)t));
        }
        if (in) atomicAdd(&counts[(b[2] * pb.g + b[1]) * pb.g + b[0]], 1u);
    }
}
__global__ __launch_bounds__(256) void probe_hist_kernel(const float *__restrict__ sub, int n_stride, const unsigned *__restrict__ n_sub_p,
                                                         ProbeBox pb, const unsigned *__restrict__ counts, unsigned *__restrict__ hist32)
{
    __shared__ unsigned s_h[32];
    if (threadIdx.x < 32) s_h[threadIdx.x] = 0u;
    __syncthreads();
    const int n_sub = (int)*n_sub_p;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n_sub; i += gridDim.x * 256) {
        const float p[3] = {sub[i], sub[(size_t)n_stride + i], sub[2 * (size_t)n_stride + i]};
        int b[3];
        bool in = true;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float t = (p[a] - pb.lo[a]) * pb.inv[a];
            in = in && t >= 0.0f && t < (float)pb.g + 1.0f;
            b[a] = min(pb.g - 1, max(0, (int)t));
        }
        if (in) {
            const unsigned c = counts[(b[2] * pb.g + b[1]) * pb.g + b[0]];
            atomicAdd(&s_h[31 - __builtin_clz(c | 1u)], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < 32 && s_h[threadIdx.x]) atomicAdd(&hist32[threadIdx.x], s_h[threadIdx.x]);
}

// A finer-level result is the exact answer iff its (k+1)-th neighbour lies inside the region this
// level guarantees to have gathered: every point outside the brick's neighbourhood is farther than
// the distance to the nearest neighbourhood face that has cells behind it (same bound and margins
// as knn_brick's boundary-aware acceptance radius).  Anything else goes to this level's knn_ring.
__global__ __launch_bounds__(256) void merge_sub_kernel(GridParams *__restrict__ gp, const float *__restrict__ sub, int n,
                                                        const unsigned *__restrict__ sub_orig,
                                                        const unsigned *__restrict__ sub_sorted,
                                                        const float *__restrict__ submean, const double *__restrict__ subkth,
                                                        int q_begin, float r_cert, float *__restrict__ mean_out,
                                                        double *__restrict__ kth_out, unsigned *__restrict__ faillist)
{
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= gp->sub_count) return;
    const unsigned so = sub_orig[i];
    if (!(so >> 31)) return;  // only gathered as a reference point
    const int orig = (int)(so & 0x7fffffffu);
    const float q[3] = {sub[i], sub[(size_t)n + i], sub[2 * (size_t)n + i]};
    const float o[3] = {gp->ox, gp->oy, gp->oz};
    const int dim[3] = {gp->nx, gp->ny, gp->nz};
    const int bd[3] = {gp->bdx, gp->bdy, gp->bdz};
    const float hf = (float)gp->hprime;
    float rsafe = r_cert > 0.0f ? r_cert : 3.0e38f;  // clipped references: see gather_sub_kernel
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int c = cell_coord(q[a], o[a], gp->inv_h, dim[a]);
        const int bb = c / bd[a];
        const int ulo = bb * bd[a] - 1, uhi = bb * bd[a] + bd[a];
        const float rel = q[a] - o[a];
        if (ulo > 0) rsafe = fminf(rsafe, rel - (float)ulo * hf - 2e-3f * hf);
        if (uhi < dim[a] - 1) rsafe = fminf(rsafe, (float)(uhi + 1) * hf - rel - 2e-3f * hf);
    }
    const double kth = subkth[i];
    if (rsafe > 0.0f && kth <= (double)rsafe * (double)rsafe) {
        mean_out[orig - q_begin] = submean[i];
        kth_emit(gp, kth_out, orig - q_begin, kth, q[0], q[1], q[2]);
    } else {
        faillist[atomicAdd(&gp->fail_count, 1u)] = sub_sorted[i];
    }
}

struct BrickLaunch {
    GridParams *gp;
    const float4 *refs;
    const unsigned *rstart;
    const float4 *qpts;
    const unsigned *qstart;
    int k;
    int64_t q_begin;
    float *mean_out;
    double *kth_out;
    unsigned *faillist;
    unsigned *ring2;      // what knn_ring_fast hands on to knn_ring
    uint2 *extra;
    unsigned *deferred;
    unsigned *heavylist;
    int64_t out_count;    // entries of mean_out (poisoned with NaN when the input is not finite)
    int64_t n_ref;        // reference points binned at this level (mean density for knn_ring_fast)
    const unsigned *fstart = nullptr;   // planned bricks: fine_start and the brick list (null: the fixed bricks)
    const uint2 *plist = nullptr;
};

template <int KCAP, bool MF, bool NET, bool PLAN = false, bool CERT = false>
static int launch_bricks(gsx_ctx *ctx, const BrickLaunch &a)
{
    const unsigned *rstart = PLAN ? a.fstart : a.rstart, *qstart = PLAN ? a.fstart : a.qstart;
    // Work is assigned STATICALLY to waves, so every launched workgroup must be resident at once:
    // the grids are sized from the occupancy the built kernels actually get (a non-resident
    // workgroup would run its share only after a resident one has finished all of its own).
    static int occ_brick = 0, occ_extra = 0;
    if (!occ_brick) {
        GSX_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ_brick, knn_brick_kernel<KCAP, false, MF, NET, PLAN, CERT>, BRICK_THREADS, 0));
        GSX_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ_extra, knn_brick_kernel<KCAP, true, MF, NET, PLAN, CERT>, BRICK_THREADS, 0));
        occ_brick = std::max(1, std::min(occ_brick, 8));
        occ_extra = std::max(1, std::min(occ_extra, 8));
    }
    ctx->wq_grid[0] = ctx->num_cu * occ_brick;
    ctx->wq_grid[1] = ctx->num_cu * occ_extra;
    GSX_CHECK(timing_begin(ctx, GSX_T_SOR_KNN));
    hipLaunchKernelGGL((knn_brick_kernel<KCAP, false, MF, NET, PLAN, CERT>), dim3(ctx->num_cu * occ_brick), dim3(BRICK_THREADS), 0, ctx->stream,
                       a.gp, a.refs, rstart, a.qpts, qstart, a.k, (int)a.q_begin, a.mean_out, a.faillist, a.extra,
                       a.deferred, a.kth_out, a.plist);
    hipLaunchKernelGGL((knn_brick_kernel<KCAP, true, MF, NET, PLAN, CERT>), dim3(ctx->num_cu * occ_extra), dim3(BRICK_THREADS), 0, ctx->stream,
                       a.gp, a.refs, rstart, a.qpts, qstart, a.k, (int)a.q_begin, a.mean_out, a.faillist, a.extra,
                       a.deferred, a.kth_out, a.plist);
    GSX_HIP(hipGetLastError());
    GSX_CHECK(timing_end(ctx, GSX_T_SOR_KNN));
    return 0;
}

// ---------------------------------------------------------------- knn_ring_fast
// First attempt at the queries knn_brick could not certify, before knn_ring's per-lane lists.  A failed query's k-th
// neighbour is just beyond its brick's searched cells, i.e. 1..1.4 cell edges away.  So: ONE pass over the cells of the
// 5x5x5 block around the query's cell that a ball of radius r_t reaches (r_t chosen so that ~5(k+1) points are expected
// inside; second attempt with 1.9 cell edges, the most 2 cells certify), with a float32 filter at r_t (relative error of
// d32 <= 3e-7) that moves the few dozen candidates that matter to LDS.  A 64-bin histogram of
// their d32 isolates the ~k+2 that can be among the k+1 nearest; those are ranked exactly in float64 (rank = number of
// candidates before mine).  If at least k+1 candidates are inside r_t, the k+1 nearest are among them and every point
// within r_t was looked at: exact.  One wave per query, < 80 VGPRs (no per-lane lists): six waves per SIMD overlap
// the dependent loads (list entry -> query -> row bounds -> candidates) of different queries.  The queries it cannot
// finish (fewer than k+1 points within 1.9 cell edges, more than CAND inside r_t, heavy rings) go to a second list for
// knn_ring -- appended per wave in batches, because same-address atomics cost ~11 ns each.
constexpr int RINGF_INFLIGHT = 4;
constexpr double RINGF_TARGET = 5.0;   // candidates expected inside r_t, in units of k+1 (3.5: +0.008 ms, 7: +0.05 ms)
constexpr int RINGF_WAVES = 6;         // 5 waves (no scratch): no change; 4: +0.015 ms (profiles/r03_variants.txt)
constexpr int RINGF_ROWS = 25;   // 5 x 5 rows of 5 cells
constexpr int RINGF_LEFT = 32;   // leftovers a wave collects before it appends them to the second list
// histogram bin of a float32 squared distance d <= thr: two roundings of monotone operations, hence monotone in d
// (bins uniform in d hold ~sqrt(d/thr) * 1.5 cnt / 64 candidates: one or two where the (k+1)-th lies)
__device__ __forceinline__ int ringf_bin(float d32, float inv_thr)
{
    return min(63, (int)(d32 * inv_thr * 64.0f));
}
constexpr int ringf_cand(int kcap) { return kcap <= 17 ? 128 : (kcap <= 33 ? 256 : 512); }
template <int KCAP>
__global__ __launch_bounds__(BRICK_THREADS, KCAP <= 33 ? RINGF_WAVES : 3) void knn_ring_fast_kernel(
    GridParams *__restrict__ gp, const float4 *__restrict__ refs, const unsigned *__restrict__ rstart,
    const float4 *__restrict__ qpts, const unsigned *__restrict__ faillist, unsigned *__restrict__ ring2, int k, int q_begin,
    int64_t n_ref, float *__restrict__ mean_out, double *__restrict__ kth_out)
{
    constexpr int CAND = ringf_cand(KCAP);
    constexpr int NF = RINGF_INFLIGHT;
    __shared__ double s_out[BRICK_THREADS / 64][KCAP];
    __shared__ int s_rs[BRICK_THREADS / 64][RINGF_ROWS];
    __shared__ int s_ro[BRICK_THREADS / 64][RINGF_ROWS + 1];
    __shared__ float4 s_cand[BRICK_THREADS / 64][CAND];   // xyz + float32 squared distance
    __shared__ float4 s_fin[BRICK_THREADS / 64][64];      // the candidates that are ranked exactly
    __shared__ double s_cd[BRICK_THREADS / 64][64];
    __shared__ int s_hist[BRICK_THREADS / 64][64];
    __shared__ unsigned s_left[BRICK_THREADS / 64][RINGF_LEFT];
    const int lane = lane_id();
    const int wv = uniform((int)(threadIdx.x >> 6));
    double *out = s_out[wv];
    int *rs = s_rs[wv], *ro = s_ro[wv];
    float4 *cand = s_cand[wv], *fin = s_fin[wv];
    double *cd = s_cd[wv];
    int *hist = s_hist[wv];
    unsigned *left = s_left[wv];
    const GridParams g = *gp;
    if (g.bad_input) return;   // knn_ring fills the output with NaN
    const int nfail = (int)g.fail_count;
    const int kk = k + 1;
    // r_t: ~5(k+1) points expected inside at the cloud's mean density, at most 1.9 cell edges (2 cells certify 1.998)
    const double per_cell = (double)n_ref / (double)max(g.ncells, 1);
    const double rt_max = 1.9 * g.hprime;
    const double rt_first = __builtin_fmin(::cbrt(RINGF_TARGET * kk / (4.18879 * per_cell)) * g.hprime, rt_max);

    int nleft = 0;   // wave-uniform
    auto flush_left = [&]() __attribute__((always_inline)) {
        unsigned base = 0;
        if (lane == 0) base = atomicAdd(&gp->ring2_count, (unsigned)nleft);
        base = (unsigned)__builtin_amdgcn_readfirstlane((int)base);
        wave_sync();
        if (lane < nleft) ring2[base + lane] = left[lane];
        wave_sync();
        nleft = 0;
    };

    WorkQueue wq;
#ifdef GSX_WAVE_STAMPS
    // phase sums of this wave (shader cycles): 0 row bounds, 1 candidate fetch and filter, 2 histogram and select,
    // 3 exact rank, 4 epilogue, 5 the rest (queue, list entry, hand-over to the second list)
    const unsigned long long ws_t0 = ws_realtime();
    unsigned long long ws_ph[WS_PHASES] = {0, 0, 0, 0, 0, 0};
    unsigned long long ws_last = ws_cycles();
#define WS_MARK(i)                              \
    do {                                        \
        const unsigned long long t_ = ws_cycles(); \
        ws_ph[i] += t_ - ws_last;               \
        ws_last = t_;                           \
    } while (0)
#else
#define WS_MARK(i) \
    do {           \
    } while (0)
#endif
    wq_init(wq, gp->ringf_ctr, nfail, BRICK_THREADS / 64);
    // the next query's list entry and point are fetched while the current one is being worked on: the chain
    // entry -> point -> row bounds -> candidates is what a wave waits for
    int t_next = uniform(wq_next(wq));
    unsigned fq_next = t_next >= 0 ? faillist[t_next] : 0u;
    float4 qp_next = t_next >= 0 ? qpts[fq_next] : make_float4(0.f, 0.f, 0.f, 0.f);
    for (;;) {
        if (t_next < 0) break;
        const float4 qp = qp_next;
        const unsigned fq = fq_next;
        t_next = uniform(wq_next(wq));
        fq_next = t_next >= 0 ? faillist[t_next] : 0u;   // consumed after this query's row bounds have arrived
        bool fetched_next = false;
        const double qxd = (double)qp.x, qyd = (double)qp.y, qzd = (double)qp.z;
        const int cx = cell_coord(qp.x, g.ox, g.inv_h, g.nx);
        const int cy = cell_coord(qp.y, g.oy, g.inv_h, g.ny);
        const int cz = cell_coord(qp.z, g.oz, g.inv_h, g.nz);
        const int x0 = max(cx - 2, 0), x1 = min(cx + 2, g.nx - 1);
        const int y0 = max(cy - 2, 0), y1 = min(cy + 2, g.ny - 1);
        const int z0 = max(cz - 2, 0), z1 = min(cz + 2, g.nz - 1);
        const int nyr = y1 - y0 + 1;
        const int nrows = nyr * (z1 - z0 + 1);
        const double ux = (qxd - (double)g.ox) * (double)g.inv_h, uy = (qyd - (double)g.oy) * (double)g.inv_h,
                     uz = (qzd - (double)g.oz) * (double)g.inv_h;
        bool solved = false;
        double rt = rt_first;
#pragma unroll 1
        for (int attempt = 0; attempt < 2 && !solved; ++attempt, rt = rt_max) {
            if (attempt == 1 && !(rt_first < rt_max)) break;
            WS_MARK(5);
            const float thr = (float)(rt * rt) * (1.0f + 1e-6f);
            const float inv_thr = 1.0f / thr;
            const double rtc = rt * (double)g.inv_h;   // r_t in cell units (<= 1.9)
            // all row bounds in parallel (one lane per row), wave scan -> flat offsets.  Each row is trimmed to the cells
            // the ball of radius r_t can reach (the kernel is bound by the candidate fetch: 37 cells instead of 125): in
            // cell units a point of cell c lies in [c - 2.5e-4, c + 1 + 2.5e-4] (the f32 cell index is off by
            // < 2.5e-4 cells, section 4.2), so with a slack of 1e-3 per side no point within r_t is missed.
            int st = 0, len = 0;
            if (lane < nrows) {
                const int yy = y0 + lane % nyr, zz = z0 + lane / nyr;
                const double dy = uy < yy - 1e-3 ? yy - 1e-3 - uy : (uy > yy + 1.001 ? uy - (yy + 1.001) : 0.0);
                const double dz = uz < zz - 1e-3 ? zz - 1e-3 - uz : (uz > zz + 1.001 ? uz - (zz + 1.001) : 0.0);
                const double rem = rtc * rtc - dy * dy - dz * dz;
                if (rem >= 0.0) {
                    const double dxc = __builtin_sqrt(rem) + 1e-3;
                    const int xa = max(x0, (int)__builtin_floor(ux - dxc)), xb = min(x1, (int)__builtin_floor(ux + dxc));
                    if (xa <= xb) {
                        const int row = row_base(g, yy, zz);
                        st = (int)rstart[row + xa];
                        len = (int)rstart[row + xb + 1] - st;
                    }
                }
            }
            int inc = len;
#pragma unroll
            for (int off = 1; off < 32; off <<= 1) {
                int o = __shfl_up(inc, off);
                if (lane >= off) inc += o;
            }
            if (lane < nrows) {
                rs[lane] = st;
                ro[lane] = inc - len;
            }
            const int total = __shfl(inc, nrows - 1);
            if (lane == 0) ro[nrows] = total;
            hist[lane] = 0;
            wave_sync();
            WS_MARK(0);
            if (!fetched_next) {
                qp_next = t_next >= 0 ? qpts[fq_next] : qp;   // in flight together with this query's candidates
                fetched_next = true;
            }
            if (g.heavy_limit > 0 && total > g.heavy_limit) break;   // wave-uniform: knn_ring routes it to knn_heavy
            int cnt = 0, row = 0;
            for (int f0 = 0; f0 < total; f0 += 64 * NF) {   // wave-uniform trip count, NF loads in flight per lane
                float4 p[NF];
                bool in[NF];
#pragma unroll
                for (int u = 0; u < NF; ++u) {
                    const int f = f0 + 64 * u + lane;
                    in[u] = f < total;
                    if (in[u]) {
                        while (f >= ro[row + 1]) ++row;
                        p[u] = refs[rs[row] + (f - ro[row])];
                    }
                }
#pragma unroll
                for (int u = 0; u < NF; ++u) {
                    bool acc = false;
                    float d32 = 0.0f;
                    if (in[u]) {
                        const float dx = qp.x - p[u].x, dy = qp.y - p[u].y, dz = qp.z - p[u].z;
                        d32 = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
                        acc = d32 <= thr;
                    }
                    const unsigned long long bal = __ballot(acc);
                    if (acc) {
                        const int pos = cnt + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
                        if (pos < CAND) {
                            p[u].w = d32;
                            cand[pos] = p[u];
                            atomicAdd(&hist[ringf_bin(d32, inv_thr)], 1);
                        }
                    }
                    cnt += (int)__builtin_popcountll(bal);
                }
            }
            wave_sync();
            WS_MARK(1);
            if (cnt > CAND) break;      // too dense around this query: knn_ring
            if (cnt < kk) continue;     // too sparse: once more with the widest certifiable radius
            // ---- the k+1 nearest are among the candidates of the first histogram bins that hold k+1 of them (bins are
            // a monotone function of d32); thr2 = the largest d32 in those bins, and a candidate with
            // d32 <= thr2 (1 + 1e-6) cannot be excluded (float32 error 3e-7 on either side)
            int incl = hist[lane];
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                int o = __shfl_up(incl, off);
                if (lane >= off) incl += o;
            }
            const int bstar = (int)__builtin_ctzll(__ballot(incl >= kk));   // exists: the bins hold cnt >= kk candidates
            float dmy[CAND / 64];
            float m32 = 0.0f;
#pragma unroll
            for (int u = 0; u < CAND / 64; ++u) {
                const int j = lane + 64 * u;
                dmy[u] = j < cnt ? cand[j].w : __builtin_inff();
                if (j < cnt && ringf_bin(dmy[u], inv_thr) <= bstar) m32 = fmaxf(m32, dmy[u]);
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) m32 = fmaxf(m32, __shfl_xor(m32, off));
            const float thr2 = m32 * (1.0f + 1e-6f);
            int cnt2 = 0;
#pragma unroll
            for (int u = 0; u < CAND / 64; ++u) {
                const bool sel = dmy[u] <= thr2;   // (+inf for the lanes beyond cnt)
                const unsigned long long bal = __ballot(sel);
                if (sel) {
                    const int pos = cnt2 + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
                    if (pos < 64) fin[pos] = cand[lane + 64 * u];
                }
                cnt2 += (int)__builtin_popcountll(bal);
            }
            wave_sync();
            WS_MARK(2);
            if (cnt2 > 64) break;   // a crowd of near-ties: knn_ring
            double dme = __builtin_inf();
            if (lane < cnt2) {
                const float4 pp = fin[lane];
                dme = dist2_f64(qxd, qyd, qzd, pp.x, pp.y, pp.z);
                cd[lane] = dme;
            }
            wave_sync();
            int rank = 0;
#pragma unroll 4
            for (int j = 0; j < cnt2; ++j) {   // exact: rank = candidates before mine (ties by position)
                const double dj = cd[j];
                rank += (dj < dme || (dj == dme && j < lane)) ? 1 : 0;
            }
            if (lane < cnt2 && rank < kk) out[rank] = dme;
            wave_sync();
            WS_MARK(3);
            const double kth = out[kk - 1];
            if (!(kth <= rt * rt)) continue;   // (the float32 filter admits a hair more than r_t: then r_t certifies nothing)
            for (int i = lane; i < kk; i += 64) out[i] = __dsqrt_rn(out[i]);
            wave_sync();
            if (lane == 0) {   // out[0] = the query itself
                double sum = pairwise_sum_le128([&](int i) { return out[1 + i]; }, k);
                mean_out[(int)__float_as_uint(qp.w) - q_begin] = mean_finish(sum, k);
                kth_emit(gp, kth_out, (int)__float_as_uint(qp.w) - q_begin, kth, qp.x, qp.y, qp.z);
            }
            wave_sync();
            solved = true;
            WS_MARK(4);
        }
        if (!fetched_next) qp_next = t_next >= 0 ? qpts[fq_next] : qp;
        if (!solved) {
            if (lane == 0) left[nleft] = fq;
            ++nleft;
            if (nleft == RINGF_LEFT) flush_left();
        }
    }
    if (nleft) flush_left();
#ifdef GSX_WAVE_STAMPS
    WS_MARK(5);
    ws_write(gp, 1, wq, ws_t0, ws_ph);
#endif
#undef WS_MARK
}

template <int KCAP>
static int launch_ring(gsx_ctx *ctx, const BrickLaunch &a)
{
    static int occ_ring = 0, occ_fast = 0;
    if (!occ_ring) {
        GSX_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ_ring, knn_ring_kernel<KCAP>, BRICK_THREADS, 0));
        occ_ring = std::max(1, std::min(occ_ring, 8));
        GSX_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ_fast, knn_ring_fast_kernel<KCAP>, BRICK_THREADS, 0));
        occ_fast = std::max(1, std::min(occ_fast, 8));
    }
    ctx->wq_grid[2] = ctx->num_cu * occ_ring;
    ctx->wq_grid[3] = ctx->num_cu * occ_fast;
    GSX_CHECK(timing_begin(ctx, GSX_T_SOR_FALLBACK));
    const bool fast = ctx->ring_fast;
    if (fast)
        hipLaunchKernelGGL((knn_ring_fast_kernel<KCAP>), dim3(ctx->num_cu * occ_fast), dim3(BRICK_THREADS), 0, ctx->stream, a.gp, a.refs,
                           a.rstart, a.qpts, a.faillist, a.ring2, a.k, (int)a.q_begin, a.n_ref, a.mean_out, a.kth_out);
    hipLaunchKernelGGL((knn_ring_kernel<KCAP>), dim3(ctx->num_cu * occ_ring), dim3(BRICK_THREADS), 0, ctx->stream, a.gp, a.refs,
                       a.rstart, a.qpts, fast ? a.ring2 : a.faillist, a.k, (int)a.q_begin, a.mean_out, a.kth_out, a.heavylist, (int)a.out_count,
                       fast ? 1 : 0);
    GSX_HIP(hipGetLastError());
    GSX_CHECK(timing_end(ctx, GSX_T_SOR_FALLBACK));
    return 0;
}

template <int KCAP>
static int launch_heavy(gsx_ctx *ctx, KnnWs &w, const BrickLaunch &a, int64_t n_ref, unsigned heavy_count)
{
    const int nchunks = div_up(n_ref, HEAVY_CHUNK);
    const int batch = (int)std::max<int64_t>(1, std::min<int64_t>(heavy_count, (256LL << 20) / ((int64_t)nchunks * KCAP * 8)));
    GSX_CHECK(w.heavypart.reserve(sizeof(double) * (size_t)batch * nchunks * KCAP));
    GSX_CHECK(timing_begin(ctx, GSX_T_SOR_FALLBACK));
    for (unsigned first = 0; first < heavy_count; first += (unsigned)batch) {
        const int count = (int)std::min<unsigned>((unsigned)batch, heavy_count - first);
        const int64_t items = (int64_t)count * nchunks;
        const int blocks = (int)std::min<int64_t>(div_up(items, BRICK_THREADS / 64), (int64_t)ctx->num_cu * 8);
        hipLaunchKernelGGL((knn_heavy_scan_kernel<KCAP>), dim3(blocks), dim3(BRICK_THREADS), 0, ctx->stream, a.refs, (int)n_ref,
                           a.qpts, a.heavylist, (int)first, count, a.k, w.heavypart.as<double>());
        hipLaunchKernelGGL((knn_heavy_merge_kernel<KCAP>), dim3(div_up(count, BRICK_THREADS / 64)), dim3(BRICK_THREADS), 0,
                           ctx->stream, a.gp, (int)n_ref, a.qpts, a.heavylist, (int)first, count, a.k, (int)a.q_begin,
                           w.heavypart.as<double>(), a.mean_out, a.kth_out);
    }
    GSX_HIP(hipGetLastError());
    GSX_CHECK(timing_end(ctx, GSX_T_SOR_FALLBACK));
    return 0;
}

static int dispatch_heavy(gsx_ctx *ctx, KnnWs &w, const BrickLaunch &a, int64_t n_ref, unsigned heavy_count)
{
    const int kk = a.k + 1;
    if (kk <= 9) return launch_heavy<9>(ctx, w, a, n_ref, heavy_count);
    if (kk <= 17) return launch_heavy<17>(ctx, w, a, n_ref, heavy_count);
    if (kk <= 26) return launch_heavy<26>(ctx, w, a, n_ref, heavy_count);
    if (kk <= 33) return launch_heavy<33>(ctx, w, a, n_ref, heavy_count);
    if (kk <= 51) return launch_heavy<51>(ctx, w, a, n_ref, heavy_count);
    return launch_heavy<65>(ctx, w, a, n_ref, heavy_count);
}

// list-capacity buckets.  Sorting-network selection (default): the list holds k neighbours, capacities 8, 16, 24,
// 32, 40, 48, 56, 64 (template argument = capacity + 1; the multiples of 8 that are no power of two: round 4, TopNet's
// padded merge).  Bubble-insert selection (phase2_net = 0, kept for A/B): k + 1
// entries incl. the query; 26 and 51 are the CLI's default k=25 and its maximum k=50 (--sor_intensity 10).
static int dispatch_bricks(gsx_ctx *ctx, const BrickLaunch &a, bool mf, bool net)
{
    const int kk = a.k + 1;
    // the certified epilogue: the 16-entry network list at k = 16, mean distances only
    const bool cert = ctx->epilogue_cert != 0 && a.k == 16 && !a.kth_out;
    if (a.plist) {   // planned bricks: knn_grid_level allows them for the MFMA + network kernels of 2x2x2-cell bricks only
        if (kk <= 9) return launch_bricks<9, true, true, true>(ctx, a);
        if (GSX_CAP4 && kk <= 13) return launch_bricks<13, true, true, true>(ctx, a);
        return cert ? launch_bricks<17, true, true, true, true>(ctx, a) : launch_bricks<17, true, true, true>(ctx, a);
    }
    if (net) {
#define GSX_BRICKS(K) (mf ? launch_bricks<K, true, true>(ctx, a) : launch_bricks<K, false, true>(ctx, a))
        // (round 5: the multiples of 4 in between as well -- --sor_intensity 1 ... 10 asks for k = 10, 14, 18, 23, 27, 32, 36, 41, 45, 50
        //  and the default is 25: -5 % of the step at k = 25 with 28 entries instead of 32, profiles/r05_variants.txt)
        if (kk <= 9) return GSX_BRICKS(9);
        if (GSX_CAP4 && kk <= 13) return GSX_BRICKS(13);
        if (cert) return mf ? launch_bricks<17, true, true, false, true>(ctx, a) : launch_bricks<17, false, true, false, true>(ctx, a);
        if (kk <= 17) return GSX_BRICKS(17);
        if (GSX_CAP4 && kk <= 21) return GSX_BRICKS(21);
        if (kk <= 25) return GSX_BRICKS(25);   // 24 and 48 entries: the reference CLI's k = 18 ... 24 and 33 ... 48
        if (GSX_CAP4 && kk <= 29) return GSX_BRICKS(29);
        if (kk <= 33) return GSX_BRICKS(33);
        if (GSX_CAP4 && kk <= 37) return GSX_BRICKS(37);
        if (kk <= 41) return GSX_BRICKS(41);   // (40 and 56 entries: -10 % at k = 36, -13 % at 40, -8 % at 56 against the next capacity)
        if (GSX_CAP4 && kk <= 45) return GSX_BRICKS(45);
        if (kk <= 49) return GSX_BRICKS(49);
        if (GSX_CAP4 && kk <= 53) return GSX_BRICKS(53);
        if (kk <= 57) return GSX_BRICKS(57);
        return GSX_BRICKS(65);
#undef GSX_BRICKS
    }
#define GSX_BRICKS(K) (mf ? launch_bricks<K, true, false>(ctx, a) : launch_bricks<K, false, false>(ctx, a))
    if (kk <= 9) return GSX_BRICKS(9);
    if (kk <= 17) return GSX_BRICKS(17);
    if (kk <= 26) return GSX_BRICKS(26);
    if (kk <= 33) return GSX_BRICKS(33);
    if (kk <= 51) return GSX_BRICKS(51);
    return GSX_BRICKS(65);
#undef GSX_BRICKS
}

static int dispatch_ring(gsx_ctx *ctx, const BrickLaunch &a)
{
    const int kk = a.k + 1;
    if (kk <= 9) return launch_ring<9>(ctx, a);
    if (kk <= 17) return launch_ring<17>(ctx, a);
    if (kk <= 26) return launch_ring<26>(ctx, a);
    if (kk <= 33) return launch_ring<33>(ctx, a);
    if (kk <= 51) return launch_ring<51>(ctx, a);
    return launch_ring<65>(ctx, a);
}

// The coarse histogram of (x,y,z)[first, first+n): per-tile bucket counts, their per-bucket scans and bk_start.
static int bin_hist(gsx_ctx *ctx, KnnWs &w, const float *x, const float *y, const float *z, int64_t stride, int64_t first,
                    int64_t n, GridParams *gp)
{
    const BinTiles bt = BinTiles::of((int)n);
    if ((size_t)bt.slots() * MAX_BUCKETS * sizeof(unsigned) > w.tileoff.cap) GSX_FAIL("sor: bin tables not reserved for %lld points", (long long)n);
    hipLaunchKernelGGL(bucket_hist_kernel, dim3(std::max(bt.ntiles, 1)), dim3(256), 0, ctx->stream, x, y, z, stride, (int)first, (int)n, gp,
                       w.tilecnt.as<unsigned short>());
    hipLaunchKernelGGL(bucket_offsets_kernel, dim3(MAX_BUCKETS / OFFSETS_BUCKETS), dim3(OFFSETS_THREADS), 0, ctx->stream, (int)n, gp, w.tilecnt.as<unsigned short>(),
                       w.tileoff.as<unsigned>(), w.bk_size, w.bk_start);   // its last workgroup scans the bucket sizes
    GSX_HIP(hipGetLastError());
    return 0;
}

// the tables of bin_hist for up to n points (grow-only)
static int reserve_bin_tables(KnnWs &w, int64_t n)
{
    const size_t slots = (size_t)BinTiles::of((int)n).slots();
    GSX_CHECK(w.tilecnt.reserve(sizeof(unsigned short) * slots * MAX_BUCKETS));
    GSX_CHECK(w.tileoff.reserve(sizeof(unsigned) * slots * MAX_BUCKETS));
    return 0;
}

// Sort (x,y,z)[first, first+n) by cell of the grid in gp: `sorted` and `start` (cell_start) are outputs.
// hist_done: bin_hist has already run on these points.
static int bin_points(gsx_ctx *ctx, KnnWs &w, const float *x, const float *y, const float *z, int64_t stride, int64_t first,
                      int64_t n, GridParams *gp, unsigned *start, float4 *sorted, int64_t cell_cap = 0, unsigned *cursor = nullptr,
                      int64_t ref_only_from = INT32_MAX, bool hist_done = false, unsigned *fine = nullptr)
{
    const bool big_path = cursor != nullptr;  // adaptive mode: oversized buckets are sorted by all workgroups
    unsigned *bk_start = w.bk_start;
    float4 *tmp = w.bucketpts.as<float4>();
    if (!hist_done) GSX_CHECK(bin_hist(ctx, w, x, y, z, stride, first, n, gp));
    hipLaunchKernelGGL(bucket_scatter_kernel, dim3(std::max(BinTiles::of((int)n).ntiles, 1)), dim3(SCATTER_THREADS), 0, ctx->stream, x, y, z, stride,
                       (int)first, (int)n, gp, bk_start, w.tileoff.as<unsigned>(), tmp, (int)std::min<int64_t>(ref_only_from, INT32_MAX));
    if (big_path) GSX_HIP(hipMemsetAsync(start, 0, sizeof(unsigned) * (size_t)(cell_cap + 1), ctx->stream));  // counts of big buckets
    if (fine)
        hipLaunchKernelGGL(bucket_sort_kernel<true>, dim3(MAX_BUCKETS), dim3(SORT_THREADS), 0, ctx->stream, gp, bk_start, tmp, sorted, start,
                           0xffffffffu, fine);
    else
        hipLaunchKernelGGL(bucket_sort_kernel<false>, dim3(MAX_BUCKETS), dim3(SORT_THREADS), 0, ctx->stream, gp, bk_start, tmp, sorted, start,
                           big_path ? BIG_BUCKET : 0xffffffffu, (unsigned *)nullptr);
    if (big_path) {
        const int chunks = div_up(n, BIG_CHUNK);
        hipLaunchKernelGGL((big_bucket_kernel<false>), dim3(chunks), dim3(256), 0, ctx->stream, gp, bk_start, (int)n, tmp, sorted,
                           start, cursor);
        hipLaunchKernelGGL(big_bucket_scan_kernel, dim3(MAX_BUCKETS), dim3(256), 0, ctx->stream, gp, bk_start, start, cursor);
        hipLaunchKernelGGL((big_bucket_kernel<true>), dim3(chunks), dim3(256), 0, ctx->stream, gp, bk_start, (int)n, tmp, sorted,
                           start, cursor);
    }
    GSX_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------- one level of the grid: knn_grid_level and its stages
// The decisions (points per cell, cell budget, histogram verdict, planned bricks, grouping, refinement sizing) live in
// grid_policy.h; the stages below are the launches, copies and synchronisations around them, in stream order.
struct GridLevel {
    // the call
    gsx_ctx *ctx;
    int level;
    KnnWs &w;
    const float *x, *y, *z;
    int64_t stride, n_ref, q_begin, q_count;
    int k;
    float *mean_out;
    double *kth_out;
    gsx_sor_info *info;
    int share, nshares;
    float parent_h;
    int64_t ref_only_from;
    double h_hint;
    const SlabKnn *sk;
    bool anyk;       // k > 64: the list-free exact path (knn_anyk_kernel) instead of knn_brick + ring kernels
    bool slab;       // slab mode (multi-GPU): every point is binned once, the halo [ref_only_from, n_ref) is flagged reference-only
    bool all;        // every reference point is a query
    bool adaptive;   // bricks may still be deferred to a finer level (the histogram stage can switch it off)
    bool trace;      // GSX_TRACE_LEVELS
    int64_t cap;     // cells the grid may have
    double pts_per_cell;
    // what the stages leave for one another
    int bbox_blocks = 0;
    bool mfma_ok = false, plan = false, adaptive_at_bbox = false, tree_ok = false, hist_done = false, have_hgp = false;
    int64_t plan_cap = 0;
    GridParams *gp = nullptr;
    float4 *refs = nullptr;
    const float4 *qpts = nullptr;
    unsigned *rstart = nullptr;
    const unsigned *qstart = nullptr;
    unsigned *fail = nullptr, *fail_rest = nullptr;   // the fail list | knn_ring_fast's leftovers (both regions of w.faillist)
    GridParams hgp;   // the grid parameters and counters as the host read them after knn_brick (have_hgp)
};

// (a refinement round calls the next level)
static int knn_grid_level(gsx_ctx *ctx, int level, const float *x, const float *y, const float *z, int64_t stride,
                          int64_t n_ref, int64_t q_begin, int64_t q_count, int k, float *mean_out, double *kth_out,
                          gsx_sor_info *info, int share, int nshares, bool adaptive, float parent_h,
                          int64_t ref_only_from = INT32_MAX, double h_hint = 0.0, const SlabKnn *sk = nullptr);

static int level_reserve(GridLevel &L)
{
    gsx_ctx *ctx = L.ctx;
    KnnWs &w = L.w;
    const int64_t n_ref = L.n_ref, q_count = L.q_count, cap = L.cap;
    L.bbox_blocks = std::min(grid_blocks(ctx, n_ref, 8), ctx->num_cu * 4);
    GSX_CHECK(w.packed.reserve(sizeof(float4) * (size_t)n_ref));
    GSX_CHECK(w.bucketpts.reserve(sizeof(float4) * (size_t)n_ref));
    GSX_CHECK(w.cellstart.reserve(sizeof(unsigned) * (size_t)(cap + 1)));
    if (!w.bkcnt.p) {  // bucket sizes | bucket starts (one past the last bucket), zeroed once
        const auto layout = [&](Carve &a) {
            w.bk_size = a.take<unsigned>(MAX_BUCKETS);
            w.bk_start = a.take<unsigned>(MAX_BUCKETS + 1, 4);
            a.take<unsigned>(7, 4);   // words the block always had behind the starts; no kernel was found to touch them
        };
        const size_t bytes = carve_measure(layout);   // (before the carve: the layout's last pass must be the placing one)
        GSX_CHECK(carve(w.bkcnt, layout));
        GSX_HIP(hipMemsetAsync(w.bkcnt.p, 0, bytes, ctx->stream));
    }
    GSX_CHECK(reserve_bin_tables(w, n_ref));   // (the queries of a partial call are a subset of the refs: fewer tiles)
    if (!w.gridparams.p) {   // the arrival tickets inside must start at zero (they reset themselves afterwards)
        GSX_CHECK(w.gridparams.reserve(sizeof(GridParams)));
        GSX_HIP(hipMemsetAsync(w.gridparams.p, 0, sizeof(GridParams), ctx->stream));
    }
    GSX_CHECK(w.bboxpart.reserve(sizeof(float) * 7 * (size_t)L.bbox_blocks));
    GSX_CHECK(carve(w.faillist, [&](Carve &a) {
        L.fail = a.take<unsigned>((size_t)std::max<int64_t>(q_count, 1));
        L.fail_rest = a.take<unsigned>((size_t)std::max<int64_t>(q_count, 1), 4);   // knn_ring_fast's leftovers
    }));
    GSX_CHECK(w.extraitems.reserve(sizeof(uint2) * (size_t)(std::max(q_count, L.slab ? n_ref : q_count) / 64 + 64)));
    if (L.adaptive) {
        GSX_CHECK(w.deferred.reserve(sizeof(unsigned) * (size_t)(cap + 64)));  // nbricks <= ncells <= cap
        GSX_CHECK(w.heavylist.reserve(sizeof(unsigned) * (size_t)std::max<int64_t>(q_count, 1)));
    }
    if (!L.all) {
        GSX_CHECK(w.qsorted.reserve(sizeof(float4) * (size_t)q_count));
        GSX_CHECK(w.qcellstart.reserve(sizeof(unsigned) * (size_t)(cap + 1)));
    }
    L.gp = w.gridparams.as<GridParams>();
    L.refs = w.packed.as<float4>();
    L.rstart = w.cellstart.as<unsigned>();
    // (the MFMA kernels' phase 2 addresses the sorted points with 32-bit byte offsets: 16 * n_ref < 2^32; larger clouds take the
    //  scalar filter, which is exact as well)
    L.mfma_ok = ctx->filter_mfma != 0 && n_ref < (int64_t(1) << 28);
    L.plan = grid_plan_eligible({ctx->brick_plan != 0, L.level, L.all, L.slab, L.sk != nullptr, L.nshares, L.k, L.mfma_ok,
                                 ctx->phase2_net != 0, L.pts_per_cell, L.h_hint, L.kth_out != nullptr});
    L.plan_cap = n_ref / 16 + 4096;
    if (L.plan) {
        GSX_CHECK(w.finestart.reserve(sizeof(unsigned) * (size_t)(4 * cap + 4)));
        GSX_CHECK(w.bricklist.reserve(sizeof(uint2) * (size_t)L.plan_cap));
        GSX_CHECK(w.bundleoff.reserve(sizeof(unsigned) * 2 * (size_t)(MAX_DIM / 2) * (MAX_DIM / 2)));
    }
    return 0;
}

// the bounding box and, in its last workgroup, the grid parameters; opens the level's first GSX_T_SOR_BIN interval
static int level_grid_params(GridLevel &L)
{
    gsx_ctx *ctx = L.ctx;
    KnnWs &w = L.w;
    const SlabKnn *sk = L.sk;
    GSX_CHECK(timing_begin(ctx, GSX_T_SOR_BIN));
    // (adaptive mode may still switch the deferral off below, once the histogram is known: defer_words is then cleared on the device)
    GridParamArgs gpa{(int)L.n_ref, L.pts_per_cell, (int)L.cap, ctx->debug_skip, L.share, L.nshares, L.adaptive ? ctx->defer_words : 0,
                      L.parent_h, L.gp, ctx->devflags.as<unsigned>(), L.h_hint, sk ? sk->cert_axis : -1, sk ? sk->cert_lo : 0.0f,
                      sk ? sk->cert_hi : 0.0f, sk ? sk->cert_count : nullptr, L.plan ? 1 : 0, (int)L.plan_cap};
#ifdef GSX_WAVE_STAMPS
    if (L.level == 0) {   // (a finer level would overwrite the records of the call's main launches)
        const int ws_cap = ctx->num_cu * 8 * (BRICK_THREADS / 64);   // the launches are capped at 8 workgroups per CU
        const size_t ws_bytes = sizeof(unsigned long long) * 2 * (size_t)ws_cap * WS_WORDS;
        GSX_CHECK(w.wavestamps.reserve(ws_bytes));
        GSX_HIP(hipMemsetAsync(w.wavestamps.p, 0, ws_bytes, ctx->stream));
        gpa.stamps = w.wavestamps.as<unsigned long long>();
        gpa.stamps_cap = ws_cap;
        ctx->ws_cap = ws_cap;
    }
#endif
    L.adaptive_at_bbox = L.adaptive;
    if (sk && sk->box.b7)
        hipLaunchKernelGGL(grid_params_known_box_kernel, dim3(1), dim3(64), 0, ctx->stream, sk->box, w.bboxpart.as<float>(), gpa);
    else
        hipLaunchKernelGGL(bbox_partial_kernel, dim3(L.bbox_blocks), dim3(256), 0, ctx->stream, L.x, L.y, L.z, L.stride, (int)L.n_ref,
                           w.bboxpart.as<float>(), gpa);   // its last workgroup computes the grid parameters
    GSX_HIP(hipGetLastError());
    if (L.adaptive) GSX_CHECK(w.qcellstart.reserve(sizeof(unsigned) * (size_t)(L.cap + 1)));  // free in this mode: the cursors
    return 0;
}

// Adaptive mode, first decision (grid_policy.h: grid_hist_verdict): an uneven cloud goes to the Morton tree, *done = it took
// the call; an even one will defer nothing.  The one host synchronisation of an adaptive call on an even cloud is here.
// (slab mode -- one rank's slab + halo of the multi-GPU exchange -- never refines, but an uneven slab still goes to the tree:
//  the grid would search its dense cells quadratically)
static int level_histogram(GridLevel &L, bool *done)
{
    gsx_ctx *ctx = L.ctx;
    KnnWs &w = L.w;
    L.tree_ok = (L.adaptive || (L.slab && ctx->adaptive)) && ctx->tree && L.level == 0 && L.k + 1 <= 65 && L.n_ref > L.k;
    if (!L.tree_ok) return 0;
    GSX_CHECK(bin_hist(ctx, w, L.x, L.y, L.z, L.stride, 0, L.n_ref, L.gp));
    static thread_local std::vector<unsigned> starts(MAX_BUCKETS + 1);
    GSX_HIP(hipMemcpyAsync(starts.data(), w.bk_start, sizeof(unsigned) * (MAX_BUCKETS + 1), hipMemcpyDeviceToHost, ctx->stream));
    GSX_HIP(hipStreamSynchronize(ctx->stream));
    const HistVerdict v = grid_hist_verdict(starts.data(), L.n_ref, L.nshares);
    L.hist_done = true;
    if (v.to_tree) {
        GSX_CHECK(timing_end(ctx, GSX_T_SOR_BIN));
        if (L.trace)
            fprintf(stderr, "[gsx] level 0: fullest bucket %u of %lld points in %u buckets -> tree path\n", v.fullest, (long long)L.n_ref, v.nonzero);
        const int rc = launch_knn_tree(ctx, L.x, L.y, L.z, L.stride, L.n_ref, L.q_begin, L.q_count, L.k, L.mean_out, L.kth_out, L.info,
                                       L.slab ? L.ref_only_from : INT32_MAX, L.share, L.nshares, true);
        if (rc != GSX_TREE_UNSUITABLE) {
            *done = true;
            return rc;
        }
        // (tens of thousands of points inside one cell of the tree's finest resolution: the refinement below re-scales)
        L.tree_ok = false;
        ctx->last_knn_algo = GSX_KNN_GRID;
        GSX_CHECK(timing_begin(ctx, GSX_T_SOR_BIN));
    }
    if (v.no_deferral) L.adaptive = false;
    return 0;
}

// the two-level sort of the references (and of the queries of a partial call), the brick plan; closes GSX_T_SOR_BIN
static int level_bin(GridLevel &L)
{
    gsx_ctx *ctx = L.ctx;
    KnnWs &w = L.w;
    GridParams *gp = L.gp;
    if (L.adaptive_at_bbox && !L.adaptive) {   // the grid parameters were written with deferral on
        GSX_HIP(hipMemsetAsync(&gp->defer_words, 0, sizeof(int), ctx->stream));
        GSX_HIP(hipMemsetAsync(&gp->heavy_limit, 0, sizeof(int), ctx->stream));
    }
    if (L.plan && L.adaptive) {   // bricks may be deferred to a finer level: the fixed bricks, exactly as before
        L.plan = false;
        GSX_HIP(hipMemsetAsync(&gp->plan, 0, sizeof(int), ctx->stream));
    }
    unsigned *fstart = L.plan ? w.finestart.as<unsigned>() : nullptr;
    GSX_CHECK(bin_points(ctx, w, L.x, L.y, L.z, L.stride, 0, L.n_ref, gp, L.rstart, L.refs, L.cap,
                         L.adaptive ? w.qcellstart.as<unsigned>() : nullptr, L.slab ? L.ref_only_from : INT32_MAX, L.hist_done, fstart));
    if (L.plan) {   // one wave per bundle of 2x2 query rows (grid-stride): count + scan, then write
        unsigned *bcnt = w.bundleoff.as<unsigned>(), *boff = bcnt + (size_t)(MAX_DIM / 2) * (MAX_DIM / 2);
        const int pblocks = ctx->num_cu * 4;
        hipLaunchKernelGGL(brick_plan_kernel<false>, dim3(pblocks), dim3(64 * PLAN_WAVES), 0, ctx->stream, gp, fstart, bcnt, boff,
                           w.bricklist.as<uint2>());
        hipLaunchKernelGGL(brick_plan_kernel<true>, dim3(pblocks), dim3(64 * PLAN_WAVES), 0, ctx->stream, gp, fstart, bcnt, boff,
                           w.bricklist.as<uint2>());
        GSX_HIP(hipGetLastError());
    }
    L.qpts = L.refs;
    L.qstart = L.rstart;
    if (!L.all) {
        GSX_CHECK(bin_points(ctx, w, L.x, L.y, L.z, L.stride, L.q_begin, L.q_count, gp, w.qcellstart.as<unsigned>(),
                             w.qsorted.as<float4>()));
        L.qpts = w.qsorted.as<float4>();
        L.qstart = w.qcellstart.as<unsigned>();
    }
    GSX_CHECK(timing_end(ctx, GSX_T_SOR_BIN));
    return 0;
}

static int level_anyk(GridLevel &L)
{
    gsx_ctx *ctx = L.ctx;
    GSX_CHECK(timing_begin(ctx, GSX_T_SOR_KNN));
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>((L.q_count + 3) / 4, (int64_t)ctx->num_cu * 2));
    hipLaunchKernelGGL(knn_anyk_kernel, dim3(blocks), dim3(BRICK_THREADS), 0, ctx->stream, L.gp, L.refs, L.rstart, L.qpts, (int)L.q_count,
                       L.k, (int)L.q_begin, L.mean_out, L.kth_out);
    GSX_HIP(hipGetLastError());
    GSX_CHECK(timing_end(ctx, GSX_T_SOR_KNN));
    return 0;
}

// One refinement round: the sub-cloud around one group of deferred bricks gets a grid of its own (level + 1) and its answers
// are merged back.  Two host synchronisations: the queries' box (the clip needs it), then the gathered count with the probe.
static int refine_group(GridLevel &L, const BrickLaunch &a, const unsigned *g_list, unsigned g_count)
{
    gsx_ctx *ctx = L.ctx;
    KnnWs &w = L.w;
    GridParams *gp = L.gp;
    const int64_t n_ref = L.n_ref;
    uint8_t *flag = w.cellflag.as<uint8_t>();
    float *sub = w.subxyz.as<float>();
    unsigned *sub_orig = w.submap.as<unsigned>(), *sub_sorted = sub_orig + n_ref;
    GSX_CHECK(timing_begin(ctx, GSX_T_SOR_BIN));
    GSX_HIP(hipMemsetAsync(flag, 0, (size_t)L.hgp.ncells, ctx->stream));
    hipLaunchKernelGGL(reset_refine_kernel, dim3(1), dim3(1), 0, ctx->stream, gp);
    hipLaunchKernelGGL(mark_cells_kernel, dim3(g_count), dim3(64), 0, ctx->stream, gp, g_list, g_count, flag, 0);
    hipLaunchKernelGGL(mark_cells_kernel, dim3(g_count), dim3(64), 0, ctx->stream, gp, g_list, g_count, flag, 1);
    hipLaunchKernelGGL(query_bbox_kernel, dim3(std::min(div_up(n_ref, 256), ctx->num_cu * 4)), dim3(256), 0, ctx->stream, gp,
                       L.refs, (int)n_ref, flag);
    GSX_HIP(hipGetLastError());
    GridParams hq;
    GSX_HIP(hipMemcpyAsync(&hq, gp, sizeof(GridParams), hipMemcpyDeviceToHost, ctx->stream));
    GSX_HIP(hipStreamSynchronize(ctx->stream));
    const RefineClip rc = refine_clip(hq.qb_lo, hq.qb_hi, hq.sub_queries, L.pts_per_cell, L.hgp.h, ctx->adaptive);
    const ClipBox clip{{rc.lo[0], rc.lo[1], rc.lo[2]}, {rc.hi[0], rc.hi[1], rc.hi[2]}, rc.r_cert};
    if (L.trace)
        fprintf(stderr, "[gsx] level %d: group of %u bricks, %u deferred queries in [%g,%g]x[%g,%g]x[%g,%g], clip margin %g\n", L.level, g_count,
                hq.sub_queries, hq.qb_lo[0], hq.qb_hi[0], hq.qb_lo[1], hq.qb_hi[1], hq.qb_lo[2], hq.qb_hi[2], (double)clip.r_cert);
    hipLaunchKernelGGL(gather_sub_kernel, dim3(div_up(n_ref, GATHER_CHUNK)), dim3(256), 0, ctx->stream, gp, L.refs, (int)n_ref,
                       flag, clip, sub, sub_orig, sub_sorted);
    GSX_HIP(hipGetLastError());
    // density probe of the gathered points (see probe_count_kernel): rides on the synchronisation that reads n_sub
    double bin_vol = 0.0;
    unsigned hist_h[32] = {0};
    if (rc.probe_g) {
        const int G = rc.probe_g;
        GSX_CHECK(w.probe.reserve(sizeof(unsigned) * ((size_t)G * G * G + 32)));
        unsigned *counts = w.probe.as<unsigned>(), *probe_hist = counts + (size_t)G * G * G;
        GSX_HIP(hipMemsetAsync(counts, 0, sizeof(unsigned) * ((size_t)G * G * G + 32), ctx->stream));
        ProbeBox pb{};
        pb.g = G;
        bin_vol = 1.0;
        for (int ax = 0; ax < 3; ++ax) {
            const double e = (double)hq.qb_hi[ax] - (double)hq.qb_lo[ax];
            pb.lo[ax] = hq.qb_lo[ax];
            pb.inv[ax] = (float)((double)G / e);
            bin_vol *= e / (double)G;
        }
        const int pblocks = std::min(div_up(n_ref, 1024), ctx->num_cu * 4);
        hipLaunchKernelGGL(probe_count_kernel, dim3(pblocks), dim3(256), 0, ctx->stream, sub, (int)n_ref, &gp->sub_count, pb, counts);
        hipLaunchKernelGGL(probe_hist_kernel, dim3(pblocks), dim3(256), 0, ctx->stream, sub, (int)n_ref, &gp->sub_count, pb, counts,
                           probe_hist);
        GSX_HIP(hipGetLastError());
        GSX_HIP(hipMemcpyAsync(hist_h, probe_hist, sizeof(hist_h), hipMemcpyDeviceToHost, ctx->stream));
    }
    unsigned n_sub = 0;
    GSX_HIP(hipMemcpyAsync(&n_sub, &gp->sub_count, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    GSX_HIP(hipStreamSynchronize(ctx->stream));
    GSX_CHECK(timing_end(ctx, GSX_T_SOR_BIN));
    const double h_hint_sub =
        rc.probe_g ? refine_probe_edge(hist_h, bin_vol, hq.qb_lo, hq.qb_hi, clip.r_cert, n_sub, rc.h_est, L.pts_per_cell) : 0.0;
    if (L.trace) fprintf(stderr, "[gsx] level %d: sub-cloud %u points, probed cell edge %g\n", L.level, n_sub, h_hint_sub);
    if (n_sub == 0) GSX_FAIL("sor: refinement gathered no points for %u deferred bricks", g_count);
    GSX_CHECK(w.submean.reserve(sizeof(float) * (size_t)n_sub));
    GSX_CHECK(w.subkth.reserve(sizeof(double) * (size_t)n_sub));
    GSX_CHECK(knn_grid_level(ctx, L.level + 1, sub, sub + n_ref, sub + 2 * n_ref, 1, (int64_t)n_sub, 0, (int64_t)n_sub, L.k,
                             w.submean.as<float>(), w.subkth.as<double>(), nullptr, 0, 1, true, L.hgp.h, INT32_MAX, h_hint_sub, nullptr));
    hipLaunchKernelGGL(merge_sub_kernel, dim3(div_up((int64_t)n_sub, 256)), dim3(256), 0, ctx->stream, gp, sub, (int)n_ref,
                       sub_orig, sub_sorted, w.submean.as<float>(), w.subkth.as<double>(), (int)L.q_begin, clip.r_cert,
                       L.mean_out, L.kth_out, a.faillist);
    GSX_HIP(hipGetLastError());
    w.refined_total += n_sub;
    return 0;
}

// After knn_brick in adaptive mode: read the counters; deferred bricks go to the tree (*done = it took the call) or, group by
// group, to a finer grid.
static int level_refine(GridLevel &L, const BrickLaunch &a, bool *done)
{
    gsx_ctx *ctx = L.ctx;
    KnnWs &w = L.w;
    GridParams &hgp = L.hgp;
    // the only host decision of the pipeline: did any brick ask for a finer grid?
    GSX_HIP(hipMemcpyAsync(&hgp, L.gp, sizeof(GridParams), hipMemcpyDeviceToHost, ctx->stream));
    GSX_HIP(hipStreamSynchronize(ctx->stream));
    L.have_hgp = true;
    if (L.trace)
        fprintf(stderr, "[gsx] level %d: n=%lld h=%.5g dims=%dx%dx%d bricks=%d defer_words=%d deferred=%u extra=%u fail=%u\n", L.level,
                (long long)L.n_ref, hgp.h, hgp.nx, hgp.ny, hgp.nz, hgp.nbricks, hgp.defer_words, hgp.deferred_count,
                hgp.extra_count, hgp.fail_count);
    if (!(hgp.deferred_count > 0 && !hgp.bad_input)) return 0;
    if (L.tree_ok && L.nshares == 1) {   // (a share sees only ITS bricks: the ranks of a replicated exchange could decide differently)
        // second decision: the histogram looked even, yet some bricks hold far more than their cells were sized for
        // (density varying inside the buckets).  The tree path takes the whole cloud over; this level's work is lost.
        if (L.trace) fprintf(stderr, "[gsx] level 0: %u deferred bricks -> tree path\n", hgp.deferred_count);
        const int rc = launch_knn_tree(ctx, L.x, L.y, L.z, L.stride, L.n_ref, L.q_begin, L.q_count, L.k, L.mean_out, L.kth_out, L.info,
                                       INT32_MAX, 0, 1, true);
        if (rc != GSX_TREE_UNSUITABLE) {
            *done = true;
            return rc;
        }
        ctx->last_knn_algo = GSX_KNN_GRID;
    }
    const unsigned nd = hgp.deferred_count;
    GSX_CHECK(w.cellflag.reserve((size_t)hgp.ncells + 64));
    GSX_CHECK(w.subxyz.reserve(sizeof(float) * 3 * (size_t)L.n_ref));
    GSX_CHECK(w.submap.reserve(sizeof(unsigned) * 2 * (size_t)L.n_ref));
    std::vector<unsigned> dl(nd);
    GSX_HIP(hipMemcpyAsync(dl.data(), a.deferred, sizeof(unsigned) * nd, hipMemcpyDeviceToHost, ctx->stream));
    GSX_HIP(hipStreamSynchronize(ctx->stream));
    const std::vector<unsigned> groups = group_deferred_bricks(dl.data(), nd, hgp.nbx, hgp.nby, hgp.nbz);
    if (groups.size() > 1) {  // one group: the device list is already it
        GSX_HIP(hipMemcpyAsync(a.deferred, dl.data(), sizeof(unsigned) * nd, hipMemcpyHostToDevice, ctx->stream));
        GSX_HIP(hipStreamSynchronize(ctx->stream));  // dl is a local
    }
    unsigned g_first = 0;
    for (const unsigned g_count : groups) {
        GSX_CHECK(refine_group(L, a, a.deferred + g_first, g_count));
        g_first += g_count;
    }
    return 0;
}

static int level_ring_heavy(GridLevel &L, const BrickLaunch &a)
{
    gsx_ctx *ctx = L.ctx;
    GridParams *gp = L.gp;
    std::chrono::steady_clock::time_point t_ring0;
    if (L.trace) {
        GSX_HIP(hipStreamSynchronize(ctx->stream));
        t_ring0 = std::chrono::steady_clock::now();
    }
    // a ring can only meet a huge cell if some brick was too populated for this level, i.e. deferred;
    // otherwise knn_ring keeps every query (no hand-over list, no second host sync)
    const bool heavy_possible = L.adaptive && L.have_hgp && L.hgp.deferred_count > 0;
    if (L.adaptive && !heavy_possible) GSX_HIP(hipMemsetAsync(&gp->heavy_limit, 0, sizeof(int), ctx->stream));
    GSX_CHECK(dispatch_ring(ctx, a));
    if (heavy_possible) {
        unsigned nheavy = 0;
        GSX_HIP(hipMemcpyAsync(&nheavy, &gp->heavy_count, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
        GSX_HIP(hipStreamSynchronize(ctx->stream));
        if (L.trace) fprintf(stderr, "[gsx] level %d: %u ring queries handed to knn_heavy\n", L.level, nheavy);
        if (nheavy > 0) GSX_CHECK(dispatch_heavy(ctx, L.w, a, L.n_ref, nheavy));
    }
    if (L.trace) {
        GSX_HIP(hipStreamSynchronize(ctx->stream));
        GridParams h3;
        GSX_HIP(hipMemcpy(&h3, gp, sizeof(GridParams), hipMemcpyDeviceToHost));
        fprintf(stderr, "[gsx] level %d: knn_ring %.3f ms for %u queries (%u exhaustive)\n", L.level,
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_ring0).count(), h3.fail_count,
                h3.exhaustive_count);
    }
    return 0;
}

// What the call reports (one more synchronisation, only when the caller asks).  The any-k path has no bricks and no ring:
// every query is a "fallback" there, its cells are the unpadded nx ny nz, and it leaves bad input to the caller's check.
static int level_info(GridLevel &L)
{
    gsx_ctx *ctx = L.ctx;
    gsx_sor_info *info = L.info;
    if (!info) return !L.anyk && L.have_hgp && L.hgp.bad_input && L.level == 0 ? gsx_ctx_check(ctx) : 0;
    GridParams h2;
    GSX_HIP(hipMemcpyAsync(&h2, L.gp, sizeof(GridParams), hipMemcpyDeviceToHost, ctx->stream));
    GSX_HIP(hipStreamSynchronize(ctx->stream));
    if (!L.anyk && h2.bad_input) return gsx_ctx_check(ctx);  // reports (and clears) the device flag
    info->algo = GSX_KNN_GRID;
    info->grid_dim[0] = h2.nx;
    info->grid_dim[1] = h2.ny;
    info->grid_dim[2] = h2.nz;
    info->cell_size = h2.h;
    info->n_cells = L.anyk ? (int64_t)h2.nx * h2.ny * h2.nz : (int64_t)h2.ncells;
    info->n_bricks = L.anyk ? 0 : h2.nbricks;
    info->n_fallback = L.anyk ? L.q_count : (int64_t)h2.fail_count;
    info->n_exhaustive = h2.exhaustive_count;
    info->n_deferred_bricks = L.anyk ? 0 : h2.deferred_count;
    info->n_refined = L.anyk ? 0 : (int64_t)L.w.refined_total;
    return 0;
}

static int knn_grid_level(gsx_ctx *ctx, int level, const float *x, const float *y, const float *z, int64_t stride,
                          int64_t n_ref, int64_t q_begin, int64_t q_count, int k, float *mean_out, double *kth_out,
                          gsx_sor_info *info, int share, int nshares, bool adaptive, float parent_h,
                          int64_t ref_only_from, double h_hint, const SlabKnn *sk)
{
    KnnWs &w = ctx->ws[level];
    if (level == 0) ctx->last_knn_algo = GSX_KNN_GRID;
    w.refined_total = 0;
    const bool anyk = k + 1 > 65;
    if (k + 1 > ANYK_MAX) GSX_FAIL("sor: k=%d not supported (k must be <= %d)", k, ANYK_MAX - 1);
    const bool slab = ref_only_from < n_ref;
    if (anyk && (nshares > 1 || slab)) GSX_FAIL("sor: k=%d > 64 is served by the single-GPU path only", k);
    const bool all = (q_begin == 0 && q_count == n_ref) || slab;
    // (a share of the bricks -- the replicated multi-GPU exchange -- refines the deferred bricks of ITS share only)
    adaptive = adaptive && !anyk && all && !slab && level + 1 < KNN_MAX_LEVELS;
    GridLevel L{ctx, level, w, x, y, z, stride, n_ref, q_begin, q_count, k, mean_out, kth_out, info, share, nshares, parent_h,
                ref_only_from, h_hint, sk, anyk, slab, all, adaptive, getenv("GSX_TRACE_LEVELS") != nullptr,
                h_hint > 0.0 ? grid_refine_cell_cap(n_ref) : grid_cell_cap(n_ref),
                ctx->grid_points_per_cell > 0.0 ? ctx->grid_points_per_cell : grid_pts_per_cell(k, n_ref)};
    GSX_CHECK(level_reserve(L));
    GSX_CHECK(level_grid_params(L));
    bool done = false;
    int rc = level_histogram(L, &done);
    if (rc != 0 || done) return rc;
    GSX_CHECK(level_bin(L));
    BrickLaunch a{L.gp, L.refs, L.rstart, L.qpts, L.qstart, k, q_begin, mean_out, kth_out, L.fail, L.fail_rest,
                  w.extraitems.as<uint2>(), w.deferred.as<unsigned>(), w.heavylist.as<unsigned>(), q_count, n_ref,
                  L.plan ? w.finestart.as<unsigned>() : nullptr, L.plan ? w.bricklist.as<uint2>() : nullptr};
    if (anyk) {
        GSX_CHECK(level_anyk(L));
        return level_info(L);
    }
    GSX_CHECK(dispatch_bricks(ctx, a, L.mfma_ok, ctx->phase2_net != 0));
    if (L.adaptive) {
        rc = level_refine(L, a, &done);
        if (rc != 0 || done) return rc;
    }
    GSX_CHECK(level_ring_heavy(L, a));
    return level_info(L);
}

int launch_knn_grid(gsx_ctx *ctx, const float *x, const float *y, const float *z, int64_t stride, int64_t n_ref,
                    int64_t q_begin, int64_t q_count, int k, float *mean_out, gsx_sor_info *info, int share, int nshares)
{
    return knn_grid_level(ctx, 0, x, y, z, stride, n_ref, q_begin, q_count, k, mean_out, nullptr, info, share, nshares,
                          ctx->adaptive != 0, 0.0f);
}

// sk (optional): the certificate evaluated inside the grid path's kernels (kth_out is then only written by the tree path:
// ctx->last_knn_algo says which ran) and a box the caller already knows
int launch_knn_slab(gsx_ctx *ctx, const float *x, const float *y, const float *z, int64_t stride, int64_t n_own,
                    int64_t n_halo, int k, float *mean_out, double *kth_out, const SlabKnn *sk)
{
    return knn_grid_level(ctx, 0, x, y, z, stride, n_own + n_halo, 0, n_own, k, mean_out, kth_out, nullptr, 0, 1, false, 0.0f,
                          n_own, 0.0, sk);
}

}  // namespace gsx
