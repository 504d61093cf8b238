// grid_policy.h -- the host-side decisions of the KNN grid (sor_grid.hip: knn_grid_level; dist_slab.hip: the slab estimate).
// Plain C++17 arithmetic on a handful of numbers: no HIP types, no context, so a host compiler can include it and a test can
// call it without a GPU (gsx_sor_debug_points_per_cell / _group_bricks / _refine_sizing, tests/test_grid_policy_host.py).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <unordered_map>
#include <vector>

namespace gsx {

// the two-level sort's limits: what the kernels of sor_grid.hip size their LDS tables with and what bounds a level's cells
constexpr int MAX_BUCKETS = 4096;         // LDS histogram bins of the coarse pass
constexpr int MAX_BUCKET_CELLS = 4096;    // LDS counters of the fine pass (16 KiB)
constexpr int64_t GRID_MAX_CELLS = (int64_t)MAX_BUCKETS * MAX_BUCKET_CELLS - 64;   // what the two-level sort can address

// ---------------------------------------------------------------- points per cell
// cell edge h is also the guaranteed search radius: the expected number of points within h is
// 4.19 * m, and a query falls back to knn_ring when fewer than k+1 are.  m = 0.47 (k+1) puts
// ~2 (k+1) points inside h (measured optimum at k = 8, 16, 25, 32: profiles/r01_sweep_m.log).
// A brick's population cells*m should stay <= ~58 so that its queries fit ONE 64-lane batch
// (at 64 on average 47 % of the bricks need a second one): k = 16 -> m = 7.25, not 8.
inline double grid_fill(int64_t n) { return n >= 4000000 ? 54.0 : 58.0; }

// The rule as it stood before the k-range caps below: what the multi-GPU slab estimate (dist_slab.hip: gsx_slab_plan; Python:
// dist_slab.pts_per_cell) sizes its halo with.  It is NOT what the grid itself uses for k = 17...20, 26...31, 35...62.
inline double grid_pts_per_cell_base(int k, int64_t n)
{
    double m = std::max(2.0, 0.47 * (double)(k + 1));
    // a brick's queries must fit ONE 64-lane batch with a margin.  Fewer points per cell = fewer candidates per
    // query in knn_brick but more queries for the ring kernels, which are cheap per query once tens of thousands
    // of them keep every wave busy and latency-bound below that (profiles/r02_variants.txt: 10M k=16 is fastest at
    // 54 / 8 cells, 1M at 58 / 8, 50M k=32 at 52-54 / 4)
    const double fill = grid_fill(n);
    for (int cells = 8; cells >= 1; cells /= 2)
        if (m * cells > fill && m * cells <= 66.0) m = fill / cells;
    return m;
}

// What knn_grid_level uses when the context's grid_points_per_cell is 0: the base rule and four k-range caps.
inline double grid_pts_per_cell(int k, int64_t n)
{
    double m = grid_pts_per_cell_base(k, n);
    const double fill = grid_fill(n);
    // k = 17 ... 20 (round 4; the reference CLI's --sor_intensity 3 is k = 18): 0.47 (k + 1) points per cell would
    // halve the brick to 2x2x1 cells -- 36 of 64 lanes busy, 12x instead of 8x its points as candidates.  Smaller cells
    // keep the 2x2x2 brick full at the price of ring queries (10M uniform, step ms: k = 18 3.16 -> 2.60 with 175 k ring
    // queries, k = 20 3.17 -> 2.90 with 186 k; from k = 23 on the ring queries cost more than the full lanes save)
    if (k >= 17 && k <= 20) m = std::min(m, fill / 8.0 + 0.375 * (double)std::max(0, k - 18));
    // ... and k = 35 ... 52 (--sor_intensity 7 ... 10: k = 36, 41, 45, 50) keeps 2x2x1 bricks instead of 2x1x1 (10M uniform, step ms:
    // k = 36 6.28 -> 4.52, k = 41 6.10 -> 5.02, k = 45 7.26 -> 5.73, k = 48 7.50 -> 6.3, k = 50 10.3 -> 8.3; k >= 56: the ring
    // queries win -- profiles/r04_variants.txt)
    if (k >= 26 && k <= 31) m = std::min(m, 12.0 * fill / 54.0);   // (k = 27: 3.49 -> 3.36, k = 30: 3.58 -> 3.42)
    if (k >= 35 && k <= 43) m = std::min(m, (k <= 38 ? 13.5 : 14.5) * fill / 54.0);
    // Round 5: with 32 parked words (1024 candidates) for the lists of more than 32 entries the cells of k >= 44 can be larger
    // again -- fewer ring queries (k = 50 at 15 points per cell: 595 k of them, 2.5 of 7.6 ms).  10M uniform, step ms, best of
    // a sweep 15 ... 26 (profiles/r05_variants.txt): k = 45 5.67 -> 5.41 (16), 47 6.01 -> 5.58 (16), 50 7.60 -> 6.37 (22), 52 8.86 ->
    // 6.14 (22), 55 7.17 -> 6.81 (22), 57 7.87 -> 7.22 (22), 60 7.87 -> 7.34 (24); k >= 63: 0.47 (k + 1) as before
    if (k >= 44 && k <= 62) m = std::min(m, k <= 49 ? 16.0 : (k <= 58 ? 22.0 : 24.0));
    return m;
}

// ---------------------------------------------------------------- cell budget of a level
// cells the grid may have.  Level 0: about one cell per two points (more would be empty cells to walk).
inline int64_t grid_cell_cap(int64_t n_ref) { return std::max<int64_t>(n_ref / 2, 64) + 64; }
// A refinement level sized by the density probe covers a box that is mostly EMPTY by construction (a blob's tails, the few
// floaters around a scene), so it gets room for 4 cells per point, within what the two-level sort can address.
inline int64_t grid_refine_cell_cap(int64_t n_ref) { return std::min<int64_t>(std::max<int64_t>(4 * n_ref, 64), GRID_MAX_CELLS) + 64; }

// ---------------------------------------------------------------- the coarse histogram's verdict
// Adaptive mode, first decision: can ONE grid resolve this cloud at all?  The coarse histogram of the two-level sort (one
// bucket = a column of cells sized for ~4096 points of a uniform cloud) says so after 0.1 ms: a cloud whose fullest bucket
// holds several times the average (a scene inside a box inflated by floaters: 2400x; Gaussian blobs: 30x+) goes to the
// Morton-tree path (sor_tree.hip) at once -- no cell size fits it, and refining level by level costs a host round trip
// and a re-binning per level (clustered 1M: 16.5 ms against 1.3 ms).
struct HistVerdict {
    unsigned fullest = 0, nonzero = 0;   // points of the fullest bucket, buckets that hold any
    bool to_tree = false;                // the fullest bucket exceeds 3x the average of the non-empty ones
    // an even histogram (fullest bucket within 1.5x of the average): no brick can be far over-full, so none is deferred and
    // the host does not have to look at the counters again -- the call costs ONE synchronisation, as before the probe existed
    bool no_deferral = false;
};
inline HistVerdict grid_hist_verdict(const unsigned *starts /* MAX_BUCKETS + 1 bucket starts */, int64_t n_ref, int nshares)
{
    HistVerdict v;
    for (int b = 0; b < MAX_BUCKETS; ++b) {
        const unsigned c = starts[b + 1] >= starts[b] ? starts[b + 1] - starts[b] : 0u;   // (entries past the last bucket repeat the total)
        v.fullest = std::max(v.fullest, c);
        v.nonzero += c > 0;
    }
    v.to_tree = v.nonzero > 0 && (double)v.fullest > 3.0 * (double)n_ref / (double)v.nonzero;
    v.no_deferral = v.nonzero > 0 && (double)v.fullest <= 1.5 * (double)n_ref / (double)v.nonzero && nshares == 1;
    return v;
}

// ---------------------------------------------------------------- planned bricks
// Planned bricks (brick_plan_kernel): the plain single-cloud call only -- every point a query of the one table, no share, no
// slab halo, no refinement level -- and the kernels they were built for: 2x2x2-cell bricks (pts_per_cell as grid_params
// decides), k <= 16, MFMA filter + network selection.  An adaptive call qualifies once the coarse histogram has shown that
// nothing will be deferred.  The grid's extent along x is checked on the device (grid_params).
struct PlanCall {
    bool enabled;             // the context's brick_plan
    int level;
    bool whole_cloud;         // every reference point is a query
    bool slab, slab_extras;   // a halo of reference-only points / launch_knn_slab's certificate or known box
    int nshares, k;
    bool mfma, net;           // MFMA filter usable for this cloud, network selection on
    double pts_per_cell, h_hint;
    bool wants_kth;
};
inline bool grid_plan_eligible(const PlanCall &c)
{
    return c.enabled && c.level == 0 && c.whole_cloud && !c.slab && !c.slab_extras && c.nshares == 1 && c.k + 1 <= 17 && c.mfma &&
           c.net && !(c.pts_per_cell * 8.0 > 66.0) && c.h_hint == 0.0 && !c.wants_kth;
}

// ---------------------------------------------------------------- grouping of the deferred bricks
// Deferred bricks that are far apart belong to different clusters with different densities:
// each connected group (bricks within 2 of each other, i.e. overlapping neighbourhoods)
// gets its own sub-cloud, hence its own bounding box and cell size.  At most 8 groups
// (the smallest ones are merged into the last).  The list is rewritten group by group, largest first; returns the groups' sizes.
constexpr int GRID_MAX_GROUPS = 8;
inline std::vector<unsigned> group_deferred_bricks(unsigned *dl, unsigned nd, int nbx, int nby, int nbz)
{
    std::vector<std::vector<unsigned>> groups;
    std::unordered_map<unsigned, int> where;  // brick id -> index in dl
    for (unsigned i = 0; i < nd; ++i) where[dl[i]] = (int)i;
    std::vector<int> comp(nd, -1);
    for (unsigned s0i = 0; s0i < nd; ++s0i) {
        if (comp[s0i] >= 0) continue;
        const int c = (int)groups.size();
        groups.emplace_back();
        std::vector<unsigned> stack{s0i};
        comp[s0i] = c;
        while (!stack.empty()) {
            const unsigned i = stack.back();
            stack.pop_back();
            groups[c].push_back(dl[i]);
            const int b = (int)dl[i];
            const int bz = b / (nbx * nby), by = (b - bz * nbx * nby) / nbx, bx = b - bz * nbx * nby - by * nbx;
            for (int dz = -2; dz <= 2; ++dz)
                for (int dy = -2; dy <= 2; ++dy)
                    for (int dx = -2; dx <= 2; ++dx) {
                        const int x2 = bx + dx, y2 = by + dy, z2 = bz + dz;
                        if (x2 < 0 || y2 < 0 || z2 < 0 || x2 >= nbx || y2 >= nby || z2 >= nbz) continue;
                        auto it = where.find((unsigned)((z2 * nby + y2) * nbx + x2));
                        if (it != where.end() && comp[it->second] < 0) {
                            comp[it->second] = c;
                            stack.push_back((unsigned)it->second);
                        }
                    }
        }
    }
    std::sort(groups.begin(), groups.end(), [](const auto &l, const auto &r) { return l.size() > r.size(); });
    while (groups.size() > (size_t)GRID_MAX_GROUPS) {
        groups[GRID_MAX_GROUPS - 1].insert(groups[GRID_MAX_GROUPS - 1].end(), groups.back().begin(), groups.back().end());
        groups.pop_back();
    }
    std::vector<unsigned> sizes;
    unsigned o = 0;
    for (auto &g : groups) {
        std::copy(g.begin(), g.end(), dl + o);
        o += (unsigned)g.size();
        sizes.push_back((unsigned)g.size());
    }
    return sizes;
}

// ---------------------------------------------------------------- refinement sizing of one group
// The neighbourhood cells reach up to two of THIS level's cells beyond the queries; a stray
// far point among them (the very outliers that inflated the bounding box) would inflate the
// finer grid again.  Reference points farther than M from the queries' box are left out, and
// the finer level's answers are accepted only up to M: M = 4 x the cell edge the finer grid
// will get, i.e. ~5x its typical (k+1)-th neighbour distance.
struct RefineClip {
    int nd3 = 0;                 // axes along which the queries' box has an extent
    double h_est = 0.0;          // cell edge the finer level would get from the box volume of the group's queries
    double M = 0.0, cert = 0.0;  // the clip margin and what of it survives the f32 rounding of lo - M / hi + M
    float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};   // the clip planes ...
    float r_cert = 0.0f;                          // ... and their certificate; 0 = no clipping (the planes are then 0 as well)
    int probe_g = 0;             // edge of the density probe's grid in bins, 8 ... 64; 0 = no probe for this group
};
inline RefineClip refine_clip(const float qb_lo[3], const float qb_hi[3], unsigned sub_queries, double pts_per_cell, float parent_h,
                              int adaptive_mode)
{
    RefineClip r;
    double vol = 1.0, amax = 0.0;
    for (int ax = 0; ax < 3; ++ax) {
        const double e = (double)qb_hi[ax] - (double)qb_lo[ax];
        if (e > 0.0) { vol *= e; ++r.nd3; }
        amax = std::max({amax, std::fabs((double)qb_lo[ax]), std::fabs((double)qb_hi[ax])});
    }
    const double per = sub_queries > 0 ? vol * pts_per_cell / (double)sub_queries : 0.0;
    r.h_est = r.nd3 == 3 ? std::cbrt(per) : (r.nd3 == 2 ? std::sqrt(per) : (r.nd3 == 1 ? per : 0.0));
    r.M = std::max(4.0 * r.h_est, 0.01 * (double)parent_h);
    r.cert = r.M * (1.0 - 1e-3) - 4e-7 * amax;  // f32 rounding of lo - M / hi + M
    if (adaptive_mode == 1 && sub_queries > 0 && r.M < 2.0 * (double)parent_h && r.cert > 0.0) {
        for (int ax = 0; ax < 3; ++ax) {
            r.lo[ax] = std::nextafterf((float)((double)qb_lo[ax] - r.M), -__builtin_inff());
            r.hi[ax] = std::nextafterf((float)((double)qb_hi[ax] + r.M), __builtin_inff());
        }
        r.r_cert = (float)r.cert;
    }
    // density probe of the gathered points (sor_grid.hip: probe_count_kernel): ~32 queries per bin of a G^3 grid over their box
    if (adaptive_mode == 1 && sub_queries > 0 && r.nd3 == 3)
        r.probe_g = std::max(8, std::min(64, (int)std::lround(std::cbrt((double)sub_queries / 32.0))));
    return r;
}

// The cell edge for the finer level from the probe's point-weighted histogram of log2(count per bin); 0 = keep the
// box-volume edge h_est.  bin_vol: volume of one probe bin; lo / hi: the queries' box; n_sub: points gathered.
inline double refine_probe_edge(const unsigned hist[32], double bin_vol, const float lo[3], const float hi[3], float r_cert,
                                unsigned n_sub, double h_est, double pts_per_cell)
{
    constexpr double probe_q = 0.85, probe_shrink = 0.7;   // measured: quantiles 0.5 / 0.7 / 0.85 on four clouds
    unsigned long long tot = 0, run = 0;
    for (int b = 0; b < 32; ++b) tot += hist[b];
    int bq = -1;
    for (int b = 0; b < 32 && tot; ++b) {
        run += hist[b];
        if ((double)run >= probe_q * (double)tot) {
            bq = b;
            break;
        }
    }
    if (!(bq >= 0 && bin_vol > 0.0)) return 0.0;
    // 85 % of the points sit in probe bins of at most ~1.5 * 2^bq points: cells sized for THAT density are
    // over-full only for the densest 15 % (a Gaussian's core is 1.4x denser than its 85 % level: no second
    // refinement), under-full for the tails, whose queries go to the ring kernels
    const double rho = 1.5 * std::ldexp(1.0, bq) / bin_vol;
    double h_hint = std::cbrt(pts_per_cell / rho);
    // a grid of that edge over the group's box must fit the cell budget, otherwise the edge would be stretched
    // to something in between and every brick of a uniform region would be over-full: keep the old sizing then
    double cells = 1.0;
    for (int ax = 0; ax < 3; ++ax) cells *= std::floor(((double)hi[ax] - (double)lo[ax] + 2.0 * (double)r_cert) / h_hint) + 1.0;
    const double budget = (double)std::min<int64_t>(4 * (int64_t)n_sub, GRID_MAX_CELLS);
    if (!(cells <= 0.8 * budget)) h_hint = 0.0;
    // a near-uniform group (the probed edge within 30 % of the box-volume edge) keeps the box-volume edge: the
    // population per cell is tuned to a few per cent there (0.92x the edge = 13x the ring queries, measured)
    if (h_hint > probe_shrink * h_est) h_hint = 0.0;
    return h_hint;
}

}  // namespace gsx
