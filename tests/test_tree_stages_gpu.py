"""-m gpu: the three stages of the Morton-tree KNN (csrc/sor_tree.hip), each made to answer for itself.

knn_leaf, knn_tree_near and knn_tree_query form a cascade in which every later stage is exact for ANY query, so it hides every
defect of the stage in front of it: a knn_leaf that certified nothing, a knn_tree_near that deferred everything, a branch of the
near kernel that a handful of queries per cloud reach -- test_sor_tree_gpu would stay bit-exact against cKDTree through all of
them.  Here the context parameters tree_cand_limit and tree_near_cell move the work between the stages, the counters of
gsx_sor_debug_tree (Context.debug_tree) say which stage answered and why the near kernel handed a query on, and the leaf
partition the device built is compared with the rule of test_tree_leaf_rule.  Every call goes through the device entry point
with algo = TREE on a fresh context (knn_device.knn); the bar is the project's: mean distances bit for bit against
oracle.sor.mean_dists_ckdtree.

Constants of sor_tree.hip the comments below refer to: TQ_CAND = 256 (values inside the ball a wave of the near kernel or of the
descent's COLLECT mode buffers), TQ_DENSE = 4096 (points of one cover cell above which the near kernel defers), 512 (cover cells
above which it defers), LEAF_TILE = 1024 (sorted points per workgroup of tree_leaf_flags_kernel)."""
import functools

import numpy as np
import pytest

from knn_device import TREE, differ, explain, knn
from oracle import datasets, sor as osor
from test_knn_variants_gpu import NET_K, _mixed, _mixed_ref, _uniform, _uniform_ref
from test_tree_leaf_rule import leaf_levels

pytestmark = pytest.mark.gpu

KEY_BITS = 63   # 21 bits per axis

# ---------------------------------------------------------------------------------------------------------------- the stage settings
# default          all three kernels
# near-radius      tree_cand_limit = 1: knn_leaf's limit becomes 1 / 64 * leaf_cap = 0 candidates, every leaf is "irregular" and
#                  every query enters knn_tree_near with a radius to try (a negative bound, widened up to two times by 1.3)
# descent-insert   ... and tree_near_cell = 0.051 (the smallest step above the setter's floor of 0.05): the cover's cells have an
#                  edge g in [0.051 r, 0.102 r), so a ball's box of 2 r + 2 fine cells spans more than 2 / 0.102 = 19.6 of them
#                  along an axis -- and at a corner of the cloud, where the box is cut to r on every axis, still more than 9.8 + 1:
#                  at least 10^3 > 512 cells for every ball whose cells are not already single fine cells.  Every query takes the
#                  descent from a radius, in INSERT mode.
# descent-collect  tree_near_cell = 0.051 alone: knn_leaf runs normally, each of its failures (k-th bound known) goes to the descent
#                  in COLLECT mode
# near-dense       tree_near_cell = 4 and 64, with and without tree_cand_limit = 1: g in [4 r, 8 r) resp. [64 r, 128 r), the wave-wide
#                  scan behind the block boxes (a cell of more than 64 points).  The plain cloud holds rho = 16 points per unit
#                  volume; a full ball of k + 1 of them has r_k = cbrt(3 (k + 1) / (4 pi rho)) -- 0.25 at k = 1, 0.49 at 7, 0.63 at
#                  16, 0.99 at 64 -- and one cut by one, two or three faces of the box 1.26, 1.59 or 2 times that.  g is the fine
#                  cell edge (10 (1 + 2^-18) / 2^21) times a power of two.  At tree_near_cell = 4 and k >= 7: g >= 1.97 means
#                  g >= 2.5, a cell of rho g^3 >= 250 points; g = 5 is an octant of the cloud, 2000 points, still below TQ_DENSE;
#                  r > 1.25 makes g the whole box, 16 000 points in one cell: reason 1.  At 64 already r >= 0.08 gives g >= 5.1 and
#                  that one cell: every query the near kernel sees takes reason 1.
#                  Which k can have 0 < fail2_count < fail_count at tree_near_cell = 4 follows from r against 1.25: up to k = 8
#                  no ball reaches it (2 r_8 = 1.02), the near kernel answers every query it gets and fail2_count is 0 unless a
#                  radius tried three times still holds fewer than k points (reason 3); from k = 16 on the balls at the corners do
#                  (2 r_16 = 1.27) and the full ones do not (r_64 = 0.99) -- but knn_leaf's failures at k = 64 are the rim's queries
#                  alone, so without tree_cand_limit = 1 nothing below 1.25 may be left.  Observed fail2_count / fail_count,
#                  k = 1, 7, 8, 16, 25, 33, 50, 63, 64: leaf running 0/276 0/261 0/266 2/748 116/2592 317/364 400/404 492/494 497/497,
#                  tree_cand_limit = 1 0 0 0 9 49 1912 15 596 15 731 15 733 of 16 000.
STAGES = {
    "default": {},
    "near-radius": {"tree_cand_limit": 1},
    "descent-insert": {"tree_cand_limit": 1, "tree_near_cell": 0.051},
    "descent-collect": {"tree_near_cell": 0.051},
    "near-dense-4": {"tree_near_cell": 4},
    "near-dense-4-radius": {"tree_near_cell": 4, "tree_cand_limit": 1},
    "near-dense-64": {"tree_near_cell": 64},
    "near-dense-64-radius": {"tree_near_cell": 64, "tree_cand_limit": 1},
}
STAGE_K = [1, 7, 8, 16, 25, 33, 50, 63, 64]
STAGE_MATRIX = [pytest.param(name, k, id="%s-k%d" % (name, k)) for name in STAGES for k in STAGE_K]
FORCED = ["near-radius", "descent-insert"]   # the two settings in which no query is answered by knn_leaf
PLAIN_N = 16000


@pytest.fixture(scope="module")
def lib(gsx):
    gsx._lib.require_hip()
    return gsx._lib


def _plain():
    """duplicate-free: datasets.uniform, 16 000 points in a box of edge 10"""
    return _uniform(PLAIN_N)


def _plain_ref(k):
    return _uniform_ref(PLAIN_N, k)


def check_counters(st, info, n, q_count):
    """what holds in EVERY tree run: the counters of the debug entry point are those of the info block, a query is handed on at
    most once per stage, and knn_tree_near counts exactly one of the reasons 0 .. 4 for every query it hands on (5 .. 7 split
    reason 1 by the attempt it happened in)"""
    why = st["defer_why"]
    assert info["algo"] == TREE, info
    assert st["n"] == n and st["nleaves"] == info["n_bricks"] and 0 < st["nleaves"] <= n, (st, info)
    assert st["fail_count"] == info["n_fallback"] and st["fail2_count"] == info["n_exhaustive"], (st, info)
    assert st["fail2_count"] <= st["fail_count"] <= q_count, st
    assert int(why[:5].sum()) == st["fail2_count"], st
    assert int(why[4]) == 0, st   # a known bound IS the distance of a k-th point the leaf found: the ball that large holds k
    assert int(why[5:8].sum()) == int(why[1]), st


def run(lib, xyz, k, window=None, columns=False, **params):
    """one tree call on a fresh context -> (mean distances, info, counters)"""
    ctx = lib.Context(0)
    try:
        got, info, _ = knn(lib, xyz, k, ctx=ctx, window=window, columns=columns, algo=TREE, **params)
        st = ctx.debug_tree()
    finally:
        ctx.close()
    check_counters(st, info, len(xyz), window[1] if window is not None else len(xyz))
    return got, info, st


def show(st):
    return "fail %d fail2 %d why %s leaves %d cap %d" % (st["fail_count"], st["fail2_count"], st["defer_why"].tolist(), st["nleaves"], st["leaf_cap"])


@pytest.mark.parametrize("name,k", STAGE_MATRIX)
def test_stage_settings_on_a_plain_cloud_and_who_answered(lib, name, k):
    """The counting assertions.  Measured on this cloud (every k of STAGE_K): at tree_near_cell = 0.051 every deferral is reason
    0, no rim query escapes."""
    xyz, n = _plain(), PLAIN_N
    got, info, st = run(lib, xyz, k, **STAGES[name])
    ref = _plain_ref(k)
    print("plain %s k=%d: %s; %s" % (name, k, show(st), explain(got, ref)))
    assert differ(got, ref) == 0, (explain(got, ref), show(st))
    why = st["defer_why"]
    if "tree_cand_limit" in STAGES[name]:
        assert st["fail_count"] == n, show(st)            # knn_leaf answered nothing
    else:
        assert 0 < st["fail_count"] <= n // 2, show(st)   # ... answered most, and left something for the stage under test
    if name == "near-radius":
        assert st["fail2_count"] < n // 2, show(st)       # the near kernel answered most of the cloud itself
        # the radius to try holds 1.3^3 * 4.19 * 0.397 (k + 1) = 3.65 (k + 1) points at the leaf's own density; widened twice by
        # 1.3 it holds 4.83 times as many -- 17.6 (k + 1), and in a corner of the box, an eighth of the ball, still 2.2 (k + 1):
        # "fewer than k inside the last radius" is left to leaves whose own density says little (a percent is generous; were
        # the ball not widened, half of the queries within a radius of two faces -- 5 % of the cloud at k = 16 -- would get there)
        assert int(why[3]) <= n // 100, show(st)
    elif name == "descent-insert":
        assert st["fail2_count"] == st["fail_count"] == n and int(why[0]) == st["fail2_count"], show(st)
    elif name == "descent-collect":
        assert st["fail2_count"] == st["fail_count"] > 0 and int(why[0]) == st["fail2_count"], show(st)
    elif name.startswith("near-dense-4"):
        assert int(why[0]) == 0, show(st)   # a ball spans at most two cells of 4 r along an axis
        if k <= 8:      # no ball reaches r = 1.25: no cell above TQ_DENSE, the near kernel answers (all but reason 3) itself
            assert int(why[1]) == 0 and st["fail2_count"] < st["fail_count"], show(st)
        elif k < 64 or "tree_cand_limit" in STAGES[name]:
            assert 0 < st["fail2_count"] < st["fail_count"], show(st)   # the near kernel did answer some itself
        else:           # k = 64 behind a running knn_leaf: rim queries only, all of which may lie beyond 1.25
            assert 0 < st["fail2_count"] <= st["fail_count"], show(st)
    elif name.startswith("near-dense-64"):
        assert int(why[1]) > 0 and int(why[5:8].sum()) == int(why[1]), show(st)
        assert int(why[1]) == st["fail2_count"] == st["fail_count"], show(st)   # one cell is the cloud: nobody gets past it


@pytest.mark.parametrize("name,k", STAGE_MATRIX)
def test_stage_settings_on_a_cloud_with_a_blob_and_duplicates(lib, name, k):
    """test_knn_variants_gpu's 12 000 points.  The groups of 800 and 147 copies give bounds of exactly 0; the 800 put more than
    TQ_CAND values at d <= T: "buffer full" (reason 2) in the near kernel, COLLECT -> INSERT overflow in the descent; the groups
    of 3 and 10 are shorter than most k."""
    xyz = _mixed()
    got, info, st = run(lib, xyz, k, **STAGES[name])
    ref = _mixed_ref(k)
    print("mixed %s k=%d: %s; %s" % (name, k, show(st), explain(got, ref)))
    assert differ(got, ref) == 0, (explain(got, ref), show(st))
    if "tree_cand_limit" in STAGES[name]:
        assert st["fail_count"] == len(xyz), show(st)
    if name == "near-radius":
        # the 801 identical points are one over-full leaf whose tight box is a point: the radius to try is half a fine cell,
        # the ball holds 800 values of 0 and the buffer 256
        assert int(st["defer_why"][2]) > 0, show(st)


# ---------------------------------------------------------------------------------------------------------------- knn_leaf certifies
# knn_tree_near / knn_tree_query answer every query knn_leaf does not certify, so a knn_leaf that certified nothing would still be
# bit-exact.  On a uniform cloud every instantiation (list capacities 9, 13, 17, ..., 57, 65: NET_K enters each with a k at both
# of its edges) must certify at least half of the queries itself.  A query fails when its k-th neighbour is farther than the
# nearest face of its leaf's box grown by half the leaf's longest side, or than 1.1 x the radius expected to hold 2 (k + 1) points.
# The cloud size per k is the smallest of 8000, 16 000, 32 000, 64 000 at which the measured n_fallback / n of the unmodified
# kernels is at most 1/4: the cap of 1/2 leaves a factor of two.
# Measured n_fallback / n of the kernels of commit 172b80a (which this file leaves untouched), datasets.uniform(n, 10.0, 43), default
# parameters (leaf capacity 64 up to k = 28, 96 up to 34, 128 above), k: share; then tree_leaf_cap, k: share
#   n = 8000 -- at most 1/4 for every k and both forced capacities, so every test below runs at 8000 points
#     1: 0.0196   3: 0.0231   7: 0.0254   8: 0.0241   9: 0.0240   12: 0.0254   13: 0.0253   16: 0.0276   17: 0.0295   20: 0.0299
#     21: 0.0305   24: 0.0305   25: 0.0328   28: 0.0335   29: 0.0316   32: 0.0335   33: 0.0335   36: 0.0387   37: 0.0403   40: 0.0436
#     41: 0.0457   44: 0.0520   45: 0.0544   48: 0.0638   49: 0.0674   52: 0.0790   53: 0.0835   56: 0.0980   57: 0.1034   64: 0.1482
#     96, 16: 0.0275   96, 29: 0.0316   96, 35: 0.0362   96, 64: 0.1676   128, 16: 0.0275   128, 29: 0.0335   128, 35: 0.0379   128, 64: 0.1482
# The share does not fall with n: it follows the SHAPE the leaves get (cubes, 2:2:1 or 2:1:1 boxes: an accident of extent / 2^21
# below 2^18 points, where no density probe runs), so the larger sizes of the ladder are partly worse -- for the record:
#   n = 16 000
#     1: 0.0173   3: 0.0170   7: 0.0163   8: 0.0166   9: 0.0175   12: 0.0233   13: 0.0266   16: 0.0467   17: 0.0568   20: 0.0930
#     21: 0.1071   24: 0.1482   25: 0.1620   28: 0.2005   29: 0.0203   32: 0.0218   33: 0.0227   36: 0.0226   37: 0.0226   40: 0.0232
#     41: 0.0238   44: 0.0239   45: 0.0245   48: 0.0249   49: 0.0252   52: 0.0255   53: 0.0262   56: 0.0279   57: 0.0278   64: 0.0311
#     96, 16: 0.0170   96, 29: 0.0203   96, 35: 0.0230   96, 64: 0.0319   128, 16: 0.0177   128, 29: 0.0194   128, 35: 0.0217   128, 64: 0.0311
#   n = 32 000
#     1: 0.0168   3: 0.0150   7: 0.0132   8: 0.0132   9: 0.0134   12: 0.0138   13: 0.0140   16: 0.0148   17: 0.0155   20: 0.0195
#     21: 0.0220   24: 0.0328   25: 0.0377   28: 0.0592   29: 0.0622   32: 0.0941   33: 0.1068   36: 0.0642   37: 0.0710   40: 0.0924
#     41: 0.1012   44: 0.1263   45: 0.1335   48: 0.1562   49: 0.1618   52: 0.1811   53: 0.1876   56: 0.2045   57: 0.2103   64: 0.2470
#     96, 16: 0.0143   96, 29: 0.0622   96, 35: 0.1363   96, 64: 0.5782   128, 16: 0.0138   128, 29: 0.0312   128, 35: 0.0578   128, 64: 0.2470
#   n = 64 000
#     1: 0.0156   3: 0.0132   7: 0.0098   8: 0.0098   9: 0.0096   12: 0.0101   13: 0.0102   16: 0.0098   17: 0.0099   20: 0.0102
#     21: 0.0106   24: 0.0103   25: 0.0102   28: 0.0107   29: 0.0103   32: 0.0107   33: 0.0112   36: 0.0126   37: 0.0132   40: 0.0160
#     41: 0.0171   44: 0.0205   45: 0.0222   48: 0.0270   49: 0.0286   52: 0.0352   53: 0.0381   56: 0.0477   57: 0.0512   64: 0.0869
#     96, 16: 0.0099   96, 29: 0.0103   96, 35: 0.0124   96, 64: 0.1036   128, 16: 0.0101   128, 29: 0.0103   128, 35: 0.0120   128, 64: 0.0869
LADDER = (8000, 16000, 32000, 64000)
LEAF_N = {k: LADDER[0] for k in NET_K}
CAP_K = [16, 29, 35, 64]
CAP_N = {(cap, k): LADDER[0] for cap in (96, 128) for k in CAP_K}
CAP_MATRIX = [pytest.param(cap, k, id="cap%d-k%d" % (cap, k)) for cap in (96, 128) for k in CAP_K]


@pytest.mark.parametrize("k", NET_K)
def test_every_knn_leaf_instantiation_certifies_half_of_a_uniform_cloud_itself(lib, k):
    n = LEAF_N[k]
    got, info, st = run(lib, _uniform(n), k)
    ref = _uniform_ref(n, k)
    print("n=%d k=%d leaf_cap=%d: n_fallback / n = %.4f; %s; %s" % (n, k, st["leaf_cap"], info["n_fallback"] / n, show(st), explain(got, ref)))
    assert differ(got, ref) == 0, (explain(got, ref), show(st))
    assert st["leaf_cap"] == (64 if k <= 28 else (96 if k <= 34 else 128)), show(st)
    assert info["n_bricks"] > 0 and info["n_fallback"] <= n // 2, info


@pytest.mark.parametrize("cap,k", CAP_MATRIX)
def test_leaves_of_96_and_128_points_certify_half_of_a_uniform_cloud_themselves(lib, cap, k):
    """the queries of a leaf are then taken 64 at a time against one candidate set, and the filter runs in passes of 896 (k <= 32)
    and 1024 candidates"""
    n = CAP_N[cap, k]
    got, info, st = run(lib, _uniform(n), k, tree_leaf_cap=cap)
    ref = _uniform_ref(n, k)
    print("n=%d k=%d tree_leaf_cap=%d: n_fallback / n = %.4f; %s; %s" % (n, k, cap, info["n_fallback"] / n, show(st), explain(got, ref)))
    assert differ(got, ref) == 0, (explain(got, ref), show(st))
    assert st["leaf_cap"] == cap, show(st)
    assert info["n_bricks"] > 0 and info["n_fallback"] <= n // 2, info


# ---------------------------------------------------------------------------------------------------------------- windows, shares, layout
GUARD = 64
GUARD_BITS = np.uint32(0x7FC0DEAD)   # a NaN no kernel produces


@pytest.mark.parametrize("k", [16, 25])
@pytest.mark.parametrize("name", FORCED)
def test_a_query_window_under_forced_stages_writes_inside_its_buffer_only(lib, name, k):
    """queries [q0, q0 + qc) only, every one of them answered by a per-query kernel: both index mean_out by self - q_begin.  The
    output has 64 guard floats in front and n - q_count + 64 behind (so that an index without - q_begin still lands inside the
    allocation); no guard bit may change."""
    xyz = _mixed()
    n = len(xyz)
    for q0, qc in ((1237, 7013), (n - 501, 501)):
        ctx = lib.Context(0)
        for pname, val in STAGES[name].items():
            ctx.set_param(pname, val)
        rows = ctx.alloc(xyz.nbytes).upload(xyz)
        buf = ctx.alloc(4 * (n + 2 * GUARD)).upload(np.full(n + 2 * GUARD, GUARD_BITS, np.uint32))
        info = ctx.sor_knn(rows.ptr, rows.ptr + 4, rows.ptr + 8, 3, n, q0, qc, k, buf.ptr + 4 * GUARD, algo=TREE, want_info=True)
        st = ctx.debug_tree()
        bits = buf.download(np.uint32, n + 2 * GUARD)
        rows.free()
        buf.free()
        ctx.close()
        check_counters(st, info, n, qc)
        assert st["fail_count"] == qc, show(st)
        assert (bits[:GUARD] == GUARD_BITS).all() and (bits[GUARD + qc:] == GUARD_BITS).all(), (q0, qc, show(st))
        got, ref = bits[GUARD:GUARD + qc].view(np.float32), _mixed_ref(k)[q0:q0 + qc]
        assert differ(got, ref) == 0, (q0, qc, explain(got, ref), show(st))


@pytest.mark.parametrize("name", FORCED)
def test_three_shares_under_forced_stages_sum_to_the_whole(lib, name):
    """gsx_sor_knn_share_dev, the pattern of test_knn_variants_gpu.test_three_shares_sum_to_the_whole: the shares (leaf ranges
    here) overwrite the whole output, are disjoint, cover every query, and their plain float32 sum is the reference; the queries
    whose mean IS zero must read +0.0 in every share"""
    xyz, k, nshares = _mixed(), 16, 3
    n = len(xyz)
    ref = _mixed_ref(k)
    nonzero = ref != 0
    assert int((~nonzero).sum()) == 41 + 148 + 801
    ctx = lib.Context(0)
    for pname, val in STAGES[name].items():
        ctx.set_param(pname, val)
    rows = ctx.alloc(xyz.nbytes).upload(xyz)
    out = ctx.alloc(4 * n)
    total = np.zeros(n, np.float32)
    owners = np.zeros(n, np.int32)
    sizes, stats = [], []
    for share in range(nshares):
        out.upload(np.full(n, np.nan, np.float32))   # the call must overwrite everything
        info = ctx.sor_knn_share(rows.ptr, rows.ptr + 4, rows.ptr + 8, 3, n, k, share, nshares, out.ptr, algo=TREE, want_info=True)
        st = ctx.debug_tree()
        check_counters(st, info, n, n)
        stats.append(show(st))
        got = out.download(np.float32, n)
        assert np.isfinite(got).all(), (share, stats)
        mine = got != 0
        assert not np.signbit(got[~mine]).any()   # +0.0, not -0.0
        owners += mine
        sizes.append(st["fail_count"])            # every query of the share's leaves went to the per-query kernels
        total = total + got
    rows.free()
    out.free()
    ctx.close()
    assert (owners[nonzero] == 1).all() and (owners[~nonzero] == 0).all(), (sizes, int((owners[nonzero] != 1).sum()))
    assert min(sizes) > 0 and sum(sizes) == n, (sizes, stats)
    assert differ(total, ref) == 0, (explain(total, ref), sizes, stats)


@pytest.mark.parametrize("name", sorted(STAGES))
def test_separate_columns_under_every_stage_setting(lib, name):
    xyz, k = _mixed(), 16
    got, info, st = run(lib, xyz, k, columns=True, **STAGES[name])
    assert differ(got, _mixed_ref(k)) == 0, (explain(got, _mixed_ref(k)), show(st))


# ---------------------------------------------------------------------------------------------------------------- the leaf partition
# tree_leaf_flags_kernel / tree_leaf_compact_kernel against the rule test_tree_leaf_rule pins in numpy.  A partition whose
# leaves are consistently larger or smaller than the rule's leaves every result exact, so the masks cannot pin it: the device's
# own sorted keys go through leaf_levels and the leaf starts must be the same.  n around the 1024-point tiles of the flag kernel:
# the window minimum of a point covers the `cap` entries before it, into the previous tile, and every entry compares a key with
# the one `cap` places on, into the next tile.  (A minimum cut at the tile edge is not of the harmless kind: neighbouring points
# then disagree about their leaf's level, and a few per cent of the distances come out wrong.)
PART_K = 16
PART_CAPS = [64, 65, 100, 128, 255, 256]


def _part_sizes(cap):
    return [n for n in (1, 65, 1023, 1024, 1025, 1024 + cap, 2048 + cap + 1, 5000) if n > PART_K]


PART_MATRIX = [pytest.param(cap, n, id="cap%d-n%d" % (cap, n)) for cap in PART_CAPS for n in _part_sizes(cap)]


@functools.lru_cache(maxsize=None)
def _clustered(n, seed):
    """a Gaussian blob (sigma = 1e-2 of the box), a uniform box of edge 10 and one point 300 times (n // 4 times in the smallest
    clouds): leaves of very different bit levels next to each other in the key order, and one fine cell holding more than any cap"""
    rng = np.random.default_rng(seed)
    ndup = min(300, n // 4)
    nblob = (n - ndup) // 2
    nbox = n - ndup - nblob
    blob = (np.float32(3.0) + rng.standard_normal((nblob, 3)) * 0.1).astype(np.float32)
    box = rng.random((nbox, 3), dtype=np.float32) * np.float32(10.0)
    dup = np.repeat(blob[:1] + np.float32(0.25), ndup, axis=0)
    xyz = np.concatenate([blob, box, dup])
    return np.ascontiguousarray(xyz[rng.permutation(n)]), ndup


def _leaves_by_the_rule(keys, cap):
    levels = leaf_levels(keys, cap, KEY_BITS)
    head = np.ones(len(keys), bool)
    head[1:] = [(int(keys[i]) >> int(levels[i])) != (int(keys[i - 1]) >> int(levels[i])) for i in range(1, len(keys))]
    return np.append(np.flatnonzero(head), len(keys)), levels


def check_partition(tree, cap, n):
    keys, starts = tree["keys"], tree["leafstart"]
    assert tree["leaf_cap"] == cap and len(keys) == n and len(starts) == tree["nleaves"] + 1
    assert (keys[1:] >= keys[:-1]).all()
    assert starts[0] == 0 and starts[-1] == n and (np.diff(starts) > 0).all(), starts
    want, levels = _leaves_by_the_rule(keys, cap)
    m = min(len(starts), len(want))
    assert np.array_equal(starts, want), ("leaves", len(starts) - 1, len(want) - 1, "first difference at leaf",
                                          np.flatnonzero(starts[:m] != want[:m])[:1], starts[:m][starts[:m] != want[:m]][:4], want[:m][starts[:m] != want[:m]][:4])
    sizes = np.diff(starts)
    overfull = [(int(s), int(e)) for s, e in zip(starts[:-1], starts[1:]) if e - s > cap]
    for s, e in overfull:
        assert keys[s] == keys[e - 1], (s, e)   # more than cap points in ONE fine cell
    return int(sizes.max()), overfull


@pytest.mark.parametrize("cap,n", PART_MATRIX)
def test_the_leaf_partition_is_the_rule_applied_to_the_devices_own_keys(lib, cap, n):
    xyz, ndup = _clustered(n, 7 * cap + n)
    ctx = lib.Context(0)
    try:
        got, info, _ = knn(lib, xyz, PART_K, ctx=ctx, algo=TREE, tree_leaf_cap=cap)
        tree = ctx.debug_tree(want_leaves=True)
    finally:
        ctx.close()
    check_counters(tree, info, n, n)
    ref = osor.mean_dists_ckdtree(xyz, PART_K)
    assert differ(got, ref) == 0, (explain(got, ref), show(tree))
    largest, overfull = check_partition(tree, cap, n)
    print("cap=%d n=%d: %d leaves, largest %d, over-full %s" % (cap, n, tree["nleaves"], largest, overfull))
    if ndup > cap:   # the copies are one leaf of their own, the only one above the capacity
        assert largest == ndup and len(overfull) == 1, (largest, overfull, ndup)
    else:
        assert largest <= cap and not overfull, (largest, overfull, ndup)
    assert tree["max_leaf"] == 0   # (the guard's counter: test_adaptive_modes_guard_reports_the_overfull_leaf)


def test_adaptive_modes_guard_reports_the_overfull_leaf(lib):
    """max_leaf is the guard's: only adaptive mode, which must know whether the key resolution is exhausted, runs that pass"""
    n, cap = 5000, 64
    xyz, ndup = _clustered(n, 11)
    ctx = lib.Context(0)
    try:
        ctx.set_param("adaptive", 1)
        got, info, _ = knn(lib, xyz, PART_K, ctx=ctx, algo=lib.KNN_AUTO, tree_leaf_cap=cap)
        assert info["algo"] == TREE, info   # half of the points in one blob: an uneven histogram
        tree = ctx.debug_tree(want_leaves=True)
    finally:
        ctx.close()
    ref = osor.mean_dists_ckdtree(xyz, PART_K)
    assert differ(got, ref) == 0, (explain(got, ref), show(tree))
    largest, overfull = check_partition(tree, cap, n)
    assert largest == ndup == 300 and tree["max_leaf"] == largest, (largest, tree["max_leaf"])


def test_the_debug_entry_point_refuses_what_it_cannot_answer(lib):
    ctx = lib.Context(0)
    try:
        with pytest.raises(lib.GsxError, match="no tree KNN call"):
            ctx.debug_tree()
        xyz = _clustered(1025, 3)[0]
        knn(lib, xyz, PART_K, ctx=ctx, algo=TREE)
        with pytest.raises(lib.GsxError, match="too small"):
            ctx.debug_tree(want_leaves=True, cap=1024)
        assert len(ctx.debug_tree(want_leaves=True, cap=1025)["keys"]) == 1025
    finally:
        ctx.close()
