"""-m gpu: knn_brick on planned bricks (context parameter brick_plan): runs of quarter-cell slabs of a 2x2
bundle of query rows, cut so that a batch holds as many queries as fit below 64.  Every comparison is bit for bit on the mean
distances: against cKDTree and against the same call on the fixed 2x2x2-cell bricks (brick_plan = 0)."""
import functools
import importlib.util
import os

import numpy as np
import pytest

from oracle import datasets, sor as osor

pytestmark = pytest.mark.gpu

GRID = 2
MAXQ, MAXRUN = 64, 10   # queries / quarter-slabs of a planned brick (csrc/sor_grid.hip: PLAN_MAXQ, PLAN_MAXRUN)


@pytest.fixture(scope="module")
def lib(gsx):
    gsx._lib.require_hip()
    return gsx._lib


@functools.lru_cache(maxsize=None)
def _uniform(n):
    return datasets.uniform(n, 10.0, 31)


@functools.lru_cache(maxsize=None)
def _uniform_ref(n, k):
    return osor.mean_dists_ckdtree(_uniform(n), k)


def _differ(a, b):
    return int(np.count_nonzero(a.view(np.uint32) != b.view(np.uint32)))


def _knn(lib, xyz, k, want_plan=False, **params):
    """one gsx_sor_knn_dev call on a fresh context -> (mean distances, info, brick plan or None)"""
    n = len(xyz)
    ctx = lib.Context(0)
    for name, val in params.items():
        ctx.set_param(name, val)
    rows = ctx.alloc(xyz.nbytes).upload(np.ascontiguousarray(xyz))
    out = ctx.alloc(4 * n)
    info = ctx.sor_knn(rows.ptr, rows.ptr + 4, rows.ptr + 8, 3, n, 0, n, k, out.ptr, algo=GRID, want_info=True)
    got = out.download(np.float32, n)
    plan = ctx.debug_brick_plan() if want_plan else None
    rows.free()
    out.free()
    ctx.close()
    return got, info, plan


# sizes whose nx is odd and whose 4 nx is no multiple of 10 (asserted below): the last run of a bundle is short and the
# candidate rows are clamped at the grid's edge.  (points per cell: 7.25 at k = 16, 4.23 at k = 8)
@pytest.mark.parametrize("n,k,nx", [(32568, 16, 17), (26784, 8, 19), (205700, 16, 31), (205700, 8, 37)])
def test_uniform_clouds_match_ckdtree_and_the_fixed_bricks(lib, n, k, nx):
    xyz = _uniform(n)
    on, info, plan = _knn(lib, xyz, k, want_plan=True)
    off, info0, plan0 = _knn(lib, xyz, k, want_plan=True, brick_plan=0)
    assert plan["plan"] == 1 and plan0["plan"] == 0, (plan["plan"], plan0["plan"])
    assert plan["nx"] == nx and nx % 2 == 1 and (4 * nx) % 10 != 0, plan["nx"]
    assert info["n_bricks"] == len(plan["runs"]) > 0
    print("n=%d k=%d: %d planned bricks against %d fixed, %d / %d fallback queries" % (
        n, k, info["n_bricks"], info0["n_bricks"], info["n_fallback"], info0["n_fallback"]))
    assert _differ(on, off) == 0
    assert _differ(on, _uniform_ref(n, k)) == 0


def test_plan_invariants(lib):
    """the runs of every bundle tile [0, 4 nx) without gap or overlap, none is longer than the cap, none holds more than 64
    queries unless it is a single quarter-slab -- and each is maximal (the cut is greedy, hence the same on every run)"""
    n, k = 205700, 16
    xyz = _uniform(n)
    _, info, plan = _knn(lib, xyz, k, want_plan=True)
    assert plan["plan"] == 1
    nx, ny, nz = plan["nx"], plan["ny"], plan["nz"]
    ox, oy, oz, inv_h = plan["origin"]
    nq4, nby, nbz = 4 * nx, (ny + 1) // 2, (nz + 1) // 2
    # the device's own f32 arithmetic
    q4 = np.minimum(((xyz[:, 0] - ox) * (np.float32(4.0) * inv_h)).astype(np.int64), nq4 - 1)
    cy = np.minimum(((xyz[:, 1] - oy) * inv_h).astype(np.int64), ny - 1)
    cz = np.minimum(((xyz[:, 2] - oz) * inv_h).astype(np.int64), nz - 1)
    cnt = np.zeros((nby * nbz, nq4), np.int64)
    np.add.at(cnt, ((cz // 2) * nby + cy // 2, q4), 1)
    csum = np.concatenate([np.zeros((nby * nbz, 1), np.int64), np.cumsum(cnt, axis=1)], axis=1)
    runs = plan["runs"]
    b, first, last = runs[:, 0], runs[:, 1], runs[:, 2]
    assert np.all(np.diff(b) >= 0) and b[0] == 0 and b[-1] == nby * nbz - 1 and len(np.unique(b)) == nby * nbz
    new = np.concatenate([[True], np.diff(b) > 0])
    assert np.all(first[new] == 0)
    assert np.all(first[1:][~new[1:]] == last[:-1][~new[1:]] + 1)     # no gap, no overlap
    assert np.all(last[np.concatenate([new[1:], [True]])] == nq4 - 1)
    assert np.all(last >= first) and np.all(last - first + 1 <= MAXRUN)
    q = csum[b, last + 1] - csum[b, first]
    assert int(q.sum()) == n
    assert np.all((q <= MAXQ) | (last == first))
    more = last + 1 < nq4   # maximal: the next quarter would not have fitted
    nxt = csum[b[more], last[more] + 2] - csum[b[more], first[more]]
    assert np.all((nxt > MAXQ) | (last[more] - first[more] + 1 == MAXRUN))
    print("%d runs, mean fill %.1f queries, mean length %.2f quarters" % (len(runs), q.mean(), (last - first + 1).mean()))


def test_points_exactly_on_quarter_boundaries(lib):
    """a lattice of spacing 1/2 along x in cells of edge 2: every point sits exactly on a quarter-slab boundary (ties in the
    quarter index), every neighbour shell is a tie"""
    gx = np.arange(93, dtype=np.float32) * np.float32(0.5)
    gyz = np.arange(24, dtype=np.float32) * np.float32(2.0)
    xyz = np.stack(np.meshgrid(gx, gyz, gyz, indexing="ij"), -1).reshape(-1, 3).copy()
    n, k = len(xyz), 4
    ppc = 8.0 * n / 46.0 ** 3   # cell edge exactly 2
    on, info, plan = _knn(lib, xyz, k, want_plan=True, grid_points_per_cell=ppc)
    off, _, _ = _knn(lib, xyz, k, grid_points_per_cell=ppc, brick_plan=0)
    assert plan["plan"] == 1 and plan["origin"][3] == np.float32(0.5) and plan["nx"] == 24, plan
    assert info["n_fallback"] < n // 2, info   # most queries are certified by knn_brick itself
    assert _differ(on, off) == 0
    assert _differ(on, osor.mean_dists_ckdtree(xyz, k)) == 0


def test_a_quarter_slab_of_a_thousand_duplicates_takes_the_multi_batch_path(lib):
    xyz = _uniform(32568).copy()
    xyz[:1000] = xyz[5000]
    k = 16
    on, info, plan = _knn(lib, xyz, k, want_plan=True)
    off, _, _ = _knn(lib, xyz, k, brick_plan=0)
    assert plan["plan"] == 1
    runs = plan["runs"]
    assert np.any(runs[:, 1] == runs[:, 2])   # the slab of the duplicates is a run of its own
    assert _differ(on, off) == 0
    assert _differ(on, osor.mean_dists_ckdtree(xyz, k)) == 0


def test_rim_queries_of_a_planar_cloud(lib):
    """the planar cloud of test_rim_queries_of_later_batches_are_not_certified_beyond_one_cell at k = 16 on planned bricks:
    along x the faces of the searched box sit at quarter positions, and the widened radius must stop at them"""
    spec = importlib.util.spec_from_file_location("fuzz_parity", os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                                              "devtools", "fuzz_parity.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    rng = np.random.default_rng(11)
    for _ in range(7):
        kind, xyz, _k = fz.make(rng)
    n, k = len(xyz), 16
    assert (kind, n) == ("plane", 256484)
    ref = osor.mean_dists_ckdtree(xyz, k)
    ctx = lib.Context(0)
    rows = ctx.alloc(xyz.nbytes).upload(xyz)
    out = ctx.alloc(4 * n)
    for rep in range(4):   # the order inside a cell varies from run to run
        ctx.sor_knn(rows.ptr, rows.ptr + 4, rows.ptr + 8, 3, n, 0, n, k, out.ptr, algo=GRID)
        assert _differ(out.download(np.float32, n), ref) == 0, rep
    assert ctx.debug_brick_plan(cap=16)["plan"] == 1
    rows.free()
    out.free()
    ctx.close()


def test_k32_and_adaptive_calls_keep_the_fixed_bricks(lib):
    n = 32568
    xyz = _uniform(n)
    on, _, plan = _knn(lib, xyz, 32, want_plan=True)
    off, _, _ = _knn(lib, xyz, 32, brick_plan=0)
    assert plan["plan"] == 0   # 2x2x1-cell bricks: not planned
    assert _differ(on, off) == 0
    assert _differ(on, _uniform_ref(n, 32)) == 0
    # adaptive mode on a cloud whose bricks ARE deferred to a finer level (grid refinement, tree = 0)
    small = datasets.scene_with_floaters(30_000, 4)
    ref = osor.mean_dists_ckdtree(small, 16)
    on, info, plan = _knn(lib, small, 16, want_plan=True, adaptive=1, tree=0)
    off, info0, _ = _knn(lib, small, 16, adaptive=1, tree=0, brick_plan=0)
    assert plan["plan"] == 0 and info["n_deferred_bricks"] > 0 and info["n_bricks"] == info0["n_bricks"], (info, info0)
    assert _differ(on, off) == 0
    assert _differ(on, ref) == 0
