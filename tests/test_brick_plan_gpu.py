"""-m gpu: knn_brick on planned bricks (context parameter brick_plan): runs of quarter-cell slabs of a 2x2
bundle of query rows, cut so that a batch holds as many queries as fit below 64.  Every comparison is bit for bit on the mean
distances: against cKDTree and against the same call on the fixed 2x2x2-cell bricks (brick_plan = 0)."""
import functools
import importlib.util
import os

import numpy as np
import pytest

from knn_device import GRID, differ as _differ, explain as _explain, knn as _knn
from oracle import datasets, sor as osor

pytestmark = pytest.mark.gpu

MAXQ, MAXRUN = 64, 10   # queries / quarter-slabs of a planned brick (csrc/sor_grid.hip: PLAN_MAXQ, PLAN_MAXRUN)
MAX_DIM = 1024          # cells per axis; planned bricks need 4 nx <= MAX_DIM (csrc/sor_grid.hip: grid_params)


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


# ---------------------------------------------------------------- the withdrawn plan
# Two places on the device clear gp->plan after the host has asked for planned bricks: grid_params when the grid is wider than
# 256 cells (4 nx > MAX_DIM), and brick_plan_kernel's last workgroup when the cut gives more runs than the list holds
# (n / 16 + 4096).  knn_brick<PLAN> then reads the fixed 2x2x2 bricks as the aligned runs [8 bx, 8 bx + 7] out of fine_start.

def _both(lib, xyz, k, ref, **params):
    """the call with brick_plan = 1 and = 0, both compared with `ref` -> (info, plan, info of the fixed bricks)"""
    on, info, plan = _knn(lib, xyz, k, want_plan=True, **params)
    off, info0, plan0 = _knn(lib, xyz, k, want_plan=True, **dict(params, brick_plan=0))
    assert plan0["plan"] == 0, plan0["plan"]
    print("nx=%d ny=%d nz=%d plan=%d: %d bricks against %d fixed, %d / %d fallback queries" % (
        plan["nx"], plan["ny"], plan["nz"], plan["plan"], info["n_bricks"], info0["n_bricks"], info["n_fallback"], info0["n_fallback"]))
    assert _differ(on, off) == 0, (_explain(on, off), info, info0)
    assert _differ(on, ref) == 0, (_explain(on, ref), info)
    return info, plan, info0


@functools.lru_cache(maxsize=None)
def _corridor():
    """24 000 uniform points in a 300 x 1 x 1 box: the cell edge is ~0.45 at k = 16, the grid ~670 x 3 x 3 cells"""
    return np.ascontiguousarray(datasets.uniform(24000, 10.0, 37) * np.array([30.0, 0.1, 0.1], np.float32))


@functools.lru_cache(maxsize=None)
def _corridor_ref(k):
    return osor.mean_dists_ckdtree(_corridor(), k)


@pytest.mark.parametrize("k", [16, 8])
def test_a_grid_wider_than_256_cells_keeps_the_fixed_bricks(lib, k):
    xyz = _corridor()
    info, plan, info0 = _both(lib, xyz, k, _corridor_ref(k))
    assert 256 < plan["nx"] <= MAX_DIM and plan["plan"] == 0, plan
    assert info["n_bricks"] == info0["n_bricks"] > 0, (info, info0)   # numbered as ever
    assert info["n_fallback"] <= len(xyz) // 2, info                   # ... and searched by knn_brick, not by the ring kernels


@pytest.mark.parametrize("nx", [256, 257])
def test_the_widest_planned_grid_and_the_first_one_too_wide(lib, nx):
    """the lattice of test_points_exactly_on_quarter_boundaries, 4 x 4 cells across: cells of edge exactly 2, the last lattice
    plane along x in a cell of its own.  256 cells are 1024 quarters, the most the plan takes; 257 are one too many"""
    gx = np.arange(4 * (nx - 1) + 1, dtype=np.float32) * np.float32(0.5)   # 0 ... 2 (nx - 1)
    gyz = np.arange(4, dtype=np.float32) * np.float32(2.0)
    xyz = np.stack(np.meshgrid(gx, gyz, gyz, indexing="ij"), -1).reshape(-1, 3).copy()
    n, k = len(xyz), 4
    ppc = 8.0 * n / (2.0 * (nx - 1) * 6.0 * 6.0)   # cell edge exactly 2: (volume * ppc / n) ** (1 / 3)
    info, plan, info0 = _both(lib, xyz, k, osor.mean_dists_ckdtree(xyz, k), grid_points_per_cell=ppc)
    assert plan["origin"][3] == np.float32(0.5) and (plan["nx"], plan["ny"], plan["nz"]) == (nx, 4, 4), plan
    assert plan["plan"] == (1 if 4 * nx <= MAX_DIM else 0), plan
    if plan["plan"] == 0:
        assert info["n_bricks"] == info0["n_bricks"] == ((nx + 1) // 2) * 2 * 2, (info, info0)
    else:
        assert info["n_bricks"] == len(plan["runs"]) > 0


def _count_runs(xyz, plan):
    """brick_plan's greedy cut restated: the number of runs of the grid `plan` describes, from the device's own f32 quarter
    and cell indices (as in test_plan_invariants)"""
    nx, ny, nz = plan["nx"], plan["ny"], plan["nz"]
    ox, oy, oz, inv_h = plan["origin"]
    nq4, nby, nbz = 4 * nx, (ny + 1) // 2, (nz + 1) // 2
    q4 = np.minimum(((xyz[:, 0] - ox) * (np.float32(4.0) * inv_h)).astype(np.int64), nq4 - 1)
    cy = np.minimum(((xyz[:, 1] - oy) * inv_h).astype(np.int64), ny - 1)
    cz = np.minimum(((xyz[:, 2] - oz) * inv_h).astype(np.int64), nz - 1)
    cnt = np.zeros((nby * nbz, nq4), np.int64)
    np.add.at(cnt, ((cz // 2) * nby + cy // 2, q4), 1)
    csum = np.concatenate([np.zeros((nby * nbz, 1), np.int64), np.cumsum(cnt, axis=1)], axis=1).tolist()
    runs = 0
    for S in csum:
        s = 0
        while s < nq4:
            e = s + 1
            while e < nq4 and e - s < MAXRUN and S[e + 1] - S[s] <= MAXQ:
                e += 1
            s = e
            runs += 1
    return runs


@functools.lru_cache(maxsize=None)
def _wires():
    """A cloud whose cut has more runs than the list holds.  A run ends after 10 quarter-slabs or before its 65th query, and the
    grid has at most n / 2 cells = n / 2 quarter-slabs of bundles, so n / 20 runs come from length and n / 32 from fill at the
    very most: above n / 16 + 4096 only for a cloud built for it, and only from some 300 000 points on.  This one has 460 800
    points in a box of 64 x 60 x 60 cells of edge 1 (two points per cell, the fewest the grid allows): 54 cell rows along x,
    each in a bundle of its own, hold 33 points in every quarter-slab -- two neighbouring slabs never fit one run, 256 runs per
    row -- and the other 846 bundles are all but empty, 26 runs each: 54 * 256 + 846 * 26 = 35 820 > 460 800 / 16 + 4096 = 32 896.
    The 4606 points left over are spread over the box (far from everything: ring queries), two of them in its corners."""
    rng = np.random.default_rng(77)
    n, nx, nyz = 460800, 64, 60
    bundles = rng.choice((nyz // 2) ** 2, 54, replace=False)
    cy = 2 * (bundles % (nyz // 2)) + rng.integers(0, 2, 54)
    cz = 2 * (bundles // (nyz // 2)) + rng.integers(0, 2, 54)
    u = 0.05 + 0.9 * rng.random((54, 4 * nx, 33, 3))     # well inside the slab: no index depends on a rounding
    x = (np.arange(4 * nx)[None, :, None] + u[..., 0]) * 0.25
    y = cy[:, None, None] + u[..., 1]
    z = cz[:, None, None] + u[..., 2]
    wires = np.stack([x, y, z], -1).reshape(-1, 3)
    rest = n - len(wires) - 2
    far = np.array([63.99, 59.99, 59.99])
    spread = rng.random((rest, 3)) * far
    xyz = np.concatenate([wires, spread, np.zeros((1, 3)), far[None, :]]).astype(np.float32)
    assert len(xyz) == n
    return np.ascontiguousarray(xyz[rng.permutation(n)])


def _wires_ppc():
    xyz = _wires()
    e = xyz.max(0).astype(np.float64) - xyz.min(0).astype(np.float64)
    return len(xyz) / float(np.prod(e))   # cell edge 1: (volume * ppc / n) ** (1 / 3)


@functools.lru_cache(maxsize=None)
def _wires_ref():
    return osor.mean_dists_ckdtree(_wires(), 8)


def test_a_cut_with_more_runs_than_the_list_holds_keeps_the_fixed_bricks(lib):
    xyz, k = _wires(), 8
    n = len(xyz)
    info, plan, info0 = _both(lib, xyz, k, _wires_ref(), grid_points_per_cell=_wires_ppc())
    assert (plan["nx"], plan["ny"], plan["nz"]) == (64, 60, 60) and plan["origin"][3] == np.float32(1.0), plan
    runs = _count_runs(xyz, plan)
    print("%d runs for a list of %d" % (runs, n // 16 + 4096))
    assert runs > n // 16 + 4096          # the cloud does what it was built for ...
    assert plan["plan"] == 0              # ... although nx = 64 allowed the plan and brick_plan = 1 asked for it
    assert info["n_bricks"] == info0["n_bricks"] == 32 * 30 * 30, (info, info0)


def test_one_point_per_cell_asked_for_still_fits_the_list(lib):
    """grid_points_per_cell = 1 on a uniform cloud: the grid's cell budget (n / 2) stretches the cells until they hold more than
    two points, ten quarter-slabs of a bundle hold ~23 queries, and the runs are cut by length: about a tenth of the cells"""
    n, k = 205700, 8
    xyz = _uniform(n)
    info, plan, _ = _both(lib, xyz, k, _uniform_ref(n, k), grid_points_per_cell=1.0)
    assert plan["nx"] * plan["ny"] * plan["nz"] <= n // 2 + 64, plan
    runs = _count_runs(xyz, plan)
    assert runs <= n // 16 + 4096, runs
    assert plan["plan"] == 1 and info["n_bricks"] == len(plan["runs"]) == runs, (info, runs)


def test_a_context_is_reusable_after_a_withdrawal(lib):
    """ticket_plan, gp->plan, the brick count and the reserved lists carry nothing from call to call: withdrawn (overflow),
    planned, withdrawn (wide grid), withdrawn (overflow) and planned again on ONE context"""
    ctx = lib.Context(0)
    n = 32568
    auto = {"grid_points_per_cell": 0.0}
    steps = [("wires", _wires(), 8, _wires_ref, {"grid_points_per_cell": _wires_ppc()}, 0),
             ("uniform", _uniform(n), 16, lambda: _uniform_ref(n, 16), auto, 1),
             ("corridor", _corridor(), 16, lambda: _corridor_ref(16), auto, 0),
             ("wires", _wires(), 8, _wires_ref, {"grid_points_per_cell": _wires_ppc()}, 0),
             ("uniform", _uniform(n), 16, lambda: _uniform_ref(n, 16), auto, 1)]
    bricks = {}
    for name, xyz, k, ref, params, want in steps:
        got, info, plan = _knn(lib, xyz, k, want_plan=True, ctx=ctx, **params)
        assert plan["plan"] == want, (name, plan["plan"])
        assert _differ(got, ref()) == 0, (name, _explain(got, ref()), info)
        assert info["n_bricks"] == (len(plan["runs"]) if want else ((plan["nx"] + 1) // 2) * ((plan["ny"] + 1) // 2) * ((plan["nz"] + 1) // 2)), (name, info)
        assert bricks.setdefault(name, info["n_bricks"]) == info["n_bricks"], (name, bricks, info)   # the same list every time
    ctx.close()


@pytest.mark.parametrize("k", [1, 3, 7, 9, 12, 13])
def test_planned_bricks_at_the_other_capacities(lib, k):
    """k < 8 (the sequential mean), capacity 13 (k = 9 ... 12) and the first k of capacity 17; the tests above use 4, 8 and 16"""
    n = 32568
    info, plan, _ = _both(lib, _uniform(n), k, _uniform_ref(n, k))
    assert plan["plan"] == 1 and info["n_bricks"] == len(plan["runs"]) > 0, (plan["plan"], info)


@pytest.mark.parametrize("params,window", [({"filter_mfma": 0}, None), ({"phase2_net": 0}, None), ({}, (4001, 20011))],
                         ids=["filter_mfma=0", "phase2_net=0", "query-window"])
def test_switches_that_turn_the_plan_off(lib, params, window):
    """planned bricks exist for the MFMA + network kernels and for calls whose queries are the whole cloud"""
    n, k = 32568, 16
    xyz = _uniform(n)
    q0, qc = window if window else (0, n)
    got, info, plan = _knn(lib, xyz, k, want_plan=True, window=window, brick_plan=1, **params)
    assert plan["plan"] == 0, plan["plan"]
    ref = _uniform_ref(n, k)[q0:q0 + qc]
    assert _differ(got, ref) == 0, (_explain(got, ref), info)
    off, info0, _ = _knn(lib, xyz, k, window=window, **dict(params, brick_plan=0))
    assert _differ(got, off) == 0 and info["n_bricks"] == info0["n_bricks"], (info, info0)
