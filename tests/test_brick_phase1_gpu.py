"""-m gpu: phase 1 of knn_brick, the MFMA filter over the candidate words (csrc/knn_mfma.h, the MF branch of knn_brick_kernel in
csrc/sor_grid.hip), on the smallest clouds that reach each path of its word loop; knn_leaf shares the operand builders.

Every case asserts two things.  The mean distances are the same 32 bits as cKDTree's.  And n_fallback, the number of queries
knn_brick did not certify itself, is what the SCALAR filter (filter_mfma = 0) leaves on the same bricks: acceptance is decided by
the exact k-th distance, so it cannot depend on the filter as long as the filter is a superset -- a candidate the matrix-core
filter dropped shows up as a larger count, or as a wrong value.  filter_mfma = 0 also withdraws the brick plan (planned bricks
exist for the MFMA kernels only, test_brick_plan_gpu.test_switches_that_turn_the_plan_off), and the widened radius of the rim
queries depends on where the bricks are cut; so a PLANNED call is compared with the count the parent of the commit that
introduced this file returned for the same call (recorded below, measured on an MI355X: the plan is a greedy cut, the same on
every run), and with the scalar filter wherever both calls run the same bricks.
A uniform cloud must certify at least half of its queries in knn_brick: the ring kernels answer whatever is left, and would
hide a filter that passes nothing (test_knn_variants_gpu measures the share at 0.0245 for these 8 000 points at k = 16)."""
import functools

import numpy as np
import pytest

from knn_device import differ, explain, knn
from oracle import datasets, sor as osor

pytestmark = pytest.mark.gpu

MAXRUN = 10   # quarter-slabs of a planned brick (csrc/sor_grid.hip: PLAN_MAXRUN)
TREE = 3

# n_fallback of the planned calls, from the parent's library (see above); key = the case's id
PLANNED_PARENT = {
    "uniform-k8": 26,          # (the fixed bricks: 28)
    "uniform-k16": 184,        # (196)
    "few-candidates": 17,      # (16)
    "slab-removed-k8": 2,      # (2)
    "slab-removed-k16": 60,    # (59)
    "widest-frame": 3,         # (2)
    "rim-bricks": 188,         # (182)
    "duplicates": 367,         # (378)
}


@pytest.fixture(scope="module")
def lib(gsx):
    gsx._lib.require_hip()
    return gsx._lib


@functools.lru_cache(maxsize=None)
def _ref(name, k):
    return osor.mean_dists_ckdtree(CLOUDS[name](), k)


def _check(lib, case, name, k, plan_on, **params):
    """the call with filter_mfma = 1 and = 0, both bit-equal to cKDTree -> (info, plan, info of the scalar filter)"""
    xyz, ref = CLOUDS[name](), _ref(name, k)
    n = len(xyz)
    got, info, plan = knn(lib, xyz, k, want_plan=True, brick_plan=plan_on, **params)
    sc, info0, plan0 = knn(lib, xyz, k, want_plan=True, brick_plan=plan_on, filter_mfma=0, **params)
    print("%s n=%d k=%d brick_plan=%d: plan %d / %d, %d bricks / %d, n_fallback %d (MFMA filter) / %d (scalar filter), parent %s" % (
        case, n, k, plan_on, plan["plan"], plan0["plan"], info["n_bricks"], info0["n_bricks"], info["n_fallback"],
        info0["n_fallback"], PLANNED_PARENT.get(case)))
    assert differ(got, ref) == 0, (explain(got, ref), info)
    assert differ(sc, ref) == 0, (explain(sc, ref), info0)
    assert plan0["plan"] == 0, plan0["plan"]
    assert info["n_bricks"] > 0
    if plan["plan"] == 0:
        assert info["n_bricks"] == info0["n_bricks"], (info, info0)
        assert info["n_fallback"] == info0["n_fallback"], (info, info0)
    else:
        assert info["n_fallback"] == PLANNED_PARENT[case], (info, PLANNED_PARENT[case])
    return info, plan, info0


# ---------------------------------------------------------------- the clouds
def _uniform8k():
    return datasets.uniform(8000, 10.0, 43)


def _few():
    return datasets.uniform(300, 10.0, 43)


def _slab_removed():
    """the 8 000 points without the middle third of the box along z: empty candidate rows, batches with lanes without a query"""
    xyz = _uniform8k()
    lo, hi = 10.0 / 3.0, 20.0 / 3.0
    return np.ascontiguousarray(xyz[(xyz[:, 2] < lo) | (xyz[:, 2] >= hi)])


def _widest():
    """A lattice of spacing 1/2 along x in cells of edge exactly 2, 256 cells = 1024 quarter-slabs long (the most the plan
    takes), 4 x 4 cells across.  The first bundle of cell rows (y in {0, 1.5, 3}, z in {0, 2}) holds six points per quarter-slab,
    so its runs are cut by length, 10 quarters = 60 queries, and with the cell either side the candidates reach |u_x| = 2.25
    from the frame's centre; the other three bundles hold three, two and one (3.1 points per cell overall: 2x2x2-cell bricks).
    One more row of points along x sits just inside the two ends of every run of the first bundle."""
    nx = 256
    gx = np.arange(4 * (nx - 1) + 1, dtype=np.float32) * np.float32(0.5)
    gy = np.array([0.0, 1.5, 3.0, 6.0], np.float32)
    gz = np.array([0.0, 2.0, 6.0], np.float32)
    xyz = np.stack(np.meshgrid(gx, gy, gz, indexing="ij"), -1).reshape(-1, 3)
    starts = np.arange(0.0, 2.0 * (nx - 1) - 5.0, 5.0, dtype=np.float32)   # a run of 10 quarters is 5 long
    ends = np.stack([np.concatenate([starts + np.float32(0.01), starts + np.float32(4.99)]),
                     np.full(2 * len(starts), 0.75, np.float32), np.full(2 * len(starts), 1.0, np.float32)], 1)
    return np.ascontiguousarray(np.concatenate([xyz, ends]).astype(np.float32))


def _widest_ppc():
    xyz = _widest()
    return 8.0 * len(xyz) / (2.0 * 255 * 6.0 * 6.0)   # cell edge exactly 2: (volume * ppc / n) ** (1 / 3)


def _rim():
    """12 x 12 x 12 cells at k = 16: most bricks touch the grid's boundary, the filter bound differs from lane to lane"""
    return datasets.uniform(11000, 10.0, 47)


def _duplicates():
    """a thousand copies of one point in one quarter-slab: more candidate words than the LDS park holds (WCAP), the batch takes
    the scalar filter"""
    xyz = _uniform8k().copy()
    xyz[:1000] = xyz[5000]
    return xyz


def _corridor():
    """24 000 uniform points in a 300 x 1 x 1 box: the grid is wider than 256 cells, the plan is withdrawn on the device and
    knn_brick<PLAN> runs the fixed bricks"""
    return np.ascontiguousarray(datasets.uniform(24000, 10.0, 37) * np.array([30.0, 0.1, 0.1], np.float32))


CLOUDS = {"uniform": _uniform8k, "few": _few, "slab": _slab_removed, "widest": _widest, "rim": _rim, "dup": _duplicates,
          "corridor": _corridor}
for _name in list(CLOUDS):
    CLOUDS[_name] = functools.lru_cache(maxsize=None)(CLOUDS[_name])


# ---------------------------------------------------------------- the cases
@pytest.mark.parametrize("plan_on", [1, 0])
@pytest.mark.parametrize("k", [8, 16])
def test_two_segment_and_partial_words(lib, k, plan_on):
    info, plan, _ = _check(lib, "uniform-k%d" % k, "uniform", k, plan_on)
    assert plan["plan"] == plan_on
    assert info["n_fallback"] <= 8000 // 2, info


@pytest.mark.parametrize("plan_on", [1, 0])
def test_fewer_than_32_candidates_in_a_batch(lib, plan_on):
    info, plan, _ = _check(lib, "few-candidates", "few", 8, plan_on)
    assert info["n_fallback"] <= 300 // 2, info


@pytest.mark.parametrize("plan_on", [1, 0])
@pytest.mark.parametrize("k", [8, 16])
def test_empty_rows_and_lanes_without_a_query(lib, k, plan_on):
    n = len(CLOUDS["slab"]())
    assert 5200 <= n <= 5450, n
    info, plan, _ = _check(lib, "slab-removed-k%d" % k, "slab", k, plan_on)
    assert info["n_fallback"] <= n // 2, info


def test_the_frame_at_its_widest(lib):
    info, plan, _ = _check(lib, "widest-frame", "widest", 4, 1, grid_points_per_cell=_widest_ppc())
    assert plan["plan"] == 1 and plan["origin"][3] == np.float32(0.5) and (plan["nx"], plan["ny"], plan["nz"]) == (256, 4, 4), plan
    runs = plan["runs"]
    assert int((runs[:, 2] - runs[:, 1] + 1).max()) == MAXRUN   # runs cut by length: the frame spans 2.5 cells + one either side
    assert info["n_fallback"] <= len(CLOUDS["widest"]()) // 2, info


@pytest.mark.parametrize("plan_on", [1, 0])
def test_rim_bricks(lib, plan_on):
    info, plan, _ = _check(lib, "rim-bricks", "rim", 16, plan_on)
    assert (plan["nx"], plan["ny"], plan["nz"]) == (12, 12, 12), plan
    assert info["n_fallback"] <= 11000 // 2, info


def test_more_words_than_the_park_holds(lib):
    info, plan, _ = _check(lib, "duplicates", "dup", 16, 1)
    assert plan["plan"] == 1
    runs = plan["runs"]
    assert np.any(runs[:, 1] == runs[:, 2])   # the slab of the duplicates is a run of its own


def test_the_withdrawn_plan(lib):
    info, plan, info0 = _check(lib, "corridor", "corridor", 16, 1)
    assert plan["nx"] > 256 and plan["plan"] == 0, plan
    assert info["n_fallback"] <= 24000 // 2, info


def test_knn_leaf_on_six_blobs(lib):
    """adaptive mode sends the six Gaussian blobs (peak densities 27 000 : 1) to the Morton tree: knn_leaf builds its candidate
    operands with the same functions"""
    xyz = datasets.clustered(20000, 5)
    res = lib.sor_filter(xyz, 16, 1.0, want_info=True)
    assert res["info"]["algo"] == TREE, res["info"]
    ref = osor.mean_dists_ckdtree(xyz, 16)
    assert differ(res["mean_dists"], ref) == 0, (explain(res["mean_dists"], ref), res["info"])
