"""-m gpu: the work queue of the KNN kernels (csrc/sor_grid_params.h) at item counts below, near and far above
the number of waves, on even and uneven clouds.  Every call writes into an output filled with NaN, so an item nobody took
shows; the mean distances are compared bit for bit with cKDTree, and the final tail counters of every group are checked
through the debug entry point: at least the tail length, at most the tail length + 8 x the waves of the launch."""
import functools

import numpy as np
import pytest

from knn_device import GRID, differ as _differ, explain as _explain
from oracle import datasets, sor as osor
from test_work_queue_host import WAVES_PER_BLOCK, wq_range

pytestmark = pytest.mark.gpu

TREE = 3


@pytest.fixture(scope="module")
def lib(gsx):
    gsx._lib.require_hip()
    return gsx._lib


def _dense_half(n):
    """the upper z half of the box holds three times as many points as the lower: the groups' item ranges are slabs along z
    (bricks are numbered z-major), so the groups of the upper half have the longer items"""
    rng = np.random.default_rng(41)
    xyz = rng.random((n, 3), dtype=np.float32) * np.float32(10.0)
    lower = np.arange(n) < n // 4
    xyz[:, 2] = np.where(lower, xyz[:, 2] * np.float32(0.5), np.float32(5.0) + xyz[:, 2] * np.float32(0.5))
    return xyz[rng.permutation(n)]


@functools.lru_cache(maxsize=None)
def _cloud(name):
    if name == "uniform3k":
        return datasets.uniform(3000, 10.0, 5)
    if name == "uniform200k":
        return datasets.uniform(200000, 10.0, 6)
    if name == "densehalf120k":
        return _dense_half(120000)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _ref(name, k):
    return osor.mean_dists_ckdtree(_cloud(name), k)


def _call(lib, xyz, k, algo=GRID, **params):
    """one gsx_sor_knn_dev call into a NaN-filled output -> (mean distances, info, work queues of the grid path or None)"""
    n = len(xyz)
    ctx = lib.Context(0)
    for name, val in params.items():
        ctx.set_param(name, val)
    buf = ctx.alloc(xyz.nbytes).upload(np.ascontiguousarray(xyz))
    out = ctx.alloc(4 * n).upload(np.full(n, np.nan, np.float32))
    info = ctx.sor_knn(buf.ptr, buf.ptr + 4, buf.ptr + 8, 3, n, 0, n, k, out.ptr, algo=algo, want_info=True)
    got = out.download(np.float32, n)
    wq = ctx.debug_work_queue() if info["algo"] == GRID else None
    buf.free()
    out.free()
    ctx.close()
    return got, info, wq


def _check_counters(wq):
    for name, q in wq.items():
        n, blocks = q["items"], q["blocks"]
        if blocks == 0:       # the kernel was not launched
            continue
        waves = blocks * WAVES_PER_BLOCK
        for y in range(8):
            lo, hi, stride, static_end = wq_range(n, y, blocks)
            tail = hi - static_end
            c = int(q["ctr"][y])
            print("%s group %d: items [%d, %d) static end %d tail %d counter %d" % (name, y, lo, hi, static_end, tail, c))
            assert tail <= c <= tail + 8 * waves, (name, y, tail, c, waves)


@pytest.mark.parametrize("name,k", [("uniform3k", 16), ("uniform200k", 16), ("densehalf120k", 16)])
def test_grid_kernels_match_ckdtree(lib, name, k):
    xyz = _cloud(name)
    got, info, wq = _call(lib, xyz, k)
    assert not np.isnan(got).any()
    assert info["algo"] == GRID and info["n_fallback"] > 0, info
    bricks, blocks = wq["knn_brick"]["items"], wq["knn_brick"]["blocks"]
    print("%s: %d bricks on %d waves, %d fallback queries" % (name, bricks, blocks * WAVES_PER_BLOCK, info["n_fallback"]))
    if name == "uniform3k":     # fewer items than waves: no static round, everything comes from the counters
        assert 0 < bricks < blocks * WAVES_PER_BLOCK
    if name == "uniform200k":   # most waves get an item, none a static round (3821 planned bricks on 5120 waves at k = 16)
        assert blocks * WAVES_PER_BLOCK // 2 < bricks < blocks * WAVES_PER_BLOCK
    assert _explain(got, _ref(name, k)) == "ok", info
    _check_counters(wq)


def test_adaptive_mode_and_the_tree_kernels_queues(lib):
    """the dense-half cloud in adaptive mode (whichever path the coarse histogram chooses), and through the tree path itself:
    knn_leaf, knn_tree_near and knn_tree_query take their items from the same queue"""
    name, k = "densehalf120k", 16
    xyz = _cloud(name)
    ref = _ref(name, k)
    for params, algo in ((dict(adaptive=1), GRID), (dict(), TREE)):
        got, info, _ = _call(lib, xyz, k, algo=algo, **params)
        assert not np.isnan(got).any()
        if algo == TREE:
            assert info["algo"] == TREE, info
        assert _explain(got, ref) == "ok", info


@pytest.mark.parametrize("n,per_wave", [(1_000_000, 3), (5_000_000, 16)])
def test_uniform_clouds_with_static_rounds(lib, n, per_wave):
    """a few items per wave (one static round and a tail) and 16 or more (several rounds and a long tail).  Too large for
    cKDTree in a test: compared with the same call on the fixed bricks (brick_plan = 0: other items through the same queue),
    which the smaller clouds of test_brick_plan_gpu tie to cKDTree"""
    xyz = datasets.uniform(n, 10.0, 3)
    on, info, wq1 = _call(lib, xyz, 16)
    off, _, wq0 = _call(lib, xyz, 16, brick_plan=0)
    q = wq1["knn_brick"]
    assert q["items"] // (q["blocks"] * WAVES_PER_BLOCK) >= per_wave, q
    assert not np.isnan(on).any() and not np.isnan(off).any()
    assert _differ(on, off) == 0, _explain(on, off)
    _check_counters(wq1)
    _check_counters(wq0)
