"""-m gpu: the k-th select of TopNet (csrc/knn_common.h) and the general branch of mean_from_net entered at both edges of each
list capacity, bit for bit against cKDTree.

The select chain `r = (at == i) ? a[i] : r` runs only when k is NOT the capacity of its list (k == L returns early), and its
index is made opaque where the chain starts (pinned_here_s), so that the L - 1 compares are made there and not kept from the
kernel's entry on; the sums of mean_from_net treat their compares with k the same way.  The capacities are 8, 12, 16, ... 64;
a capacity L is entered with k = L - 3 and k = L - 1:
  (a) the planned bricks (the call's defaults): L = 12 and 16;
  (b) the fixed bricks (brick_plan = 0): L = 20, 32 and 64;
  (c) knn_leaf on the tree path, chosen by adaptive mode for a clustered cloud: L = 16 and 28;
  (d) the k-th squared distance itself (kth_out), which only the slab entry point hands out on one GPU.
Every uniform case also asserts that knn_brick certified more than half of the queries itself: the ring kernels answer whatever
it does not, so a knn_brick that certified nothing would still be bit-exact (test_knn_variants_gpu records a share of at
most 0.07 at these sizes)."""
import functools

import numpy as np
import pytest

from knn_device import TREE, differ, explain, knn
from oracle import datasets, sor as osor

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(gsx):
    gsx._lib.require_hip()
    return gsx._lib


@functools.lru_cache(maxsize=None)
def _uniform(n):
    return datasets.uniform(n, 10.0, 43)


@functools.lru_cache(maxsize=None)
def _mixed():
    """12 000 points: a uniform box, a tight blob of 2000 points inside one or two bricks, and 1000 exact copies of five points
    in groups of 3, 10, 40, 147 and 800: for every k some group is shorter and some longer than k + 1, the list ends on ties"""
    rng = np.random.default_rng(2025)
    box = datasets.uniform(9000, 10.0, 47)
    blob = (np.float32(5.0) + rng.standard_normal((2000, 3)) * 1e-2).astype(np.float32)
    base = np.concatenate([box, blob])
    src = [23, 4000, 8998, 9000 + 7, 9000 + 1998]
    dup = np.concatenate([np.repeat(base[s:s + 1], c, axis=0) for s, c in zip(src, (3, 10, 40, 147, 800))])
    xyz = np.concatenate([base, dup])
    assert len(xyz) == 12000
    return np.ascontiguousarray(xyz[rng.permutation(len(xyz))])


@functools.lru_cache(maxsize=None)
def _clustered():
    return datasets.clustered(8000, 5)


CLOUDS = {"uniform8k": lambda: _uniform(8000), "uniform16k": lambda: _uniform(16000), "mixed": _mixed, "clustered": _clustered}


@functools.lru_cache(maxsize=None)
def _ref(cloud, k):
    return osor.mean_dists_ckdtree(CLOUDS[cloud](), k)


def check(got, cloud, k, info, certifies):
    ref = _ref(cloud, k)
    n = len(ref)
    text = explain(got, ref)
    print("%s k=%d: n_fallback / n = %.4f; %s %s" % (cloud, k, info["n_fallback"] / n, text, info))
    assert differ(got, ref) == 0, (text, info)
    if certifies:
        assert info["n_bricks"] > 0 and info["n_fallback"] < n // 2, info


@pytest.mark.parametrize("k", [9, 11, 13, 15])
@pytest.mark.parametrize("cloud", ["uniform8k", "mixed"])
def test_planned_bricks_at_both_edges_of_a_capacity(lib, cloud, k):
    got, info, plan = knn(lib, CLOUDS[cloud](), k, want_plan=True)
    print("plan", plan["plan"], "bricks", plan["bricks"])
    assert plan["plan"] == 1, plan
    check(got, cloud, k, info, certifies=cloud == "uniform8k")


@pytest.mark.parametrize("k", [17, 19, 29, 31, 61, 63])
def test_fixed_bricks_at_both_edges_of_a_capacity(lib, k):
    cloud = "uniform8k" if k < 32 else "uniform16k"
    got, info, plan = knn(lib, CLOUDS[cloud](), k, want_plan=True, brick_plan=0)
    assert plan["plan"] == 0, plan
    check(got, cloud, k, info, certifies=True)


@pytest.mark.parametrize("k", [13, 15, 25, 27])
def test_knn_leaf_at_both_edges_of_a_capacity(lib, k):
    got, info, _ = knn(lib, _clustered(), k, algo=lib.KNN_AUTO, adaptive=1)
    assert info["algo"] == TREE, info   # blobs of very different density and far flyers: adaptive mode leaves the grid
    check(got, "clustered", k, info, certifies=False)


def _kth_sq_exact(xyz, k):
    """the k-th neighbour's squared distance in cKDTree's arithmetic: ((dx*dx) + dy*dy) + dz*dz in float64, no FMA; entry k of
    the ascending row, the query itself being entry 0"""
    x = xyz.astype(np.float64)
    out = np.empty(len(x))
    for lo in range(0, len(x), 500):
        d = x[lo:lo + 500, None, :] - x[None, :, :]
        s = (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]
        out[lo:lo + 500] = np.partition(s, k, axis=1)[:, k]
    return out


def test_the_kth_distance_output_behind_the_select(gsx, lib):
    """gsx_sor_knn_slab_dev with no halo: every row is a query, kth_out is written by whichever kernel finished the query"""
    import importlib
    slab = importlib.import_module("3dgsconverter_amd.dist_slab")
    k, xyz = 13, _uniform(8000)
    n = len(xyz)
    ctx = lib.Context(0)   # (its own, closed below: adaptive mode stays off, a uniform cloud is the grid's either way)
    try:
        be = slab.HipSlabBackend(0, ctx=ctx)
        rows, mean, kth = be.buf("kth_test_rows", xyz.nbytes), be.buf("kth_test_mean", 4 * n), be.buf("kth_test_kth", 8 * n)
        be.from_host(rows, xyz)
        be.zero(kth, 8 * n)
        be.knn_slab(rows, n, 0, k, mean, kth)
        got, got_kth = be.to_host(mean, np.float32, n), be.to_host(kth, np.float64, n)
    finally:
        ctx.close()
    ref = _ref("uniform8k", k)
    assert differ(got, ref) == 0, explain(got, ref)
    want = _kth_sq_exact(xyz, k)
    bad = np.nonzero(got_kth.view(np.uint64) != want.view(np.uint64))[0]
    assert len(bad) == 0, (len(bad), bad[:8], got_kth[bad[:8]], want[bad[:8]])
