"""-m gpu: knn_brick's certified epilogue (context parameter epilogue_cert; csrc/knn_mean_cert.h).

At k = 16 the network kernels leave the wave's last block unsorted, take 16 short float64 roots (no residual correction), and
store (float)(sum / 16) where a certificate says that the exact epilogue would store the same float32; where it does not, the
wave sorts the list and runs the exact epilogue.  So epilogue_cert = 1 and = 0 must agree on every bit, with each other and
with cKDTree, and leave the same fail list: the k-th distance the acceptance test reads is the same value either way.  The
certificate itself is checked against rational arithmetic without a GPU (tests/test_mean_cert_host.py); here the short root is
held against the bound the certificate was derived from, on the GPU the suite runs on."""
import functools
import os
import re

import numpy as np
import pytest

import epilogue_cases as ec
from knn_device import differ as _differ, explain as _explain, knn as _knn
from oracle import datasets, sor as osor

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib(gsx):
    gsx._lib.require_hip()
    return gsx._lib


# ---------------------------------------------------------------- the clouds
@functools.lru_cache(maxsize=None)
def _uniform8k():
    return datasets.uniform(8000, 10.0, 43)


@functools.lru_cache(maxsize=None)
def _duplicates():
    """a thousand copies of one point in one quarter-slab: batches on the scalar filter, which drains more than once, and
    lists of sixteen zeros"""
    xyz = _uniform8k().copy()
    xyz[:1000] = xyz[5000]
    return xyz


@functools.lru_cache(maxsize=None)
def _lattice():
    """20 x 20 x 20 points of spacing 1: six neighbours at 1 and twelve at sqrt(2), of which ten are taken -- every block
    and every list is full of equal distances, every interior mean is the same number"""
    g = np.arange(20, dtype=np.float32)
    return np.ascontiguousarray(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3))


LATTICE_PPC = 8.0 * 8000 / 19.0 ** 3      # cell edge exactly 2: (volume * ppc / n) ** (1 / 3)
CLOUDS = {"uniform": (_uniform8k, {}), "dup": (_duplicates, {}), "lattice": (_lattice, {"grid_points_per_cell": LATTICE_PPC})}


@functools.lru_cache(maxsize=None)
def _ref(name, k):
    return osor.mean_dists_ckdtree(CLOUDS[name][0](), k)


def _on_off(lib, xyz, k, fallback_count=True, **params):
    on, info_on, plan = _knn(lib, xyz, k, want_plan=True, epilogue_cert=1, **params)
    off, info_off, plan_off = _knn(lib, xyz, k, want_plan=True, epilogue_cert=0, **params)
    assert plan["plan"] == plan_off["plan"]
    assert info_on["n_bricks"] == info_off["n_bricks"], (info_on, info_off)
    if fallback_count:
        assert info_on["n_fallback"] == info_off["n_fallback"], (info_on, info_off)
    assert _differ(on, off) == 0, _explain(on, off)
    return on, info_on, plan


@pytest.mark.parametrize("plan_on", [1, 0])
@pytest.mark.parametrize("name", list(CLOUDS))
def test_same_bits_with_and_without_the_certificate(lib, name, plan_on):
    make, params = CLOUDS[name]
    xyz = make()
    got, info, plan = _on_off(lib, xyz, 16, brick_plan=plan_on, **params)
    if name != "lattice":     # (the lattice's cells of edge 2 hold too few points for the plan: fixed bricks both times)
        assert plan["plan"] == plan_on
    print("%s plan=%d: %d of %d queries left to the fallback" % (name, plan_on, info["n_fallback"], len(xyz)))
    if name == "uniform":
        assert info["n_fallback"] <= len(xyz) // 2, info       # knn_brick itself answers most queries
    assert _differ(got, _ref(name, 16)) == 0, _explain(got, _ref(name, 16))


@pytest.mark.parametrize("filter_mfma", [1, 0])
def test_fixed_bricks_with_either_filter(lib, filter_mfma):
    """the scalar filter's kernel is an instantiation of its own (MF = false), and the only one that drains more than once
    per batch on an ordinary cloud"""
    got, info, _ = _on_off(lib, _uniform8k(), 16, brick_plan=0, filter_mfma=filter_mfma)
    assert _differ(got, _ref("uniform", 16)) == 0, _explain(got, _ref("uniform", 16))


@pytest.mark.parametrize("k", [8, 12])
def test_other_k_are_untouched(lib, k):
    got, _, _ = _on_off(lib, _uniform8k(), k)
    assert _differ(got, _ref("uniform", k)) == 0


# ---------------------------------------------------------------- a tie on purpose
def _tie_cloud(n_near):
    """One query with `n_near` duplicate neighbours at distance exactly 1 and 16 - n_near at exactly 1 + 2^-23, all along x:
    the query at x = 1 + 2^-23, the near group at x = 2^-23, the far group at x = 0 (float32 values; the differences, their
    squares 1 and 1 + 2^-22 + 2^-46 and the roots are exact in float64).  Around them 8000 uniform points in a box of edge
    20 (one per unit volume: cells of edge ~1.93 at k = 16), none within 1.5 of the query, so that the sixteen are its
    neighbours and their distances lie inside the radius knn_brick certifies, 0.999 cell edges.  Returns (xyz, query index)."""
    eps = np.float32(2.0 ** -23)
    q = np.array([np.float32(1.0) + eps, 10.0, 10.0], np.float32)
    fill = datasets.uniform(8000, 20.0, 5) + np.array([-9.0, 0.0, 0.0], np.float32)
    fill = fill[np.linalg.norm(fill.astype(np.float64) - q, axis=1) > 1.5]
    near = np.tile(np.array([eps, 10.0, 10.0], np.float32), (n_near, 1))
    far = np.tile(np.array([0.0, 10.0, 10.0], np.float32), (16 - n_near, 1))
    xyz = np.ascontiguousarray(np.concatenate([fill, near, far, q[None]]).astype(np.float32))
    return xyz, len(xyz) - 1


@pytest.mark.parametrize("plan_on", [1, 0])
@pytest.mark.parametrize("n_near,exact_mean", [(8, 1.0 + 2.0 ** -24), (9, 1.0 + 7 * 2.0 ** -27)], ids=["tie", "off-tie"])
def test_a_mean_on_a_float32_tie(lib, n_near, exact_mean, plan_on):
    """8 + 8: the exact mean is 1 + 2^-24, halfway between 1 and the next float32; the answer is 1 (ties to even), and short
    roots that are an ulp off would land on either side -- the certificate has to refuse (tests/test_mean_cert_host.py:
    test_the_tie_of_the_device_test) and the wave recompute.  9 + 7 is 2^-27 below the tie: certified, also 1."""
    xyz, qi = _tie_cloud(n_near)
    d2 = np.sort(((xyz.astype(np.float64) - xyz[qi].astype(np.float64)) ** 2).sum(1))[1:18]
    assert np.array_equal(d2[:n_near], np.ones(n_near)) and np.array_equal(d2[n_near:16], np.full(16 - n_near, (1.0 + 2.0 ** -23) ** 2))
    assert d2[16] > 2.25 and np.sqrt(d2[:16]).sum() / 16 == exact_mean
    # The fail counts of the two settings are compared on planned bricks only.  On the fixed bricks this cloud's count is
    # not one number: a fixed brick may hold more than 64 queries (here the one that received the 17 planted points does),
    # which of them land in its second batch is the order the binning leaves in a cell, and a later batch certifies less
    # than the first (knn_brick: no widened radius at the rim) -- with ONE setting (epilogue_cert = 0, the earlier kernel) eight runs in a row gave 200, 200, 200, 200, 201,
    # 201, 200, 200 fallback queries, the mean distances the same bits every time.  (The three clouds above give one count
    # on every run, on either kind of brick; a planned brick never holds more than 64 queries.)
    got, info, plan = _on_off(lib, xyz, 16, fallback_count=plan_on == 1, brick_plan=plan_on)
    assert plan["plan"] == plan_on
    h = 1.0 / float(plan["origin"][3])
    assert 1.0 + 2.0 ** -23 < 0.99 * h, h        # inside knn_brick's acceptance radius, 0.999 h at least: not a fallback query
    ref = osor.mean_dists_ckdtree(xyz, 16)
    assert ref[qi] == np.float32(1.0)
    assert got[qi] == np.float32(1.0), got[qi]
    assert _differ(got, ref) == 0, _explain(got, ref)


# ---------------------------------------------------------------- the short root
def _short_root_bound():
    text = open(os.path.join(ROOT, "3dgsconverter_amd", "csrc", "knn_mean_cert.h")).read()
    return float.fromhex(re.search(r"KNN_SHORT_ROOT_BOUND\s*=\s*(0x[0-9a-fA-F.]+p[-+]?\d+)", text).group(1))


def test_short_root_stays_within_the_bound_the_certificate_assumes(lib):
    """sqrt_short_dist2 against np.sqrt over the inputs of test_knn_epilogue_gpu's root test (every binade of the domain, dense
    mantissas, near-ties, exact squares; 4.3M values): KNN_SHORT_ROOT_BOUND is 64 times the largest error measured on MI355X,
    the factor standing for mantissas no sample holds.  Asserted here with a factor of 16 still in hand, so that hardware
    whose seed is worse fails this test well before the certificate's premise does.  (np.sqrt is correctly rounded: 2^-53
    of the figure is its own.)"""
    x = ec.root_inputs()
    ctx = lib.Context(0)
    d_in = ctx.alloc(x.nbytes).upload(x)
    d_out = ctx.alloc(x.nbytes)
    try:
        ctx.knn_probe_root_short(d_in.ptr, len(x), lib.PROBE_SHORT_ROOT, d_out.ptr)
        got = d_out.download(np.float64, len(x))
    finally:
        d_in.free()
        d_out.free()
        ctx.close()
    want = np.sqrt(x)
    zero = x == 0
    assert zero.any() and np.all(got[zero] == 0.0)
    rel = np.abs(got[~zero] - want[~zero]) / want[~zero]
    bound = _short_root_bound()
    print("short root: largest relative error %.4g = 2^%.2f over %d inputs; bound 2^%.0f" % (
        rel.max(), np.log2(rel.max()), len(x), np.log2(bound)))
    assert rel.max() <= bound / 16
