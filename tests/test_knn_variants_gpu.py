"""-m gpu: every instantiation of knn_brick that dispatch_bricks (csrc/sor_grid.hip) can select, bit for bit against cKDTree.

The context switches filter_mfma (phase 1: MFMA filter / scalar filter) and phase2_net (phase 2: sorting-network selection, list
capacities 9, 13, 17, ..., 57, 65 / bubble insert, capacities 9, 17, 26, 33, 51, 65) pick the kernel, k picks the capacity; every
capacity is entered with a k at both of its edges.  brick_plan = 0 throughout: the planned bricks are test_brick_plan_gpu's.
Every call goes through the device entry point with algo = GRID on a fresh context (knn_device.knn): adaptive mode is off and
nothing is diverted to the tree or to brute force."""
import functools

import numpy as np
import pytest

from knn_device import GRID, differ, explain, knn
from oracle import datasets, sor as osor

pytestmark = pytest.mark.gpu

# (filter_mfma, phase2_net); (1, 1) is the default form -- here on the fixed bricks at every k
PAIRS = [(0, 1), (1, 0), (0, 0), (1, 1)]
# network selection holds k entries in capacities 8, 12, 16, ... 56, 64 (k < 8: the sequential mean) ...
NET_K = [1, 3, 7, 8, 9, 12, 13, 16, 17, 20, 21, 24, 25, 28, 29, 32, 33, 36, 37, 40, 41, 44, 45, 48, 49, 52, 53, 56, 57, 64]
# ... the bubble insert k + 1 entries (the query included) in capacities 9, 17, 26, 33, 51, 65
BUBBLE_K = [1, 7, 8, 9, 16, 17, 25, 26, 32, 33, 50, 51, 64]
MATRIX = [pytest.param(mf, net, k, id="mfma%d-net%d-k%d" % (mf, net, k))
          for mf, net in PAIRS for k in (NET_K if net else BUBBLE_K)]
SWITCHED = PAIRS[:3]   # the three pairs no other test file runs


@pytest.fixture(scope="module")
def lib(gsx):
    gsx._lib.require_hip()
    return gsx._lib


@functools.lru_cache(maxsize=None)
def _mixed():
    """12 000 points: a uniform box of edge 10; a Gaussian blob of 2000 points with sigma = 1e-3 of the box, all inside one or two
    bricks (more than 64 queries each: the EXTRA launch runs); 1000 exact copies of five of those points in groups of 3, 10, 40,
    147 and 800, so that for every k some group is shorter and some longer than k + 1 (zero distances, ties at the list's end).
    Shuffled, so that an index window holds points of all three parts."""
    rng = np.random.default_rng(2024)
    box = datasets.uniform(9000, 10.0, 41)
    blob = (np.float32(5.0) + rng.standard_normal((2000, 3)) * 1e-2).astype(np.float32)
    base = np.concatenate([box, blob])
    src = [17, 4321, 8999, 9000 + 5, 9000 + 1999]   # three of the box, two of the blob
    dup = np.concatenate([np.repeat(base[s:s + 1], c, axis=0) for s, c in zip(src, (3, 10, 40, 147, 800))])
    xyz = np.concatenate([base, dup])
    assert len(xyz) == 12000
    return np.ascontiguousarray(xyz[rng.permutation(len(xyz))])


@functools.lru_cache(maxsize=None)
def _mixed_ref(k):
    return osor.mean_dists_ckdtree(_mixed(), k)


# The second cloud, plain datasets.uniform: knn_ring_fast / knn_ring answer every query knn_brick does not certify, so a
# knn_brick that certified nothing would still be bit-exact.  On a uniform cloud it must certify at least half of the queries.
# A query goes to the ring kernels when fewer than k + 1 points lie within its guaranteed radius -- one cell edge h', more at
# the cloud's rim only as far as the searched box reaches.  The share is a few per cent inside the cloud and larger within a
# cell of its faces, and a cell holds about 0.47 (k + 1) points, so the cloud is larger for the larger k: the grid stays
# eight cells across or more.  Measured n_fallback / n of the default form (filter_mfma = phase2_net = 1, fixed bricks) at these sizes:
#   n = 8000 (k <= 32), k: share
#     1: 0.0000   3: 0.0000   7: 0.0000   8: 0.0035   9: 0.0073   12: 0.0053   13: 0.0075   16: 0.0245
#     17: 0.0331   20: 0.0331   21: 0.0205   24: 0.0059   25: 0.0083   26: 0.0079   28: 0.0134   29: 0.0170
#     32: 0.0307
#   n = 16 000 (k > 32), k: share
#     33: 0.0191   36: 0.0331   37: 0.0398   40: 0.0591   41: 0.0658   44: 0.0476   45: 0.0532   48: 0.0699
#     49: 0.0769   50: 0.0092   51: 0.0103   52: 0.0114   53: 0.0136   56: 0.0183   57: 0.0205   64: 0.0265
#   (at n = 4000 the largest is 0.18, at k = 49; from 32 000 points on every k is below 0.07)
def _uniform_n(k):
    return 8000 if k <= 32 else 16000


@functools.lru_cache(maxsize=None)
def _uniform(n):
    return datasets.uniform(n, 10.0, 43)


@functools.lru_cache(maxsize=None)
def _uniform_ref(n, k):
    return osor.mean_dists_ckdtree(_uniform(n), k)


def _switches(mf, net):
    return {"filter_mfma": mf, "phase2_net": net, "brick_plan": 0}


@pytest.mark.parametrize("mf,net,k", MATRIX)
def test_every_kernel_variant_on_a_cloud_with_a_blob_and_duplicates(lib, mf, net, k):
    xyz = _mixed()
    got, info, _ = knn(lib, xyz, k, **_switches(mf, net))
    text = explain(got, _mixed_ref(k))
    print(text, info)
    assert differ(got, _mixed_ref(k)) == 0, (text, info)


@pytest.mark.parametrize("mf,net,k", MATRIX)
def test_every_kernel_variant_certifies_half_of_a_uniform_cloud_itself(lib, mf, net, k):
    n = _uniform_n(k)
    xyz = _uniform(n)
    got, info, _ = knn(lib, xyz, k, **_switches(mf, net))
    text = explain(got, _uniform_ref(n, k))
    print("n=%d k=%d filter_mfma=%d phase2_net=%d: n_fallback / n = %.4f; %s %s" % (n, k, mf, net, info["n_fallback"] / n, text, info))
    assert differ(got, _uniform_ref(n, k)) == 0, (text, info)
    assert info["n_bricks"] > 0 and info["n_fallback"] <= n // 2, info


@pytest.mark.parametrize("k", [16, 25])
@pytest.mark.parametrize("mf,net", SWITCHED)
def test_a_query_window_takes_the_separate_query_tables(lib, mf, net, k):
    """queries [q0, q0 + qc) only: they are binned a second time (qsorted, qcellstart) against all 12 000 references"""
    xyz = _mixed()
    for q0, qc in ((1237, 7013), (len(xyz) - 501, 501)):
        got, info, _ = knn(lib, xyz, k, window=(q0, qc), **_switches(mf, net))
        ref = _mixed_ref(k)[q0:q0 + qc]
        assert differ(got, ref) == 0, (q0, qc, explain(got, ref), info)


@pytest.mark.parametrize("mf,net", SWITCHED)
def test_three_shares_sum_to_the_whole(lib, mf, net):
    """gsx_sor_knn_share_dev (test_sor_gpu.test_query_shares_sum_to_the_whole is the pattern): the shares overwrite the whole
    output, are disjoint, cover every query and their plain float32 sum is the reference.  Who owns a query shows in its
    non-zero mean distance; the queries whose mean IS zero (16 or more copies of themselves) must read +0.0 in every share."""
    xyz, k, nshares = _mixed(), 16, 3
    n = len(xyz)
    ref = _mixed_ref(k)
    nonzero = ref != 0
    assert int((~nonzero).sum()) == 41 + 148 + 801   # the groups of 40, 147 and 800 copies, each with the point they copy
    ctx = lib.Context(0)
    for name, val in _switches(mf, net).items():
        ctx.set_param(name, val)
    rows = ctx.alloc(xyz.nbytes).upload(xyz)
    out = ctx.alloc(4 * n)
    total = np.zeros(n, np.float32)
    owners = np.zeros(n, np.int32)
    sizes, infos = [], []
    for share in range(nshares):
        out.upload(np.full(n, np.nan, np.float32))   # the call must overwrite everything
        infos.append(ctx.sor_knn_share(rows.ptr, rows.ptr + 4, rows.ptr + 8, 3, n, k, share, nshares, out.ptr, algo=GRID, want_info=True))
        got = out.download(np.float32, n)
        assert np.isfinite(got).all(), (share, infos)
        mine = got != 0
        assert not np.signbit(got[~mine]).any()   # +0.0, not -0.0
        owners += mine
        sizes.append(int(mine.sum()))
        total = total + got   # what the sum all-reduce does
    rows.free()
    out.free()
    ctx.close()
    assert (owners[nonzero] == 1).all() and (owners[~nonzero] == 0).all(), (sizes, int((owners[nonzero] != 1).sum()))
    assert min(sizes) > 0, sizes
    assert differ(total, ref) == 0, (explain(total, ref), sizes, infos)


def test_interleaved_rows_and_separate_columns_give_the_same_bits(lib):
    xyz, k = _mixed(), 16
    rows, info, _ = knn(lib, xyz, k, **_switches(0, 0))
    cols, info_c, _ = knn(lib, xyz, k, columns=True, **_switches(0, 0))
    assert differ(rows, cols) == 0, (explain(rows, cols), info, info_c)
    assert differ(rows, _mixed_ref(k)) == 0, (explain(rows, _mixed_ref(k)), info)


@pytest.mark.parametrize("k", [16, 25])
@pytest.mark.parametrize("mf,net", SWITCHED)
def test_the_switched_variants_hand_over_to_knn_ring_alone(lib, mf, net, k):
    """ring_fast = 0 together with the other switches: knn_ring takes every query knn_brick leaves"""
    xyz = _mixed()
    got, info, _ = knn(lib, xyz, k, ring_fast=0, **_switches(mf, net))
    assert info["n_fallback"] > 0, info
    assert differ(got, _mixed_ref(k)) == 0, (explain(got, _mixed_ref(k)), info)
