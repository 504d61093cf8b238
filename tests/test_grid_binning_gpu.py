"""The coarse pass of the grid sort (csrc/sor_grid.hip: bucket_hist -> bucket_offsets -> bucket_scatter): per-tile bucket
counts, their per-bucket scans over the tiles' slots, and every point written to bk_start[b] + tile_off[slot][b] + rank.

The host test restates that arithmetic in numpy against a stable argsort by bucket; the GPU tests run the clouds whose
tables are unusual (one tile, a partial last tile, empty buckets, one bucket for every point, a slab's reference-only
rows) and compare the SOR mean distances bit for bit with cKDTree."""
import os
import re

import numpy as np
import pytest

from oracle import datasets, sor as osor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID = 2


def _constants():
    src = open(os.path.join(ROOT, "3dgsconverter_amd", "csrc", "sor_grid.hip")).read()
    tile = int(re.search(r"#define GSX_BIN_TILE (\d+)", src).group(1))
    xcds = int(re.search(r"#define GSX_BIN_XCDS (\d+)", src).group(1))
    return tile, xcds


def _coarse_pass(bucket, nb, tile, xcds, rng):
    """numpy restatement of the three kernels: destination of every point in the bucket-grouped array"""
    n = len(bucket)
    ntiles = -(-n // tile)
    per_xcd = -(-ntiles // xcds)
    slots = xcds * per_xcd
    t_of = np.arange(n) // tile
    slot_of_tile = (np.arange(ntiles) % xcds) * per_xcd + np.arange(ntiles) // xcds
    assert len(np.unique(slot_of_tile)) == ntiles and slot_of_tile.max() < slots
    tile_of_slot = (np.arange(slots) % per_xcd) * xcds + np.arange(slots) // per_xcd
    np.testing.assert_array_equal(tile_of_slot[slot_of_tile], np.arange(ntiles))
    # bucket_hist: tile_cnt[slot][b] (rows of slots that hold no tile stay unwritten: bucket_offsets reads them as 0)
    cnt = np.zeros((slots, nb), np.int64)
    np.add.at(cnt, (slot_of_tile[t_of], bucket), 1)
    assert cnt.max() <= 65535
    cnt[tile_of_slot >= ntiles] = 0
    # bucket_offsets: exclusive scan down each column, sizes, bk_start
    off = np.cumsum(cnt, axis=0) - cnt
    size = cnt.sum(axis=0)
    start = np.concatenate([[0], np.cumsum(size)])
    # bucket_scatter: rank inside the (tile, bucket) run is the LDS atomic's arrival order -- any permutation of the run
    dest = np.empty(n, np.int64)
    for t in range(ntiles):
        lo, hi = t * tile, min(n, (t + 1) * tile)
        b = bucket[lo:hi]
        order = rng.permutation(hi - lo)
        rank = np.empty(hi - lo, np.int64)
        for bb in np.unique(b):
            sel = order[b[order] == bb]
            rank[sel] = np.arange(len(sel))
        dest[lo:hi] = start[b] + off[slot_of_tile[t], b] + rank
    return dest, start, slot_of_tile[t_of]


@pytest.mark.parametrize("n,nb,kind", [(1, 1, "uniform"), (5000, 7, "uniform"), (3 * 8192 + 123, 3249, "uniform"),
                                       (20 * 8192 + 5, 3249, "uniform"), (9 * 8192, 64, "gaps"), (50000, 3249, "one")])
def test_offsets_match_a_stable_argsort_by_bucket(n, nb, kind):
    tile, xcds = _constants()
    rng = np.random.default_rng(n + nb)
    if kind == "uniform":
        bucket = rng.integers(0, nb, n)
    elif kind == "gaps":   # most buckets empty
        bucket = rng.choice(np.array([0, 5, 6, 63]), n)
    else:                  # every point in one bucket
        bucket = np.full(n, nb // 2)
    dest, start, slot = _coarse_pass(bucket, nb, tile, xcds, rng)
    # a permutation of [0, n) ...
    np.testing.assert_array_equal(np.sort(dest), np.arange(n))
    inv = np.empty(n, np.int64)
    inv[dest] = np.arange(n)
    # ... grouped exactly like a stable argsort by bucket: same bucket ranges, same points in each
    stable = np.argsort(bucket, kind="stable")
    np.testing.assert_array_equal(bucket[inv], bucket[stable])
    np.testing.assert_array_equal(start[:-1], np.searchsorted(bucket[stable], np.arange(nb)))
    # inside a bucket the tiles' runs follow the slot order, and inside one run the points of that tile
    key = slot[inv]
    same = bucket[inv][1:] == bucket[inv][:-1]
    assert np.all(key[1:][same] >= key[:-1][same])
    for b in np.unique(bucket)[:16]:
        np.testing.assert_array_equal(np.sort(inv[start[b]:start[b + 1]]), stable[start[b]:start[b + 1]])


# ---------------------------------------------------------------- GPU: SOR mean distances against cKDTree
@pytest.fixture(scope="module")
def lib(gsx):
    gsx._lib.require_hip()
    return gsx._lib


def _bits_equal(got, ref):
    bad = np.nonzero(got.view(np.uint32) != ref.view(np.uint32))[0]
    return "ok" if len(bad) == 0 else "%d / %d differ, first %s" % (len(bad), len(ref), bad[:8])


def _knn_dev(lib, xyz, k, params=()):
    ctx = lib.Context(0)
    try:
        for name, v in params:
            ctx.set_param(name, v)
        cols = [np.ascontiguousarray(xyz[:, a]) for a in range(3)]
        d = [ctx.alloc(4 * len(xyz)).upload(c) for c in cols]
        out = ctx.alloc(4 * len(xyz))
        info = ctx.sor_knn(d[0].ptr, d[1].ptr, d[2].ptr, 1, len(xyz), 0, len(xyz), k, out.ptr, algo=GRID, want_info=True)
        md = out.download(np.float32, len(xyz))
        for a in d + [out]:
            a.free()
        return md, info
    finally:
        ctx.close()


def _uniform(n, seed):
    return datasets.uniform(n, 10.0, seed)


def _gapped(n, seed):
    """two slabs in z with an empty band between them: whole rows of buckets are empty"""
    rng = np.random.default_rng(seed)
    p = rng.random((n, 3)).astype(np.float32) * 10
    p[:, 2] = np.where(p[:, 2] < 5, p[:, 2] * 0.3, 7 + (p[:, 2] - 5) * 0.6)
    return p


def _one_bucket(n, seed):
    """a thin rod along x: a single column of buckets, every point in ONE of them"""
    rng = np.random.default_rng(seed)
    p = np.zeros((n, 3), np.float32)
    p[:, 0] = rng.random(n) * 100
    p[:, 1:] = rng.random((n, 2)) * 0.05
    return p


@pytest.mark.gpu
@pytest.mark.parametrize("name,make,n,k", [("one_tile", _uniform, 5000, 16), ("partial_last_tile", _uniform, 3 * 8192 + 123, 16),
                                           ("many_tiles", _uniform, 300_001, 8), ("empty_buckets", _gapped, 120_000, 16),
                                           ("one_bucket", _one_bucket, 60_000, 16)])
def test_sor_mean_dists_match_ckdtree(lib, name, make, n, k):
    xyz = make(n, 11)
    ref = osor.sor(xyz, k, 1.0)
    res = lib.sor_filter(xyz, k, 1.0, want_info=True)
    assert _bits_equal(res["mean_dists"], ref["mean_dists"]) == "ok", (name, res["info"])
    np.testing.assert_array_equal(res["mask"], ref["mask"])
    md, info = _knn_dev(lib, xyz, k, (("adaptive", 0),))   # the plain grid path, whatever the histogram says
    assert info["algo"] == GRID and _bits_equal(md, ref["mean_dists"]) == "ok", (name, info)


@pytest.mark.gpu
def test_one_bucket_takes_the_big_bucket_path(lib):
    """adaptive grid without the tree: a bucket of more than BIG_BUCKET points is sorted by every workgroup from bk_start"""
    xyz = _one_bucket(100_000, 12)
    ref = osor.mean_dists_ckdtree(xyz, 16)
    md, info = _knn_dev(lib, xyz, 16, (("adaptive", 1), ("tree", 0)))
    assert info["algo"] == GRID and _bits_equal(md, ref) == "ok", info


@pytest.mark.gpu
def test_slab_with_reference_only_rows(lib):
    """gsx_sor_knn_slab_dev: the first n_own rows are queries, the halo rows after them reference-only (bit 31 of the index
    word); the boundary between them falls inside a tile"""
    rng = np.random.default_rng(13)
    own = (rng.random((20_000, 3)) * [5.0, 10.0, 10.0]).astype(np.float32)
    halo = (rng.random((6_000, 3)) * [1.0, 10.0, 10.0] + [5.0, 0.0, 0.0]).astype(np.float32)
    rows = np.ascontiguousarray(np.concatenate([own, halo]))
    ref = osor.mean_dists_ckdtree(rows, 16)[:len(own)]
    ctx = lib.Context(0)
    try:
        d = ctx.alloc(rows.nbytes).upload(rows)
        out = ctx.alloc(4 * len(own))
        kth = ctx.alloc(8 * len(own))
        rc = ctx.lib.gsx_sor_knn_slab_dev(ctx.handle, d.ptr, len(own), len(halo), 16, out.ptr, kth.ptr)
        assert rc == 0, lib.last_error() if hasattr(lib, "last_error") else rc
        md = out.download(np.float32, len(own))
        for a in (d, out, kth):
            a.free()
    finally:
        ctx.close()
    assert _bits_equal(md, ref) == "ok"
