"""-m "not gpu": the fixtures of test_density_components_gpu.py keep their own promises (dense counts, cluster sizes, ties --
the oracle alone), and the new entry points fail loudly without the library."""
import numpy as np
import pytest

import density_components_cases as cases
from oracle import density as oden


def _cluster_sizes(dense):
    """sizes of the 6-connected clusters of `dense`, largest first: the oracle's BFS run once per cluster (every cluster is
    the single survivor of the voxels that are left)"""
    left = dense
    sizes = []
    while len(left):
        valid, _, max_len = oden.cluster_dense_voxels(left, False)
        sizes.append(max_len)
        left = np.array([k for k in left.tolist() if tuple(k) not in valid], dtype=np.int64).reshape(-1, 3)
    return sizes


@pytest.mark.parametrize("name", cases.NAMES)
def test_fixture_has_the_promised_clusters(name):
    voxel, thr, n_dense, top_sizes, tie = cases.promised(name)
    xyz = cases.cloud(name)
    # voxel centres are exact in float32: the keys the filter derives are the keys the cloud was built from
    min_points, uniq, inverse, dense = cases.occupancy(name)
    assert len(dense) == n_dense and n_dense > 1024
    want = cases.PROMISES.get(name, {})
    if name in ("crowd", "clustered"):
        # thousands of clusters: all sizes from one labelling pass (scipy-free: the oracle per cluster would be quadratic)
        sizes = _sizes_by_union(dense)
    else:
        sizes = _cluster_sizes(dense)
    assert sizes[:len(top_sizes)] == top_sizes and (len(sizes) == len(top_sizes) or name in ("crowd", "clustered"))
    assert sum(sizes) == n_dense
    assert (len(sizes) > 1 and sizes[0] == sizes[1]) == tie
    if "clusters" in want:
        assert len(sizes) == want["clusters"]
    if "min_points" in want:
        assert min_points == want["min_points"]
    if "unique" in want:
        assert len(uniq) == want["unique"]
    for multi in (False, True):
        exp = cases.expected(name, multi)
        ref = oden.density_filter(xyz, voxel, thr, keep_multicluster=multi)     # the helper is the oracle, step for step
        np.testing.assert_array_equal(exp["mask"], ref["mask"])
        assert (exp["kept_clusters"], exp["max_len"], exp["unique_voxels"], exp["min_points"]) == \
               (ref["kept_clusters"], ref["max_len"], ref["unique_voxels"], ref["min_points"])
        assert exp["max_len"] == top_sizes[0]
        floor = top_sizes[0] * 0.05 if multi else top_sizes[0]
        assert exp["kept_clusters"] == (sum(s >= floor for s in sizes) if multi else 1)
        if "rows" in want:
            assert int(exp["mask"].sum()) == want["rows"][int(multi)]
        if multi and "multi_clusters" in want:
            assert exp["kept_clusters"] == want["multi_clusters"]
    if tie:
        assert cases.expected(name, True)["mask"].all()


def _sizes_by_union(dense):
    index = {tuple(k): i for i, k in enumerate(dense.tolist())}
    parent = list(range(len(dense)))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for (x, y, z), i in index.items():
        for nb in ((x + 1, y, z), (x, y + 1, z), (x, y, z + 1)):
            j = index.get(nb)
            if j is not None:
                a, b = find(i), find(j)
                if a != b:
                    parent[max(a, b)] = min(a, b)
    counts = {}
    for i in range(len(dense)):
        r = find(i)
        counts[r] = counts.get(r, 0) + 1
    return sorted(counts.values(), reverse=True)


def test_union_sizes_agree_with_the_oracle_bfs():
    """the one-pass labelling used for the two big fixtures gives the oracle's sizes where both are affordable"""
    for name in ("snakes_v1", "five_percent", "wide", "bridge"):
        dense = cases.occupancy(name)[3]
        assert _sizes_by_union(dense) == _cluster_sizes(dense)


def test_snake_is_one_long_path():
    keys = cases.snake((-30, -7, -3), 64, 32)
    assert len(keys) == 2079 and len(np.unique(keys, axis=0)) == 2079
    assert keys[:, 0].min() == -30 and keys[:, 1].min() == -7      # negative kmin
    # every row is joined to the next by exactly one voxel: remove a connector and the snake falls apart
    odd = keys[(keys[:, 1] - -7) % 2 == 1]
    assert len(odd) == 31
    cut = np.array([k for k in keys.tolist() if k != odd[15].tolist()], dtype=np.int64)
    assert _cluster_sizes(np.unique(cut, axis=0)) == [16 * 64 + 15, 16 * 64 + 15]


def test_new_entry_points_fail_loudly_without_the_library(gsx):
    if gsx.has_hip():
        pytest.skip("a GPU is present")
    lib = gsx._lib
    keys = cases.occupancy("tie")[3]
    with pytest.raises(lib.GsxError):
        lib.voxel_clusters(keys, False)
    with pytest.raises(lib.GsxError):
        lib.DeviceChain(cases.cloud("tie")).density_filter_large(1.0, 0, False)
    # the eager class above the switch reaches gsx_voxel_clusters only through density_voxels, which fails first
    with pytest.raises(lib.GsxError):
        gsx.DataProcessor(cases.struct(cases.cloud("tie"))).apply_density_filter(voxel_size=1.0, threshold_percentage=0.0)
