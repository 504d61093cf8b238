"""-m gpu: the 6-connected clusters of MORE than 1024 dense voxels on the device (gsx_density_filter_large_dev,
gsx_voxel_clusters) through all four routes -- the device chain, the key-list entry point, the lazy class, the eager class --
against oracle/density.py, which is pinned to the reference.  Bar: masks, kept_clusters, largest and the status lines equal."""
import importlib

import numpy as np
import pytest

import density_components_cases as cases
from oracle import datasets, density as oden

pytestmark = pytest.mark.gpu

MULTI = [False, True]


def _dpmod():
    return importlib.import_module("3dgsconverter_amd.processing.data_processor")


def _chain_mask(ch, n):
    got = np.zeros(n, dtype=bool)
    got[ch.survivors()] = True
    return got


def _rows(proc, n):
    got = np.zeros(n, dtype=bool)
    got[proc.data["orig"]] = True
    return got


def _through_class(monkeypatch, xyz, voxel, thr, multi, lazy):
    """-> (survivor mask, status lines) of apply_density_filter"""
    dpmod = _dpmod()
    said = []
    monkeypatch.setattr(dpmod, "status_print", lambda *a, **k: said.append(" ".join(map(str, a))))
    proc = dpmod.DataProcessor(cases.struct(xyz), lazy=lazy)
    out = proc.apply_density_filter(voxel_size=voxel, threshold_percentage=thr, keep_multicluster=multi)
    assert (out is None) if lazy else (out is proc.data)
    return _rows(proc, len(xyz)), said


@pytest.mark.parametrize("multi", MULTI)
@pytest.mark.parametrize("name", cases.NAMES)
def test_device_chain_clusters_any_number_of_dense_voxels(gsx, name, multi):
    lib = gsx._lib
    voxel, thr, n_dense, _, tie = cases.promised(name)
    xyz, exp = cases.cloud(name), cases.expected(name, multi)
    ch = lib.DeviceChain(xyz)
    try:
        res = ch.density_filter_large(voxel, exp["min_points"], multi)
        if tie and not multi:
            assert res["status"] == lib.DENSITY_HOST and res["left"] is None and ch.n == len(xyz)     # nothing applied
            return
        assert res["status"] == lib.DENSITY_OK
        assert (res["n_unique"], res["kept_clusters"], res["largest"]) == (exp["unique_voxels"], exp["kept_clusters"], exp["max_len"])
        np.testing.assert_array_equal(_chain_mask(ch, len(xyz)), exp["mask"])
        assert res["left"] == int(exp["mask"].sum()) == ch.n
    finally:
        ch.close()


@pytest.mark.parametrize("multi", MULTI)
@pytest.mark.parametrize("name", cases.NAMES)
def test_voxel_clusters_on_the_oracles_dense_keys(gsx, name, multi):
    lib = gsx._lib
    tie = cases.promised(name)[4]
    dense, exp = cases.occupancy(name)[3], cases.expected(name, multi)
    res = lib.voxel_clusters(dense, multi)
    if tie and not multi:
        assert res["status"] == lib.DENSITY_HOST
        return
    assert res["status"] == lib.DENSITY_OK
    assert res["keep"].dtype == np.bool_ and res["keep"].shape == (len(dense),)
    assert set(map(tuple, dense[res["keep"]].tolist())) == exp["valid"]
    assert (res["kept_clusters"], res["largest"]) == (exp["kept_clusters"], exp["max_len"])
    # input order, whatever it is: the same keys shuffled give the same flags, shuffled
    perm = np.random.default_rng(3).permutation(len(dense))
    np.testing.assert_array_equal(lib.voxel_clusters(dense[perm], multi)["keep"], res["keep"][perm])


@pytest.mark.parametrize("lazy", [True, False], ids=["lazy", "eager"])
@pytest.mark.parametrize("multi", MULTI)
@pytest.mark.parametrize("name", cases.NAMES)
def test_classes_return_the_oracles_rows_and_lines(gsx, monkeypatch, name, multi, lazy):
    voxel, thr = cases.promised(name)[:2]
    exp = cases.expected(name, multi)
    mask, said = _through_class(monkeypatch, cases.cloud(name), voxel, thr, multi, lazy)
    np.testing.assert_array_equal(mask, exp["mask"])
    assert said == exp["messages"]


def test_voxel_clusters_refuses_keys_it_cannot_frame(gsx):
    lib = gsx._lib
    keys = np.array([[0, 0, 0], [0, 1 << 31, 0]], dtype=np.int64)
    with pytest.raises(lib.GsxError, match="span"):
        lib.voxel_clusters(keys, True)
    # far from the origin but close together: the frame is the keys' own
    far = cases.block((1 << 40, -(1 << 40), 7), (12, 12, 12))
    res = lib.voxel_clusters(np.concatenate([far, far[:5] + np.array([100, 0, 0])]), True)
    assert res["status"] == lib.DENSITY_OK and (res["kept_clusters"], res["largest"]) == (1, 1728)
    assert res["keep"].tolist() == [True] * 1728 + [False] * 5
    assert lib.voxel_clusters(np.zeros((0, 3), np.int64), False)["status"] == lib.DENSITY_EMPTY


def test_large_filter_with_a_box_that_is_not_a_superset(gsx):
    """the contract of density_filter: a stale box (rows outside it) must neither wrap into valid voxels nor overfill the
    table -- the call notices and repeats itself with the frame of the rows"""
    lib = gsx._lib
    xyz, exp = cases.cloud("crowd"), cases.expected("crowd", False)
    ch = lib.DeviceChain(xyz)
    try:
        ch._box = np.array([0, 0, 0, 2, 2, 2], dtype=np.float32)
        res = ch.density_filter_large(0.3, exp["min_points"], False)
        assert res["status"] == lib.DENSITY_OK and res["largest"] == exp["max_len"]
        np.testing.assert_array_equal(_chain_mask(ch, len(xyz)), exp["mask"])
    finally:
        ch.close()


def test_stage_clocks_are_recorded_while_timing_is_on(gsx):
    lib = gsx._lib
    ch = lib.DeviceChain(cases.cloud("crowd"))
    try:
        ch.ctx.set_timing(True)
        assert ch.density_filter_large(0.3, 0, True)["status"] == lib.DENSITY_OK
        clocks = ch.ctx.density_stage_clocks()
        ch.ctx.set_timing(False)
        assert tuple(clocks) == lib.DENSITY_STAGES and all(0.0 < v < 1000.0 for v in clocks.values()), clocks
    finally:
        ch.close()


def test_large_filter_random_shapes(gsx):
    """random clouds / voxel sizes / thresholds near 0, wide keys included: whenever the device decides, its rows are the
    oracle's -- and it decides at least half of the time (ties are the only thing it may hand back)"""
    lib = gsx._lib
    rng = np.random.default_rng(23)
    trials, host = 24, 0
    for trial in range(trials):
        kind = ["clustered", "two_blobs", "uniform", "scene_with_floaters"][trial % 4]
        n = int(rng.integers(2000, 120000))
        spec = {"kind": kind, "n": n, "seed": int(rng.integers(0, 1 << 20))}
        xyz = datasets.make(spec)
        voxel = float(rng.choice([0.1, 0.33, 0.5]))
        thr = float(rng.choice([0.0, 0.001, 0.002]))
        multi = bool(rng.integers(0, 2))
        if trial % 5 == 4:
            # > 2^21 voxels per axis: the WIDE key layout.  Every voxel is a singleton there, a tie without keep_multicluster
            xyz, voxel, multi = (xyz * np.float32(3.0e4)).astype(np.float32), 0.1, True
        ref = oden.density_filter(xyz, voxel, thr, keep_multicluster=multi)
        ch = lib.DeviceChain(xyz)
        res = ch.density_filter_large(voxel, ref["min_points"], multi)
        what = str((spec, voxel, thr, multi))
        if res["status"] == lib.DENSITY_OK:
            np.testing.assert_array_equal(_chain_mask(ch, len(xyz)), ref["mask"], err_msg=what)
            assert (res["n_unique"], res["kept_clusters"], res["largest"]) == (ref["unique_voxels"], ref["kept_clusters"], ref["max_len"]), what
        elif res["status"] == lib.DENSITY_EMPTY:
            assert not ref["mask"].any(), what
        else:
            assert not multi, what            # only a tie comes back, and keep_multicluster has none to break
            host += 1
        ch.close()
    assert 2 * host <= trials, host


def test_the_host_steps_are_really_gone(gsx, monkeypatch):
    """above 1024 dense voxels neither class walks the voxels in Python any more; a tie for the largest cluster still does"""
    dpmod = _dpmod()
    real = dpmod._clusters.connected_clusters

    def refuse(*a, **k):
        raise AssertionError("processing/clusters.py was asked to cluster the voxels")
    monkeypatch.setattr(dpmod._clusters, "connected_clusters", refuse)
    for name in ("crowd", "snakes_v1"):
        voxel, thr = cases.promised(name)[:2]
        for lazy in (True, False):
            mask, said = _through_class(monkeypatch, cases.cloud(name), voxel, thr, False, lazy)
            np.testing.assert_array_equal(mask, cases.expected(name, False)["mask"])
            assert said == cases.expected(name, False)["messages"]
    calls = []
    monkeypatch.setattr(dpmod._clusters, "connected_clusters", lambda *a, **k: calls.append(1) or real(*a, **k))
    for lazy in (True, False):
        mask, said = _through_class(monkeypatch, cases.cloud("tie"), 1.0, 0.0, False, lazy)
        np.testing.assert_array_equal(mask, cases.expected("tie", False)["mask"])
        assert said == cases.expected("tie", False)["messages"]
    assert len(calls) == 2
    for lazy in (True, False):        # keep_multicluster: no tie to break, no host steps
        mask, _ = _through_class(monkeypatch, cases.cloud("tie"), 1.0, 0.0, True, lazy)
        assert mask.all()
    assert len(calls) == 2


def test_below_the_switch_nothing_changes(gsx, monkeypatch):
    """1024 dense voxels or fewer: the eager class never calls gsx_voxel_clusters; density_filter itself still hands a crowd back"""
    lib = gsx._lib
    calls = []
    real = lib.voxel_clusters
    monkeypatch.setattr(lib, "voxel_clusters", lambda *a, **k: calls.append(1) or real(*a, **k))
    keys = np.concatenate([cases.block((0, 0, 0), (10, 10, 10)), cases.block((20, 0, 0), (4, 3, 2))])      # exactly 1024 voxels
    assert len(keys) == 1024
    xyz = cases.centres(keys, 1.0)
    ref = oden.density_filter(xyz, 1.0, 0.0)
    mask, said = _through_class(monkeypatch, xyz, 1.0, 0.0, False, False)
    np.testing.assert_array_equal(mask, ref["mask"])
    assert said[0] == "Density Filter: Kept 1 clusters (largest: 1000 voxels)." and not calls
    # one voxel more and the device clusters them
    xyz = cases.centres(np.concatenate([keys, [[40, 0, 0]]]), 1.0)
    mask, _ = _through_class(monkeypatch, xyz, 1.0, 0.0, False, False)
    np.testing.assert_array_equal(mask, oden.density_filter(xyz, 1.0, 0.0)["mask"])
    assert len(calls) == 1
    ch = lib.DeviceChain(cases.cloud("crowd"))
    try:
        assert ch.density_filter(0.3, 0, False)["status"] == lib.DENSITY_HOST and ch.n == 60000
    finally:
        ch.close()
