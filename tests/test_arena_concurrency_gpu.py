"""-m gpu: every user of the process-wide DeviceArena (3dgsconverter_amd/_lib.py) on several threads of one process at once.

The arena's named buffers are grow-only: growing one frees the old allocation.  Every user holds the lease of its buffers'
group for as long as it uses them, and a second user of the same group at the same moment runs on private allocations.
Each case first computes every output sequentially (that path is pinned to the reference's fixtures by the writers' and
filters' own tests), then runs the threads -- each on a different table, the second one larger, so that a buffer grown
mid-call would free memory the other thread still uses -- and requires identical bytes."""
import gzip
import importlib
import io
import os
import sys
import threading
import time
import zipfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spz_numpy  # noqa: E402
from oracle import datasets  # noqa: E402

pytestmark = pytest.mark.gpu

L = importlib.import_module("3dgsconverter_amd._lib")
dp = importlib.import_module("3dgsconverter_amd.processing.data_processor")
sd = importlib.import_module("3dgsconverter_amd.formats.sog_device")
W = {nm: importlib.import_module("3dgsconverter_amd.formats." + nm) for nm in
     ("sog_writer", "compressed_ply_writer", "spz_writer", "splat_writer", "ksplat_writer")}

JOIN_S = 300

_seed = threading.local()


@pytest.fixture(autouse=True)
def per_call_draws(monkeypatch):
    """the SOG write seeds its draws from numpy's global stream, which threads share: each call here gets a seed of its own,
    the same one in the sequential run and in the threads"""
    monkeypatch.setattr(sd, "_draws", lambda: np.random.default_rng(_seed.value))
    yield
    L.release_arenas()


def _run(jobs):
    """jobs: callables started together (threading.Barrier); -> their results; any exception fails the test"""
    start = threading.Barrier(len(jobs))
    out, errors = [None] * len(jobs), []

    def run(i):
        try:
            start.wait()
            out[i] = jobs[i]()
        except BaseException as e:      # noqa: BLE001
            errors.append((i, repr(e)))
    th = [threading.Thread(target=run, args=(i,)) for i in range(len(jobs))]
    for t in th:
        t.start()
    for t in th:
        t.join(JOIN_S)
    assert not any(t.is_alive() for t in th), "a thread hangs"
    assert not errors, errors
    return out


# ---- one call of each user -> its output as bytes -------------------------------------------------------------------------

def _sog(table, path, seed, level=5):
    _seed.value = seed
    W["sog_writer"].write_sog(table, str(path), compression_level=level, device_resident=True)   # (True: NotEligible raises)
    with zipfile.ZipFile(str(path)) as zf:       # (members, not the archive: its entries carry the time they were written)
        return {nm: zf.read(nm) for nm in zf.namelist()}


def _cply(table, path):
    W["compressed_ply_writer"].write_compressed_ply(table, str(path))
    return path.read_bytes()


def _spz(table, path):
    W["spz_writer"].write_spz(table, str(path), compression_level=0)
    return gzip.decompress(path.read_bytes())


def _splat(table, path):
    W["splat_writer"].write_splat(table, str(path))
    return path.read_bytes()


def _ksplat(table, path):
    W["ksplat_writer"].write_ksplat(table, str(path), 1)
    return path.read_bytes()


def _eager(table):
    p = dp.DataProcessor(table)
    p.remove_flyers(k=16, threshold_factor=2.0)
    p.apply_density_filter(voxel_size=2.0, threshold_percentage=0.05)
    p.add_rgb_from_sh()
    d = p.data
    return d.dtype.descr, d.tobytes()


def _lazy(table):
    p = dp.DataProcessor(table, lazy=True)
    p.apply_density_filter(voxel_size=2.0, threshold_percentage=0.05)
    p.remove_flyers(k=16, threshold_factor=2.0)
    d = p.data
    return d.dtype.descr, d.tobytes()


def _scene(n, seed):
    return datasets.sog_scene(n, seed)


def _assert_same(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "%s: output %d differs from its sequential result" % (what, i)


# ---- the cases ------------------------------------------------------------------------------------------------------------

def test_two_sog_writes_at_once(gsx, tmp_path):
    """race: two write_sog calls on the same sog_* buffers and the arena's sog contexts (ar.context / ar.side); the second
    call now runs on a private arena"""
    tables = [_scene(150_000, 1), _scene(300_001, 2)]
    want = [_sog(t, tmp_path / ("seq%d.sog" % i), 100 + i) for i, t in enumerate(tables)]
    assert "sog_0" in L.arena(0)._bufs       # the device-resident core ran on the arena

    def job(i):
        return lambda: [_sog(tables[i], tmp_path / ("t%d_%d.sog" % (i, r)), 100 + i) for r in range(3)]
    got = _run([job(0), job(1)])
    for i in range(2):
        _assert_same(got[i], [want[i]] * 3, "sog %d" % i)


def test_two_compressed_ply_writes_at_once(gsx, tmp_path):
    """race: two resident-row compressed-PLY writes on the same cply_* buffers and context"""
    tables = [_scene(200_000, 3), _scene(350_001, 4)]
    want = [_cply(t, tmp_path / ("seq%d.ply" % i)) for i, t in enumerate(tables)]
    assert "cply_rows" in L.arena(0)._bufs   # n >= 1024, contiguous <f4 fields: the resident path

    def job(i):
        return lambda: [_cply(tables[i], tmp_path / ("t%d_%d.ply" % (i, r))) for r in range(3)]
    got = _run([job(0), job(1)])
    for i in range(2):
        _assert_same(got[i], [want[i]] * 3, "compressed ply %d" % i)


def test_two_eager_processors_at_once(gsx):
    """race: two eager DataProcessors gathering into the pinned eager_xyz / rgb_in buffers, which their device calls read"""
    tables = [_scene(150_000, 5), _scene(250_001, 6)]
    want = [_eager(t) for t in tables]
    assert {"eager_xyz", "rgb_in"} <= set(L.arena(0)._pinned)     # >= 65 536 rows: the page-locked staging path
    got = _run([lambda t=t: [_eager(t) for _ in range(2)] for t in tables])
    for i in range(2):
        _assert_same(got[i], [want[i]] * 2, "eager %d" % i)


def test_two_lazy_processors_built_at_once(gsx):
    """race: DeviceChain.__init__ checking for the chain lease, gathering into chain_xyz and leasing only afterwards"""
    tables = [_scene(120_000, 7), _scene(200_001, 8)]
    want = [_lazy(t) for t in tables]
    assert "chain_xyz" in L.arena(0)._pinned
    got = _run([lambda t=t: [_lazy(t) for _ in range(2)] for t in tables])
    for i in range(2):
        _assert_same(got[i], [want[i]] * 2, "lazy %d" % i)


def test_every_user_at_once_and_a_release_in_between(gsx, tmp_path):
    """races: users of different lease groups that shared one context (and its per-context work buffers) before each group
    got its own, and release_arenas() freeing the buffers of whoever held no lease"""
    t = {"sog": _scene(150_000, 9), "cply": _scene(200_000, 10), "splat": spz_numpy.random_table(300_000, 11, rgb=True),
         "spz": spz_numpy.random_table(250_000, 12), "ksplat": spz_numpy.random_table(200_001, 13),
         "eager": _scene(150_000, 14), "lazy": _scene(120_000, 15)}
    calls = {"sog": lambda p: _sog(t["sog"], p, 7), "cply": lambda p: _cply(t["cply"], p), "splat": lambda p: _splat(t["splat"], p),
             "spz": lambda p: _spz(t["spz"], p), "ksplat": lambda p: _ksplat(t["ksplat"], p),
             "eager": lambda p: _eager(t["eager"]), "lazy": lambda p: _lazy(t["lazy"])}
    names = sorted(calls)
    want = {nm: calls[nm](tmp_path / ("seq_" + nm)) for nm in names}
    released = []

    def releaser():
        for _ in range(4):
            time.sleep(0.05)
            L.release_arenas()
            released.append(1)

    def job(nm):
        return lambda: [calls[nm](tmp_path / ("%s_%d" % (nm, r))) for r in range(2)]
    got = _run([job(nm) for nm in names] + [releaser])
    assert len(released) == 4
    for nm, g in zip(names, got):
        _assert_same(g, [want[nm]] * 2, nm)


def test_a_failing_writer_does_not_free_a_running_sog_write(gsx, tmp_path, monkeypatch):
    """race: a writer's GsxError path calls release_arenas() while another thread's SOG write is on the arena"""
    table = _scene(300_001, 16)
    want = _sog(table, tmp_path / "seq.sog", 9)
    spz_table = spz_numpy.random_table(100_000, 17)

    def injected(*a, **k):
        raise L.GsxError("injected failure")
    monkeypatch.setattr(L, "spz_layout", injected)      # (inside spz_pack_table's try: its GsxError path runs)

    def failing():
        n = 0
        for r in range(6):
            try:
                _spz(spz_table, tmp_path / ("f%d.spz" % r))
            except L.GsxError as e:
                assert "injected" in str(e)
                n += 1
            time.sleep(0.02)
        return n
    got = _run([lambda: [_sog(table, tmp_path / ("t%d.sog" % r), 9) for r in range(3)], failing])
    _assert_same(got[0], [want] * 3, "sog next to a failing writer")
    assert got[1] == 6
