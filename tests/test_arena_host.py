"""CPU: the process-wide DeviceArena (3dgsconverter_amd/_lib.py) and its users under concurrency, without a GPU.

The arena keeps named GROW-ONLY buffers: growing one frees the old allocation.  Every buffer belongs to a lease group (the part
of its name before the first "_") and is only served while that group is leased, so two threads never share one.  Here the
device calls are stubbed and only the allocator is faked (numpy memory; a "freed" block is poisoned with NaN bytes but stays
mapped): the real grow-only and lease logic, the real threaded host gathers and the real DataProcessor / DeviceChain code run.
threading.Event forces the one interleaving that hurts: thread A gathers, thread B gathers and finishes, then A reads."""
import ctypes
import importlib
import threading
import types

import numpy as np
import pytest

L = importlib.import_module("3dgsconverter_amd._lib")
dp = importlib.import_module("3dgsconverter_amd.processing.data_processor")

WAIT = 20.0     # seconds an event may take before the test gives up (a wrong lock would otherwise hang the suite)


class _StubArray:
    """a device allocation: remembers what was uploaded into it"""

    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes, self.ptr, self.freed, self.uploaded = ctx, int(nbytes), 1, False, None

    def upload(self, arr):
        self.uploaded = np.array(arr, copy=True)
        return self

    def free(self):
        self.freed, self.ptr = True, None


class _StubLib:
    """page-locked host memory as numpy blocks; a free fills the block with 0xff (NaN as float32) and keeps it alive"""

    def __init__(self):
        self.blocks, self.freed = {}, []

    def gsx_host_pinned_alloc(self, handle, nbytes, pref):
        a = np.zeros(int(nbytes), np.uint8)
        self.blocks[a.ctypes.data] = a
        pref._obj.value = a.ctypes.data
        return 0

    def gsx_host_pinned_free(self, handle, ptr):
        a = self.blocks.pop(ptr.value)
        a[:] = 0xFF
        self.freed.append(a)
        return 0


@pytest.fixture
def fake(monkeypatch):
    """_lib.Context -> a stub (no GPU); a fresh, empty arena registry"""
    stub_lib = _StubLib()

    class StubContext:
        lib = stub_lib
        made = []

        def __init__(self, device=0, stream=None, own_stream=False):
            self.handle, self.own_stream, self.params = 1, own_stream, {}
            StubContext.made.append(self)

        def alloc(self, nbytes):
            return _StubArray(self, nbytes)

        def set_param(self, name, value):
            self.params[name] = value

        def synchronize(self):
            pass

        def close(self):
            self.handle = None

    monkeypatch.setattr(L, "Context", StubContext)
    monkeypatch.setattr(L, "_arenas", {})
    return StubContext


def _table(n, seed):
    dt = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("f_dc_0", "<f4"), ("f_dc_1", "<f4"), ("f_dc_2", "<f4"),
                   ("opacity", "<f4")])
    rng = np.random.default_rng(seed)
    t = np.zeros(n, dt)
    for nm in dt.names:
        t[nm] = rng.standard_normal(n).astype(np.float32) * 10
    return t


def _cols(t, names):
    return np.column_stack([t[nm] for nm in names]).astype(np.float32)


# ---- the arena's rule ---------------------------------------------------------------------------------------------------

def test_lease_groups_are_the_name_before_the_first_underscore():
    g = L.DeviceArena.group
    assert [g(n) for n in ("eager_xyz", "rgb_in", "chain_list3", "sog_12", "cply_unc_count", "spz_rows", "ksplat_body",
                           "splat_rows")] == ["eager", "rgb", "chain", "sog", "cply", "spz", "ksplat", "splat"]


def test_unleased_group_is_refused(fake):
    ar = L.DeviceArena(0)
    for call in (lambda: ar.buf("sog_rows", 64), lambda: ar.pinned("eager_xyz", 64), lambda: ar.context("cply"),
                 lambda: ar.side("sog")):
        with pytest.raises(RuntimeError, match="lease"):
            call()
    assert not ar._bufs and not ar._pinned and not fake.made       # nothing was allocated on the way to the refusal
    with ar.leased("sog") as won:
        assert won
        with pytest.raises(RuntimeError, match="'cply'"):          # another group's lease does not cover it
            ar.buf("cply_rows", 64)
        with pytest.raises(RuntimeError, match="'eager'"):
            ar.pinned("eager_xyz", 64)


def test_leased_group_grows_and_keeps_its_buffers(fake):
    ar = L.DeviceArena(0)
    with ar.leased("sog") as won:
        assert won
        assert not ar.lease("sog")                                 # one holder at a time
        b = ar.buf("sog_rows", 1000)
        assert b.nbytes >= 1000 and ar.buf("sog_rows", 10) is b     # grow-only: a smaller request is the same buffer
        b2 = ar.buf("sog_rows", 5000)
        assert b.freed and not b2.freed and b2.nbytes >= 5000
        assert b2.ctx is ar.context("sog")                         # allocated on the group's own context ...
        p = ar.pinned("sog_host", 100)
        assert p.dtype == np.uint8 and len(p) >= 100
        with ar.leased("cply"):
            assert ar.context("cply") is not ar.context("sog")     # ... which no other group shares
            assert ar.side("sog") is not ar.context("sog") and ar.side("sog").own_stream
    assert not ar._leases


def test_context_manager_returns_the_lease_on_an_exception(fake):
    ar = L.DeviceArena(0)
    with pytest.raises(ZeroDivisionError):
        with ar.leased("spz") as won:
            assert won
            ar.buf("spz_rows", 64)
            1 / 0
    assert "spz" not in ar._leases
    with ar.leased("spz") as won:
        assert won
    with ar.leased("spz") as won:
        with ar.leased("spz") as won2:                            # a second user at the same moment does not get it ...
            assert won and not won2
        assert "spz" in ar._leases                                 # ... and leaving its block does not take the first one's


def test_release_arenas_spares_a_leased_arena(fake):
    ar = L.arena(0)
    assert ar.lease("cply")
    b = ar.buf("cply_rows", 256)
    ar.unlease("cply")
    assert ar.lease("eager")
    p = ar.pinned("eager_xyz", 1200)
    p[:] = 7
    L.release_arenas()
    assert L.arena(0) is ar and not b.freed and np.all(p == 7)    # the eager lease keeps the whole arena: cply_rows too
    ar.unlease("eager")
    L.release_arenas()
    assert b.freed and len(fake.lib.freed) == 1 and np.all(p == 0xFF)
    assert all(c.handle is None for c in fake.made)                # every context of the arena closed
    assert not ar.lease("eager")                                   # a released arena hands out no more leases
    assert L.arena(0) is not ar


# ---- eager DataProcessors on two threads --------------------------------------------------------------------------------

class _Race:
    """the first stub call of thread A blocks until thread B has run its whole method; every stub records a copy of what it
    was handed AFTER that point, i.e. what A's device call would read"""

    def __init__(self):
        self.a_in, self.b_done = threading.Event(), threading.Event()
        self.seen, self.errors = [], []

    def hit(self, stub, arr):
        if threading.current_thread().name == "A" and not self.a_in.is_set():
            self.a_in.set()
            if not self.b_done.wait(WAIT):
                raise AssertionError("thread B did not finish")
        self.seen.append((threading.current_thread().name, stub, np.array(arr, copy=True)))

    def run(self, method_a, method_b):
        def a():
            try:
                method_a()
            except BaseException as e:      # noqa: BLE001
                self.errors.append(("A", repr(e)))

        def b():
            try:
                if not self.a_in.wait(WAIT):
                    raise AssertionError("thread A never reached its device call")
                method_b()
            except BaseException as e:      # noqa: BLE001
                self.errors.append(("B", repr(e)))
            finally:
                self.b_done.set()
        th = [threading.Thread(target=a, name="A"), threading.Thread(target=b, name="B")]
        for t in th:
            t.start()
        for t in th:
            t.join(3 * WAIT)
        assert not any(t.is_alive() for t in th), "a thread hangs"
        assert not self.errors, self.errors


@pytest.fixture
def stubs(monkeypatch, fake):
    race = _Race()

    def sor_filter(xyz, k, threshold_factor, want_mean=False):
        race.hit("sor_filter", xyz)
        return {"mean": 0.0, "std": 0.0, "threshold": 0.0, "mask": np.ones(len(xyz), bool)}

    def density_voxels(cols, voxel_size, min_points):
        race.hit("density_voxels", cols)
        return {"n_unique": 1, "dense_keys": np.zeros((1, 3), np.int64), "dense_counts": np.array([len(cols)], np.int64)}

    def density_mask(cols, voxel_size, kept_keys):
        race.hit("density_mask", cols)
        return np.ones(len(cols), bool)

    def rgb_from_sh(f_dc):
        race.hit("rgb_from_sh", np.asarray(f_dc).reshape(-1, 3))
        return np.zeros(len(f_dc), np.uint8)

    for nm, f in (("sor_filter", sor_filter), ("density_voxels", density_voxels), ("density_mask", density_mask),
                  ("rgb_from_sh", rgb_from_sh)):
        monkeypatch.setattr(L, nm, f)
    monkeypatch.setattr(L, "require_hip", L.load)                 # (add_rgb_from_sh asks for the device before it gathers)
    return race


@pytest.mark.parametrize("method,stub_names,cols", [
    ("remove_flyers", ["sor_filter"], ("x", "y", "z")),
    ("apply_density_filter", ["density_voxels", "density_mask"], ("x", "y", "z")),
    ("add_rgb_from_sh", ["rgb_from_sh"], ("f_dc_0", "f_dc_1", "f_dc_2")),
])
def test_two_eager_processors_each_see_their_own_rows(stubs, method, stub_names, cols):
    """A gathers (>= 65 536 rows: the arena's page-locked buffer), B -- a larger table, so the buffer would grow and free A's --
    gathers and finishes, then A's device call reads its input: it must still be A's columns"""
    ta, tb = _table(70_001, 1), _table(100_003, 2)
    pa, pb = dp.DataProcessor(ta), dp.DataProcessor(tb)
    stubs.run(getattr(pa, method), getattr(pb, method))
    want = {"A": _cols(ta, cols), "B": _cols(tb, cols)}
    for who in "AB":
        got = [(stub, arr) for w, stub, arr in stubs.seen if w == who]
        assert [s for s, _ in got] == stub_names, (who, got)
        for stub, arr in got:
            np.testing.assert_array_equal(arr, want[who], err_msg="%s's %s read another table's rows" % (who, stub))
    ar = L.arena(0)
    name = "rgb_in" if method == "add_rgb_from_sh" else "eager_xyz"
    assert ar._pinned[name][1] == 12 * len(ta)       # the lease holder's buffer, never grown under it
    assert not ar._leases                            # every lease given back


def test_lone_eager_processor_gathers_into_the_arena(stubs):
    """one caller at a time always wins the lease: the page-locked path of round 6, unchanged"""
    t = _table(80_000, 3)
    stubs.a_in.set()
    stubs.b_done.set()
    dp.DataProcessor(t).remove_flyers()
    dp.DataProcessor(t).add_rgb_from_sh()
    ar = L.arena(0)
    assert ar._pinned["eager_xyz"][1] == ar._pinned["rgb_in"][1] == 12 * len(t)
    assert not ar._leases
    np.testing.assert_array_equal(stubs.seen[0][2], _cols(t, ("x", "y", "z")))


def test_small_eager_tables_do_not_touch_the_arena(stubs):
    t = _table(1000, 4)
    stubs.a_in.set()
    stubs.b_done.set()
    dp.DataProcessor(t).remove_flyers()
    assert not L._arenas or not L.arena(0)._pinned


# ---- DeviceChain: the lease before the gather ---------------------------------------------------------------------------

def test_two_device_chains_built_at_once_upload_their_own_rows(fake, monkeypatch):
    """A's chain gathers its coordinates, B's chain (larger table) gathers too, then A uploads: B must not have written (or
    grown and freed) the pinned chain_xyz buffer A uploads from.  The lease is taken before the gather; the loser gathers
    into an array of its own and runs on a private context"""
    monkeypatch.setattr(L, "require_hip", L.load)
    real = L.host_gather_xyz
    a_gathered, b_gathered = threading.Event(), threading.Event()

    def gather(vertices, names=("x", "y", "z"), out=None, exact=True):
        r = real(vertices, names, out=out, exact=exact)
        if threading.current_thread().name == "A":
            a_gathered.set()
            if not b_gathered.wait(WAIT):
                raise AssertionError("thread B never gathered")
        else:
            b_gathered.set()
        return r
    monkeypatch.setattr(L, "host_gather_xyz", gather)
    ta, tb = _table(5000, 5), _table(9000, 6)
    chains, errors = {}, []

    def build(name, t, wait):
        try:
            if wait is not None and not wait.wait(WAIT):
                raise AssertionError("thread A never gathered")
            chains[name] = L.DeviceChain(table=t)
        except BaseException as e:      # noqa: BLE001
            errors.append((name, repr(e)))
            b_gathered.set()
    th = [threading.Thread(target=build, args=("A", ta, None), name="A"),
          threading.Thread(target=build, args=("B", tb, a_gathered), name="B")]
    for t in th:
        t.start()
    for t in th:
        t.join(3 * WAIT)
    try:
        assert not any(t.is_alive() for t in th) and not errors, errors
        for name, t in (("A", ta), ("B", tb)):
            np.testing.assert_array_equal(chains[name].rows.uploaded, _cols(t, ("x", "y", "z")),
                                          err_msg="chain %s uploaded another table's rows" % name)
        ar = L.arena(0)
        assert ar._pinned["chain_xyz"][1] == 12 * len(ta)
        assert sum(c._ar is not None for c in chains.values()) == 1 and ar._leases == {"chain"}
    finally:
        for c in chains.values():
            c.close()
    assert not L.arena(0)._leases


def test_device_chain_that_loses_the_lease_leaves_chain_xyz_alone(fake, monkeypatch):
    monkeypatch.setattr(L, "require_hip", L.load)
    ta, tb = _table(6000, 7), _table(12000, 8)
    first = L.DeviceChain(table=ta)
    try:
        held = L.arena(0).pinned("chain_xyz", 1).copy()            # (the lease holder may look)
        second = L.DeviceChain(table=tb)
        try:
            assert second._ar is None and first._ar is not None
            np.testing.assert_array_equal(L.arena(0).pinned("chain_xyz", 1), held)
            np.testing.assert_array_equal(second.rows.uploaded, _cols(tb, ("x", "y", "z")))
        finally:
            second.close()
        assert second.ctx is None and all(b.freed for b in (second.rows, second.spare, second.mask))
    finally:
        first.close()
    assert not L.arena(0)._leases


# ---- ArenaSession: one call's use of a lease group (the six table readers and writers) ----------------------------------

GROUPS = ("cply", "spz", "ksplat", "splat", "cplyread", "ksread")


@pytest.mark.parametrize("group", GROUPS)
def test_session_with_the_lease_runs_on_the_arena(fake, group):
    with L.ArenaSession(group, 0) as s:
        ar = L.arena(0)
        assert s.leased and ar._leases == {group} and s.ctx is ar.context(group)
        b = s.buf("rows", 1000)
        assert b is ar._bufs[group + "_rows"] and b.ctx is ar.context(group) and b.nbytes >= 1000
    assert not ar._leases and not b.freed and L.arena(0) is ar
    assert all(c.handle is not None for c in fake.made)            # the arena keeps its context
    with L.ArenaSession(group, 0) as s:
        assert s.buf("rows", 10) is b                              # a second call finds the buffer


def test_session_without_the_lease_is_private_and_cleans_up(fake):
    ar = L.arena(0)
    assert ar.lease("spz")                                         # another user of the group, mid-call
    made = len(fake.made)
    with L.ArenaSession("spz", 0) as s:
        assert not s.leased and len(fake.made) == made + 1 and s.ctx is fake.made[-1]
        ctx, bufs = s.ctx, [s.buf("rows", 1000), s.buf("count", 0)]
        assert bufs[0].ctx is ctx and bufs[1].nbytes == 16 and not ar._bufs
        assert not any(b.freed for b in bufs) and ctx.handle is not None
    assert all(b.freed for b in bufs) and ctx.handle is None
    assert ar._leases == {"spz"} and not ar._bufs and L.arena(0) is ar


def test_session_without_the_lease_frees_its_buffers_before_its_context(fake):
    ar = L.arena(0)
    assert ar.lease("ksread")
    order = []
    with L.ArenaSession("ksread", 0) as s:
        b = s.buf("in", 64)
        b.free = lambda: order.append("free")
        s.ctx.close = lambda: order.append("close")
    assert order == ["free", "close"]


def test_session_gsx_error_gives_the_lease_back_and_releases_the_arena(fake):
    with pytest.raises(L.GsxError, match="boom"):
        with L.ArenaSession("ksplat", 0) as s:
            ar, b = L.arena(0), s.buf("rows", 64)
            raise L.GsxError("boom")
    assert not ar._leases and ar.closed and b.freed and all(c.handle is None for c in fake.made)
    assert L.arena(0) is not ar


def test_session_gsx_error_spares_an_arena_another_group_holds(fake):
    ar = L.arena(0)
    assert ar.lease("chain")                                       # e.g. a DeviceChain with pending filters
    with pytest.raises(L.GsxError):
        with L.ArenaSession("ksplat", 0) as s:
            b = s.buf("rows", 64)
            raise L.GsxError("boom")
    assert ar._leases == {"chain"} and not ar.closed and not b.freed and L.arena(0) is ar


def test_session_gsx_error_without_the_lease_leaves_the_arena_alone(fake):
    ar = L.arena(0)
    assert ar.lease("splat")
    kept = ar.buf("splat_rows", 64)
    with pytest.raises(L.GsxError):
        with L.ArenaSession("splat", 0) as s:
            ctx, b = s.ctx, s.buf("rows", 64)
            raise L.GsxError("boom")
    assert b.freed and ctx.handle is None
    assert ar._leases == {"splat"} and not ar.closed and not kept.freed


def test_session_other_exception_keeps_the_arena(fake):
    with pytest.raises(ZeroDivisionError):
        with L.ArenaSession("cplyread", 0) as s:
            ar, b = L.arena(0), s.buf("in", 64)
            1 / 0
    assert not ar._leases and not ar.closed and not b.freed and L.arena(0) is ar
    assert ar._bufs["cplyread_in"] is b


def test_session_gives_the_lease_back_when_its_context_cannot_be_made(fake, monkeypatch):
    ar = L.arena(0)

    def no_context(device=0, stream=None, own_stream=False):
        raise L.GsxError("gsx_ctx_create: no device")
    monkeypatch.setattr(L, "Context", no_context)
    with pytest.raises(L.GsxError, match="gsx_ctx_create"):
        with L.ArenaSession("spz", 0):
            raise AssertionError("the block must not run")
    assert not ar._leases and ar.closed and L.arena(0) is not ar   # a GsxError with the lease won: the arena is released too
    assert L.arena(0).lease("ksplat")
    with pytest.raises(L.GsxError, match="gsx_ctx_create"):        # and a private context that cannot be made has nothing to undo
        with L.ArenaSession("ksplat", 0):
            raise AssertionError("the block must not run")
    assert L.arena(0)._leases == {"ksplat"}


def test_session_on_a_callers_context_takes_no_lease_and_does_not_close_it(fake):
    mine = fake()
    with L.ArenaSession("cply", 0, ctx=mine, shared=False) as s:
        assert s.ctx is mine and not s.leased
        b = s.buf("mat", 100)
        assert b.ctx is mine
    assert b.freed and mine.handle is not None and fake.made == [mine] and not L._arenas
    with pytest.raises(L.GsxError):
        with L.ArenaSession("cply", 0, ctx=mine) as s:              # (a context decides it: shared or not, the arena is not asked)
            raise L.GsxError("boom")
    assert mine.handle is not None and not L._arenas


def test_session_that_is_not_shared_never_asks_the_arena(fake):
    with L.ArenaSession("cply", 0, shared=False) as s:             # cply_pack_table's rows that are not resident
        assert not s.leased and s.ctx is fake.made[-1] and not L._arenas
        ctx = s.ctx
    assert ctx.handle is None and not L._arenas


def test_session_stage_clock(fake, monkeypatch):
    syncs = []
    monkeypatch.setattr(fake, "synchronize", lambda self: syncs.append(self))
    with L.ArenaSession("spz", 0, None) as s:
        s.mark("a")
        s.mark("b")
    assert not syncs                                               # no clock asked for: no synchronisation
    ticks = iter([10.0, 10.0012344, 10.0032344, 10.5])
    monkeypatch.setattr(L, "time", types.SimpleNamespace(perf_counter=lambda: next(ticks)))
    st = {}
    with L.ArenaSession("spz", 0, st) as s:                        # the clock starts here
        s.mark("a")
        assert st == {"a": 1.234} and len(syncs) == 1
        s.mark("a")
        assert len(syncs) == 2 and syncs[0] is s.ctx
        s.mark("b")
    assert list(st) == ["a", "b"] and st["a"] == 3.234 and st["b"] == 496.766
    assert all(round(v, 3) == v for v in st.values())


def test_session_staging_is_page_locked_only_under_the_lease(fake):
    with L.ArenaSession("ksread", 0) as s:
        ar = L.arena(0)
        h = s.staging("in", 1000)
        addr, size = ar._pinned["ksread_in"]
        assert h.dtype == np.uint8 and len(h) == 1000 and h.ctypes.data == addr and size >= 1000
        with L.ArenaSession("ksread", 0) as t:                     # a second user at the same moment
            p = t.staging("in", 1000)
            assert not t.leased and p.dtype == np.uint8 and p.shape == (1000,) and p.ctypes.data != addr
            assert list(ar._pinned) == ["ksread_in"]
    assert not ar._leases


def test_session_uploads_page_locked_staging_plainly_and_pageable_staging_through_the_lanes(fake):
    calls = []

    class Lib:
        def gsx_dev_upload(self, handle, dst, src, nbytes):
            calls.append(("plain", dst, src, nbytes))
            return 0

        def gsx_dev_upload_staged(self, handle, dst, src, nbytes):
            calls.append(("staged", dst, src, nbytes))
            return 0
    with L.ArenaSession("cplyread", 0) as s, L.ArenaSession("cplyread", 0) as t:
        hs, ht = s.staging("in", 48), t.staging("in", 32)
        s.upload_staging(Lib(), 7, hs)
        t.upload_staging(Lib(), 9, ht)
    assert calls == [("plain", 7, hs.ctypes.data, 48), ("staged", 9, ht.ctypes.data, 32)]


# ---- the six table readers: one sequence (stage_in, ArenaSession.upload_in, .download_rows) -----------------------------

class _ReaderLib:
    """every gsx_* entry point a reader calls is recorded and answers 0; the staged download fills its destination with 0xAB"""

    def __init__(self, events):
        self.events = events

    def __getattr__(self, name):
        def call(*args):
            self.events.append(name)
            if name == "gsx_dev_download_staged":
                ctypes.memset(args[1], 0xAB, args[3])
            return 0
        return call


@pytest.fixture
def reader(fake, monkeypatch):
    """-> the list of events of one reader call: "staging", "fill" (the caller's fill, or read_exact), then the device work --
    "alloc" / "upload" / "download" of a device buffer and the name of every entry point"""
    events = []

    class Array(_StubArray):
        def upload(self, arr):
            events.append("upload")
            return super().upload(arr)

        def download(self, dtype, count):
            events.append("download")
            return np.zeros(count, dtype)

    def alloc(self, nbytes):
        events.append("alloc")
        return Array(self, nbytes)

    def staging(self, name, nbytes, real=L.ArenaSession.staging):
        events.append("staging")
        return real(self, name, nbytes)

    def read_exact(f, view, *a, real=L.read_exact, **k):
        events.append("fill")
        return real(f, view, *a, **k)
    monkeypatch.setattr(fake, "alloc", alloc)
    monkeypatch.setattr(L.ArenaSession, "staging", staging)
    monkeypatch.setattr(L, "read_exact", read_exact)
    monkeypatch.setattr(L, "require_hip", lambda: _ReaderLib(events))
    monkeypatch.setattr(L, "_np_log_checked", True)
    return events


def _rows_dtype(itemsize):
    return np.dtype([("b", "u1", (itemsize,))])


def _file(tmp_path, nbytes):
    p = tmp_path / "body.bin"
    p.write_bytes(bytes(nbytes))
    return str(p)


class _Damaged(Exception):
    pass


def _fill(events, good):
    def fill(view, place=None):
        events.append("fill")
        if not good:
            raise _Damaged("the stream ends early")
        view[:] = 1
    return fill


SOG_PLACE_BYTES = 6 * 32 + 768      # n = 5, one band, a palette of 1: six textures of 20 -> 32 bytes, one centroid row of 4 * 64 * 3


def _read_cply(tmp_path, events, good, st):
    seg = {"chunk": (0, 72), "vertex": (72, 16 * 300), "sh": None}
    return L.cply_unpack_table(_file(tmp_path, 72 + 16 * 300 - (0 if good else 1)), seg, L.CplyReadLayout(), 1, 300, _rows_dtype(68), st)


def _read_ksplat(tmp_path, events, good, st):
    return L.ksplat_unpack_table(_file(tmp_path, 108 if good else 107), 8, 100, 0, [L.KsplatReadSection()], np.arange(2), 0, 3, _rows_dtype(68), st)


def _read_spz(tmp_path, events, good, st):
    return L.spz_unpack_table(_fill(events, good), 95, 2, 0, 12, 5, _rows_dtype(71), st, fill_stage="gunzip")


def _read_sog(tmp_path, events, good, st):
    tables = dict(zip(L.SOG_READ_TABLES, [np.zeros(256, np.float32)] * 5 + [np.zeros((3, 65536), np.float32)]))
    return L.sog_unpack_table(_fill(events, good), 5, 1, 1, tables, _rows_dtype(104), stage_ms=st)


def _read_splat(tmp_path, events, good, st):
    return L.splat_unpack_table(_file(tmp_path, 128 if good else 127), 4, _rows_dtype(71), st)


def _read_ply(tmp_path, events, good, st):
    lay = L.PlyReadLayout(in_stride=20, out_stride=12)
    return L.ply_unpack_table(_file(tmp_path, 21 + 60 - (0 if good else 1)), 21, 3, lay, _rows_dtype(12), st)


# group -> (the call, the stage clock's keys, the arena's buffers in the order they are asked for: (name, bytes), what a short file raises)
READERS = {
    "cplyread": (_read_cply, ["file_read", "upload", "kernel", "download"],
                 [("in", 96 + 4816), ("tables", 8 * 4352 + 4 * 512), ("out", 256 * 68)], ValueError),
    "ksread": (_read_ksplat, ["file_read", "upload", "kernel", "download"],
               [("in", 100 + 32), ("tables", 4 * 512), ("prefix", 16), ("out", 3 * 68)], ValueError),
    "spzread": (_read_spz, ["gunzip", "upload", "kernel", "download"],
                [("in", 95 + 32), ("tables", 4 * 2560), ("out", 5 * 71)], _Damaged),
    "sogread": (_read_sog, ["decode", "upload", "kernel", "download"],
                [("in", SOG_PLACE_BYTES + 32), ("tables", 4 * (1280 + 3 * 65536)), ("flag", 16), ("out", 5 * 104)], _Damaged),
    "splatread": (_read_splat, ["file_read", "upload", "kernel", "download"],
                  [("in", 4 * 32), ("tables", 4 * 512), ("out", 4 * 71)], ValueError),
    "plyread": (_read_ply, ["file_read", "upload", "kernel", "download"],
                [("in", 96), ("out", 3 * 12)], ValueError),       # 5 bytes before row 0, 60 of rows, 16 spare: 81 -> 96
}


@pytest.mark.parametrize("group", list(READERS))
def test_reader_stages_and_fills_before_any_device_work(reader, tmp_path, group):
    call, stages, bufs, _ = READERS[group]
    st = {}
    rows = call(tmp_path, reader, True, st)
    assert reader[0] == "staging" and reader[1] == "fill", reader
    first = [e for e in reader if e not in ("staging", "fill")][0]
    assert first == "alloc" and reader.index("alloc") > max(i for i, e in enumerate(reader) if e == "fill"), reader
    entry = {"cplyread": "gsx_cply_unpack_dev", "ksread": "gsx_ksplat_unpack_dev", "spzread": "gsx_spz_unpack_dev",
             "sogread": "gsx_sog_unpack_dev", "splatread": "gsx_splat_unpack_dev", "plyread": "gsx_ply_unpack_dev"}[group]
    assert reader.count(entry) == 1 and reader.count("gsx_dev_download_staged") == 1 and reader[-1] == "gsx_dev_download_staged"
    assert reader.index("gsx_dev_upload") < reader.index(entry) < reader.index("gsx_dev_download_staged")
    assert list(st) == stages
    ar = L.arena(0)
    assert [(name, b.nbytes - 256) for name, b in ar._bufs.items()] == [(group + "_" + name, size) for name, size in bufs]
    staged = {"cplyread": 96 + 4816, "ksread": 100, "spzread": 95, "sogread": SOG_PLACE_BYTES, "splatread": 4 * 32, "plyread": 96}[group]
    assert list(ar._pinned) == [group + "_in"] and ar._pinned[group + "_in"][1] == staged
    assert not ar._leases and not ar.closed
    flat = rows.view(np.uint8).reshape(len(rows), -1)
    n_dec = 256 if group == "cplyread" else len(rows)
    assert np.all(flat[:n_dec] == 0xAB) and not flat[n_dec:].any()       # the download's bytes; compressed PLY: zero past 256 n_chunks
    assert len(rows) == {"cplyread": 300, "ksread": 3, "spzread": 5, "sogread": 5, "splatread": 4, "plyread": 3}[group]


@pytest.mark.parametrize("group", list(READERS))
def test_reader_whose_fill_raises_has_done_no_device_work(reader, tmp_path, group):
    call, _, _, error = READERS[group]
    st = {}
    with pytest.raises(error) as e:
        call(tmp_path, reader, False, st)
    assert "early" in str(e.value)                                       # read_exact's message, or the fill's own: unchanged
    assert set(reader) == {"staging", "fill"} and reader[0] == "staging", reader
    ar = L.arena(0)
    assert not ar._leases and not ar.closed and not ar._bufs and list(ar._pinned) == [group + "_in"]
    assert not st                                                        # not even the fill stage's mark
    with L.ArenaSession(group, 0) as s:                                  # the lease is there for the next call
        assert s.leased


def test_read_exact_fills_the_view_or_names_the_early_end(tmp_path):
    p = tmp_path / "body.bin"
    p.write_bytes(bytes(range(100)))
    buf = np.zeros(100, np.uint8)
    with open(p, "rb") as f:
        f.seek(10)
        L.read_exact(f, buf[:90], str(p))
        assert bytes(buf[:90]) == bytes(range(10, 100)) and f.tell() == 100
    with open(p, "rb") as f:
        f.seek(40)
        with pytest.raises(ValueError) as e:
            L.read_exact(f, buf[:90], "a%b.ply", " in element %r" % "vertex")
        assert str(e.value) == "a%b.ply: early end of file in element 'vertex' (60 of 90 bytes)"
    with open(p, "rb") as f:
        with pytest.raises(ValueError) as e:
            L.read_exact(f, np.zeros(101, np.uint8), "x.ksplat", unit="payload bytes")
        assert str(e.value) == "x.ksplat: early end of file (100 of 101 payload bytes)"
