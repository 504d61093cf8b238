"""-m "not gpu": the host side of the resident rows, no device touched -- the eligibility rule as a function of two dtypes and the
row counts, ``ResidentRows.close`` and the readers' ``keep=`` bookkeeping (``with_keep``) on stand-ins, and ``Converter`` when the
reader kept nothing, kept rows the processor does not take, or was told not to keep."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resident_cases as rc  # noqa: E402

lib = importlib.import_module("3dgsconverter_amd._lib")
conv = importlib.import_module("3dgsconverter_amd.converter")
dp = importlib.import_module("3dgsconverter_amd.processing.data_processor")


class _Freed:
    def __init__(self):
        self.calls = 0

    def free(self):
        self.calls += 1

    close = free


def stub_rows(n, dtype):
    """a ResidentRows that owns stand-ins instead of a context and a buffer"""
    rr = object.__new__(lib.ResidentRows)
    rr.n, rr.dtype, rr.device, rr.first_byte, rr.ptr = int(n), np.dtype(dtype), 0, 0, 4096
    rr._buf, rr._ctx = _Freed(), _Freed()
    lib.ResidentRows.open_count += 1
    return rr


def test_close_is_idempotent_and_counts():
    before = lib.ResidentRows.open_count
    rr = stub_rows(5, rc.scene(1, np.random.default_rng(0)).dtype)
    buf, ctx = rr._buf, rr._ctx
    assert lib.ResidentRows.open_count == before + 1 and not rr.closed and rr.nbytes == 5 * 248
    rr.close()
    rr.close()
    assert rr.closed and rr.ptr is None and (buf.calls, ctx.calls) == (1, 1) and lib.ResidentRows.open_count == before
    with pytest.raises(ValueError, match="closed"):
        rr.download()
    rr.__del__()
    assert lib.ResidentRows.open_count == before


def test_eligibility_is_a_function_of_two_dtypes_and_the_counts():
    f4 = rc.scene(1, np.random.default_rng(0)).dtype
    with_rgb = np.dtype(f4.descr + [("red", "u1"), ("green", "u1"), ("blue", "u1")])
    ok = lib.resident_eligible
    assert ok(f4, 10, f4, 10) and ok(with_rgb, 1, with_rgb, 1)
    assert ok(np.dtype(f4.descr), 10, f4, 10)                                      # an equal dtype, not the same object
    assert not ok(f4, 10, f4, 11) and not ok(f4, 0, f4, 0) and not ok(f4, 10, with_rgb, 10) and not ok(None, 10, f4, 10)
    for name in ("x", "opacity", "f_dc_1", "f_rest_44"):                           # a field the processor reads as words, of another type
        for other in ("<f8", ">f4", "<f2", "<i4"):
            dt = np.dtype([(nm, other if nm == name else "<f4") for nm in f4.names])
            assert not ok(dt, 10, dt, 10), (name, other)
            assert lib.resident_same_rows(dt, 10, dt, 10) == (dt.itemsize <= 512)   # (the writer's rule asks for shapes alone)
    other_field = np.dtype(f4.descr + [("label", "<i8"), ("tag", "u1")])           # fields the processor does not read: any type
    assert ok(other_field, 3, other_field, 3)
    no_z = np.dtype([(nm, "<f4") for nm in f4.names if nm != "z"])
    assert not ok(no_z, 3, no_z, 3)
    no_opacity = np.dtype([(nm, "<f4") for nm in f4.names if nm != "opacity"])
    assert ok(no_opacity, 3, no_opacity, 3)
    wide = np.dtype(f4.descr + [("pad", "u1", (300,))])
    assert wide.itemsize > 512 and not ok(wide, 3, wide, 3) and not lib.resident_same_rows(wide, 3, wide, 3)
    assert not ok(np.dtype("<f4"), 3, np.dtype("<f4"), 3)                          # no structured dtype
    t = np.zeros(4, f4)
    rr = stub_rows(4, f4)
    assert lib.resident_matches(rr, t) and not lib.resident_matches(rr, t[:3]) and not lib.resident_matches(None, t)
    rr.close()
    assert not lib.resident_matches(rr, t)


def test_with_keep_drops_rows_that_are_not_the_returned_tables():
    f4 = rc.scene(1, np.random.default_rng(0)).dtype
    table, other = np.zeros(4, f4), np.zeros(4, f4)
    before = lib.ResidentRows.open_count

    def reader(keep, returns, rows_of, fail=False):
        def read():
            rr = stub_rows(len(rows_of), rows_of.dtype)
            keep["rows"], keep["table"] = rr, rows_of
            made.append(rr)
            if fail:
                raise ValueError("a damaged file")
            return returns
        return read
    made = []
    keep = {"stale": 1}
    assert lib.with_keep(keep, reader(keep, (table, "extras"), table))[0] is table
    assert sorted(keep) == ["rows"] and keep["rows"] is made[0] and not made[0].closed
    made[0].close()
    keep = {}
    assert lib.with_keep(keep, reader(keep, other, table)) is other                # a fallback's table: not the rows' own
    assert keep == {} and made[1].closed
    keep = {}
    with pytest.raises(ValueError, match="a damaged file"):
        lib.with_keep(keep, reader(keep, table, table, fail=True))
    assert keep == {} and made[2].closed
    keep = {}
    assert lib.with_keep(keep, lambda: table) is table and keep == {}              # a reader that kept nothing
    assert lib.with_keep(None, lambda: table) is table
    assert lib.keep_kw(None) == {} and lib.keep_kw(keep) == {"keep": keep}
    assert lib.ResidentRows.open_count == before


BIG_510 = np.dtype([(nm, "<f4") for nm in ["x", "y", "z", "f_dc_0", "f_dc_1", "f_dc_2", "opacity"] + ["f_rest_%d" % i for i in range(45)]]
                   + [("more_%d" % i, "<f4") for i in range(75)] + [("tail", "u1", (2,))])


def test_the_take_is_refused_by_the_widened_dtype_alone():
    f4 = rc.scene(1, np.random.default_rng(0)).dtype
    rgb = ("red", "green", "blue")
    wide = lib.resident_take_dtype(f4, rgb)
    assert f4.itemsize == 248 and wide.itemsize == 251 and wide.names[:-3] == f4.names
    assert [wide.fields[nm][1] for nm in rgb] == [248, 249, 250] and all(wide[nm] == np.dtype("u1") for nm in rgb)
    assert lib.resident_take_dtype(f4) == f4 and lib.resident_take_dtype(f4, ()) == f4
    assert BIG_510.itemsize == 510 and lib.resident_eligible(BIG_510, 33, BIG_510, 33)
    assert lib.resident_take_dtype(BIG_510) == BIG_510 and lib.resident_take_dtype(BIG_510, rgb) is None      # 513 > RESIDENT_MAX_ROW_BYTES
    assert lib.resident_take_dtype(BIG_510, ("red", "green")).itemsize == 512
    # an aligned dtype: `descr` names its 3 bytes of padding as a field of their own, ('', '|V3') behind 'tag', so the dtype built
    # from descr + the colours is packed, 16 + 3 bytes, with the colours at 16, 17, 18.  The expression this rule was taken from
    # (tail_ok: every colour at itemsize + i; and new itemsize == itemsize + 3 <= 512), evaluated by hand on it: True, 19 == 19,
    # 19 <= 512 -> taken.  So is it here
    aligned = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("tag", "u1")], align=True)
    assert aligned.itemsize == 16 and aligned.descr[-1] == ("", "|V3")
    got = lib.resident_take_dtype(aligned, rgb)
    assert got is not None and got.itemsize == 19 and [got.fields[nm][1] for nm in rgb] == [16, 17, 18]
    assert [got.fields[nm][1] for nm in ("x", "y", "z", "tag")] == [0, 4, 8, 12]
    # ... and ResidentRows.take answers None before it makes anything
    before = lib.ResidentRows.open_count
    rr = stub_rows(33, BIG_510)
    assert rr.take(None, 33, (), 4096, rgb) is None and lib.ResidentRows.open_count == before + 1 and not rr.closed
    rr.close()


class _TakingRows:
    """the processor's resident rows: ``take`` records what it was asked for and answers with stand-in rows of that shape"""

    def __init__(self, table):
        self.n, self.dtype, self.device, self.first_byte, self.ptr = len(table), table.dtype, 0, 0, 4096
        self.asked, self.closed, self.made = [], False, []

    def take(self, idx_ptr, n_out, zero_names=(), extra_ptr=None, extra_names=(), ctx=None, stage_ms=None):
        self.asked.append(dict(idx_ptr=idx_ptr, n_out=n_out, zero=list(zero_names), extra_ptr=extra_ptr, extra=tuple(extra_names), ctx=ctx))
        out = stub_rows(n_out, lib.resident_take_dtype(self.dtype, extra_names))
        out.download_into = lambda host: host                                      # (no device: the table stays as allocated)
        self.made.append(out)
        return out

    def close(self):
        self.closed = True


class _Buffer:
    def __init__(self, ptr):
        self.ptr, self.uploaded, self.freed = ptr, None, 0

    def upload(self, arr):
        self.uploaded = arr
        return self

    def free(self):
        self.freed += 1


def chain_over(rows, n, empty=False, orig=0x2000):
    """a DeviceChain over `rows` that never saw a device: its state after filters left `n` rows (a survivor list at `orig`, or
    None before any filter ran), a private chain (no arena) whose buffers are stand-ins"""
    ch = object.__new__(lib.DeviceChain)
    ch.resident, ch.n0, ch.n, ch.empty, ch.ctx, ch._ar = rows, rows.n, n, empty, "chain-ctx", None
    ch.orig = _Buffer(orig) if orig is not None else None
    ch.bufs = []
    ch._alloc = lambda nbytes, name: ch.bufs.append((name, nbytes, _Buffer(0x3000))) or ch.bufs[-1][2]
    ch.close = lambda: setattr(ch, "ctx", None)                                   # (DeviceChain.close with no context: nothing to do)
    return ch


def test_the_chain_selects_the_survivor_list_and_releases_the_colours():
    table = rc.scene(8, np.random.default_rng(2))
    before = lib.ResidentRows.open_count
    rgb3 = ("red", "green", "blue")
    rows = _TakingRows(table)
    out = chain_over(rows, 5).take(["f_rest_44"])                                  # a compaction happened: the composed list
    assert rows.asked[-1] == dict(idx_ptr=0x2000, n_out=5, zero=["f_rest_44"], extra_ptr=None, extra=(), ctx="chain-ctx")
    assert out is rows.made[-1] and out.n == 5 and out.dtype == table.dtype
    chain_over(rows, 8).take()                                                     # filters ran and removed nothing: the identity
    assert rows.asked[-1] == dict(idx_ptr=None, n_out=8, zero=[], extra_ptr=None, extra=(), ctx="chain-ctx")
    chain_over(rows, 8, orig=None).take()                                          # no filter ran
    assert rows.asked[-1]["idx_ptr"] is None and rows.asked[-1]["n_out"] == 8
    ch = chain_over(rows, 0, empty=True, orig=None)                                # keep_none() as the first filter
    host_rgb = np.arange(24, dtype=np.uint8).reshape(8, 3)
    out = ch.take((), host_rgb)
    assert rows.asked[-1] == dict(idx_ptr=None, n_out=0, zero=[], extra_ptr=None, extra=rgb3, ctx="chain-ctx")
    assert out.n == 0 and out.dtype.itemsize == 251 and ch.bufs == []             # no row: nothing uploaded
    ch = chain_over(rows, 5)                                                       # host colours: uploaded into "rgbhost", freed after
    ch.take(["f_rest_9"], host_rgb)
    (name, nbytes, buf), = ch.bufs
    assert (name, nbytes) == ("rgbhost", 3 * 8 + 16) and buf.uploaded.tobytes() == host_rgb.tobytes() and buf.freed == 1
    assert rows.asked[-1] == dict(idx_ptr=0x2000, n_out=5, zero=["f_rest_9"], extra_ptr=0x3000, extra=rgb3, ctx="chain-ctx")
    dev = object.__new__(lib.DeviceArray)                                          # the chain's own device colours: freed after
    dev.ptr, freed = 0x5000, []
    dev.free = lambda: freed.append(1)
    ch = chain_over(rows, 5)
    ch.take((), dev)
    assert rows.asked[-1]["extra_ptr"] == 0x5000 and rows.asked[-1]["extra"] == rgb3 and freed == [1] and ch.bufs == []
    rows.take = lambda *a, **k: (_ for _ in ()).throw(lib.GsxError("a failed launch"))
    ch, freed[:] = chain_over(rows, 5), []
    with pytest.raises(lib.GsxError, match="a failed launch"):
        ch.take((), dev)
    assert freed == [1]                                                            # ... on every way out
    for made in rows.made:
        made.close()
    assert lib.ResidentRows.open_count == before


class _Chain:
    """the public surface of a DeviceChain the processor's ``.data`` reads"""

    def __init__(self, rows, n, empty=False):
        self.rows, self.n0, self.n, self.empty, self.ctx = rows, rows.n, n, empty, "chain-ctx"
        self.asked, self.closed = [], 0

    def take(self, zero_names=(), rgb=None, stage_ms=None):
        self.asked.append((list(zero_names), rgb))
        return self.rows.take("survivors" if self.n != self.n0 else None, self.n, zero_names, None if rgb is None else "colours",
                              ("red", "green", "blue") if rgb is not None else (), ctx=self.ctx, stage_ms=stage_ms)

    def close(self):
        self.closed += 1


@pytest.mark.parametrize("case", ["nothing_pending", "zero_fields_only", "chain_removed_rows", "chain_after_keep_none", "host_colours"])
def test_what_data_asks_the_rows_in_hbm_for(case):
    table = rc.scene(8, np.random.default_rng(3))
    before = lib.ResidentRows.open_count
    rows = _TakingRows(table)
    p = dp.ChainedDataProcessor(table, resident=rows)
    assert p._rr is rows
    colours = np.arange(24, dtype=np.uint8).reshape(8, 3)
    ch = None
    if case in ("chain_removed_rows", "host_colours"):
        p._chain = ch = _Chain(rows, 5)
    elif case == "chain_after_keep_none":
        p._chain = ch = _Chain(rows, 0, empty=True)
    if case == "zero_fields_only":
        assert p.cap_sh_degree(2) is None
    if case == "host_colours":
        p.cap_sh_degree(0)
        p._pending_rgb = colours
    data = p.data
    if case == "nothing_pending":
        assert rows.asked == [] and data is table and p.resident is rows and not rows.closed and p.resident_ms == {"take": 0.0}
        p.close()
        assert rows.closed
        return
    asked, = rows.asked
    want = {"zero_fields_only": dict(idx_ptr=None, n_out=8, zero=["f_rest_%d" % i for i in range(24, 45)], extra_ptr=None, extra=(), ctx=None),
            "chain_removed_rows": dict(idx_ptr="survivors", n_out=5, zero=[], extra_ptr=None, extra=(), ctx="chain-ctx"),
            "chain_after_keep_none": dict(idx_ptr="survivors", n_out=0, zero=[], extra_ptr=None, extra=(), ctx="chain-ctx"),
            "host_colours": dict(idx_ptr="survivors", n_out=5, zero=sorted("f_rest_%d" % i for i in range(45)), extra_ptr="colours",
                                 extra=("red", "green", "blue"), ctx="chain-ctx")}[case]
    assert asked == want
    if ch is not None:
        assert ch.closed == 1 and p._chain is None and (ch.asked[0][1] is colours) == (case == "host_colours")
    out, = rows.made
    assert rows.closed and p.resident is out and not out.closed                     # the source rows are closed, the new ones owned
    assert data is p.data and len(data) == want["n_out"] and data.dtype == out.dtype and data is not table
    assert p._pending_zero == [] and p._pending_rgb is None
    assert ("download" in p.resident_ms) == (want["n_out"] > 0) and (want["n_out"] > 0 or p.resident_ms == {"take": 0.0})
    p.close()
    assert out.closed and lib.ResidentRows.open_count == before


def test_a_failed_take_closes_the_rows_and_the_chain():
    table = rc.scene(8, np.random.default_rng(3))
    before = lib.ResidentRows.open_count
    rows = _TakingRows(table)
    p = dp.ChainedDataProcessor(table, resident=rows)
    p._chain = ch = _Chain(rows, 5)
    ch.take = lambda *a, **k: (_ for _ in ()).throw(lib.GsxError("a failed launch"))
    with pytest.raises(lib.GsxError, match="a failed launch"):
        p.data
    assert rows.closed and ch.closed == 1 and p._rr is None and p._chain is None and p._data is table
    assert lib.ResidentRows.open_count == before


class _Handler(conv.SourceHandler):
    """a format handler without a device: read() hands out a table, its profile and -- like the readers -- rows it kept or not"""
    table, rows, written = None, None, None

    def read(self, path, stage_ms=None):
        self.opens += 1
        self.profile = {"rest_nonzero": (1 << 45) - 1, "lo": (0.0,) * 3, "hi": (1.0,) * 3, "nan_axes": 0, "n": len(self.table)}
        self.resident = type(self).rows(self.table) if (self.keep and type(self).rows is not None) else None
        return self.table

    def write(self, data, path, stage_ms=None, **kwargs):
        type(self).written = (data, dict(kwargs))


@pytest.fixture()
def modelled(monkeypatch, tmp_path):
    src = tmp_path / "scene.spz"
    src.write_bytes(b"")
    _Handler.table, _Handler.rows, _Handler.written = rc.scene(50, np.random.default_rng(4)), None, None
    monkeypatch.setattr(conv.Converter, "_get_format_handler",
                        lambda self, name: setattr(h := _Handler(name), "keep", self.resident) or h)
    return str(src), str(tmp_path / "out.ply")


def test_converter_when_the_reader_kept_nothing(modelled, capsys):
    src, dst = modelled
    before = lib.ResidentRows.open_count
    c = conv.Converter(src, dst, "3dgs")
    assert c.resident is True
    c.run()
    data, kwargs = _Handler.written
    assert data is _Handler.table and "resident" not in kwargs
    assert "process" in c.stage_ms and not any(k.startswith("process_") for k in c.stage_ms)
    assert capsys.readouterr().out.strip().split("\n")[-1] == "Conversion completed: Saved to %s" % dst
    assert lib.ResidentRows.open_count == before


def test_converter_closes_rows_the_processor_does_not_take(modelled):
    src, dst = modelled
    before = lib.ResidentRows.open_count
    made = []
    _Handler.rows = staticmethod(lambda table: made.append(stub_rows(len(table) - 1, table.dtype)) or made[-1])   # the rows of another table
    c = conv.Converter(src, dst, "3dgs")
    c.run()
    assert len(made) == 1 and made[0].closed and lib.ResidentRows.open_count == before
    assert _Handler.written[0] is _Handler.table and not any(k.startswith("process_") for k in c.stage_ms)
    c = conv.Converter(src, dst, "3dgs")                                           # a load without a run: close() frees what was kept
    c.load_source_only()
    assert len(made) == 2 and not made[1].closed
    c.close()
    c.close()
    assert made[1].closed and lib.ResidentRows.open_count == before
    c = conv.Converter(src, dst, "3dgs", resident=False)                           # told not to keep: the reader is not asked
    c.run()
    assert len(made) == 2 and c.resident is False


def test_converter_closes_the_kept_rows_when_a_step_fails(modelled, monkeypatch):
    src, dst = modelled
    before = lib.ResidentRows.open_count
    made = []
    _Handler.rows = staticmethod(lambda table: made.append(stub_rows(len(table), table.dtype)) or made[-1])       # rows the processor takes
    monkeypatch.setattr(_Handler, "write", lambda self, *a, **k: (_ for _ in ()).throw(OSError("disk full")))
    c = conv.Converter(src, dst, "3dgs")
    with pytest.raises(OSError, match="disk full"):
        c.run()                                                                    # (no filter, no pending work: no device call)
    assert len(made) == 1 and made[0].closed and lib.ResidentRows.open_count == before
    assert c.stage_ms.get("process_take") == 0.0


def test_an_eager_processor_closes_its_resident_rows():
    table = rc.scene(8, np.random.default_rng(1))
    rr = stub_rows(8, table.dtype)
    p = dp.DataProcessor(table, lazy=False, resident=rr)
    assert rr.closed and p._rr is None and p.data is table
    rr = stub_rows(8, table.dtype)
    p = dp.ChainedDataProcessor(table, resident=rr)
    assert p._rr is rr and p.resident is rr and p.data is table and p.resident_ms == {"take": 0.0}
    p.data = table[:4]                                                             # another table: the rows were the old one's
    assert rr.closed and p.resident is None
    p.close()
