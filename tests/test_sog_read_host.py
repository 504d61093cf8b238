"""-m "not gpu": the SOG reader's host side -- the numpy restatement against the reference's rows (tests/golden/sog_read_ref.npz),
the reference's exceptions before any device work, what is refused and where it goes, the host tables, the staging layout, the
threaded decode's error order, and the install() binding of SogFormat.read with uninstall()'s restoring of read and write."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sog_read_numpy as srn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "sog_read_ref.npz")
EXCEPTIONS = {"builtins.ValueError": ValueError, "builtins.KeyError": KeyError, "builtins.IndexError": IndexError}
N_CASES, N_ERRORS = 40, 14


@pytest.fixture(scope="module")
def gold():
    g = np.load(GOLD)
    return g, json.loads(bytes(g["spec"]).decode())


@pytest.fixture(scope="module")
def reader():
    return importlib.import_module("3dgsconverter_amd.formats.sog_reader")


@pytest.fixture(scope="module")
def lib():
    return importlib.import_module("3dgsconverter_amd._lib")


def _file(g, name, tmp_path):
    p = tmp_path / (name + ".sog")
    p.write_bytes(g[name + "__file"].tobytes())
    return str(p)


def _readable(spec):
    return {n: r for n, r in spec.items() if "error" not in r}


def _assert_case(g, name, rec, rows):
    assert list(rows.dtype.names) == rec["names"] and [rows.dtype[f].str for f in rows.dtype.names] == rec["dtype"], name
    assert rows.dtype.itemsize == rec["itemsize"] and len(rows) == rec["rows"], name
    if name + "__rows" in g:
        assert np.array_equal(np.ascontiguousarray(rows).view(np.uint8).reshape(-1), g[name + "__rows"]), name
    else:
        assert srn.sha(rows) == g[name + "__sha256"].tobytes(), name


class _HostSession:
    """an ArenaSession without a device: staging is plain memory, anything else is device work"""
    asked = []

    def __init__(self, group, device=0, stage_ms=None):
        assert group == "sogread"

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False

    def staging(self, name, nbytes):
        _HostSession.asked.append(nbytes)
        return np.empty(nbytes, np.uint8)

    def __getattr__(self, name):
        raise AssertionError("device work started (%s)" % name)


def _no_device(monkeypatch, lib):
    """the session's staging may be filled (the textures decode into it); nothing may be uploaded or launched"""
    monkeypatch.setattr(lib, "ArenaSession", _HostSession)
    monkeypatch.setattr(lib, "require_hip", lambda: None)
    _HostSession.asked = []


def _model_device(monkeypatch, lib, seen=None):
    """the device entry point replaced by the restatement's decode of the staged texels: what read_sog stages, where, and what
    it hands the table builder are what the rows then depend on"""
    asked = []
    real_tables = lib.sog_read_tables

    def tables_spy(mins, maxs, scale_cb, sh0_cb, shn_cb=None):
        asked.append((mins, maxs, (scale_cb, sh0_cb, shn_cb)))
        return real_tables(mins, maxs, scale_cb, sh0_cb, shn_cb)

    def fake(fill, n_rows, bands, palette, tables, dtype, on_flag=None, stage_ms=None, device=0):
        assert n_rows > 0 and lib.sog_read_table_words(tables).size == 1280 + 3 * 65536
        place, total = lib.sog_texel_layout(n_rows, bands, palette)
        host = np.full(total, 0xEE, np.uint8)
        fill(host, place)
        rows, flag = srn.staged_rows(host, place, n_rows, bands, palette, *asked[-1])
        if seen is not None:
            seen.append((n_rows, bands, palette, total))
        if flag:
            on_flag(host, place)
            raise AssertionError("on_flag did not raise")
        assert rows.dtype == dtype
        return rows
    monkeypatch.setattr(lib, "sog_read_tables", tables_spy)
    monkeypatch.setattr(lib, "sog_unpack_table", fake)


def test_golden_spec_covers_the_cases_the_feature_names(gold):
    _, spec = gold
    ok = _readable(spec)
    assert len(spec) == N_CASES and len(ok) == N_CASES - N_ERRORS
    assert {"b0", "b1", "b2", "b3", "n0_b0", "n0_b2", "larger_textures", "other_width", "modes", "mode_l", "writer_layout", "every_quat_alpha",
            "long_codebooks", "double_codebooks", "smooth_b3"} <= set(ok)
    assert {"palette_%d" % p for p in (1, 63, 64, 65, 128, 300)} <= set(ok)
    assert [spec["b%d" % b]["itemsize"] for b in range(4)] == [68, 104, 164, 248]
    errors = set(spec) - set(ok)
    assert {"err_not_zip", "err_no_meta", "err_missing_key", "err_missing_texture", "err_short_scales", "err_short_sh0", "err_short_shN"} <= errors
    assert {"err_small_" + t for t in srn.TEXTURES} <= errors and len(srn.TEXTURES) == 7
    assert {r["error"][0] for r in spec.values() if "error" in r} == set(EXCEPTIONS)
    assert spec["err_short_shN"]["error"][1] == "index 212 is out of bounds for axis 0 with size 200"


def test_restatement_equals_every_golden_case(gold, tmp_path):
    g, spec = gold
    for name, rec in _readable(spec).items():
        _assert_case(g, name, rec, srn.read(_file(g, name, tmp_path)))
    for name, rec in spec.items():
        if "error" in rec:
            with pytest.raises(EXCEPTIONS[rec["error"][0]]) as e:
                srn.read(_file(g, name, tmp_path))
            assert str(e.value) == rec["error"][1], name


def test_the_readers_centroid_pixel_parts_from_the_writers_above_64_entries(gold, tmp_path):
    """sog.py:192-194 against :584-588 -- the recorded rows of `writer_layout` are NOT what a linear reading would give"""
    i = np.arange(200)[:, None]
    j = np.arange(8)[None, :]
    same = srn.centroid_pixel(i, j, 24) == i * 8 + j
    assert same[:64].all() and not same[64:].any()
    g, spec = gold
    rows = srn.read(_file(g, "writer_layout", tmp_path))
    _assert_case(g, "writer_layout", spec["writer_layout"], rows)


def test_read_sog_through_the_model_of_the_kernel_equals_every_golden_case(gold, reader, lib, tmp_path, monkeypatch):
    """meta.json, the threaded decode into the staging layout, the compacted centroid image, the tables and the dtype"""
    g, spec = gold
    seen = []
    _model_device(monkeypatch, lib, seen)
    for name, rec in _readable(spec).items():
        st = {}
        _assert_case(g, name, rec, reader.read_sog(_file(g, name, tmp_path), stage_ms=st))
        assert "parse" in st, name
    assert len(seen) == N_CASES - N_ERRORS - 2           # the two empty files never reach the device entry point
    n, bands, palette, total = [s for s in seen if s[0] == 20000][0]
    assert total == 6 * 4 * 20000 + 4 * 64 * 15 * 16     # only the first n texels; of the centroid image a third of each row


def test_recorded_errors_are_raised_before_any_device_work(gold, reader, lib, tmp_path, monkeypatch):
    g, spec = gold
    _no_device(monkeypatch, lib)
    errors = {n: r for n, r in spec.items() if "error" in r}
    assert len(errors) == N_ERRORS
    for name, rec in errors.items():
        kind, text = rec["error"]
        _HostSession.asked = []
        with pytest.raises(EXCEPTIONS[kind]) as e:
            reader.read_sog(_file(g, name, tmp_path))
        assert type(e.value) is EXCEPTIONS[kind] and str(e.value) == text, name
        # a texture's size and a short codebook's indices show once the textures are decoded: into the staging, nothing uploaded
        assert len(_HostSession.asked) == (1 if name.startswith(("err_small_", "err_short_")) or name == "err_missing_texture" else 0), name
    for name in ("n0_b0", "n0_b2"):
        _HostSession.asked = []
        rows = reader.read_sog(_file(g, name, tmp_path))
        assert len(rows) == 0 and list(rows.dtype.names) == spec[name]["names"] and not _HostSession.asked


def test_an_empty_file_still_performs_every_read_and_its_errors(reader, lib, tmp_path, monkeypatch):
    _no_device(monkeypatch, lib)
    rng = np.random.default_rng(4)
    t = srn.random_texels(0, 1, 7, rng)
    members = srn.encode_textures(t, 0, 1, 7)
    ok = srn.write_bundle(str(tmp_path / "ok.sog"), srn.meta_for(0, 1, 7, rng), members)
    assert len(reader.read_sog(ok)) == 0
    srn.write_bundle(str(tmp_path / "m.sog"), srn.meta_for(0, 1, 7, rng), {k: v for k, v in members.items() if k != "quats.webp"})
    with pytest.raises(KeyError, match="quats.webp"):
        reader.read_sog(str(tmp_path / "m.sog"))
    small = dict(members)
    small["shN_centroids.webp"] = srn.webp(t["shN_centroids"][:575], 25, 23)
    srn.write_bundle(str(tmp_path / "s.sog"), srn.meta_for(0, 1, 7, rng), small)
    with pytest.raises(ValueError, match="Image shN_centroids.webp too small: 575 < 576"):
        reader.read_sog(str(tmp_path / "s.sog"))
    t["shN_centroids"][:, :3] = 250                      # the palette's own gather does not depend on the row count (:208)
    srn.write_bundle(str(tmp_path / "c.sog"), srn.meta_for(0, 1, 7, rng, sizes=(256, 256, 100)), srn.encode_textures(t, 0, 1, 7))
    for read in (reader.read_sog, srn.read):
        with pytest.raises(IndexError, match="index 250 is out of bounds for axis 0 with size 100"):
            read(str(tmp_path / "c.sog"))
    assert not _HostSession.asked


def test_errors_are_raised_in_texture_order_not_in_completion_order(reader, lib, tmp_path, monkeypatch):
    """two textures fail (outside what the reader promises for the rows, but the order of the pool's results is its own): the
    earlier one by position is raised although it fails last -- its decode is held until the later one has failed.  The pool
    is as wide as the textures, 8 at the most, whatever the machine's CPU count says."""
    import threading
    _no_device(monkeypatch, lib)
    rng = np.random.default_rng(6)
    n = 41
    t = srn.random_texels(n, 0, 0, rng)
    members = srn.encode_textures(t, n)
    members["means_u.webp"] = srn.webp(t["means_u"][:40], 8, 5)
    members["sh0.webp"] = srn.webp(t["sh0"][:40], 8, 5)
    path = srn.write_bundle(str(tmp_path / "two.sog"), srn.meta_for(n, 0, 0, rng), members)
    real = reader._decode_texture
    later_failed = threading.Event()
    order, widths = [], []

    def held(zf, filename, expected):
        if filename == "means_u.webp":
            assert later_failed.wait(60), "sh0.webp was never decoded beside means_u.webp"
        try:
            return real(zf, filename, expected)
        except ValueError:
            order.append(filename)
            raise
        finally:
            if filename == "sh0.webp":
                later_failed.set()

    class Pool(reader.ThreadPoolExecutor):
        def __init__(self, max_workers=None, **kw):
            widths.append(max_workers)
            super().__init__(max_workers=max_workers, **kw)
    monkeypatch.setattr(reader, "_decode_texture", held)
    monkeypatch.setattr(reader, "ThreadPoolExecutor", Pool)
    for cpus in (1, 256):
        monkeypatch.setattr(os, "cpu_count", lambda: cpus)
        later_failed.clear()
        del order[:]
        with pytest.raises(ValueError, match="Image means_u.webp too small: 40 < 41"):
            reader.read_sog(path)
        assert order == ["sh0.webp", "means_u.webp"]
    assert widths == [5, 5] and reader.MAX_DECODE_THREADS == 8
    srn.write_bundle(str(tmp_path / "seven.sog"), srn.meta_for(0, 3, 70, rng), srn.encode_textures(srn.random_texels(0, 3, 70, rng), 0, 3, 70))
    monkeypatch.setattr(reader, "MAX_DECODE_THREADS", 4)
    assert len(reader.read_sog(str(tmp_path / "seven.sog"))) == 0 and widths[-1] == 4


def test_files_the_device_path_does_not_take_go_to_the_fallback_or_raise(reader, lib, tmp_path, monkeypatch):
    _no_device(monkeypatch, lib)
    rng = np.random.default_rng(9)
    n = 12
    t = srn.random_texels(n, 1, 7, rng)
    members = srn.encode_textures(t, n, 1, 7)

    def variant(change):
        meta = srn.meta_for(n, 1, 7, rng)
        change(meta)
        return srn.write_bundle(str(tmp_path / "v.sog"), meta, members)

    def put(section, key, value):
        def change(meta):
            (meta[section] if section else meta)[key] = value
        return change
    changes = [put("shN", "bands", 0), put("shN", "bands", 4), put("shN", "bands", -1), put("shN", "bands", 2.0), put(None, "count", -1),
               put(None, "count", 12.0), put(None, "count", "12"), put(None, "count", True), put("shN", "count", 0), put("shN", "count", 65537),
               put("means", "mins", [0.0, 1.0]), put("means", "maxs", "abc"), put("scales", "codebook", {"a": 1}), put("sh0", "codebook", [1.0, "x"]),
               put("quats", "files", "quats.webp"), put(None, "shN", [1, 2]), put("means", "files", ["means_l.webp"]), put(None, "scales", 3)]
    for change in changes:
        path = variant(change)
        with pytest.raises(reader.UnsupportedSogError, match="does not take this file"):
            reader.read_sog(path)
        assert reader.read_sog(path, fallback=lambda p: ("ref", p)) == ("ref", path)
    assert issubclass(reader.UnsupportedSogError, ValueError) and not _HostSession.asked
    srn.write_bundle(str(tmp_path / "list.sog"), [1, 2, 3], members)
    assert reader.read_sog(str(tmp_path / "list.sog"), fallback=lambda p: "ref") == "ref"


def test_host_tables_are_numpys_results_of_the_references_expressions(lib):
    b = np.arange(256, dtype=np.uint8)
    cb = [[0.5 * k for k in range(256)], [1.25, -3.0], list(range(300))]
    t = lib.sog_read_tables(srn.MINS, srn.MAXS, *cb)
    assert tuple(t) == lib.SOG_READ_TABLES == ("scale_cb", "sh0_cb", "shn_cb", "opacity", "quat", "pos")
    assert all(v.dtype == np.float32 for v in t.values())
    assert [t[k].shape for k in lib.SOG_READ_TABLES] == [(256,), (2,), (300,), (256,), (256,), (3, 65536)]
    qv = np.arange(65536).astype(np.uint16)
    for a in range(3):
        want = srn.position_of(qv, srn.MINS[a], srn.MAXS[a])
        assert want.dtype == np.float64 and t["pos"][a].tobytes() == want.astype(np.float32).tobytes()
    assert (qv / 65535.0).dtype == np.float64                                          # what makes :80-82 float64
    assert t["opacity"].tobytes() == srn.opacity_of(b).tobytes() and srn.opacity_of(b).dtype == np.float32
    assert t["quat"].tobytes() == srn.quat_component_of(b).tobytes() and srn.quat_component_of(b).dtype == np.float32
    assert np.isfinite(t["opacity"]).all() and t["opacity"][0] == t["opacity"][1] < -5 and t["opacity"][255] > 9
    assert t["quat"][0] == -1 and t["quat"][255] == 1 and not (t["quat"] == 0).any()
    assert lib.sog_read_tables(srn.MINS, srn.MAXS, cb[0], cb[1])["shn_cb"].shape == (0,)
    words = lib.sog_read_table_words(t)
    assert words.dtype == np.uint32 and words.size == 1280 + 3 * 65536
    assert np.array_equal(words[:256], t["scale_cb"].view(np.uint32)) and np.array_equal(words[256:258], t["sh0_cb"].view(np.uint32))
    assert not words[258:512].any() and np.array_equal(words[512:768], t["shn_cb"][:256].view(np.uint32))
    assert np.array_equal(words[768:1024], t["opacity"].view(np.uint32)) and np.array_equal(words[1280:], t["pos"].reshape(-1).view(np.uint32))


def test_the_rotation_table_and_the_kernels_order_of_operations_give_numpys_sum_of_squares(lib):
    """np.sum(q_rest ** 2, axis=1) of the reference (:115) against what csrc/sog_read.hip computes -- the entries of the host's
    `quat` table, (c0 c0 + c1 c1) + c2 c2 in float32 -- on 2^18 byte triples that include the ones next to a sum of 1 (all
    2^24, on the device: tests/devtools/check_sog_read_quat.py)"""
    rng = np.random.default_rng(2)
    tri = np.concatenate([rng.integers(0, 256, (1 << 18, 3), dtype=np.uint8), srn.edge_triples()])
    quat = lib.sog_read_tables(srn.MINS, srn.MAXS, [0.0], [0.0])["quat"]
    c = [quat[tri[:, a]] for a in range(3)]
    mine = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]
    assert mine.dtype == np.float32
    theirs = np.sum(((tri.astype(np.float32) / 255.0 - 0.5) * 2.0) ** 2, axis=1)
    assert np.array_equal(mine, theirs)
    assert (mine[-4:-2] < 1).all() and (mine[-2:] > 1).all() and np.abs(mine[-4:] - 1).max() < 1e-4


def test_staging_layout_holds_only_what_the_kernel_reads(lib):
    place, total = lib.sog_texel_layout(1001, 3, 130)
    assert list(place) == list(lib.SOG_READ_TEXTURES) and total % 16 == 0
    assert all(off % 16 == 0 for off, _ in place.values())
    assert [place[k][1] for k in lib.SOG_READ_TEXTURES[:6]] == [4004] * 6 and place["shN_centroids"][1] == 4 * 64 * 15 * 3
    ends = sorted((off, off + nb) for off, nb in place.values())
    assert all(a[1] <= b[0] for a, b in zip(ends, ends[1:])) and ends[-1][1] <= total
    place0, total0 = lib.sog_texel_layout(5, 0, 0)
    assert list(place0) == list(lib.SOG_READ_TEXTURES[:5]) and total0 == 5 * 32
    assert lib.sog_texel_layout(1, 3, 65536)[0]["shN_centroids"][1] == 3932160       # 3.9 MB at the most


_STANDIN = {
    "gsconverter/__init__.py": "",
    "gsconverter/processing/__init__.py": "from . import gpu_ops\nfrom .data_processor import DataProcessor\n",
    "gsconverter/processing/gpu_ops.py": "HAS_TAICHI = False\n",
    "gsconverter/processing/data_processor.py": "class DataProcessor:\n    def __init__(self, data):\n        self.data = data\n",
    "gsconverter/converter.py": "from .processing import DataProcessor\n",
    "gsconverter/formats/__init__.py": "",
    "gsconverter/formats/sog.py": ("from ..processing import gpu_ops\n\nclass SogFormat:\n    def read(self, path, **kw):\n        return ('own', path, kw)\n"
                                   "    def write(self, data, path, **kw):\n        return 'w'\n"),
    "gsconverter/formats/splat.py": ("class SplatFormat:\n    def read(self, path, **kw):\n        return 'splat rows'\n"
                                     "    def write(self, data, path, **kw):\n        return 'w'\n"),
}


def test_install_rebinds_sog_read_on_a_stand_in_and_uninstall_restores_read_and_write(gsx, gold, reader, lib, tmp_path, monkeypatch):
    g, spec = gold
    for rel, src in _STANDIN.items():
        (tmp_path / rel).parent.mkdir(parents=True, exist_ok=True)
        (tmp_path / rel).write_text(src)
    saved = {m: sys.modules.pop(m) for m in list(sys.modules) if m == "gsconverter" or m.startswith("gsconverter.")}
    mine = importlib.import_module("3dgsconverter_amd.processing.data_processor")
    monkeypatch.setattr(mine, "_REFERENCE_CLASS", None)
    monkeypatch.syspath_prepend(str(tmp_path))
    _model_device(monkeypatch, lib)
    try:
        import gsconverter.formats.sog as rsog
        import gsconverter.formats.splat as rsplat
        own = (rsog.SogFormat.read, rsog.SogFormat.write, rsplat.SplatFormat.read, rsplat.SplatFormat.write)

        def now():
            return (rsog.SogFormat.read, rsog.SogFormat.write, rsplat.SplatFormat.read, rsplat.SplatFormat.write)
        rng = np.random.default_rng(12)
        meta = srn.meta_for(12, 1, 7, rng)
        meta["shN"]["bands"] = 4
        refused = str(tmp_path / "bands4.sog")
        srn.write_bundle(refused, meta, srn.encode_textures(srn.random_texels(12, 1, 7, rng), 12, 1, 7))
        try:
            gsx.install(sog_reader=False)
            assert now()[0] is own[0] and now()[1] is not own[1] and now()[2] is own[2] and now()[3] is not own[3]
            gsx.uninstall()
            assert now() == own
            gsx.install(sog_writer=False, splat_writer=False)
            assert now()[0] is not own[0] and now()[1:] == own[1:]
            gsx.uninstall()
            assert now() == own                       # a saved ("sogformat", "read") goes back to read, not over write
            gsx.install()
            assert now()[0] is not own[0] and now()[1] is not own[1] and now()[2] is own[2] and now()[3] is not own[3]
            assert rsog.SogFormat.read.__wrapped__ is own[0]
            rows = rsog.SogFormat().read(_file(g, "palette_65", tmp_path))
            _assert_case(g, "palette_65", spec["palette_65"], rows)
            assert rsog.SogFormat().read(refused, extra=1) == ("own", refused, {"extra": 1})     # a refused file: the original's result
            assert reader.read_sog(refused) == ("own", refused, {})                             # read_sog itself finds the saved original
            with pytest.raises(IndexError, match="index 212"):
                rsog.SogFormat().read(_file(g, "err_short_sh0", tmp_path))
        finally:
            gsx.uninstall()
        assert now() == own
        with pytest.raises(reader.UnsupportedSogError):
            reader.read_sog(refused)
    finally:
        for m in [m for m in sys.modules if m == "gsconverter" or m.startswith("gsconverter.")]:
            del sys.modules[m]
        sys.modules.update(saved)


def test_install_and_uninstall_on_the_reference_itself(gsx):
    from oracle import refload
    if not refload.available():
        pytest.skip("the reference is not mounted")
    refload.load()
    import gsconverter.formats.sog as rsog  # type: ignore
    import gsconverter.formats.splat as rsplat  # type: ignore
    own = (rsog.SogFormat.read, rsog.SogFormat.write, rsplat.SplatFormat.read, rsplat.SplatFormat.write)
    gsx.install()
    try:
        assert rsog.SogFormat.read.__wrapped__ is own[0] and rsog.SogFormat.write is not own[1] and rsplat.SplatFormat.write is not own[3]
    finally:
        gsx.uninstall()
    assert (rsog.SogFormat.read, rsog.SogFormat.write, rsplat.SplatFormat.read, rsplat.SplatFormat.write) == own


def test_golden_file_regenerates_identically_when_the_reference_is_there(tmp_path):
    from oracle import refload
    if not refload.available():
        pytest.skip("the reference is not mounted")
    env = dict(os.environ, PYTHONWARNINGS="ignore")
    code = ("import sys, runpy; sys.path.insert(0, %r); m = runpy.run_path(%r); m['main'].__globals__['OUT'] = %r; m['main']()"
            % (ROOT, os.path.join(ROOT, "tests", "devtools", "make_golden_sog_read.py"), str(tmp_path / "again.npz")))
    subprocess.run([sys.executable, "-c", code], check=True, env=env, capture_output=True, cwd=ROOT)
    a, b = np.load(GOLD), np.load(str(tmp_path / "again.npz"))
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
