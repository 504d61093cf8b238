"""-m "not gpu": the SPZ reader's host side -- the numpy restatement against the reference's rows (tests/golden/spz_read_ref.npz),
the header, the streamed inflate and the reference's exceptions before any device work, what is refused and where it goes, the
host tables, the bounded staging, and the install() binding of SpzFormat.read."""
import gzip
import importlib
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spz_read_numpy as srn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "spz_read_ref.npz")
EXCEPTIONS = {"builtins.ValueError": ValueError, "builtins.EOFError": EOFError, "gzip.BadGzipFile": gzip.BadGzipFile}
N_CASES, N_ERRORS = 71, 36


@pytest.fixture(scope="module")
def gold():
    g = np.load(GOLD)
    return g, json.loads(bytes(g["spec"]).decode())


@pytest.fixture(scope="module")
def reader():
    return importlib.import_module("3dgsconverter_amd.formats.spz_reader")


@pytest.fixture(scope="module")
def lib():
    return importlib.import_module("3dgsconverter_amd._lib")


def _file(g, name, tmp_path):
    p = tmp_path / (name + ".spz")
    p.write_bytes(g[name + "__file"].tobytes())
    return str(p)


def _readable(spec):
    return {n: r for n, r in spec.items() if "error" not in r and n != "degree4"}


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
        assert group == "spzread"

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
    """the session's staging may be filled (a gzip stream's end shows only then); nothing may be uploaded or launched"""
    monkeypatch.setattr(lib, "ArenaSession", _HostSession)
    monkeypatch.setattr(lib, "require_hip", lambda: None)
    _HostSession.asked = []


def _model_device(monkeypatch, lib):
    """the device entry point replaced by the restatement's decode of the staged bytes"""
    def fake(fill, body_bytes, version, degree, bits, n_rows, dtype, stage_ms=None, device=0, fill_stage="file_read"):
        assert body_bytes == srn.body_bytes(version, degree, n_rows) and n_rows > 0
        host = np.full(body_bytes, 0xEE, np.uint8)
        fill(host)
        rows = srn.decode(host.tobytes(), version, n_rows, degree, bits)
        assert rows.dtype == dtype
        return rows
    monkeypatch.setattr(lib, "spz_unpack_table", fake)


def test_golden_spec_covers_the_cases_the_feature_names(gold):
    _, spec = gold
    ok = _readable(spec)
    assert len(spec) == N_CASES and len(ok) == N_CASES - N_ERRORS - 1
    for v in (1, 2, 3):
        for d in (0, 1, 2, 3):
            assert "v%d_d%d" % (v, d) in ok
    assert {"bits0", "bits12", "bits24", "bits127", "bits128", "bits255", "n0_v1", "n0_v3", "n0_plain", "plain", "gzip0", "gzip6", "gzip9",
            "two_members", "zero_padding", "bytes_after_body", "bytes_after_body_plain", "flags_reserved"} <= set(ok)
    assert {"err_trailing_garbage", "err_truncated_stream", "err_crc", "err_short_plain", "err_gzip_magic_only", "err_magic", "err_version0",
            "err_version4"} <= set(spec) - set(ok)
    assert len([n for n in spec if n.startswith("err_short_v")]) == 17       # one byte short at the end of each section
    assert spec["degree4"]["rows"] == 9 and len(spec["degree4"]["names"]) == 17 + 72 + 3 and "dtype" not in spec["degree4"]
    assert spec["larger_v1"]["nan_words"] > 0 and {r["error"][0] for r in spec.values() if "error" in r} == set(EXCEPTIONS)


def test_restatement_equals_every_golden_case(gold, tmp_path):
    g, spec = gold
    for name, rec in _readable(spec).items():
        _assert_case(g, name, rec, srn.read(_file(g, name, tmp_path)))
    for name, rec in spec.items():
        if "error" in rec:
            with pytest.raises(EXCEPTIONS[rec["error"][0]]) as e:
                srn.read(_file(g, name, tmp_path))
            assert str(e.value) == rec["error"][1], name


def test_restated_dtypes_are_the_ones_the_arithmetic_notes_name():
    b, c = np.arange(256, dtype=np.uint8), np.arange(1024, dtype=np.uint32)
    assert srn.opacity_of(b).dtype == srn.f_dc_of(b).dtype == srn.sh_of(b).dtype == srn.legacy_component_of(b).dtype == np.float32
    assert srn.scale_of(b).dtype == np.float64 and srn.v3_component_of(c).dtype == np.float64
    v = srn.v3_component_of(c)
    assert np.array_equal(v, v.astype(np.float32).astype(np.float64))         # float32 values carried as float64
    assert np.signbit(v[512]) and v[512] == 0 and v[511] == np.float32(np.float32(1.0) * np.float32(0.707106781186547524401))
    with np.errstate(all="ignore"):
        q = np.array([5, -5, 0], np.int32).astype(np.float32) / (1 << 128)     # the divisor is float32: inf
    assert q.dtype == np.float32 and list(q.view(np.uint32)) == [0, 0x80000000, 0]


def test_read_spz_through_the_model_of_the_device_equals_every_golden_case(gold, reader, lib, tmp_path, monkeypatch):
    """the header, both ways of filling the staging (file read, streamed inflate across members and padding) and the dtype"""
    g, spec = gold
    _model_device(monkeypatch, lib)
    for name, rec in _readable(spec).items():
        st = {}
        _assert_case(g, name, rec, reader.read_spz(_file(g, name, tmp_path), stage_ms=st))
        assert "parse" in st, name


def test_recorded_errors_are_raised_before_any_device_work(gold, reader, lib, tmp_path, monkeypatch):
    g, spec = gold
    _no_device(monkeypatch, lib)
    errors = {n: r for n, r in spec.items() if "error" in r}
    assert len(errors) == N_ERRORS
    for name, rec in errors.items():
        kind, text = rec["error"]
        _HostSession.asked = []
        with pytest.raises(EXCEPTIONS[kind]) as e:
            reader.read_spz(_file(g, name, tmp_path))
        assert type(e.value) is EXCEPTIONS[kind] and str(e.value) == text, name
        data = g[name + "__file"].tobytes()
        if data[:2] != b"\x1f\x8b" or kind != "builtins.ValueError" or text != reader.SMALLER:
            continue
        assert len(_HostSession.asked) == 1, name          # a short body inside a gzip stream shows at the stream's end
    for name in ("err_short_plain", "err_magic", "err_version4_plain", "err_short_v2_d3_s0", "err_magic_gzip", "err_version0", "err_short_gzip"):
        _HostSession.asked = []
        with pytest.raises(ValueError):
            reader.read_spz(_file(g, name, tmp_path))
        assert not _HostSession.asked, name                # no session at all
    for name in ("n0_v1", "n0_v3", "n0_plain"):
        rows = reader.read_spz(_file(g, name, tmp_path))
        assert len(rows) == 0 and list(rows.dtype.names) == spec[name]["names"] and not _HostSession.asked


def test_degree_above_three_goes_to_the_fallback_or_raises(gold, reader, lib, tmp_path, monkeypatch):
    g, spec = gold
    _no_device(monkeypatch, lib)
    path = _file(g, "degree4", tmp_path)
    with pytest.raises(reader.UnsupportedSpzError, match="SH degree 4"):
        reader.read_spz(path)
    assert issubclass(reader.UnsupportedSpzError, ValueError)
    want = np.zeros(spec["degree4"]["rows"], [(f, "f4") for f in spec["degree4"]["names"]])
    assert reader.read_spz(path, fallback=lambda p: (want, p)) == (want, path)
    plain = tmp_path / "d4_plain.spz"
    plain.write_bytes(gzip.decompress(g["degree4__file"].tobytes()))
    assert reader.read_spz(str(plain), fallback=lambda p: "ref") == "ref"


def test_host_tables_are_numpys_results(lib):
    t = lib.spz_read_tables()
    b, c = np.arange(256, dtype=np.uint8), np.arange(1024, dtype=np.uint32)
    want = {"opacity": srn.opacity_of(b), "f_dc": srn.f_dc_of(b), "rgb": srn.colour_byte_of(srn.f_dc_of(b)),
            "scale": srn.scale_of(b).astype(np.float32), "sh": srn.sh_of(b), "rot_legacy": srn.legacy_component_of(b),
            "rot_v3": srn.v3_component_of(c).astype(np.float32)}
    assert tuple(t) == lib.SPZ_READ_TABLES == tuple(want)
    for k, w in want.items():
        assert t[k].dtype == w.dtype and t[k].shape == w.shape and t[k].tobytes() == w.tobytes(), k
    assert all(np.isfinite(t[k]).all() for k in t) and t["opacity"][0] < -16 and t["opacity"][255] > 15
    # the two tables the kernel computes instead: exact in float32, so the products and differences are the table's values
    assert np.array_equal(t["scale"], b.astype(np.float32) * np.float32(0.0625) - np.float32(10))
    assert np.array_equal(srn.scale_of(b), t["scale"].astype(np.float64))
    assert np.array_equal(t["sh"], (b.astype(np.int32) - 128).astype(np.float32) * np.float32(0.0078125))
    words = lib.spz_read_table_words()
    assert words.dtype == np.uint32 and words.size == 2560 and np.array_equal(words[512:768], t["rgb"])
    assert np.array_equal(words[1536:], t["rot_v3"].view(np.uint32)) and words[1536 + 512] == 0x80000000


def test_streamed_inflate_is_bounded_and_never_asks_for_more_than_the_body(reader, lib, tmp_path, monkeypatch):
    rng = np.random.default_rng(8)
    n = 40000                                        # 44 n = 1.76 MB: several chunks
    payload = srn.header(3, n, 2) + srn.random_body(3, 2, n, rng)
    extra = bytes(3 << 20)                           # behind the body: inflated, dropped, never staged
    path = tmp_path / "big.spz"
    path.write_bytes(srn.wrap(payload[:100000], 6) + srn.wrap(payload[100000:] + extra, 1))
    _model_device(monkeypatch, lib)
    real = lib.spz_unpack_table
    sizes, chunks = [], []

    def spy(fill, body_bytes, *a, **k):
        sizes.append(body_bytes)
        return real(fill, body_bytes, *a, **k)
    monkeypatch.setattr(lib, "spz_unpack_table", spy)
    real_chunks = reader.inflate_chunks

    def watch(f, chunk=reader.CHUNK):
        for c in real_chunks(f, chunk):
            chunks.append(len(c))
            yield c
    monkeypatch.setattr(reader, "inflate_chunks", watch)
    rows = reader.read_spz(str(path))
    assert sizes == [len(payload) - 16] and srn.sha(rows) == srn.sha(srn.decode(payload[16:], 3, n, 2, 12))
    assert sum(chunks) == len(payload) + len(extra) and max(chunks) <= reader.CHUNK and len(chunks) >= 4
    # a small chunk size walks every path of the generator: output limit hit, members, zero padding, the file's end
    small = tmp_path / "small.spz"
    small.write_bytes(srn.wrap(payload[:700], 9) + bytes(40) + srn.wrap(payload[700:5000], 0) + bytes(9))
    with open(small, "rb") as f:
        got = list(real_chunks(f, 64))
    assert b"".join(got) == payload[:5000] and max(map(len, got)) <= 64
    with open(small, "rb") as f, pytest.raises(EOFError):
        list(real_chunks(io.BytesIO(f.read()[:-20]), 64))


_STANDIN = {
    "gsconverter/__init__.py": "",
    "gsconverter/processing/__init__.py": "from . import gpu_ops\nfrom .data_processor import DataProcessor\n",
    "gsconverter/processing/gpu_ops.py": "HAS_TAICHI = False\n",
    "gsconverter/processing/data_processor.py": "class DataProcessor:\n    def __init__(self, data):\n        self.data = data\n",
    "gsconverter/converter.py": "from .processing import DataProcessor\n",
    "gsconverter/formats/__init__.py": "",
    "gsconverter/formats/spz.py": ("class SpzFormat:\n    def read(self, path, **kw):\n        return ('own', path, kw)\n"
                                   "    def write(self, data, path, **kw):\n        return 'w'\n"),
    "gsconverter/formats/ksplat.py": "class KSplatFormat:\n    def write(self, data, path, compression_level=0, **kw):\n        return 'w'\n",
}


def test_install_rebinds_spz_read_on_a_stand_in_and_uninstall_restores_read_and_write(gsx, gold, reader, lib, tmp_path, monkeypatch):
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
        import gsconverter.formats.ksplat as rks
        import gsconverter.formats.spz as rspz
        own_read, own_write = rspz.SpzFormat.read, rspz.SpzFormat.write
        d4 = _file(g, "degree4", tmp_path)
        try:
            gsx.install(spz_reader=False)
            assert rspz.SpzFormat.read is own_read and rspz.SpzFormat.write is not own_write
            gsx.uninstall()
            assert rspz.SpzFormat.read is own_read and rspz.SpzFormat.write is own_write
            gsx.install(spz_writer=False)
            assert rspz.SpzFormat.read is not own_read and rspz.SpzFormat.write is own_write
            gsx.uninstall()
            assert rspz.SpzFormat.read is own_read
            gsx.install()
            assert rspz.SpzFormat.read is not own_read and rspz.SpzFormat.write is not own_write
            assert rspz.SpzFormat.read.__wrapped__ is own_read
            assert not hasattr(rks.KSplatFormat, "read")               # a reference class without `read` is left alone
            rows = rspz.SpzFormat().read(_file(g, "two_members", tmp_path))
            _assert_case(g, "two_members", spec["two_members"], rows)
            assert rspz.SpzFormat().read(d4, extra=1) == ("own", d4, {"extra": 1})     # a refused file: the original's result
            assert reader.read_spz(d4) == ("own", d4, {})                             # read_spz itself finds the saved original
            with pytest.raises(gzip.BadGzipFile):
                rspz.SpzFormat().read(_file(g, "err_crc", tmp_path))
        finally:
            gsx.uninstall()
        assert rspz.SpzFormat.read is own_read and rspz.SpzFormat.write is own_write and not hasattr(rks.KSplatFormat, "read")
        with pytest.raises(reader.UnsupportedSpzError):
            reader.read_spz(d4)
    finally:
        for m in [m for m in sys.modules if m == "gsconverter" or m.startswith("gsconverter.")]:
            del sys.modules[m]
        sys.modules.update(saved)


def test_golden_file_regenerates_identically_when_the_reference_is_there(tmp_path):
    from oracle import refload
    if not refload.available():
        pytest.skip("the reference is not mounted")
    env = dict(os.environ, PYTHONWARNINGS="ignore")
    code = ("import sys, runpy; sys.path.insert(0, %r); m = runpy.run_path(%r); m['main'].__globals__['OUT'] = %r; m['main']()"
            % (ROOT, os.path.join(ROOT, "tests", "devtools", "make_golden_spz_read.py"), str(tmp_path / "again.npz")))
    subprocess.run([sys.executable, "-c", code], check=True, env=env, capture_output=True, cwd=ROOT)
    a, b = np.load(GOLD), np.load(str(tmp_path / "again.npz"))
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
