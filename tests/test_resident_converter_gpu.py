"""-m gpu: ``Converter(..., resident=True)`` -- the reader's rows kept in HBM through the filters, one device materialise, the
.splat writer reading them where they lie -- on every stored run of the reference's own ``Converter.run``
(tests/golden/converter_ref.npz): the reference's output and status lines, as tests/test_converter_gpu.py compares them; the
resident path's clocks where the source reader kept its rows, no upload in a .splat target's writer; nothing left open in HBM
after a run, a failed run or a load without a run; and ``resident=False`` writes the same file."""
import contextlib
import gzip
import importlib
import io
import json
import os
import sys
import zipfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import converter_cases as cc  # noqa: E402
import ply_write_numpy as pw  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = cc.load_cases()


def _have_parquet():
    try:
        import pandas  # noqa: F401
        import pyarrow  # noqa: F401
        return True
    except ImportError:
        return False


def _have_webp():
    try:
        from PIL import features
        return bool(features.check("webp"))
    except ImportError:
        return False


def _skip_reason(case):
    """tests/test_converter_gpu.py's rules"""
    formats = {case.target, case.input_name.rsplit(".", 1)[1]}
    if "parquet" in formats and not _have_parquet():
        return "pyarrow is missing"
    if "sog" in formats and not _have_webp():
        return "Pillow lacks WebP"
    return None


@pytest.fixture(scope="module")
def lib():
    lib = importlib.import_module("3dgsconverter_amd._lib")
    lib.require_hip()
    return lib


@pytest.fixture(scope="module")
def conv(lib):
    return importlib.import_module("3dgsconverter_amd.converter")


@pytest.fixture(scope="module")
def cli():
    return importlib.import_module("3dgsconverter_amd.cli")


def _stdout_of(call):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), np.errstate(all="ignore"):
        call()
    return buf.getvalue().split("\n")


def _convert(conv, lib, src, dst, case, resident):
    """one run -> (lines, stage_ms, did the source reader keep rows the processor takes?, ResidentRows open after the run)"""
    seen = {}
    real = conv.SourceHandler.read

    def watched(self, path, stage_ms=None):
        data = real(self, path, stage_ms)
        rr = self.resident
        seen["kept"] = rr is not None and lib.resident_eligible(rr.dtype, rr.n, data.dtype, len(data))
        return data
    conv.SourceHandler.read = watched
    try:
        c = conv.Converter(src, dst, case.target, resident=resident)
        lines = _stdout_of(lambda: c.run(**dict(case.kwargs)))
    finally:
        conv.SourceHandler.read = real
    return lines, dict(c.stage_ms), seen["kept"], lib.ResidentRows.open_count


@pytest.fixture(scope="module")
def runs(conv, lib, tmp_path_factory):
    """every case once with resident=True: {name: (tmp root, output path, lines, stage_ms, kept, open after, open before)}"""
    root = tmp_path_factory.mktemp("resident_converter")
    out = {}
    for case in CASES:
        if _skip_reason(case):
            continue
        work = root / case.name
        work.mkdir()
        src = str(work / case.input_name)
        dst = str(work / ("out" + conv.EXTENSIONS[case.target]))
        with open(src, "wb") as f:
            f.write(case.input)
        before = lib.ResidentRows.open_count
        out[case.name] = (str(root), dst) + _convert(conv, lib, src, dst, case, True) + (before,)
    return out


def _run_of(runs, case):
    why = _skip_reason(case)
    if why:
        pytest.skip(why)
    return runs[case.name]


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_status_lines(runs, cli, case):
    root, _, lines = _run_of(runs, case)[:3]
    assert lines == cc.expected_lines(case.lines, root, cli.__version__)


def _check_output(case, dst):
    """tests/test_converter_gpu.py::test_output's comparison"""
    with open(dst, "rb") as f:
        blob = f.read()
    if case.target == "spz":
        assert gzip.decompress(blob) == case.output["payload"].tobytes()
    elif case.target == "parquet":
        table = importlib.import_module("3dgsconverter_amd.formats.parquet_reader").read_parquet(dst)
        assert pw.dtype_descr(table.dtype) == json.loads(bytes(case.output["descr"])) and len(table) == int(case.output["rows"][0])
        assert np.ascontiguousarray(table).tobytes() == case.output["table"].tobytes()
    elif case.target == "sog":
        from PIL import Image
        with zipfile.ZipFile(dst) as zf:
            meta = json.loads(zf.read("meta.json"))
            image = lambda name: np.array(Image.open(io.BytesIO(zf.read(name))).convert("RGBA"))   # noqa: E731
            np.testing.assert_array_equal(image(meta["means"]["files"][0]), case.output["means_l"])
            np.testing.assert_array_equal(image(meta["means"]["files"][1]), case.output["means_u"])
            np.testing.assert_array_equal(image(meta["quats"]["files"][0]), case.output["quats"])
            np.testing.assert_array_equal(image(meta["sh0"]["files"][0])[..., 3], case.output["opacity"])
        for key in ("scales", "sh0", "shN"):
            if key in meta and "codebook" in meta[key]:
                meta[key] = dict(meta[key], codebook=None)
        assert json.loads(json.dumps(meta, sort_keys=True)) == json.loads(bytes(case.output["meta"]))
    else:
        assert blob == case.output["file"].tobytes()


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_output(runs, case):
    _check_output(case, _run_of(runs, case)[1])


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_clocks_and_nothing_left_open(runs, case):
    _, _, _, stage_ms, kept, open_after, open_before = _run_of(runs, case)
    assert open_after == open_before                                    # every ResidentRows of the run is closed
    assert ("process_take" in stage_ms) == kept, stage_ms               # the resident path ran where the reader kept the rows
    assert "process" in stage_ms
    if kept and case.target == "splat":
        assert "write_upload" not in stage_ms and "write_key_pack" in stage_ms, stage_ms


def test_the_stored_cases_reach_the_resident_path(runs):
    """the stored sources that are no PLY file keep their rows (the PLY sources are the trainer's layout: read on the host)"""
    kept = {n for n, r in runs.items() if r[4]}
    assert kept == {n for n in runs if n.startswith("from_") and n not in ("from_3dgs", "from_cc")} and len(kept) >= 4


@pytest.mark.parametrize("name", ["from_spz", "from_ksplat", "to_splat"])
def test_a_stored_case_without_resident_rows(runs, conv, cli, lib, tmp_path, name):
    case = next(c for c in CASES if c.name == name)
    if _skip_reason(case):
        pytest.skip(_skip_reason(case))
    work = tmp_path / case.name
    work.mkdir()
    src, dst = str(work / case.input_name), str(work / ("out" + conv.EXTENSIONS[case.target]))
    with open(src, "wb") as f:
        f.write(case.input)
    lines, stage_ms, kept, open_after = _convert(conv, lib, src, dst, case, False)
    assert not kept and not any(k.startswith("process_") for k in stage_ms)
    assert lines == cc.expected_lines(case.lines, str(tmp_path), cli.__version__)
    _check_output(case, dst)
    with open(dst, "rb") as a, open(runs[name][1], "rb") as b:
        assert a.read() == b.read()


# ---- conversions of a scene the filters all remove rows from, from a PLY file whose rows are kept (float64 x: transcoded on the
# device), each with and without the resident rows: the same file, the same lines

OWN = {
    "splat_plain": ("splat", {}),
    "splat_filters": ("splat", {"sh_level": 0, "bbox": (-8.0, -8.0, -8.0, 8.0, 8.0, 8.0), "min_opacity": 40, "density_voxel_size": 1.0,
                                "density_threshold": 0.32, "sor_k": 12, "sor_sigma": 1.5, "auto_bbox": True}),
    "spz_filters": ("spz", {"min_opacity": 40, "density_sensitivity": 0.3, "sor_intensity": 5, "auto_bbox": True, "sh_level": 1}),
    "cc_alpha": ("cc", {"min_opacity": 128}),
    "ksplat_everything_removed": ("ksplat", {"bbox": (100.0, 100.0, 100.0, 101.0, 101.0, 101.0)}),
    "ksplat_few_left": ("ksplat", {"min_opacity": 254}),
}


@pytest.fixture(scope="module")
def own_source(tmp_path_factory):
    import ply_read_numpy as pn
    import resident_cases as rc
    rng = np.random.default_rng(0x6f776e)
    fields = [(f, "f8" if f == "x" else t) for f, t in pn.canonical_fields(3)]
    t = pn.build(5000, fields, rng)
    s = rc.scene(5000, rng)
    for nm in ("x", "y", "z", "opacity"):
        t[nm] = s[nm]
    path = str(tmp_path_factory.mktemp("resident_own") / "scene.ply")
    pn.write_ply(path, [("vertex", t)])
    return path


class _Own:
    def __init__(self, target, kwargs):
        self.target, self.kwargs = target, kwargs


@pytest.mark.parametrize("name", list(OWN))
def test_with_and_without_resident_rows_the_same_file_and_lines(conv, lib, own_source, tmp_path, name):
    target, kwargs = OWN[name]
    case = _Own(target, kwargs)
    got = {}
    for resident in (True, False):
        dst = str(tmp_path / ("%s_%d%s" % (name, resident, conv.EXTENSIONS[target])))
        before = lib.ResidentRows.open_count
        try:
            lines, stage_ms, kept, open_after = _convert(conv, lib, own_source, dst, case, resident)
            exc = None
        except Exception as e:      # noqa: BLE001  (a writer that refuses an empty table refuses it both ways)
            lines, stage_ms, kept, open_after, exc = None, {}, resident, lib.ResidentRows.open_count, (type(e).__name__, str(e))
        assert open_after == before
        blob = None
        if exc is None:
            with open(dst, "rb") as f:
                blob = f.read()
            blob = gzip.decompress(blob) if target == "spz" else blob
            lines = [ln.replace(dst, "<DST>") for ln in lines]
        got[resident] = (blob, lines, exc, stage_ms, kept)
    assert got[True][:3] == got[False][:3]
    ms, ms_host = got[True][3], got[False][3]
    assert got[True][4] and not got[False][4]
    assert not any(k.startswith("process_") for k in ms_host)
    if got[True][2] is None:
        assert "process_take" in ms and "process_gather" in ms and "read_download" in ms
        if target == "splat":
            assert "write_upload" not in ms and "write_upload" in ms_host and "process_download" in ms
        if "filters" in name:
            assert any("retained" in ln.lower() for ln in got[True][1]) and any(ln.startswith("Auto-BBox Applied") for ln in got[True][1])


def test_a_failed_run_and_a_load_without_a_run_leave_nothing_open(conv, lib, tmp_path):
    case = next(c for c in CASES if c.name == "filters_to_spz")
    src = str(tmp_path / case.input_name)
    with open(src, "wb") as f:
        f.write(case.input)
    before = lib.ResidentRows.open_count
    c = conv.Converter(src, str(tmp_path / "missing_dir" / "out.spz"), "spz")
    with pytest.raises(OSError):
        _stdout_of(lambda: c.run(**dict(case.kwargs)))                  # the writer cannot create its file
    assert lib.ResidentRows.open_count == before
    c = conv.Converter(src, str(tmp_path / "out.spz"), "spz")
    c.load_source_only()
    held = lib.ResidentRows.open_count - before
    c.close()
    c.close()
    assert lib.ResidentRows.open_count == before and held in (0, 1)
    c = conv.Converter(src, str(tmp_path / "out.spz"), "spz")
    c.load_source_only()
    _stdout_of(lambda: c.run(**dict(case.kwargs)))                      # run() takes the loaded rows over and closes them
    assert lib.ResidentRows.open_count == before and c.source_handler.opens == 1
    _check_output(case, str(tmp_path / "out.spz"))
