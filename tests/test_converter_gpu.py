"""-m gpu: the stand-alone converter end to end through real kernels -- every stored run of the reference's own ``Converter.run``
(tests/golden/converter_ref.npz) through this package's ``Converter.run``: the written file, the stdout lines and the info
blocks of the input and of the output equal the stored ones; and one case through ``cli.main``, which decodes its source once.

What is compared of an output is what the fixture's tool stores: the file's bytes (3dgs, cc, compressed_ply, ksplat, splat), the
inflated payload (spz: gzip stamps the time), the table read back (parquet: the bytes depend on the pyarrow version) and the
members that do not depend on the codebooks' random seeds (sog: means_l, means_u, quats, the opacity byte, meta.json without its
codebooks).  For the last two the `Size:` line of the output's info block is the file's own and is not compared.  The lines
that name the backend are the reference's without Taichi there and this package's here (converter_cases.BACKEND_WORDING).
Parquet cases skip only without pyarrow, SOG cases only without WebP in Pillow."""
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
    formats = {case.target, case.input_name.rsplit(".", 1)[1]}
    if "parquet" in formats and not _have_parquet():
        return "pyarrow is missing"
    if "sog" in formats and not _have_webp():
        return "Pillow lacks WebP"
    return None


@pytest.fixture(scope="module")
def conv():
    importlib.import_module("3dgsconverter_amd._lib").require_hip()
    return importlib.import_module("3dgsconverter_amd.converter")


@pytest.fixture(scope="module")
def cli():
    return importlib.import_module("3dgsconverter_amd.cli")


def _stdout_of(call):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), np.errstate(all="ignore"):
        call()
    return buf.getvalue().split("\n")


@pytest.fixture(scope="module")
def runs(conv, cli, tmp_path_factory):
    """every case once: {name: (tmp root, output path, run lines, info lines of the input, info lines of the output)}"""
    root = tmp_path_factory.mktemp("converter")
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
        lines = _stdout_of(lambda: conv.Converter(src, dst, case.target).run(**dict(case.kwargs)))
        out[case.name] = (str(root), dst, lines, _stdout_of(lambda: cli.report_info(src)), _stdout_of(lambda: cli.report_info(dst)))
    return out


def _run_of(runs, case):
    why = _skip_reason(case)
    if why:
        pytest.skip(why)
    return runs[case.name]


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_status_lines(runs, cli, case):
    root, _, lines, _, _ = _run_of(runs, case)
    assert lines == cc.expected_lines(case.lines, root, cli.__version__)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_info_blocks(runs, cli, case):
    root, _, _, info_in, info_out = _run_of(runs, case)
    assert info_in == cc.expected_lines(case.info_in, root, cli.__version__)
    want = cc.expected_lines(case.info_out, root, cli.__version__)
    if case.target in ("sog", "parquet"):
        info_out, want = ([ln for ln in block if not ln.startswith("Size: ")] for block in (info_out, want))
    assert info_out == want


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_output(runs, case):
    _, dst, _, _, _ = _run_of(runs, case)
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


def test_cli_decodes_the_source_once(conv, cli, tmp_path, monkeypatch):
    case = next(c for c in CASES if c.name == "filters_to_spz")
    src, dst = str(tmp_path / case.input_name), str(tmp_path / "made" / "out.spz")
    with open(src, "wb") as f:
        f.write(case.input)
    reads, real = [], conv.SourceHandler.read

    def counted(self, path, stage_ms=None):
        reads.append(os.path.abspath(path))
        return real(self, path, stage_ms)
    monkeypatch.setattr(conv.SourceHandler, "read", counted)
    argv = ["-i", src, "-f", "spz", "-o", dst, "--bbox", "-5", "-5", "-5", "5", "5", "5", "--min_opacity", "20", "--density_voxel_size", "2.0",
            "--density_threshold", "1.0", "--sor_k", "8", "--sor_sigma", "1.5", "--auto_bbox", "--rgb"]
    lines = _stdout_of(lambda: cli.main(argv))
    assert reads == [os.path.abspath(src), os.path.abspath(dst)]           # the source once, the written file once
    with open(dst, "rb") as f:
        assert gzip.decompress(f.read()) == case.output["payload"].tobytes()
    at_source, at_target = lines.index(">>> SOURCE FILE INFO"), lines.index(">>> TARGET FILE INFO")
    run_lines = cc.expected_lines(case.lines, "<TMP>", cli.__version__)[:-2]       # up to the `Conversion completed` line
    assert [ln for ln in lines[at_source:at_target] if ln in run_lines] == run_lines
    assert lines[at_target - 2] == "Conversion completed: Saved to %s" % dst
