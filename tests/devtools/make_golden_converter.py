"""Build box only: run the reference's own ``Converter.run`` and ``report_info`` (gsconverter/converter.py, main.py) on every
converter case and record what they printed and wrote -> tests/golden/converter_ref.npz (data only).

plyfile is not installed here: ``PlyData.read`` is the numpy parser of tests/ply_read_numpy.py and ``PlyElement.describe`` /
``PlyData(...).write`` the stand-ins of tests/ply_write_numpy.py, as in the other make_golden_* tools.  Two rules hold for
every case:

  no ties       the case runs twice, as the reference stands and with ``np.argsort`` made stable inside its format modules
                (the one change); both runs must write the same file (no equal Morton codes, no equal .splat metrics)
  applied SOR   the reference's branch without Taichi computes its mask and returns the table unfiltered: the
                mask it computed is applied, and its `retained` line is printed with the mask's count

Per case: the input file's bytes and name, the target and kwargs, the stdout lines of the run (status_print goes through
tqdm.write; the temporary directory reads <TMP>), the report_info lines of the input and of the output, the decision record
(the source table's field names, its f_rest activity word, the degree handed to cap_sh_degree, whether add_rgb_from_sh ran), and
the output: file bytes (3dgs, cc, compressed_ply, ksplat, splat), the inflated payload (spz: gzip stamps the time), the
read-back table (parquet: the bytes depend on the pyarrow version) or the deterministic members (sog: means_l, means_u, quats,
the opacity byte, meta.json without its codebooks).

usage: python tests/devtools/make_golden_converter.py [--check]     (--check: run again and compare with the stored file)"""
import contextlib
import gzip
import io
import json
import os
import sys
import tempfile
import types
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import refload          # noqa: E402
import ply_read_numpy as pn          # noqa: E402
import ply_write_numpy as pw         # noqa: E402

DST = os.path.join(ROOT, "tests", "golden", "converter_ref.npz")
N = 300                              # two full 128-row tiles and a partial one
EXT = {"3dgs": ".ply", "cc": ".ply", "compressed_ply": ".ply", "sog": ".sog", "splat": ".splat", "ksplat": ".ksplat", "spz": ".spz",
       "parquet": ".parquet"}
FORMATS = list(EXT)


class _Prop:
    def __init__(self, name):
        self.name = name


class _Element:
    def __init__(self, name, data):
        self.name, self.data = name, data
        self.properties = tuple(_Prop(n) for n in data.dtype.names)


class RefPlyData:
    """what the reference uses of plyfile.PlyData, reading and writing"""

    def __init__(self, elements, text=False, byte_order="<"):
        assert byte_order == "<" and not text
        self.elements = list(elements)

    def __contains__(self, name):
        return any(e.name == name for e in self.elements)

    def __getitem__(self, name):
        return next(e for e in self.elements if e.name == name)

    def write(self, path):
        pn.write_ply(path, [(e.name, e.data) for e in self.elements])

    @staticmethod
    def read(path):
        return RefPlyData([_Element(n, d) for n, d in pn.parse(path)])


class _StableNp:
    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def argsort(a, *args, **kw):
        return np.argsort(a, kind="stable")


def setup():
    stub = types.ModuleType("plyfile")
    stub.PlyData, stub.PlyElement = RefPlyData, pw.StandInElement
    sys.modules["plyfile"] = stub
    refload.load()
    import gsconverter.converter as conv
    import gsconverter.main as main
    import gsconverter.formats.compressed_ply as m_cply
    import gsconverter.formats.ply_3dgs as m_3dgs
    import gsconverter.formats.ply_cc as m_cc
    import gsconverter.formats.splat as m_splat
    import gsconverter.formats.ksplat as m_ksplat
    import gsconverter.processing.data_processor as dpmod
    for m in (m_cply, m_3dgs, m_cc):
        m.PlyData, m.PlyElement = RefPlyData, pw.StandInElement
    return conv, main, dpmod, (m_cply, m_splat, m_ksplat)


def recording_processor(dpmod, record):
    """the reference's DataProcessor with its SOR mask applied and the orchestrator's decisions written down"""
    base = dpmod.DataProcessor

    class Recording(base):
        def cap_sh_degree(self, degree):
            names = self.data.dtype.names
            with np.errstate(all="ignore"):
                word = sum(int(bool(np.any(self.data[f"f_rest_{i}"] != 0))) << i for i in range(45) if f"f_rest_{i}" in names)
            record.update(names=list(names), rest_nonzero=word, final_degree=int(degree), add_rgb=False)
            return super().cap_sh_degree(degree)

        def add_rgb_from_sh(self):
            record["add_rgb"] = True
            return super().add_rgb_from_sh()

        def remove_flyers(self, *a, **kw):
            cap, saved = {}, dpmod.status_print

            def spy(*args, **k2):
                loc = sys._getframe(1).f_locals
                if "mask" in loc and "all_mean_dists" in loc:
                    cap["mask"] = np.array(loc["mask"], copy=True)
                    return saved(f"After removing flyers, retained {int(cap['mask'].sum())} out of {loc['num_points']} vertices.")
                return saved(*args, **k2)
            dpmod.status_print = spy
            try:
                with np.errstate(invalid="ignore"):
                    super().remove_flyers(*a, **kw)
            finally:
                dpmod.status_print = saved
            self.data = self.data[cap["mask"]]
            return self.data
    return Recording


@contextlib.contextmanager
def captured():
    out = io.StringIO()
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(io.StringIO()):
        yield out


def lines_of(buf, tmp):
    return [ln.replace(tmp, "<TMP>") for ln in buf.getvalue().split("\n")]


def convert(env, tmp, src, dst, target, kwargs, stable=False):
    conv, main, dpmod, sort_modules = env
    record = {}
    saved_dp, saved_np = conv.DataProcessor, [m.np for m in sort_modules]
    conv.DataProcessor = recording_processor(dpmod, record)
    try:
        if stable:
            for m in sort_modules:
                m.np = _StableNp()
        with captured() as buf, np.errstate(all="ignore"):
            conv.Converter(src, dst, target).run(**dict(kwargs))
    finally:
        conv.DataProcessor = saved_dp
        for m, s in zip(sort_modules, saved_np):
            m.np = s
    return lines_of(buf, tmp), record


def info(env, tmp, path):
    with captured() as buf, np.errstate(all="ignore"):
        env[1].report_info(path)
    return lines_of(buf, tmp)


def output_record(env, target, path):
    """-> {key: array}: what of the written file is stored"""
    with open(path, "rb") as f:
        blob = f.read()
    if target == "spz":
        return {"payload": np.frombuffer(gzip.decompress(blob), np.uint8)}
    if target == "parquet":
        import gsconverter.formats.parquet as m
        t = np.ascontiguousarray(m.ParquetFormat().read(path))
        return {"table": np.frombuffer(t.tobytes(), np.uint8), "descr": np.frombuffer(json.dumps(pw.dtype_descr(t.dtype)).encode(), np.uint8),
                "rows": np.array([len(t)])}
    if target == "sog":
        from PIL import Image
        out = {}
        with zipfile.ZipFile(path) as zf:
            meta = json.loads(zf.read("meta.json"))
            for member in ("means_l", "means_u", "quats"):
                out[member] = np.array(Image.open(io.BytesIO(zf.read(meta[member if member != "means_l" and member != "means_u" else "means"]["files"][0 if member != "means_u" else 1]))).convert("RGBA"))
            sh0 = np.array(Image.open(io.BytesIO(zf.read(meta["sh0"]["files"][0]))).convert("RGBA"))
            out["opacity"] = np.ascontiguousarray(sh0[..., 3])
        for key in ("scales", "sh0", "shN"):
            if key in meta and "codebook" in meta[key]:
                meta[key] = dict(meta[key], codebook=None)
        out["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), np.uint8)
        return out
    return {"file": np.frombuffer(blob, np.uint8)}


def base_table(seed, degree=3):
    """a plausible scene in the canonical 62-field table: no two rows share a Morton cell or a .splat metric"""
    rng = np.random.default_rng(seed)
    grid = lambda a, steps: (np.round(np.asarray(a) * steps) / steps).astype(np.float32)   # noqa: E731  (short mantissas: the fixture deflates)
    t = np.zeros(N, [(f, "<f4") for f in pn.FLOAT_FIELDS])
    for a in ("x", "y", "z"):
        t[a] = grid(rng.uniform(-4.0, 4.0, N), 256)
    t["x"][:12] = grid(rng.uniform(30.0, 60.0, 12), 256)                  # a few flyers and a sparse fringe for the filters
    for f in ("f_dc_0", "f_dc_1", "f_dc_2"):
        t[f] = grid(rng.normal(0.0, 1.0, N), 128)
    n_rest = 3 * ((degree + 1) ** 2 - 1)
    for i in range(n_rest):
        t["f_rest_%d" % i] = grid(rng.normal(0.0, 0.2, N), 256)
    t["opacity"] = grid(rng.normal(1.0, 2.0, N), 128)
    for f in ("scale_0", "scale_1", "scale_2"):
        t[f] = grid(rng.normal(-4.0, 0.7, N), 128)
    q = grid(rng.normal(size=(N, 4)), 128)
    for c in range(4):
        t["rot_%d" % c] = q[:, c]
    return t


def ply_bytes(table, extras=()):
    return pw.file_bytes([("vertex", table)] + list(extras))


CAMERA = [("extrinsic", np.arange(16, dtype="<f4").view([("m%d" % i, "<f4") for i in range(16)])),
          ("image_size", np.array([(640, 480)], [("w", "<i4"), ("h", "<i4")]))]
FILTERS = dict(bbox=[-5.0, -5.0, -5.0, 5.0, 5.0, 5.0], min_opacity=20, density_voxel_size=2.0, density_threshold=1.0, sor_k=8, sor_sigma=1.5,
               auto_bbox=True, rgb=True)


def case_list(env, tmp):
    """-> [(name, input file name, input bytes, target, kwargs)]"""
    full = base_table(1)
    deg1 = base_table(2, degree=1)
    zero_sh = base_table(3, degree=0)
    nan_only = base_table(4, degree=0)
    nan_only["f_rest_30"][N - 1] = np.nan
    negzero = base_table(5, degree=1)
    negzero["f_rest_40"][:] = -0.0
    base_ply = ply_bytes(full)
    cases = []
    src_path = os.path.join(tmp, "base.ply")                               # the sources: a degree-1 scene (36 zero columns deflate)
    with open(src_path, "wb") as f:
        f.write(ply_bytes(deg1))
    for fmt in FORMATS:                                                    # every source format -> 3dgs
        made = os.path.join(tmp, "made_" + fmt + EXT[fmt])
        convert(env, tmp, src_path, made, fmt, {"compression_level": 1} if fmt == "ksplat" else {})
        with open(made, "rb") as f:
            blob = f.read()
        if fmt == "spz":                                                   # (gzip stamps the time into its header: a fixed stamp)
            blob = gzip.compress(gzip.decompress(blob), compresslevel=0, mtime=0)
        cases.append(("from_" + fmt, "scene" + EXT[fmt], blob, "3dgs", {}))
    for fmt in FORMATS:                                                    # 3dgs -> every target
        cases.append(("to_" + fmt, "scene.ply", base_ply, fmt, {}))
    cases.append(("filters_to_spz", "scene.ply", base_ply, "spz", dict(FILTERS)))
    cases.append(("filters_to_cc", "scene.ply", base_ply, "cc", dict(FILTERS)))
    cases.append(("sh_level_over_limit_ksplat", "scene.ply", base_ply, "ksplat", {"sh_level": 3}))
    cases.append(("sh_level_over_limit_splat", "scene.ply", base_ply, "splat", {"sh_level": 2}))
    cases.append(("sh_level_over_source", "scene.ply", ply_bytes(deg1), "3dgs", {"sh_level": 3}))
    cases.append(("degree1_in_45_columns", "scene.ply", ply_bytes(deg1), "spz", {}))
    cases.append(("all_zero_sh", "scene.ply", ply_bytes(zero_sh), "spz", {}))
    cases.append(("nan_only_column", "scene.ply", ply_bytes(nan_only), "3dgs", {"crop_sh": True}))
    cases.append(("negative_zero_column", "scene.ply", ply_bytes(negzero), "3dgs", {"crop_sh": True}))
    with_extras = ply_bytes(full, CAMERA)
    for keep in (True, False):
        cases.append(("extras_present_keep_%s" % keep, "scene.ply", with_extras, "3dgs", {"maintain_extra_elements": keep}))
        cases.append(("extras_absent_keep_%s" % keep, "scene.ply", base_ply, "3dgs", {"maintain_extra_elements": keep}))
    cases.append(("extras_present_to_spz", "scene.ply", with_extras, "spz", {"maintain_extra_elements": True}))
    return cases


def keep(out, array):
    """store an array once under its hash -> the key (many cases share an input, and an untouched table is its own output)"""
    import hashlib
    array = np.ascontiguousarray(array)
    key = "blob_" + hashlib.sha256(array.tobytes() + str((array.dtype.str, array.shape)).encode()).hexdigest()[:16]
    out[key] = array
    return key


def build():
    env = setup()
    out, spec = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, in_name, blob, target, kwargs in case_list(env, tmp):
            work = os.path.join(tmp, name)
            os.makedirs(work)
            src, dst = os.path.join(work, in_name), os.path.join(work, "out" + EXT[target])
            with open(src, "wb") as f:
                f.write(blob)
            lines, record = convert(env, tmp, src, dst, target, kwargs)
            stored = output_record(env, target, dst)
            if target != "sog":                                            # (the SOG codebooks start from random seeds)
                os.remove(dst)
                convert(env, tmp, src, dst, target, kwargs, stable=True)
                again = output_record(env, target, dst)
                assert all(np.array_equal(stored[k], again[k]) for k in stored), "%s: ties decide the output" % name
            spec[name] = {"input": in_name, "target": target, "kwargs": kwargs, "lines": lines, "record": record,
                          "info_in": info(env, tmp, src), "info_out": info(env, tmp, dst), "output": sorted(stored)}
            keys = {"input": keep(out, np.frombuffer(blob, np.uint8))}
            keys.update({k: keep(out, v) for k, v in stored.items()})
            spec[name]["blobs"] = keys
            print(name, target, {k: v.size for k, v in stored.items()}, record.get("final_degree"), flush=True)
    out["spec"] = np.frombuffer(json.dumps(spec, sort_keys=True).encode(), np.uint8)
    return out


def main():
    out = build()
    if "--check" in sys.argv:
        with np.load(DST) as g:
            skip = lambda k: k in ("from_sog", "to_sog")                # noqa: E731  (codebooks from random seeds: from_sog's input too)
            a, b = json.loads(bytes(g["spec"])), json.loads(bytes(out["spec"]))
            assert sorted(a) == sorted(b)
            bad = [k for k in a if not skip(k) and a[k] != b[k]]             # (equal blob keys: equal bytes)
            assert not bad, bad
        print("the reference reproduces every stored case")
        return
    np.savez_compressed(DST, **out)
    print("wrote", DST, os.path.getsize(DST), "bytes")


if __name__ == "__main__":
    main()
