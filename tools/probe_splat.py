"""GPU box: the .splat writer end to end -- per-stage clock (PROBE_N splats, 248-byte rows): upload, key + pack, sort, permute,
download, file write; then the sort-first variant (keys pass, sort, records gathered from the raw rows in sorted order) on the same
table, and the numpy restatement's time on this host's CPU for scale.
    python tools/probe_splat.py            # PROBE_N=10000000 PROBE_REPS=3 PROBE_RGB=1 (251-byte rows)"""
import importlib, json, os, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from tools.probe_sog import table   # noqa: E402


def main():
    n = int(os.environ.get("PROBE_N", 10_000_000))
    reps = int(os.environ.get("PROBE_REPS", 3))
    w = importlib.import_module("3dgsconverter_amd.formats.splat_writer")
    lib = importlib.import_module("3dgsconverter_amd._lib")
    data = table(n, 7)
    if os.environ.get("PROBE_RGB"):
        wide = np.zeros(n, data.dtype.descr + [("red", "u1"), ("green", "u1"), ("blue", "u1")])
        for f in data.dtype.names:
            wide[f] = data[f]
        data = wide
    runs, stages = [], None
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "probe.splat")
        for _ in range(reps):
            st = {}
            t = time.perf_counter()
            w.write_splat(data, path, stage_ms=st)
            runs.append(round((time.perf_counter() - t) * 1e3, 2))
            stages = {k: round(v, 3) for k, v in st.items()}
        size = os.path.getsize(path)
    print(json.dumps({"variant": "pack_then_permute", "n": n, "row_bytes": data.dtype.itemsize, "runs_ms": runs, "stage_ms_last": stages,
                      "file_bytes": size}), flush=True)
    runs, stages, outs = [], None, []
    for _ in range(reps):
        st = {}
        t = time.perf_counter()
        outs = [lib.splat_pack_table(data, variant="gather", stage_ms=st)]
        runs.append(round((time.perf_counter() - t) * 1e3, 2))
        stages = {k: round(v, 3) for k, v in st.items()}
    print(json.dumps({"variant": "sort_then_gather", "n": n, "runs_ms": runs, "stage_ms_last": stages}), flush=True)
    if os.environ.get("PROBE_NUMPY", "1") == "1":
        import splat_numpy
        t = time.perf_counter()
        ref = splat_numpy.file_bytes(data)
        print(json.dumps({"numpy_restatement_ms": round((time.perf_counter() - t) * 1e3, 1),
                          "equal_to_gather_variant": ref == outs[0].tobytes()}), flush=True)


if __name__ == "__main__":
    main()
