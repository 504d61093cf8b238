"""GPU box: the .ksplat writer end to end -- per-stage clock (PROBE_N splats, degree-3 table capped to 2, 248-byte rows): upload,
SH-degree scan, bucket centres, pack, download, host patch of the listed rows, file write.
    python tools/probe_ksplat.py            # PROBE_N=10000000 PROBE_REPS=3 PROBE_LEVEL=1 PROBE_RGB=1 (251-byte rows)"""
import importlib, json, os, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.probe_sog import table   # noqa: E402


def main():
    n = int(os.environ.get("PROBE_N", 10_000_000))
    reps = int(os.environ.get("PROBE_REPS", 3))
    level = int(os.environ.get("PROBE_LEVEL", 1))
    w = importlib.import_module("3dgsconverter_amd.formats.ksplat_writer")
    data = table(n, 7)
    if os.environ.get("PROBE_RGB"):
        wide = np.zeros(n, data.dtype.descr + [("red", "u1"), ("green", "u1"), ("blue", "u1")])
        for f in data.dtype.names:
            wide[f] = data[f]
        data = wide
    runs, stages = [], None
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "probe.ksplat")
        for _ in range(reps):
            st = {}
            t = time.perf_counter()
            w.write_ksplat(data, path, level, stage_ms=st)
            runs.append(round((time.perf_counter() - t) * 1e3, 2))
            stages = {k: round(v, 3) for k, v in st.items()}
        size = os.path.getsize(path)
    print(json.dumps({"n": n, "row_bytes": data.dtype.itemsize, "level": level, "runs_ms": runs, "stage_ms_last": stages,
                      "file_bytes": size}))


if __name__ == "__main__":
    main()
