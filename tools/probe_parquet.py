"""GPU box: the Parquet writer and reader end to end -- per-stage clocks of a PROBE_N-row degree-3 table (248 bytes a row, 62
float32 fields, every value its own random number so that no column dictionary-encodes, 1 % NaN in f_rest_0 so that one
column carries a bitmap).  write_parquet: plan, upload, kernel, download, table (the Arrow table around the staging),
encode_write (pq.write_table: pages, snappy, the file), total.  read_parquet of the file just written: plan, decode
(pq.read_table), gather (Arrow's chunks into page-locked staging), upload, kernel, download, total.  The kernel stages are host
clocks around the launch and a stream synchronisation.  (The reference's own times: tests/devtools/time_reference_parquet.py.)
    python tools/probe_parquet.py            # PROBE_N=10000000 PROBE_REPS=3"""
import importlib, json, os, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import parquet_numpy as pqn        # noqa: E402


def table(n, seed=5):
    """the canonical degree-3 table of n rows, every float its own random number; 1 % of f_rest_0 is NaN"""
    rng = np.random.default_rng(seed)
    dt = np.dtype(pqn.canonical_fields(False))
    flat = np.empty((n, len(dt.names)), np.float32)
    step = 1 << 18
    for a in range(0, n, step):
        flat[a:a + step] = rng.random((min(step, n - a), flat.shape[1]), dtype=np.float32)
    t = flat.reshape(-1).view(dt)
    t["f_rest_0"][rng.integers(0, n, n // 100)] = np.nan
    return t


def main():
    n = int(os.environ.get("PROBE_N", 10_000_000))
    reps = int(os.environ.get("PROBE_REPS", 3))
    writer = importlib.import_module("3dgsconverter_amd.formats.parquet_writer")
    reader = importlib.import_module("3dgsconverter_amd.formats.parquet_reader")
    import pandas, pyarrow
    t = table(n)
    with tempfile.TemporaryDirectory(dir=os.environ.get("PROBE_TMP")) as tmp:
        path = os.path.join(tmp, "probe.parquet")
        stages = []
        for _ in range(reps):
            st = {}
            t0 = time.perf_counter()
            plan = writer.write_parquet(t, path, stage_ms=st)
            st["total"] = round((time.perf_counter() - t0) * 1e3, 3)
            stages.append(st)
        best = min(s["kernel"] for s in stages)
        print(json.dumps({"call": "write_parquet", "n": n, "in_stride": plan.in_stride, "columns": len(plan.columns), "file_bytes": os.path.getsize(path),
                          "pyarrow": pyarrow.__version__, "pandas": pandas.__version__, "stage_ms": stages, "kernel_best_ms": best,
                          "kernel_GBps_by_algorithmic_bytes": round(2 * plan.in_stride * n / best / 1e6, 1)}), flush=True)
        back = []
        for _ in range(reps):
            st = {}
            t0 = time.perf_counter()
            rows = reader.read_parquet(path, stage_ms=st)
            st["total"] = round((time.perf_counter() - t0) * 1e3, 3)
            back.append(st)
            same = bool(np.array_equal(rows["x"], t["x"]) and np.array_equal(rows["f_rest_44"], t["f_rest_44"])
                        and np.array_equal(np.isnan(rows["f_rest_0"]), np.isnan(t["f_rest_0"])))
            stride = rows.dtype.itemsize
            del rows
        best = min(s["kernel"] for s in back)
        print(json.dumps({"call": "read_parquet", "n": n, "out_stride": stride, "rows_match_the_table": same, "stage_ms": back, "kernel_best_ms": best,
                          "kernel_GBps_by_algorithmic_bytes": round(2 * stride * n / best / 1e6, 1)}), flush=True)


if __name__ == "__main__":
    main()
