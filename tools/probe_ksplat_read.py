"""GPU box: the .ksplat reader end to end -- per-stage clock of a PROBE_N-row level-PROBE_LEVEL degree-2 read (parse, file read
into page-locked staging, upload, kernel, download, total) and the kernel's rate by algorithmic bytes (the splat rows in, the
float32 rows out).  The kernel stage is a host clock around the launch and a stream synchronisation.
    python tools/probe_ksplat_read.py            # PROBE_N=10000000 PROBE_LEVEL=1 PROBE_REPS=3"""
import importlib, json, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ksplat_read_numpy as krn        # noqa: E402


def main():
    n = int(os.environ.get("PROBE_N", 10_000_000))
    level = int(os.environ.get("PROBE_LEVEL", 1))
    reps = int(os.environ.get("PROBE_REPS", 3))
    reader = importlib.import_module("3dgsconverter_amd.formats.ksplat_reader")
    with tempfile.TemporaryDirectory() as tmp:
        path = krn.random_file(os.path.join(tmp, "probe.ksplat"), level, 2, n, 5)
        size = os.path.getsize(path)
        runs, stages = [], []
        for _ in range(reps):
            st = {}
            t = time.perf_counter()
            rows, meta = reader.read_ksplat(path, stage_ms=st)
            st["total"] = round((time.perf_counter() - t) * 1e3, 3)
            runs.append(st["total"])
            stages.append(st)
            del rows
    bytes_in, bytes_out = krn.row_bytes(level, 2) * n, 164 * n
    best = min(s["kernel"] for s in stages)
    print(json.dumps({"n": n, "level": level, "file_bytes": size, "runs_ms": runs, "stage_ms": stages,
                      "kernel_bytes_in": bytes_in, "kernel_bytes_out": bytes_out,
                      "kernel_best_ms": best, "kernel_GBps_by_algorithmic_bytes": round((bytes_in + bytes_out) / best / 1e6, 1)}), flush=True)


if __name__ == "__main__":
    main()
