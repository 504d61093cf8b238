"""GPU box: the SOG reader end to end -- per-stage clock of a PROBE_N-row degree-3 read with a 65 536-entry palette (parse,
threaded WebP decode into page-locked staging, upload, kernel, download, total), from a file of random texels and from one of
smooth texels (WebP decodes them at different rates), and the kernel's rate by algorithmic bytes (six texels and the gathered
centroid pixels in, the packed rows out).  The kernel stage is a host clock around the launch and a stream synchronisation.
(The reference's own time per 1M rows: tests/devtools/time_reference_sog_read.py.)
    python tools/probe_sog_read.py            # PROBE_N=10000000 PROBE_REPS=3"""
import importlib, json, os, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sog_read_numpy as srn        # noqa: E402


def main():
    with tempfile.TemporaryDirectory() as tmp:
        n = int(os.environ.get("PROBE_N", 10_000_000))
        reps = int(os.environ.get("PROBE_REPS", 3))
        bands, palette = 3, 65536
        reader = importlib.import_module("3dgsconverter_amd.formats.sog_reader")
        for kind in ("random", "smooth"):
            rng = np.random.default_rng(5)
            t = time.perf_counter()
            texels = srn.random_texels(n, bands, palette, rng) if kind == "random" else srn.smooth_texels(n, bands, palette)
            path = srn.build_file(os.path.join(tmp, "probe_%s.sog" % kind), n, bands, palette, rng, texels=texels)
            del texels
            build_s = round(time.perf_counter() - t, 1)
            stages = []
            for _ in range(reps):
                st = {}
                t = time.perf_counter()
                rows = reader.read_sog(path, stage_ms=st)
                st["total"] = round((time.perf_counter() - t) * 1e3, 3)
                stages.append(st)
                del rows
            bytes_in, bytes_out = (6 * 4 + 15 * 4) * n, 248 * n
            best = min(s["kernel"] for s in stages)
            print(json.dumps({"n": n, "texels": kind, "bands": bands, "palette": palette, "file_bytes": os.path.getsize(path),
                              "file_build_s": build_s, "stage_ms": stages, "kernel_bytes_in": bytes_in, "kernel_bytes_out": bytes_out,
                              "kernel_best_ms": best, "kernel_GBps_by_algorithmic_bytes": round((bytes_in + bytes_out) / best / 1e6, 1)}),
                  flush=True)


if __name__ == "__main__":
    main()
