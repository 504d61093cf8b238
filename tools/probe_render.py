"""GPU box: the preview renderer at PROBE_N rows of 248 bytes (the canonical degree-3 table; tools/probe_decimate.py's scene:
uniformly random positions in a cube of side 64, log-scales in (-7, -4.5), alphas up to 0.4), the camera render.plan_camera
frames on the scene's box from the default view, at 960 x 540 and 1920 x 1080.

Per size ``ResidentRows.render`` runs 2 warm-up calls and PROBE_REPS timed ones; the six stage clocks are the stream's own (hip
events around the launches of gsx_rows_render_plan_dev and gsx_rows_render_draw_dev), the minimum over the runs of each.  Next
to them: the visible rows, the (tile, splat) instances, the bytes of instance workspace, the whole call (workspaces allocated,
image downloaded) and the blend's rate in pixel-splat pairs per second -- the pairs OFFERED to the blend, 256 per instance (one
per lane of the tile's workgroup); finished pixels and pixels outside a splat's rectangle skip theirs, so the rate says how
fast the scene's instances are consumed, not how many exponentials are evaluated.
    python tools/probe_render.py [output file]      # PROBE_N=10000000 PROBE_REPS=5"""
import importlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from probe_decimate import scene   # noqa: E402

SIZES = ((960, 540), (1920, 1080))


def main():
    n = int(os.environ.get("PROBE_N", 10_000_000))
    reps = int(os.environ.get("PROBE_REPS", 5))
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out is not None:
            out.write(line + "\n")
            out.flush()
    lib = importlib.import_module("3dgsconverter_amd._lib")
    rd = importlib.import_module("3dgsconverter_amd.render")
    lib.require_hip()
    table = scene(n)
    rr = lib.ResidentRows.from_host(table)
    try:
        prof = rr.profile()
        for w, h in SIZES:
            plan = rd.plan_render(table.dtype, rd.plan_camera(prof["lo"], prof["hi"], (w, h)))
            runs, total, info, image = [], [], None, None
            for _ in range(2 + reps):
                ms = {}
                t = time.perf_counter()
                image = rr.render(plan, stage_ms=ms)
                total.append((time.perf_counter() - t) * 1e3)
                info = rr.render_info
                runs.append(ms)
            best = {k: round(min(r[k] for r in runs[2:]), 3) for k in lib.RENDER_STAGES}
            pairs = 256 * info["instances"]
            emit({"what": "ResidentRows.render, stage clocks", "n": n, "row_bytes": table.dtype.itemsize, "width": w, "height": h, **info,
                  "instance_bytes": 24 * info["instances"], "stages_ms": best, "stages_sum_ms": round(sum(best.values()), 3),
                  "call_min_ms": round(min(total[2:]), 3), "download_min_ms": round(min(r["download"] for r in runs[2:]), 3),
                  "blend_pairs_offered": pairs, "blend_Gpairs_per_s": round(pairs / max(best["blend"], 1e-6) / 1e6, 1),
                  "image_mean": [round(float(v), 2) for v in image.reshape(-1, 3).mean(axis=0)]})
    finally:
        rr.close()
    if out is not None:
        out.close()


if __name__ == "__main__":
    main()
