"""GPU box: the view scores at PROBE_N rows of 248 bytes (tools/probe_render.py's scene), from the ring of views.plan_views on
the scene's box at 512 x 512: one view and 32 views.

Per view count ``ResidentRows.view_scores`` runs 2 warm-up calls and PROBE_REPS timed ones; the six stage clocks are the stream's
own (hip events around the launches of gsx_rows_render_plan_dev and gsx_rows_render_score_dev, summed over the views), the
minimum over the runs of each; "blend" is the score kernel.  Beside it, from the same process and the first view's camera:
``ResidentRows.render``'s clocks, whose "blend" is the image's blend kernel -- unchanged code, the number the score kernel is
read against.  Next to them: the rows no view blended, the rows under a peak of 0.01, and the whole call (workspaces allocated,
both arrays downloaded).
    python tools/probe_view_scores.py [output file]      # PROBE_N=10000000 PROBE_REPS=5"""
import importlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from probe_decimate import scene   # noqa: E402

VIEWS = (1, 32)
SIZE = (512, 512)


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
    import numpy as np
    lib = importlib.import_module("3dgsconverter_amd._lib")
    rd = importlib.import_module("3dgsconverter_amd.render")
    vw = importlib.import_module("3dgsconverter_amd.views")
    lib.require_hip()
    table = scene(n)
    rr = lib.ResidentRows.from_host(table)
    try:
        prof = rr.profile()
        for V in VIEWS:
            cams = vw.plan_views(prof["lo"], prof["hi"], views=V, size=SIZE)
            plans = [vw.plan_scores(table.dtype, cam) for cam in cams]
            runs, total, peak, tot = [], [], None, None
            for _ in range(2 + reps):
                ms = {}
                t = time.perf_counter()
                peak, tot = rr.view_scores(plans, stage_ms=ms)
                total.append((time.perf_counter() - t) * 1e3)
                runs.append(ms)
            info = rr.view_scores_info
            best = {k: round(min(r[k] for r in runs[2:]), 3) for k in lib.RENDER_STAGES}
            image_plan = rd.plan_render(table.dtype, cams[0], sh_degree=0)
            blends = []
            for _ in range(2 + reps):
                ms = {}
                rr.render(image_plan, stage_ms=ms)
                blends.append(ms)
            image_best = {k: round(min(r[k] for r in blends[2:]), 3) for k in lib.RENDER_STAGES}
            pairs = 256 * sum(info["instances"])
            emit({"what": "ResidentRows.view_scores, stage clocks summed over the views", "n": n, "row_bytes": table.dtype.itemsize, "views": V,
                  "width": SIZE[0], "height": SIZE[1], "visible_first_view": info["visible"][0], "instances": sum(info["instances"]),
                  "stages_ms": best, "stages_sum_ms": round(sum(best.values()), 3), "score_ms_per_view": round(best["blend"] / V, 3),
                  "call_min_ms": round(min(total[2:]), 3), "download_min_ms": round(min(r["download"] for r in runs[2:]), 3),
                  "score_Gpairs_per_s": round(pairs / max(best["blend"], 1e-6) / 1e6, 1),
                  "image_first_view_stages_ms": image_best, "score_over_blend_first_view": None if V != 1 else
                  round(best["blend"] / max(image_best["blend"], 1e-6), 2),
                  "never_seen": int(np.count_nonzero(peak == 0)), "peak_under_0.01": int(np.count_nonzero(peak < np.float32(0.01))),
                  "total_max": int(tot.max()) if n else 0})
    finally:
        rr.close()
    if out is not None:
        out.close()


if __name__ == "__main__":
    main()
