"""GPU box: the fidelity measurement at PROBE_N rows of 248 bytes (tools/probe_decimate.py's scene) against a second table --
the same rows with every opacity lowered by 0.25, a loss every pixel sees --, over 8 views of 512 x 512 framed on the scene's
box: the stage clocks of one ``fidelity.compare_rows`` (the six render stages summed over both tables and all views, and the
compare kernel), the whole call, and the figures; then ``gsx_image_compare_dev`` alone on two random 1920 x 1080 images, 2
warm-up calls and PROBE_REPS timed ones, the minimum of the stream's own clock and the bytes it read per second (each image once:
2 x 6.2 MB).
    python tools/probe_fidelity.py [output file]      # PROBE_N=10000000 PROBE_REPS=5"""
import importlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from probe_decimate import scene   # noqa: E402

import numpy as np   # noqa: E402

VIEWS, SIZE, FRAME = 8, (512, 512), (1920, 1080)


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
    fid = importlib.import_module("3dgsconverter_amd.fidelity")
    vw = importlib.import_module("3dgsconverter_amd.views")
    lib.require_hip()
    table = scene(n)
    ra = lib.ResidentRows.from_host(table)
    table["opacity"] -= np.float32(0.25)
    rb = lib.ResidentRows.from_host(table)
    try:
        prof = ra.profile()
        cams = vw.plan_views(prof["lo"], prof["hi"], views=VIEWS, size=SIZE)
        runs, total, res = [], [], None
        for _ in range(1 + reps):
            ms = {}
            t = time.perf_counter()
            res = fid.compare_rows(ra, rb, cams, stage_ms=ms)
            total.append((time.perf_counter() - t) * 1e3)
            runs.append(ms)
        best = {k: round(min(r[k] for r in runs[1:]), 3) for k in lib.RENDER_STAGES + ("compare",)}
        emit({"what": "fidelity.compare_rows, stage clocks over both tables and all views", "n": n, "row_bytes": table.dtype.itemsize,
              "views": VIEWS, "width": SIZE[0], "height": SIZE[1], "stages_ms": best, "render_sum_ms": round(sum(best[k] for k in lib.RENDER_STAGES), 3),
              "compare_ms": best["compare"], "call_min_ms": round(min(total[1:]), 3), "psnr": round(res["psnr"], 4), "ssim": round(res["ssim"], 6),
              "worst_view": res["worst_view"], "sse": list(res["sse"]), "ssim_fixed": list(res["ssim_fixed"])})
    finally:
        ra.close()
        rb.close()
    rng = np.random.default_rng(7)
    w, h = FRAME
    a, b = (rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(2))
    ctx = lib.Context()
    bufs = [ctx.alloc(a.nbytes).upload(a), ctx.alloc(b.nbytes).upload(b)]
    try:
        clocks, words = [], None
        for _ in range(2 + reps):
            ms = {}
            words = lib.image_compare_dev(ctx, bufs[0].ptr, bufs[1].ptr, w, h, stage_ms=ms)
            clocks.append(ms["compare"])
        best = min(clocks[2:])
        emit({"what": "gsx_image_compare_dev alone", "width": w, "height": h, "kernel_min_ms": round(best, 4),
              "image_GB_per_s": round(2 * a.nbytes / max(best, 1e-6) / 1e6, 1), "windows": words["windows"], "sse": list(words["sse"]),
              "ssim_fixed": list(words["ssim"])})
    finally:
        for buf in bufs:
            buf.free()
        ctx.close()
    if out is not None:
        out.close()


if __name__ == "__main__":
    main()
