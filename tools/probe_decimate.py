"""GPU box: voxel decimation at PROBE_N rows of 248 bytes (the canonical degree-3 table), three scenes of uniformly random
positions in a cube: a voxel size that leaves ~1 row per group, one that leaves ~8, and the whole scene in one voxel.

Per scene ``ResidentRows.decimate`` runs 2 warm-up calls and PROBE_REPS timed ones; the five stage clocks are the stream's own
(hip events around the launches of gsx_rows_decimate_plan_dev and gsx_rows_decimate_write_dev), the minimum over the runs of
each.  Next to each stage: the bytes it has to move -- keys: the 128-byte line that holds a row's position and its neighbour's
scales, rotation and opacity (the eleven fields are the first 12 and the last 44 bytes of a row: one line per row at least, two at
most), 12 n out; order: eight 8-bit passes over
12 n bytes of (key, place) pairs, read and written; heads: three passes over the sorted keys, six 4 n arrays written, three
scans; sums: the members of the merged groups in, their rows out; finish: the single rows in and out -- and that over the
minimum as GB/s beside what ``ResidentRows.take`` of all rows achieves on the same table in the same run (a plain copy of
the rows through the same 16-byte loads and stores) and the MI355X's 8 TB/s HBM peak.
    python tools/probe_decimate.py [output file]      # PROBE_N=10000000 PROBE_REPS=5"""
import importlib, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ply_read_numpy as pn        # noqa: E402

BLOCK = 65536
HBM_PEAK_GBPS = 8000.0
SIDE = 64.0


def scene(n, seed=13):
    """n canonical rows: a random block repeated, positions uniform in [0, SIDE)^3, small scales, alphas up to 0.4"""
    block = pn.build(min(BLOCK, n), pn.canonical_fields(3), np.random.default_rng(seed))
    table = np.tile(block, (n + len(block) - 1) // len(block))[:n].copy()
    rng = np.random.default_rng(seed + 1)
    for a in "xyz":
        table[a] = rng.random(n, dtype=np.float32) * np.float32(SIDE)
    for a in ("scale_0", "scale_1", "scale_2"):
        table[a] = rng.random(n, dtype=np.float32) * np.float32(2.5) - np.float32(7.0)
    alpha = rng.random(n) * 0.35 + 0.05
    table["opacity"] = np.log(alpha / (1 - alpha)).astype(np.float32)
    return table


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
    dec = importlib.import_module("3dgsconverter_amd.decimate")
    lib.require_hip()
    table = scene(n)
    rb = table.dtype.itemsize
    rr = lib.ResidentRows.from_host(table)
    try:
        take_ms = []
        for _ in range(2 + reps):
            t = time.perf_counter()
            rr.take(None, n).close()
            take_ms.append((time.perf_counter() - t) * 1e3)
        take_gbps = round(2 * n * rb / min(take_ms[2:]) / 1e6, 1)
        emit({"what": "ResidentRows.take of every row: the copy rate the stages are held against", "n": n, "row_bytes": rb,
              "min_ms": round(min(take_ms[2:]), 3), "GBps": take_gbps, "hbm_peak_GBps": HBM_PEAK_GBPS})
        cases = (("about_1_row_per_group", SIDE / (16.0 * n) ** (1.0 / 3.0)), ("about_8_rows_per_group", SIDE / (n / 8.0) ** (1.0 / 3.0)),
                 ("one_cell", 2.0 * SIDE))
        for name, H in cases:
            plan = dec.plan_decimate(table.dtype, H)
            runs, info, total = [], None, []
            for _ in range(2 + reps):
                ms = {}
                t = time.perf_counter()
                merged = rr.decimate(plan, stage_ms=ms)
                total.append((time.perf_counter() - t) * 1e3)
                info = merged.decimate_info
                merged.close()
                runs.append(ms)
            best = {k: min(r[k] for r in runs[2:]) for k in lib.DECIMATE_STAGES}
            singles = info["passed_through"]
            members = n - singles
            moved = {"keys": 128 * n + 12 * n, "order": 8 * 2 * 12 * n, "heads": 3 * 8 * n + 6 * 4 * n + 3 * 8 * n,
                     "sums": members * rb + info["merged_groups"] * rb, "finish": 2 * singles * rb}
            stages = {k: {"min_ms": round(best[k], 3), "bytes": moved[k], "GBps": round(moved[k] / max(best[k], 1e-6) / 1e6, 1),
                          "of_take": round(moved[k] / max(best[k], 1e-6) / 1e6 / take_gbps, 3),
                          "of_hbm_peak": round(moved[k] / max(best[k], 1e-6) / 1e6 / HBM_PEAK_GBPS, 3)} for k in lib.DECIMATE_STAGES}
            emit({"what": "ResidentRows.decimate, stage clocks", "case": name, "n": n, "row_bytes": rb, "voxel_size": H, **info,
                  "rows_per_group": round(n / max(info["groups"], 1), 2), "stages": stages, "stages_ms": round(sum(best.values()), 3),
                  "call_min_ms": round(min(total[2:]), 3)})
    finally:
        rr.close()
    if out is not None:
        out.close()


if __name__ == "__main__":
    main()
