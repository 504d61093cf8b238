"""GPU box: the scene transform at PROBE_N rows of 248 bytes (the canonical degree-3 table, every f_rest field set).

The kernel alone on resident rows -- gsx_rows_transform_dev with every part active (rotation, scale, translation), in place and
into a second buffer, and with the position alone (a translation) -- beside gsx_rows_take_dev of every row of the same table,
which moves the same 2 n stride bytes without arithmetic.  Each figure is a host clock around a call that ends in a stream
synchronisation: 2 warm-up calls, PROBE_REPS timed ones, the minimum and the median; GB/s is 2 n stride over the minimum, and
the fraction is of the MI355X's 8 TB/s HBM peak.  Then the stage clocks of ``apply_transform`` on a lazy processor over
resident rows (transform, download) and of ``rows_transform_table`` from the host table (upload, transform, download).
    python tools/probe_transform.py [output file]      # PROBE_N=10000000 PROBE_REPS=10"""
import importlib, json, os, statistics, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ply_read_numpy as pn        # noqa: E402

BLOCK = 65536
HBM_PEAK_GBPS = 8000.0


def scene(n, seed=11):
    """n canonical rows: a random block repeated, coordinates of their own"""
    block = pn.build(min(BLOCK, n), pn.canonical_fields(3), np.random.default_rng(seed))
    table = np.tile(block, (n + len(block) - 1) // len(block))[:n].copy()
    rng = np.random.default_rng(seed + 1)
    for a in ("x", "y", "z"):
        table[a] = rng.standard_normal(n, dtype=np.float32) * 3
    return table


def clock(call, reps):
    for _ in range(2):
        call()
    ms = []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t) * 1e3)
    return {"min_ms": round(min(ms), 3), "median_ms": round(statistics.median(ms), 3)}


def main():
    n = int(os.environ.get("PROBE_N", 10_000_000))
    reps = int(os.environ.get("PROBE_REPS", 10))
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out is not None:
            out.write(line + "\n")
            out.flush()
    lib = importlib.import_module("3dgsconverter_amd._lib")
    tf = importlib.import_module("3dgsconverter_amd.transform")
    dp = importlib.import_module("3dgsconverter_amd.processing.data_processor")
    lib.require_hip()
    table = scene(n)
    rb = table.dtype.itemsize
    moved = 2 * n * rb
    R = tf.rotation_from_euler_deg(-130.0, 15.5, 200.0)
    full = lib.transform_layout(tf.plan_transform(table.dtype, R, 1.25, (-4.0, 0.125, 1e-3)))
    shift = lib.transform_layout(tf.plan_transform(table.dtype, None, None, (-4.0, 0.125, 1e-3)))
    rr = lib.ResidentRows.from_host(table)
    ctx = lib.Context(0)
    d_out = ctx.alloc(table.nbytes + 64)

    def run(lay, dst):
        lib.rows_transform_dev(ctx, rr.ptr, 0, rb, n, lay, dst)
        ctx.synchronize()
    try:
        figures = {"all_parts_second_buffer": clock(lambda: run(full, d_out.ptr), reps),
                   "all_parts_in_place": clock(lambda: run(full, rr.ptr), reps),
                   "position_only_in_place": clock(lambda: run(shift, rr.ptr), reps),
                   "take_all_rows": clock(lambda: lib.rows_take_dev(ctx, rr.ptr, 0, rb, n, None, n, (), None, 0, d_out.ptr), reps)}
    finally:
        d_out.free()
        ctx.close()
        rr.close()
    for v in figures.values():
        v["GBps"] = round(moved / v["min_ms"] / 1e6, 1)
        v["of_hbm_peak"] = round(v["GBps"] / HBM_PEAK_GBPS, 3)
    emit({"what": "gsx_rows_transform_dev beside gsx_rows_take_dev on the same resident rows", "n": n, "row_bytes": rb,
          "bytes_moved_2_n_stride": moved, "hbm_peak_GBps": HBM_PEAK_GBPS, **figures,
          "transform_over_take": round(figures["all_parts_in_place"]["min_ms"] / figures["take_all_rows"]["min_ms"], 2)})

    for rep in range(2):                                            # (twice: the first run warms the arenas)
        p = dp.ChainedDataProcessor(table, resident=lib.ResidentRows.from_host(table))
        t = time.perf_counter()
        p.apply_transform(rotation=R, translation=(-4.0, 0.125, 1e-3), scale=1.25)
        got = p.data
        total = round((time.perf_counter() - t) * 1e3, 3)
        emit({"what": "apply_transform on resident rows, then .data", "run": rep, "n": n, "total_ms": total, "stage_ms": dict(p.resident_ms)})
        p.close()
        ms = {}
        t = time.perf_counter()
        host = lib.rows_transform_table(table, tf.plan_transform(table.dtype, R, 1.25, (-4.0, 0.125, 1e-3)), stage_ms=ms)
        total = round((time.perf_counter() - t) * 1e3, 3)
        emit({"what": "rows_transform_table from the host table", "run": rep, "n": n, "total_ms": total, "stage_ms": ms,
              "same_table_as_resident": bool(host.tobytes() == got.tobytes())})
        del got, host
    if out is not None:
        out.close()


if __name__ == "__main__":
    main()
