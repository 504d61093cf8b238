"""GPU box: the splat budget at PROBE_N rows of 248 bytes (the canonical degree-3 table).

The kernels alone, on resident rows: the gather of the four metric fields (gsx_rows_columns_f32_dev), gsx_limit_keys_dev,
gsx_limit_select_dev at a budget of n / 2 over the table's keys and over an all-equal key array (every row a tie: the tie rule
decides everything), and, as the baseline, gsx_splat_order_dev -- the full stable radix sort of (key, row) pairs that was the
tree's only ranking primitive -- on the same keys.  Each figure is a host clock around a call that ends in a stream
synchronisation: 2 warm-up calls, PROBE_REPS timed ones, the minimum and the median; the bytes are what the method has to move
(the gather 2 n stride is not counted: n (stride + 16); the keys 20 n; the select 5 reads of 4 n and n mask bytes), GB/s is bytes
over the minimum, and the fraction is of the MI355X's 8 TB/s HBM peak.  The select's mask is checked against the sort's order
on the way.  Then ``limit_splats`` on a lazy processor over resident rows, with its stage clocks.
    python tools/probe_limit.py [output file]      # PROBE_N=10000000 PROBE_REPS=10"""
import importlib, json, os, statistics, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ply_read_numpy as pn        # noqa: E402

BLOCK = 65536
HBM_PEAK_GBPS = 8000.0


def scene(n, seed=11):
    """n canonical rows: a random block repeated, scales and opacities of their own"""
    block = pn.build(min(BLOCK, n), pn.canonical_fields(3), np.random.default_rng(seed))
    table = np.tile(block, (n + len(block) - 1) // len(block))[:n].copy()
    rng = np.random.default_rng(seed + 1)
    for a in ("scale_0", "scale_1", "scale_2"):
        table[a] = rng.standard_normal(n, dtype=np.float32) - 4
    table["opacity"] = rng.standard_normal(n, dtype=np.float32) * 3
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
    dp = importlib.import_module("3dgsconverter_amd.processing.data_processor")
    L = lib.require_hip()
    table = scene(n)
    rb = table.dtype.itemsize
    N = n // 2
    rr = lib.ResidentRows.from_host(table)
    ctx = lib.Context(0)
    d_cols, d_keys, d_ties, d_mask, d_order = ctx.alloc(16 * n), ctx.alloc(4 * n), ctx.alloc(4 * n), ctx.alloc(n + 16), ctx.alloc(4 * n)
    d_ties.upload(np.full(n, 0x3f8ccccd, np.uint32))
    infos = {}

    def gather():
        lib.rows_columns_dev(ctx, rr.ptr, rr.first_byte, rr.dtype, n, lib.LIMIT_FIELDS, d_cols.ptr)
        ctx.synchronize()

    def keys():
        lib.limit_keys_dev(ctx, d_cols.ptr, n, d_keys.ptr)
        ctx.synchronize()

    def select(name, d):
        infos[name] = lib.limit_select_dev(ctx, d.ptr, None, n, N, d_mask.ptr)      # (synchronises: the three words come back)

    def order():
        lib.check(L.gsx_splat_order_dev(ctx.handle, d_keys.ptr, n, d_order.ptr), "gsx_splat_order_dev")
        ctx.synchronize()
    try:
        figures = {"gather_4_fields": clock(gather, reps), "limit_keys": clock(keys, reps),
                   "limit_select_half": clock(lambda: select("half", d_keys), reps)}
        mask = d_mask.download(np.uint8, n).view(np.bool_)
        figures["limit_select_all_ties"] = clock(lambda: select("all_ties", d_ties), reps)
        ties_mask = d_mask.download(np.uint8, n).view(np.bool_)
        figures["splat_order_pairs_sort"] = clock(order, reps)
        first = d_order.download(np.uint32, n)[:N]
        same = bool(mask.sum() == N and mask[first].all())
        ties_ok = bool(ties_mask[:N].all() and not ties_mask[N:].any())
    finally:
        for d in (d_cols, d_keys, d_ties, d_mask, d_order):
            d.free()
        ctx.close()
        rr.close()
    moved = {"gather_4_fields": n * (rb + 16), "limit_keys": 20 * n, "limit_select_half": 21 * n, "limit_select_all_ties": 21 * n,
             "splat_order_pairs_sort": 4 * 16 * n}      # (the sort: four 8-bit passes, each reads and writes 8 n bytes of pairs)
    for k, v in figures.items():
        v["bytes"] = moved[k]
        v["GBps"] = round(moved[k] / v["min_ms"] / 1e6, 1)
        v["of_hbm_peak"] = round(v["GBps"] / HBM_PEAK_GBPS, 3)
    emit({"what": "gsx_limit_keys_dev and gsx_limit_select_dev beside gsx_splat_order_dev on the same keys", "n": n, "row_bytes": rb,
          "budget": N, "hbm_peak_GBps": HBM_PEAK_GBPS, **figures, "info_half": {k: (float(v) if k == "threshold" else v) for k, v in infos["half"].items()},
          "info_all_ties": {k: (float(v) if k == "threshold" else v) for k, v in infos["all_ties"].items()},
          "select_is_the_head_of_the_sorted_order": same, "all_ties_keeps_the_first_rows": ties_ok,
          "select_over_sort": round(figures["limit_select_half"]["min_ms"] / figures["splat_order_pairs_sort"]["min_ms"], 3)})

    for rep in range(2):                                            # (twice: the first run warms the arenas)
        p = dp.ChainedDataProcessor(table, resident=lib.ResidentRows.from_host(table))
        t = time.perf_counter()
        p.limit_splats(N)
        filtered = round((time.perf_counter() - t) * 1e3, 3)
        got = p.data
        total = round((time.perf_counter() - t) * 1e3, 3)
        emit({"what": "limit_splats on resident rows, then .data", "run": rep, "n": n, "kept": len(got), "limit_ms": filtered, "total_ms": total,
              "stage_ms": dict(p.resident_ms)})
        p.close()
        del got
    if out is not None:
        out.close()


if __name__ == "__main__":
    main()
