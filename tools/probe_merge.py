"""GPU box: the merge's row remap at PROBE_N rows per source, beside gsx_rows_take_dev of as many rows.

``ResidentRows.concat`` of two sources of PROBE_N rows each -- the .spz reader's degree-1 rows (107 bytes) and the 248-byte 3DGS
rows -- into 251-byte rows (degree 3 with colours): two gsx_rows_remap_dev launches and one join, stage_ms["remap"]; the same
two launches one at a time; the 248-byte rows into a 248-byte layout with three fields moved (no word of the image crosses a run
or a row: the descriptor lookup without the byte-by-byte words); and gsx_rows_take_dev without an index list over 2 PROBE_N rows of 248 bytes, which moves the same
order of bytes through the same staging and stores.  Each figure is a host clock around calls that end in a stream
synchronisation: 2 warm-up calls, PROBE_REPS timed ones, the minimum and the median; GB/s is the bytes read plus the bytes
written over the minimum, and the fraction is of the MI355X's 8 TB/s HBM peak.  The first and last 1000 rows of each source's
range of the union are compared with the numpy definition (tests/merge_numpy.py): the union is 2.5 GB, past 2^31 bytes.

PROBE_TAKE_ONLY=1 times the take alone, and PROBE_ROOT=<another checkout of this repository, built> imports the package from
there: the take of an earlier commit on the same machine, in the same call.
    python tools/probe_merge.py [output file]      # PROBE_N=5000000 PROBE_REPS=10"""
import importlib, json, os, statistics, sys, time
import numpy as np
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.abspath(os.environ.get("PROBE_ROOT", HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(HERE, "tests"))

HBM_PEAK_GBPS = 8000.0


def clock(call, reps):
    for _ in range(2):
        call()
    ms = []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t) * 1e3)
    return {"min_ms": round(min(ms), 3), "median_ms": round(statistics.median(ms), 3)}


def rates(figure, moved):
    figure["bytes_moved"] = moved
    figure["GBps"] = round(moved / figure["min_ms"] / 1e6, 1)
    figure["of_hbm_peak"] = round(figure["GBps"] / HBM_PEAK_GBPS, 3)
    return figure


def tiled(dtype, n, seed):
    """n rows: a block of 65536 rows of random bytes, repeated"""
    block = np.random.default_rng(seed).integers(0, 256, min(n, 65536) * dtype.itemsize, dtype=np.uint8)
    return np.resize(block, n * dtype.itemsize).view(dtype)


def main():
    n = int(os.environ.get("PROBE_N", 5_000_000))
    reps = int(os.environ.get("PROBE_REPS", 10))
    take_only = os.environ.get("PROBE_TAKE_ONLY") == "1"
    out = open(sys.argv[1], "a") if len(sys.argv) > 1 else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out is not None:
            out.write(line + "\n")
            out.flush()
    lib = importlib.import_module("3dgsconverter_amd._lib")
    lib.require_hip()
    import merge_cases as mc
    import merge_numpy as mn
    wide = tiled(mc.standard_dtype(), 2 * n, 5)
    rr = lib.ResidentRows.from_host(wide)
    ctx = lib.Context(0)
    d_out = ctx.alloc(wide.nbytes + 64)
    try:
        take = clock(lambda: lib.rows_take_dev(ctx, rr.ptr, 0, 248, 2 * n, None, 2 * n, (), None, 0, d_out.ptr), reps)
    finally:
        d_out.free()
        ctx.close()
        rr.close()
    emit({"what": "gsx_rows_take_dev, every row, no index list", "package": os.environ.get("PROBE_ROOT", "this tree"), "rows": 2 * n, "row_bytes": 248, **rates(take, 2 * wide.nbytes)})
    if take_only:
        return
    merge = importlib.import_module("3dgsconverter_amd.merge")
    union = mc.DESTINATIONS[251]
    a, b = tiled(mc.spz_dtype(1), n, 6), wide[:n]
    runs = [merge.remap_runs(t.dtype, union) for t in (a, b)]
    parts = [lib.ResidentRows.from_host(a), lib.ResidentRows.from_host(b)]
    dst = lib.ResidentRows(2 * n, union)
    ctx = lib.Context(0)
    try:
        got = lib.ResidentRows.concat(parts, union, runs)
        try:
            for k, (t, row0) in enumerate(((a, 0), (b, n))):
                for lo in (0, n - 1000):
                    rows = np.empty(1000, union)
                    lib.check(ctx.lib.gsx_dev_download(ctx.handle, rows.ctypes.data, got.ptr + (row0 + lo) * 251, rows.nbytes), "gsx_dev_download")
                    assert rows.tobytes() == mn.merge_tables([t[lo:lo + 1000]], union).tobytes(), (k, lo)
        finally:
            got.close()

        def both():
            ms = {}
            lib.ResidentRows.concat(parts, union, runs, stage_ms=ms).close()
            return ms["remap"]

        def one(k):
            p = parts[k]
            lib.rows_remap_dev(ctx, p.ptr, 0, p.dtype.itemsize, n, runs[k], dst.ptr, 0, 251, k * n, 2 * n)
            ctx.synchronize()
        for _ in range(2):
            both()
        ms = [both() for _ in range(reps)]
        remap = {"min_ms": round(min(ms), 3), "median_ms": round(statistics.median(ms), 3)}
        singles = [clock(lambda k=k: one(k), reps) for k in (0, 1)]
        # the same 248-byte rows into a 248-byte layout with the normals moved behind the last field: three runs, every word of
        # the image inside one run and one row, so no word is assembled byte by byte -- the descriptor lookup alone
        std = mc.standard_dtype()
        moved_normals = np.dtype([(nm, "<f4") for nm in std.names if nm not in ("nx", "ny", "nz")] + [(nm, "<f4") for nm in ("nx", "ny", "nz")])
        aligned_runs = merge.remap_runs(std, moved_normals)

        def aligned():
            lib.rows_remap_dev(ctx, parts[1].ptr, 0, 248, n, aligned_runs, dst.ptr, 0, 248, 0, n)
            ctx.synchronize()
        whole_words = clock(aligned, reps)
    finally:
        ctx.close()
        dst.close()
        for p in parts:
            p.close()
    moved = [t.nbytes + n * 251 for t in (a, b)]
    emit({"what": "ResidentRows.concat: stage_ms['remap'] of two sources into 251-byte rows", "rows": 2 * n, "source_row_bytes": [107, 248],
          "runs_per_row": [len(r) for r in runs], **rates(remap, sum(moved)),
          "source_107_alone": rates(singles[0], moved[0]), "source_248_alone": rates(singles[1], moved[1]),
          "source_248_into_248_whole_words": dict(rates(whole_words, 2 * n * 248), runs_per_row=len(aligned_runs)),
          "time_per_byte_over_take": round((remap["min_ms"] / sum(moved)) / (take["min_ms"] / (2 * wide.nbytes)), 3)})


if __name__ == "__main__":
    main()
