"""GPU box: the table profile at PROBE_N rows of 248 bytes (the canonical degree-3 table) -- the fused pass
(gsx_table_profile_dev) beside the two passes it stands for on the same resident rows, the SH scan of the writers
(gsx_spz_rest_nonzero_dev, all 45 fields) and the chain's box kernel (DeviceChain.bbox, which reads the chain's own 12-byte
coordinate rows), then the host twin (gsx_table_profile_host) and numpy's strided column expressions on the host table.  Each
device figure is a host clock around a call that ends in a stream synchronisation: 2 warm-up calls, PROBE_REPS timed ones, the
minimum and the median.  The scene is degree 1 in 45 columns (the padded table a 3DGS read hands over).
On the same resident rows, in the same run, csrc/resident_rows.hip's kernels: gsx_rows_columns_f32_dev for the chain's (n, 3)
coordinates and for one column, gsx_rows_take_dev for every row (36 fields zeroed, three colour bytes appended) and for a
scattered quarter of them -- each beside the profile pass, which reads the same bytes.  Then two conversions, each without and
with the resident rows (``Converter(resident=False)`` is the path through the host table): .ply -> .splat with no filter, and
.ply -> alpha, density, SOR, auto_bbox -> .spz.
    python tools/probe_converter.py            # PROBE_N=10000000 PROBE_REPS=10"""
import importlib, json, os, statistics, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ply_read_numpy as pn        # noqa: E402

BLOCK = 65536


def scene(n, seed=11):
    """n canonical rows, a random block repeated under coordinates of their own; f_rest_9 .. f_rest_44 zero"""
    block = pn.build(min(BLOCK, n), pn.canonical_fields(3), np.random.default_rng(seed))
    for i in range(9, 45):
        block["f_rest_%d" % i] = 0.0
    table = np.tile(block, (n + len(block) - 1) // len(block))[:n].copy()
    rng = np.random.default_rng(seed + 1)
    for a in ("x", "y", "z"):                                  # no two rows at one place: the filters see a scene
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
    lib = importlib.import_module("3dgsconverter_amd._lib")
    lib.require_hip()
    table = scene(n)
    rb = table.dtype.itemsize
    ctx = lib.Context(0)
    d = ctx.alloc(table.nbytes + 16)
    lib.upload_table(lib.load(), ctx, d.ptr, table)
    lay = lib.spz_layout(table.dtype)
    fused = clock(lambda: lib.table_profile_dev(ctx, d, 0, n, table.dtype), reps)
    scan = clock(lambda: lib.rest_nonzero_word(lib.load(), ctx, d, lay, n, range(45)), reps)
    prof = lib.table_profile_dev(ctx, d, 0, n, table.dtype)
    assert prof["rest_nonzero"] == lib.rest_nonzero_word(lib.load(), ctx, d, lay, n, range(45)) == (1 << 9) - 1
    resident_kernels(lib, ctx, d, table, n, reps, fused)
    d.free()
    chain = lib.DeviceChain(table=table)
    box = clock(chain._bbox_dev, reps)
    lo, hi = chain._bbox_dev()
    assert all(float(lo[a]) == prof["lo"][a] and float(hi[a]) == prof["hi"][a] for a in range(3))
    chain.close()
    ctx.close()
    print(json.dumps({"what": "device passes over resident rows", "n": n, "row_bytes": rb, "table_profile_dev": fused,
                      "spz_rest_nonzero_dev_45_fields": scan, "chain_bbox_dev_12_byte_rows": box,
                      "sum_of_the_two_min_ms": round(scan["min_ms"] + box["min_ms"], 3),
                      "table_profile_GBps": round(n * rb / fused["min_ms"] / 1e6, 1)}), flush=True)
    host = clock(lambda: lib.host_table_profile(table), max(3, reps // 3))
    t = time.perf_counter()
    word = sum(int(np.any(table["f_rest_%d" % i] != 0)) << i for i in range(45))
    t_any = (time.perf_counter() - t) * 1e3
    t = time.perf_counter()
    ext = [(table[a].min(), table[a].max()) for a in ("x", "y", "z")]
    t_minmax = (time.perf_counter() - t) * 1e3
    assert word == prof["rest_nonzero"] and all(float(ext[a][0]) == prof["lo"][a] for a in range(3))
    print(json.dumps({"what": "host passes over the table", "n": n, "host_table_profile": host,
                      "numpy_45_strided_any_ms": round(t_any, 1), "numpy_per_column_ms": round(t_any / 45, 1),
                      "numpy_six_strided_minmax_ms": round(t_minmax, 1)}), flush=True)
    conversion(table, n)


def resident_kernels(lib, ctx, d, table, n, reps, fused):
    """csrc/resident_rows.hip on the uploaded rows `d`, each call ending in a stream synchronisation like the profile's"""
    rb = table.dtype.itemsize
    fields = table.dtype.fields
    d_cols, d_take = ctx.alloc(16 * n + 16), ctx.alloc(n * (rb + 3) + 64)
    d_extra, d_idx = ctx.alloc(3 * n + 16), ctx.alloc(4 * n + 16)
    lib.check(lib.load().gsx_dev_memset(ctx.handle, d_extra.ptr, 7, 3 * n), "gsx_dev_memset")
    idx = np.flatnonzero(np.random.default_rng(5).random(n) < 0.25).astype(np.uint32)
    d_idx.upload(idx)
    zero = [fields["f_rest_%d" % i][1] for i in range(9, 45)]

    def columns(names):
        lib.rows_columns_dev(ctx, d.ptr, 0, table.dtype, n, names, d_cols.ptr)
        ctx.synchronize()
    try:
        xyz = clock(lambda: columns(("x", "y", "z")), reps)
        one = clock(lambda: columns(("opacity",)), reps)
        assert np.array_equal(d_cols.download(np.float32, 1000), table["opacity"][:1000])
        take_all = clock(lambda: lib.rows_take_dev(ctx, d.ptr, 0, rb, n, None, n, zero, d_extra.ptr, 3, d_take.ptr), reps)
        take_quarter = clock(lambda: lib.rows_take_dev(ctx, d.ptr, 0, rb, n, d_idx.ptr, len(idx), zero, d_extra.ptr, 3, d_take.ptr), reps)
        got = d_take.download(np.uint8, 4 * (rb + 3)).reshape(4, rb + 3)
        assert got[:, :36].tobytes() == table[idx[:4]].view(np.uint8).reshape(4, rb)[:, :36].tobytes() and (got[:, rb:] == 7).all()
    finally:
        for b in (d_cols, d_take, d_extra, d_idx):
            b.free()
    base = fused["min_ms"]
    print(json.dumps({"what": "resident_rows.hip on the same rows", "n": n, "row_bytes": rb, "table_profile_dev_min_ms": base,
                      "columns_xyz": xyz, "columns_one": one, "take_all_rows_zero36_rgb": take_all,
                      "take_scattered_quarter_zero36_rgb": dict(take_quarter, n_out=int(len(idx))),
                      "times_the_profile_pass": {"columns_xyz": round(xyz["min_ms"] / base, 2), "columns_one": round(one["min_ms"] / base, 2),
                                                 "take_all": round(take_all["min_ms"] / base, 2),
                                                 "take_quarter": round(take_quarter["min_ms"] / base, 2)},
                      "take_all_GBps_read_plus_written": round(n * (2 * rb + 6) / take_all["min_ms"] / 1e6, 1)}), flush=True)


def conversion(table, n):
    """the stage clocks of .ply -> .splat (no filter) and of .ply -> filters -> .spz, each through the host table
    (resident=False) and with the reader's rows kept in HBM; the file has no normals, so its 236-byte rows are not the
    table's and the read takes the device path (upload, transcode, profile, download)"""
    import tempfile
    import numpy.lib.recfunctions as rfn
    conv = importlib.import_module("3dgsconverter_amd.converter")
    with tempfile.TemporaryDirectory() as tmp:
        src, dst = os.path.join(tmp, "scene.ply"), os.path.join(tmp, "scene.spz")
        names = [f for f in table.dtype.names if f not in ("nx", "ny", "nz")]
        with open(src, "wb") as f:
            f.write(pn.header_text([("vertex", n, [(nm, "f4") for nm in names])]))
            f.write(memoryview(rfn.repack_fields(table[names])))
        jobs = ((".ply -> .splat, no filter", "splat", os.path.join(tmp, "scene.splat"), {}),
                (".ply -> alpha, density, SOR, auto_bbox -> .spz", "spz", dst,
                 dict(min_opacity=5, density_sensitivity=0.3, sor_intensity=5, auto_bbox=True, compression_level=1)))
        for what, target, out, kwargs in jobs:
            for resident in (False, True, False, True):             # (twice each: the first run of a kind warms the arenas)
                c = conv.Converter(src, out, target, resident=resident)
                t = time.perf_counter()
                c.run(**kwargs)
                total = round((time.perf_counter() - t) * 1e3, 1)
                ms = c.stage_ms
                print(json.dumps({"what": what, "resident": resident, "n_in": n, "n_out": len(c.data), "total_ms": total,
                                  "process_plus_write_upload_ms": round(ms["process"] + ms.get("write_upload", 0.0), 3),
                                  "stage_ms": ms}), flush=True)
                del c


if __name__ == "__main__":
    main()
