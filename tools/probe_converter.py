"""GPU box: the table profile at PROBE_N rows of 248 bytes (the canonical degree-3 table) -- the fused pass
(gsx_table_profile_dev) beside the two passes it stands for on the same resident rows, the SH scan of the writers
(gsx_spz_rest_nonzero_dev, all 45 fields) and the chain's box kernel (DeviceChain.bbox, which reads the chain's own 12-byte
coordinate rows), then the host twin (gsx_table_profile_host) and numpy's strided column expressions on the host table.  Each
device figure is a host clock around a call that ends in a stream synchronisation: 2 warm-up calls, PROBE_REPS timed ones, the
minimum and the median.  The scene is degree 1 in 45 columns (the padded table a 3DGS read hands over).
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


def conversion(table, n):
    """the stage clocks of one .ply -> filters -> .spz conversion; the file has no normals, so its 236-byte rows are not the
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
        c = conv.Converter(src, dst, "spz")
        t = time.perf_counter()
        c.run(min_opacity=5, density_sensitivity=0.3, sor_intensity=5, auto_bbox=True, compression_level=1)
        total = round((time.perf_counter() - t) * 1e3, 1)
        print(json.dumps({"what": ".ply -> alpha, density, SOR, auto_bbox -> .spz", "n_in": n, "n_out": len(c.data), "total_ms": total,
                          "stage_ms": c.stage_ms}), flush=True)


if __name__ == "__main__":
    main()
