"""GPU box: the 3DGS / CloudCompare PLY writers end to end -- per-stage clocks of a PROBE_N-row write (plan, upload, sh_detect,
pack, download, file_write, total) of five tables: degree 3 with red green blue -> CloudCompare (the rows are the file's rows
under other names: the identity path, no device stage), the same table without nx ny nz -> CloudCompare (239 bytes in, 251
out: the device path at an odd stride), degree 3 whose f_rest are all zero -> 3DGS with crop_sh (248 bytes in, 68 out: the scan
and the pack), degree 3 without nx ny nz -> 3DGS (236 in, 248 out) and the canonical degree-3 table -> 3DGS (identity).  The
pack stage is a host clock around the launch and a stream synchronisation.  The 68-byte file is then read back by
read_ply_3dgs in the same process: ply_unpack_kernel at the mirrored shape (68 in, 248 out).  The rows are a 65 536-row random
block repeated.  (The reference's own time per 1M rows: tests/devtools/time_reference_ply_write.py.)
    python tools/probe_ply_write.py            # PROBE_N=10000000 PROBE_REPS=3"""
import importlib, json, os, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ply_read_numpy as pn        # noqa: E402

BLOCK = 65536
RGB = [(c, "u1") for c in pn.COLOURS]
NORMALS = ("nx", "ny", "nz")


def probe_tables():
    """-> [(name, fields, zero f_rest, dialect, crop_sh)]"""
    no_normals = [f for f in pn.canonical_fields(3) if f[0] not in NORMALS]
    return [("rgb_degree3_to_cc", pn.canonical_fields(3) + RGB, False, "cc", False),
            ("rgb_no_normals_to_cc", no_normals + RGB, False, "cc", False),
            ("degree3_zero_rest_crop", pn.canonical_fields(3), True, "3dgs", True),
            ("no_normals_to_3dgs", no_normals, False, "3dgs", False),
            ("canonical_degree3", pn.canonical_fields(3), False, "3dgs", False)]


def repeated_table(fields, n, zero_rest=False, seed=5):
    """a table of n rows: one random block of BLOCK rows, repeated"""
    block = pn.build(min(BLOCK, n), fields, np.random.default_rng(seed))
    if zero_rest:
        for f in block.dtype.names:
            if f.startswith("f_rest_"):
                block[f] = 0
    table = np.empty(n, block.dtype)
    for start in range(0, n, len(block)):
        table[start:start + len(block)] = block[:min(len(block), n - start)]
    return table


def main():
    n = int(os.environ.get("PROBE_N", 10_000_000))
    reps = int(os.environ.get("PROBE_REPS", 3))
    writer = importlib.import_module("3dgsconverter_amd.formats.ply_writer")
    reader = importlib.import_module("3dgsconverter_amd.formats.ply_reader")
    with tempfile.TemporaryDirectory() as tmp:
        for name, fields, zero_rest, dialect, crop in probe_tables():
            table = repeated_table(fields, n, zero_rest)
            write = writer.write_ply_3dgs if dialect == "3dgs" else writer.write_ply_cc
            path = os.path.join(tmp, name + ".ply")
            stages, plan = [], None
            for _ in range(reps):
                st = {}
                t = time.perf_counter()
                plan = write(table, path, stage_ms=st, crop_sh=crop)
                st["total"] = round((time.perf_counter() - t) * 1e3, 3)
                stages.append(st)
            rec = {"table": name, "writer": dialect, "crop_sh": crop, "n": n, "file_bytes": os.path.getsize(path), "in_stride": plan.in_stride,
                   "out_stride": plan.out_stride, "fields": len(plan.fields), "runs": len(plan.runs), "identity": plan.identity,
                   "last_idx": plan.last_idx, "stage_ms": stages}
            if not plan.identity:
                best = min(s["pack"] for s in stages)
                rec["pack_best_ms"] = best
                rec["pack_GBps_by_algorithmic_bytes"] = round((plan.in_stride + plan.out_stride) * n / best / 1e6, 1)
            print(json.dumps(rec), flush=True)
            del table
            if name == "degree3_zero_rest_crop":                  # the mirrored shape through the reader's kernel, same process
                back = []
                for _ in range(reps):
                    st = {}
                    rows, _ = reader.read_ply_3dgs(path, stage_ms=st)
                    back.append(st)
                    del rows
                best = min(s["kernel"] for s in back)
                print(json.dumps({"file": name, "reader": "3dgs", "n": n, "in_stride": plan.out_stride, "out_stride": 248, "stage_ms": back,
                                  "kernel_best_ms": best, "kernel_GBps_by_algorithmic_bytes": round((plan.out_stride + 248) * n / best / 1e6, 1)}), flush=True)
            os.remove(path)


if __name__ == "__main__":
    main()
