"""GPU box: the 3DGS / CloudCompare PLY readers end to end -- per-stage clocks of a PROBE_N-row read (parse, file read, upload,
kernel, download, total) of three files: a degree-0 3DGS file (68 bytes a row in, padded to 248 out: the device path), a
CloudCompare file with colours and two extras (259 bytes in and out, every float field renamed: the device path) and the
canonical degree-3 file (the identity layout: read on the host alone, no device stage).  The kernel stage is a host clock
around the launch and a stream synchronisation.  The rows are a 65 536-row random block repeated.  (The reference's own time
per 1M rows: tests/devtools/time_reference_ply_read.py.)
    python tools/probe_ply_read.py            # PROBE_N=10000000 PROBE_REPS=3"""
import importlib, json, os, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ply_read_numpy as pn        # noqa: E402

BLOCK = 65536


def probe_files():
    """-> [(name, fields, dialect)]"""
    return [("3dgs_degree0", pn.canonical_fields(0), "3dgs"), ("cc_rgb_two_extras", pn.cc_fields(3), "cc"),
            ("canonical_degree3", pn.canonical_fields(3), "3dgs")]


def write_repeated(path, fields, n, seed=5):
    """a PLY file of n rows: one random block of BLOCK rows, repeated"""
    block = pn.build(min(BLOCK, n), fields, np.random.default_rng(seed))
    spec = [("vertex", n, [(f, block.dtype[f].str[1:]) for f in block.dtype.names])]
    raw = block.tobytes()
    with open(path, "wb") as f:
        f.write(pn.header_text(spec))
        for start in range(0, n, len(block)):
            f.write(raw[:min(len(block), n - start) * block.dtype.itemsize])
    return path


def main():
    n = int(os.environ.get("PROBE_N", 10_000_000))
    reps = int(os.environ.get("PROBE_REPS", 3))
    reader = importlib.import_module("3dgsconverter_amd.formats.ply_reader")
    with tempfile.TemporaryDirectory() as tmp:
        for name, fields, dialect in probe_files():
            path = write_repeated(os.path.join(tmp, name + ".ply"), fields, n)
            read = reader.read_ply_3dgs if dialect == "3dgs" else reader.read_ply_cc
            stages, row_bytes = [], None
            for _ in range(reps):
                st = {}
                t = time.perf_counter()
                rows, _ = read(path, stage_ms=st)
                st["total"] = round((time.perf_counter() - t) * 1e3, 3)
                stages.append(st)
                row_bytes = rows.dtype.itemsize
                del rows
            p = reader.plan(reader.parse_header(path), dialect)
            rec = {"file": name, "reader": dialect, "n": n, "file_bytes": os.path.getsize(path), "in_stride": p.in_stride, "out_stride": row_bytes,
                   "fields": len(p.fields), "identity": p.identity, "stage_ms": stages}
            if not p.identity:
                best = min(s["kernel"] for s in stages)
                rec["kernel_best_ms"] = best
                rec["kernel_GBps_by_algorithmic_bytes"] = round((p.in_stride + row_bytes) * n / best / 1e6, 1)
            print(json.dumps(rec), flush=True)
            os.remove(path)


if __name__ == "__main__":
    main()
