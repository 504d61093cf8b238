"""GPU box: the ASCII body of a 3DGS PLY end to end -- per-stage clocks of a PROBE_N-row read of a degree-3 file written with
%.9g (parse, file_read, upload, scan, kernel, patch, unpack, download, total), the reader's stats (tokens, host_tokens, chunks),
the bytes the scan and parse kernels move over their time as a fraction of the 8 TB/s HBM peak, and the binary reader's clocks
for the same rows (the canonical layout: read on the host alone).  The scan and kernel stages are host clocks around the
launches and a stream synchronisation, summed over the chunks.  The rows are an 8 192-row random block repeated.
    python tools/probe_ply_text.py            # PROBE_N=1000000 PROBE_REPS=3 PROBE_CHUNK_BYTES=<_lib.PLY_TEXT_CHUNK_BYTES>"""
import importlib, io, json, os, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ply_read_numpy as pn        # noqa: E402

BLOCK = 8192
HBM_PEAK_GBPS = 8000.0


def write_repeated(path_text, path_binary, n, seed=5):
    """the same n rows as an ASCII and as a binary PLY: one random block of BLOCK rows, repeated"""
    block = pn.build(min(BLOCK, n), pn.canonical_fields(3), np.random.default_rng(seed))
    props = [(f, "f4") for f in block.dtype.names]
    buf = io.BytesIO()
    np.savetxt(buf, block.view(np.float32).reshape(len(block), -1).astype(np.float64), fmt="%.9g")
    lines = buf.getvalue().splitlines(keepends=True)
    with open(path_text, "wb") as ft, open(path_binary, "wb") as fb:
        ft.write(pn.header_text([("vertex", n, props)], "ascii"))
        fb.write(pn.header_text([("vertex", n, props)]))
        for start in range(0, n, len(block)):
            k = min(len(block), n - start)
            ft.write(b"".join(lines[:k]))
            fb.write(block[:k].tobytes())


def main():
    n = int(os.environ.get("PROBE_N", 1_000_000))
    reps = int(os.environ.get("PROBE_REPS", 3))
    chunk = int(os.environ.get("PROBE_CHUNK_BYTES", 0)) or None
    reader = importlib.import_module("3dgsconverter_amd.formats.ply_reader")
    with tempfile.TemporaryDirectory() as tmp:
        text, binary = os.path.join(tmp, "ascii.ply"), os.path.join(tmp, "binary.ply")
        write_repeated(text, binary, n)
        want = None
        for name, path, kw in (("binary", binary, {}), ("ascii", text, {"ascii_body": True, "chunk_bytes": chunk})):
            stages, stats = [], {}
            for _ in range(reps):
                st = {}
                t = time.perf_counter()
                rows, _ = reader.read_ply_3dgs(path, stage_ms=st, **(dict(kw, stats=stats) if kw else {}))
                st["total"] = round((time.perf_counter() - t) * 1e3, 3)
                stages.append(st)
            if want is None:
                want = rows.tobytes()
            rec = {"file": name, "n": n, "file_bytes": os.path.getsize(path), "row_bytes": rows.dtype.itemsize, "stage_ms": stages,
                   "equals_binary": rows.tobytes() == want}
            if kw:
                body = os.path.getsize(path)
                scan, kern = min(s["scan"] for s in stages), min(s["kernel"] for s in stages)
                moved_scan, moved_parse = body, body + n * 248
                rec.update(stats=stats, scan_best_ms=scan, kernel_best_ms=kern,
                           scan_GBps=round(moved_scan / scan / 1e6, 1), parse_GBps=round(moved_parse / kern / 1e6, 1),
                           scan_fraction_of_hbm_peak=round(moved_scan / scan / 1e6 / HBM_PEAK_GBPS, 4),
                           parse_fraction_of_hbm_peak=round(moved_parse / kern / 1e6 / HBM_PEAK_GBPS, 4))
            print(json.dumps(rec), flush=True)
            del rows


if __name__ == "__main__":
    main()
