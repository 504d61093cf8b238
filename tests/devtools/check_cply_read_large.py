"""GPU box: the compressed-PLY reader at sizes beyond the pytest suite's 1M rows, against the numpy restatement
(tests/cply_read_numpy.py), by sha256: degree-3 files of random words and bounds, with a NaN-payload, an infinite and a
denormal chunk.
usage: python tests/devtools/check_cply_read_large.py [n ...]          (default: 10000000 50000000)"""
import importlib, os, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cply_read_numpy as crn        # noqa: E402
reader = importlib.import_module("3dgsconverter_amd.formats.compressed_ply_reader")


def check(n, tmp):
    path = crn.scene_file(os.path.join(tmp, "large.ply"), n, 3, 23)
    el = crn.read_ply(path)
    ch = el["chunk"]
    u = ch.view(np.uint32).reshape(len(ch), 18)
    u[7, 0] = 0x7F800123          # NaN min_x with a payload
    u[11, 15] = 0xFFC00456        # NaN max_r
    u[13, 6], u[13, 9] = 0xFF800000, 0x7F800000   # -inf / inf scale bounds
    u[17, 1], u[17, 4] = 0x00000003, 0x00000009   # denormal y bounds
    crn.write_ply(path, [("chunk", ch), ("vertex", el["vertex"]), ("sh", el["sh"])])
    t = time.perf_counter()
    rows, meta = reader.read_compressed_ply(path)
    t_gpu = time.perf_counter() - t
    got = crn.sha(rows).hex()
    del rows
    t = time.perf_counter()
    want_rows, wmeta = crn.decode(ch, el["vertex"], el["sh"])
    want = crn.sha(want_rows).hex()
    ok = got == want and meta == wmeta
    print("check_cply_read_large: n=%d: device %s, restatement %s -> %s (read %.2f s, restatement %.1f s)"
          % (n, got[:16], want[:16], "EQUAL" if ok else "DIFFER", t_gpu, time.perf_counter() - t), flush=True)
    return ok


if __name__ == "__main__":
    sizes = [int(a) for a in sys.argv[1:]] or [10_000_000, 50_000_000]
    with tempfile.TemporaryDirectory() as tmp:
        runs = [check(n, tmp) for n in sizes]
    sys.exit(0 if all(runs) else 1)
