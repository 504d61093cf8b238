"""GPU box: every 30-bit (v0, v1, v2) triple of the compressed-PLY rotation word through the device reader against numpy
float64 (compressed_ply.py:364-378: the float64 square root of clip(1 - ((dv0^2 + dv1^2) + dv2^2), 0, 1), rounded to float32),
in batches of 2^24 words, `largest` cycling through 0..3.  Exhaustive over the sqrt's inputs: a device sqrt that is not correctly
rounded shows here wherever it changes a float32 component.
usage: python tests/devtools/check_cply_quat.py [batches]          (default: all 64)"""
import importlib, os, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cply_read_numpy as crn        # noqa: E402
reader = importlib.import_module("3dgsconverter_amd.formats.compressed_ply_reader")
B = 1 << 24


def expected(words):
    """the reference's four float32 components (compressed_ply.py:364-378)"""
    largest = words >> 30
    dv = [(((words >> s) & 0x3FF) / 1023.0 - 0.5) / 0.7071067811865476 for s in (20, 10, 0)]
    missing = np.sqrt(np.clip(1.0 - (dv[0] ** 2 + dv[1] ** 2 + dv[2] ** 2), 0, 1))
    q = np.zeros((len(words), 4), np.float32)
    for L in range(4):
        sel = largest == L
        q[sel, L] = missing[sel]
        for j, i in enumerate(i for i in range(4) if i != L):
            q[sel, i] = dv[j][sel]
    return q


def main():
    batches = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    ch = np.zeros(B // 256, [(f, "<f4") for f in crn.CHUNK_FIELDS])
    vt = np.zeros(B, [(f, "<u4") for f in crn.VERTEX_FIELDS])
    bad_total, t0 = 0, time.perf_counter()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "q.ply")
        for b in range(batches):
            low = np.arange(b * B, (b + 1) * B, dtype=np.uint64)
            vt["packed_rotation"] = ((b % 4) << 30 | low).astype(np.uint32)
            crn.write_ply(path, [("chunk", ch), ("vertex", vt)])
            rows, _ = reader.read_compressed_ply(path)
            got = np.stack([rows["rot_%d" % i] for i in range(4)], 1).view(np.uint32)
            want = expected(vt["packed_rotation"]).view(np.uint32)
            bad = int(np.count_nonzero((got != want).any(1)))
            bad_total += bad
            print("check_cply_quat: batch %2d (words 0x%08x..) largest %d: %d mismatching words" % (b, int(vt["packed_rotation"][0]), b % 4, bad), flush=True)
    print("check_cply_quat: %d words, %d mismatches, %.0f s" % (batches * B, bad_total, time.perf_counter() - t0), flush=True)
    return bad_total == 0


if __name__ == "__main__":
    sys.exit(0 if main() else 1)
