"""GPU box: every rotation code through the SPZ reader's kernel against the numpy restatement (tests/spz_read_numpy.py): all
2^30 version-3 component triples (with the idx of the chunk's number mod 4; the largest component does not depend on it, and
every triple's placement under every idx is the pytest suite's pattern file) and all 2^24 legacy triples, rot_0..3 compared
bit for bit, in chunks of 2^24 rows of degree 0.
usage: python tests/devtools/check_spz_read_quat.py [first_chunk [chunks]]          (default: all 64 version-3 chunks)"""
import importlib, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import spz_read_numpy as srn        # noqa: E402
lib = importlib.import_module("3dgsconverter_amd._lib")
reader = importlib.import_module("3dgsconverter_amd.formats.spz_reader")
CHUNK = 1 << 24


def device_rotations(version, rot_bytes: np.ndarray) -> np.ndarray:
    """-> float32 bits [CHUNK, 4] of rot_0..3 for a body that is zero but for its rotation section"""
    per = srn.section_bytes(version, 0)
    start = CHUNK * sum(per[:4])

    def fill(host):
        host[:] = 0
        host[start:start + rot_bytes.size] = rot_bytes
    rows = lib.spz_unpack_table(fill, srn.body_bytes(version, 0, CHUNK), version, 0, 12, CHUNK, reader.define_dtype(0))
    return np.stack([rows["rot_%d" % a].view(np.uint32) for a in range(4)], axis=1)


def check(version, chunk) -> bool:
    i = np.arange(CHUNK, dtype=np.uint32)
    if version == 3:
        packed = (np.uint32(chunk % 4) << 30) | ((np.uint32(chunk) << 24) + i)
        want = srn.v3_rotation(packed)
        raw = packed.astype("<u4").view(np.uint8)
    else:
        tri = np.stack([i & 0xFF, (i >> 8) & 0xFF, i >> 16], axis=1).astype(np.uint8)
        want = srn.legacy_rotation(tri)
        raw = tri.reshape(-1)
    want = np.stack([w.astype(np.float32).view(np.uint32) for w in want], axis=1)
    got = device_rotations(version, raw)
    bad = np.nonzero((got != want).any(axis=1))[0]
    if len(bad):
        print("check_spz_read_quat: version %d chunk %d: %d rows differ, first code %d: %s != %s"
              % (version, chunk, len(bad), bad[0], got[bad[0]], want[bad[0]]), flush=True)
    return not len(bad)


if __name__ == "__main__":
    first = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    count = int(sys.argv[2]) if len(sys.argv) > 2 else 64 - first
    t = time.perf_counter()
    ok = check(2, 0) if first == 0 else True
    print("check_spz_read_quat: all 2^24 legacy triples: %s" % ("EQUAL" if ok else "DIFFER"), flush=True)
    for c in range(first, first + count):
        ok = check(3, c) and ok
        print("check_spz_read_quat: version-3 chunk %d of 64 done (%.0f s) %s" % (c, time.perf_counter() - t, "ok" if ok else "DIFFER"), flush=True)
    print("check_spz_read_quat: %s" % ("EQUAL" if ok else "DIFFER"))
    sys.exit(0 if ok else 1)
