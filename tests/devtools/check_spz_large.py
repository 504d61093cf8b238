"""GPU box: the SPZ writer's payload at sizes beyond the pytest suite's 1M, against the numpy restatement (tests/spz_numpy.py),
by sha256 of the whole uncompressed payload.
usage: python tests/devtools/check_spz_large.py [n ...]          (default: 10000000 50000000)"""
import hashlib, importlib, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import spz_numpy                     # noqa: E402
from tools.probe_sog import table    # noqa: E402
writer = importlib.import_module("3dgsconverter_amd.formats.spz_writer")


def restated_sha(data, chunk=2_000_000):
    """sha256 of the restated payload, computed over blocks of rows (the section order of the whole payload kept) to bound
    the restatement's float temporaries.  Per-row results only: a NaN rotation component's cast depends on its position in
    the WHOLE array (tests/test_spz_gpu.py covers those at 1M rows), so the tables here have none."""
    deg = spz_numpy.sh_degree(data)
    secs = [[] for _ in range(6)]
    for a in range(0, len(data), chunk):
        for s, part in enumerate(spz_numpy.sections(data[a:a + chunk], deg)):
            secs[s].append(np.ascontiguousarray(part))
    h = hashlib.sha256(spz_numpy.header(len(data), deg))
    for parts in secs:
        for p in parts:
            h.update(p)
    return h.hexdigest()


def check(n):
    data = table(n, 11)
    data["opacity"][::100_003] = np.nan
    data["x"][5::300_007] = np.inf
    data["y"][7::300_011] = 3e6
    t = time.perf_counter()
    out, degree = writer.encode(data)
    t_gpu = time.perf_counter() - t
    got = hashlib.sha256(out).hexdigest()
    t = time.perf_counter()
    want = restated_sha(data)
    ok = got == want
    print("check_spz_large: n=%d degree %d: device %s, restatement %s -> %s (encode %.2f s, restatement %.1f s)"
          % (n, degree, got[:16], want[:16], "EQUAL" if ok else "DIFFER", t_gpu, time.perf_counter() - t), flush=True)
    return ok


if __name__ == "__main__":
    sizes = [int(a) for a in sys.argv[1:]] or [10_000_000, 50_000_000]
    sys.exit(0 if all([check(n) for n in sizes]) else 1)
