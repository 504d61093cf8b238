"""GPU box: the .splat writer's whole file at sizes beyond the pytest suite's 1M, against the numpy restatement
(tests/splat_numpy.py), by sha256: a 248-byte table with scattered NaN / +-inf / underflowing rows, and a tie-heavy table.
usage: python tests/devtools/check_splat_large.py [n ...]          (default: 10000000 50000000)"""
import hashlib, importlib, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import splat_numpy                   # noqa: E402
from tools.probe_sog import table    # noqa: E402
writer = importlib.import_module("3dgsconverter_amd.formats.splat_writer")


def restated_sha(data, chunk=4_000_000):
    """sha256 of the restated file: the order over the whole table, the records restated over blocks of it"""
    order = splat_numpy.order(data)
    sha = hashlib.sha256()
    for a in range(0, len(data), chunk):
        sha.update(splat_numpy.records(data[order[a:a + chunk]]).tobytes())
    return sha.hexdigest()


def check(n, kind):
    data = table(n, 11)
    if kind == "ties":
        rng = np.random.default_rng(5)
        for f in ("scale_0", "scale_1", "scale_2"):
            data[f] = np.log(rng.integers(1, 9, n).astype(np.float32) / np.float32(64))
        data["opacity"] = rng.choice(np.array([-3.0, -1.0, 0.0, 2.0, 5.0], np.float32), n)
    data["opacity"][::100_003] = np.nan
    data["x"][5::300_007] = np.inf
    data["rot_2"][7::300_011] = np.nan
    data["scale_1"][9::200_003] = 40.0
    data["scale_0"][13::200_009] = -150.0
    t = time.perf_counter()
    out = writer.encode(data)
    t_gpu = time.perf_counter() - t
    got = hashlib.sha256(out).hexdigest()
    del out
    t = time.perf_counter()
    want = restated_sha(data)
    ok = got == want
    print("check_splat_large: n=%d %s: device %s, restatement %s -> %s (encode %.2f s, restatement %.1f s)"
          % (n, kind, got[:16], want[:16], "EQUAL" if ok else "DIFFER", t_gpu, time.perf_counter() - t), flush=True)
    return ok


if __name__ == "__main__":
    sizes = [int(a) for a in sys.argv[1:]] or [10_000_000, 50_000_000]
    runs = []
    for n in sizes:
        for kind in ("random", "ties"):
            runs.append(check(n, kind))
    sys.exit(0 if all(runs) else 1)
