"""GPU box: the SPZ reader at sizes beyond the pytest suite's 250 077 rows, against the numpy restatement
(tests/spz_read_numpy.py), by sha256: degree-3 files of random bytes, version 3 gzipped at level 0 and version 1 plain (every
float16 pattern, NaNs included).
usage: python tests/devtools/check_spz_read_large.py [n ...]          (default: 10000000 50000000)"""
import importlib, os, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import spz_read_numpy as srn        # noqa: E402
reader = importlib.import_module("3dgsconverter_amd.formats.spz_reader")


def check(n, version, level, tmp):
    path = srn.build_file(os.path.join(tmp, "large.spz"), version, 3, n, np.random.default_rng(23 + version), frac_bits=10, gzip_level=level)
    t = time.perf_counter()
    rows = reader.read_spz(path)
    t_gpu = time.perf_counter() - t
    got = srn.sha(rows).hex()
    del rows
    print("check_spz_read_large: n=%d version %d: device read done in %.2f s, running the restatement" % (n, version, t_gpu), flush=True)
    t = time.perf_counter()
    want = srn.sha(srn.read(path)).hex()
    print("check_spz_read_large: n=%d version %d gzip %s: device %s, restatement %s -> %s (read %.2f s, restatement %.1f s)"
          % (n, version, level, got[:16], want[:16], "EQUAL" if got == want else "DIFFER", t_gpu, time.perf_counter() - t), flush=True)
    return got == want


if __name__ == "__main__":
    sizes = [int(a) for a in sys.argv[1:]] or [10_000_000, 50_000_000]
    with tempfile.TemporaryDirectory() as tmp:
        runs = [check(n, version, level, tmp) for n in sizes for version, level in ((3, 0), (1, None))]
    sys.exit(0 if all(runs) else 1)
