"""GPU box: the .ksplat reader at sizes beyond the pytest suite's 1M rows, against the numpy restatement
(tests/ksplat_read_numpy.py), by sha256: level-1 degree-2 files of random row bytes (every float16 pattern, NaNs included) in
two sections, the second with many partially filled buckets and a NaN and an infinite bucket centre.
usage: python tests/devtools/check_ksplat_read_large.py [n ...]          (default: 10000000 50000000)"""
import importlib, os, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ksplat_read_numpy as krn        # noqa: E402
reader = importlib.import_module("3dgsconverter_amd.formats.ksplat_reader")


def check(n, tmp):
    rng = np.random.default_rng(23)
    n2 = n // 4
    lens = rng.integers(0, 2 * (n2 // 2000) + 1, 2000)
    lens[-1] += max(0, n2 - int(lens.sum()))
    a = krn.section(1, 2, n - n2, rng, bucket_size=256, max_splats=n - n2 + 3)
    b = krn.section(1, 1, n2, rng, bucket_size=100, block_size=0.37, full_buckets=0, partial=lens)
    b["centres"].view(np.uint32)[7] = (0x7F800123, 0x7F800000, 0xFFC00456)
    path = krn.build_file(os.path.join(tmp, "large.ksplat"), 1, [a, b])
    del a, b
    t = time.perf_counter()
    rows, meta = reader.read_ksplat(path)
    t_gpu = time.perf_counter() - t
    got = krn.sha(rows).hex()
    del rows
    print("check_ksplat_read_large: n=%d: device read done in %.2f s, running the restatement" % (n, t_gpu), flush=True)
    t = time.perf_counter()
    want_rows, wmeta = krn.read(path)
    want = krn.sha(want_rows).hex()
    ok = got == want and repr(meta) == repr(wmeta)
    print("check_ksplat_read_large: n=%d: device %s, restatement %s -> %s (read %.2f s, restatement %.1f s)"
          % (n, got[:16], want[:16], "EQUAL" if ok else "DIFFER", t_gpu, time.perf_counter() - t), flush=True)
    return ok


if __name__ == "__main__":
    sizes = [int(a) for a in sys.argv[1:]] or [10_000_000, 50_000_000]
    with tempfile.TemporaryDirectory() as tmp:
        runs = [check(n, tmp) for n in sizes]
    sys.exit(0 if all(runs) else 1)
