"""GPU box: the SOG reader at sizes beyond the pytest suite's 65 536 rows, against the numpy restatement
(tests/sog_read_numpy.py), by sha256: degree-3 files with a 65 536-entry palette, random texels and smooth texels.
usage: python tests/devtools/check_sog_read_large.py [n ...]          (default: 10000000)"""
import importlib, os, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sog_read_numpy as srn        # noqa: E402
reader = importlib.import_module("3dgsconverter_amd.formats.sog_reader")


def check(n, kind, tmp):
    rng = np.random.default_rng(23)
    texels = srn.random_texels(n, 3, 65536, rng) if kind == "random" else srn.smooth_texels(n, 3, 65536)
    path = srn.build_file(os.path.join(tmp, "large.sog"), n, 3, 65536, rng, texels=texels)
    del texels
    t = time.perf_counter()
    rows = reader.read_sog(path)
    t_gpu = time.perf_counter() - t
    got = srn.sha(rows).hex()
    del rows
    print("check_sog_read_large: n=%d %s texels: device read done in %.2f s, running the restatement" % (n, kind, t_gpu), flush=True)
    t = time.perf_counter()
    want = srn.sha(srn.read(path)).hex()
    print("check_sog_read_large: n=%d %s texels: device %s, restatement %s -> %s (read %.2f s, restatement %.1f s)"
          % (n, kind, got[:16], want[:16], "EQUAL" if got == want else "DIFFER", t_gpu, time.perf_counter() - t), flush=True)
    return got == want


if __name__ == "__main__":
    sizes = [int(a) for a in sys.argv[1:]] or [10_000_000]
    with tempfile.TemporaryDirectory() as tmp:
        runs = [check(n, kind, tmp) for n in sizes for kind in ("random", "smooth")]
    sys.exit(0 if all(runs) else 1)
