"""GPU box: the .ksplat writer's whole file at sizes beyond the pytest suite's 1M, against the numpy restatement
(tests/ksplat_numpy.py), by sha256, at levels 0, 1 and 2.
usage: python tests/devtools/check_ksplat_large.py [n ...]          (default: 10000000 50000000)"""
import hashlib, importlib, os, struct, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ksplat_numpy                  # noqa: E402
from tools.probe_sog import table    # noqa: E402
writer = importlib.import_module("3dgsconverter_amd.formats.ksplat_writer")


def restated_sha(data, level, kw, chunk=2_048_000):
    """sha256 of the restated file, the rows restated over blocks of whole buckets (bounded float temporaries)"""
    level, sh_level, bs, blk = ksplat_numpy.options(level, **kw)
    degree = ksplat_numpy.sh_degree(data, sh_level)
    h, s, word, nb = ksplat_numpy.heads(len(data), level, bs, blk, degree)
    sha = hashlib.sha256(h + s + word)
    cen = ksplat_numpy.centres(data, bs) if level >= 1 else None
    if level >= 1:
        sha.update(cen.tobytes())
    step = max(bs, chunk // bs * bs)
    for a in range(0, len(data), step):
        sha.update(ksplat_numpy.rows(data[a:a + step], min(level, 3), ksplat_numpy.n_sh(degree), cen, bs, blk, first_row=a).tobytes())
    return sha.hexdigest()


def check(n, level, kw):
    data = table(n, 11)
    data["opacity"][::100_003] = np.nan
    data["x"][5::300_007] = np.inf
    data["y"][7::300_011] = 3e6
    data["scale_1"][9::200_003] = 40.0
    t = time.perf_counter()
    try:
        out, degree = writer.encode(data, level, **kw)
    except struct.error as e:        # a payload past the header's 32-bit size: the reference refuses it too
        try:
            restated_sha(data, level, kw)
            ok = False
        except struct.error as e2:
            ok = str(e) == str(e2)
        print("check_ksplat_large: n=%d level %d %r: struct.error %r (restatement raises the same: %s)" % (n, level, kw, str(e), ok), flush=True)
        return ok
    t_gpu = time.perf_counter() - t
    got = hashlib.sha256(out).hexdigest()
    t = time.perf_counter()
    want = restated_sha(data, level, kw)
    ok = got == want
    print("check_ksplat_large: n=%d level %d %r degree %d: device %s, restatement %s -> %s (encode %.2f s, restatement %.1f s)"
          % (n, level, kw, degree, got[:16], want[:16], "EQUAL" if ok else "DIFFER", t_gpu, time.perf_counter() - t), flush=True)
    return ok


if __name__ == "__main__":
    sizes = [int(a) for a in sys.argv[1:]] or [10_000_000, 50_000_000]
    runs = []
    for n in sizes:
        for level in (0, 1, 2):
            runs.append(check(n, level, {}))
        if n * 140 >= 1 << 32:           # level 0 at degree 2 is past 4 GiB: the same rows at sh_level 1 still fit
            runs.append(check(n, 0, dict(sh_level=1)))
    sys.exit(0 if all(runs) else 1)
