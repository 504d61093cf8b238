"""Build box: the reference's own SplatFormat.read (CPU) on a PROBE_N-row file of realistic records, three runs -- the figure
profiles/splat_reader_10m.txt sets the device reader's call against.
    python tests/devtools/time_reference_splat_read.py            # PROBE_N=1000000"""
import json, os, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import splat_read_numpy as sn        # noqa: E402
from oracle import refload          # noqa: E402


def main(tmp):
    refload.load()
    import gsconverter.formats.splat as mod  # type: ignore
    n = int(os.environ.get("PROBE_N", 1_000_000))
    path = sn.write_file(os.path.join(tmp, "ref.splat"), sn.realistic_records(n, np.random.default_rng(5)))
    runs = []
    for _ in range(3):
        t = time.perf_counter()
        with np.errstate(all="ignore"):
            mod.SplatFormat().read(path)
        runs.append(round(time.perf_counter() - t, 3))
    print(json.dumps({"reference_SplatFormat_read_s": runs, "n": n}), flush=True)


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as tmp:
        main(tmp)
