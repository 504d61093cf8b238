"""Build box: the reference's own SogFormat.read (CPU) on a PROBE_N-row degree-3 file of random texels with a 65 536-entry
palette, three runs -- the figure profiles/sog_reader_10m.txt sets the device reader's call against.
    python tests/devtools/time_reference_sog_read.py            # PROBE_N=1000000"""
import json, os, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sog_read_numpy as srn        # noqa: E402
from oracle import refload          # noqa: E402


def main(tmp):
    refload.load()
    import gsconverter.formats.sog as mod  # type: ignore
    n = int(os.environ.get("PROBE_N", 1_000_000))
    path = srn.build_file(os.path.join(tmp, "ref.sog"), n, 3, 65536, np.random.default_rng(5))
    runs = []
    for _ in range(3):
        t = time.perf_counter()
        with np.errstate(all="ignore"):
            mod.SogFormat().read(path)
        runs.append(round(time.perf_counter() - t, 3))
    print(json.dumps({"reference_SogFormat_read_s": runs, "n": n, "bands": 3, "palette": 65536, "texels": "random"}), flush=True)


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as tmp:
        main(tmp)
