"""Build box only: run the reference's own ``SpzFormat.write`` (gsconverter/formats/spz.py) on every SPZ case and record what
it wrote -> tests/golden/spz_ref.npz.

  spec         JSON: one recipe per case (tests/spz_numpy.py: case_table), with "error" = the reference's ValueError message
               for the cases it refuses
  <case>       the decompressed payload (small cases) -- or <case>__sha256, the payload's sha256 (the 4096-row tables)
  edges__table the explicit edge rows themselves

usage: python tests/devtools/make_golden_spz.py"""
import gzip
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import refload          # noqa: E402
import spz_numpy                     # noqa: E402

CASES = {
    "d3_248": dict(kind="random", n=4096, seed=1),
    "d3_251_rgb": dict(kind="random", n=4096, seed=2, rgb=True),
    "no_opacity": dict(kind="random", n=1000, seed=3, opacity=False),
    "no_dc": dict(kind="random", n=1000, seed=4, dc=False),
    "low_degree": dict(kind="random", n=1000, seed=5, sh_upto=9),
    "content_degree2": dict(kind="random", n=1000, seed=11, sh_upto=24),
    "sh_zero": dict(kind="random", n=1000, seed=6, sh_scale=0.0),
    "c9_zero": dict(kind="random", n=500, seed=7, n_rest=9, sh_scale=0.0),
    "c24_zero": dict(kind="random", n=500, seed=8, n_rest=24, sh_scale=0.0),
    "c9_nonzero": dict(kind="random", n=500, seed=9, n_rest=9),
    "c24_nonzero": dict(kind="random", n=500, seed=10, n_rest=24),
    "c24_low": dict(kind="random", n=500, seed=14, n_rest=24, sh_upto=9),
    "n0": dict(kind="random", n=0, seed=0),
    "n1": dict(kind="random", n=1, seed=12),
    "n1000": dict(kind="random", n=1000, seed=13),
    "edges": dict(kind="edges"),
}
HASH_ONLY = {"d3_248", "d3_251_rgb"}


def main():
    refload.load()
    from gsconverter.formats.spz import SpzFormat
    out = {}
    spec = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, rec in CASES.items():
            table = spz_numpy.case_table(rec)
            path = os.path.join(tmp, name + ".spz")
            rec = dict(rec)
            try:
                with np.errstate(all="ignore"):
                    SpzFormat().write(table, path, compression_level=0)
            except ValueError as e:
                rec["error"] = str(e)
                assert not os.path.exists(path)
                spec[name] = rec
                print(name, "ValueError:", e)
                continue
            with open(path, "rb") as f:
                payload = gzip.decompress(f.read())
            rec["degree"] = payload[12]
            rec["bytes"] = len(payload)
            if name in HASH_ONLY:
                out[name + "__sha256"] = np.frombuffer(hashlib.sha256(payload).digest(), np.uint8)
            else:
                out[name] = np.frombuffer(payload, np.uint8)
            if name == "edges":
                out["edges__table"] = table
            spec[name] = rec
            print(name, "degree", rec["degree"], "bytes", len(payload))
    out["spec"] = np.frombuffer(json.dumps(spec, sort_keys=True).encode(), np.uint8)
    dst = os.path.join(ROOT, "tests", "golden", "spz_ref.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
