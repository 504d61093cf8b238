"""Build box only: run the reference's own ``SplatFormat.write`` (gsconverter/formats/splat.py) on every .splat case and record
what it wrote -> tests/golden/splat_ref.npz.

Every case runs twice: as the reference stands, and with ``np.argsort`` made stable inside that module only (the one change;
equal metrics then keep input order, the order this project's writer defines).  Tie-free cases must give the same file both
ways and record the unpatched one; for a case with ties the two files must differ only by a permutation of records inside runs
of equal metric, and the stable one is recorded.

  spec         JSON: one recipe per case (tests/splat_numpy.py: case_table), with "ties" (bool: the metric has equal values),
               "bytes", and "error" = [exception type, message] for the cases the reference refuses (it then creates no file)
  <case>       the whole file -- or <case>__sha256, the file's sha256 (tables of 4096 rows)
  edges__table the explicit edge rows themselves

usage: python tests/devtools/make_golden_splat.py"""
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
import splat_numpy                   # noqa: E402

R = dict(kind="random")
CASES = {
    "d3_248": dict(R, n=4096, seed=1),
    "d3_251_rgb": dict(R, n=4096, seed=2, rgb=True),
    "minimal": dict(kind="minimal", n=4096, seed=3),
    "minimal_small": dict(kind="minimal", n=333, seed=4),
    "shuffled": dict(kind="shuffled", n=4096, seed=5),
    "shuffled_small": dict(kind="shuffled", n=301, seed=6),
    "rgb_u1": dict(kind="rgb", n=4096, seed=7),
    "rgb_u1_small": dict(kind="rgb", n=259, seed=8),
    "edges": dict(kind="edges"),
    "ties_all": dict(kind="ties", tie_kind="all", n=300, seed=9),
    "ties_quant": dict(kind="ties", tie_kind="quant", n=4096, seed=10),
    "ties_quant_small": dict(kind="ties", tie_kind="quant", n=517, seed=11),
    "ties_zeros_nans": dict(kind="ties", tie_kind="zeros_nans", n=613, seed=12),
}
for n in (0, 1, 2, 15, 17, 63, 64, 65, 127, 129, 255, 1000, 1023):
    CASES[f"n{n}"] = dict(R, n=n, seed=20 + n)
CASES["n65_251"] = dict(R, n=65, seed=19, rgb=True)
HASH_ONLY = {k for k, v in CASES.items() if v.get("n", 0) >= 4096}
MISSING = {"err_no_opacity": "opacity", "err_no_scale_2": "scale_2", "err_no_y": "y", "err_no_rot_3": "rot_3", "err_no_f_dc_1": "f_dc_1"}
MISSING_RGB = {"err_rgb_no_green": "green"}


class _StableNp:
    def __init__(self, np_mod):
        self._np = np_mod

    def __getattr__(self, name):
        return getattr(self._np, name)

    def argsort(self, a, *args, **kw):
        return self._np.argsort(a, kind="stable")


def _write(mod, t, path, stable):
    saved = mod.np
    try:
        if stable:
            mod.np = _StableNp(np)
        with np.errstate(all="ignore"):
            mod.SplatFormat().write(t, path)
    finally:
        mod.np = saved
    with open(path, "rb") as f:
        return f.read()


def main():
    refload.load()
    import gsconverter.formats.splat as mod
    out, spec = {}, {}
    cases = dict(CASES)
    for name, field in MISSING.items():
        cases[name] = dict(R, n=10, seed=31, drop=field)
    for name, field in MISSING_RGB.items():
        cases[name] = dict(kind="rgb", n=10, seed=32, drop=field)
    with tempfile.TemporaryDirectory() as tmp:
        for name, rec in cases.items():
            t = splat_numpy.case_table(rec)
            path = os.path.join(tmp, name + ".splat")
            rec = dict(rec)
            try:
                plain = _write(mod, t, path, False)
            except Exception as e:                   # noqa: BLE001  (the reference's own exception, recorded)
                rec["error"] = [type(e).__name__, str(e)]
                assert not os.path.exists(path), name
                spec[name] = rec
                print(name, type(e).__name__, e)
                continue
            stable = _write(mod, t, path, True)
            runs = splat_numpy.tie_runs(t)
            rec["ties"] = bool(len(runs) and runs[-1] + 1 < len(t))
            if not rec["ties"]:
                assert plain == stable, name
            assert splat_numpy.same_up_to_ties(plain, stable, t), name
            if name.startswith("ties_"):
                assert rec["ties"], name
            elif name != "edges":
                assert not rec["ties"], name             # the plain cases are tie-free: the unpatched reference's own file
            data = stable
            rec["bytes"] = len(data)
            if name in HASH_ONLY:
                out[name + "__sha256"] = np.frombuffer(hashlib.sha256(data).digest(), np.uint8)
            else:
                out[name] = np.frombuffer(data, np.uint8)
            spec[name] = rec
            print(name, "bytes", len(data), "ties" if rec["ties"] else "", "(unpatched order differs)" if plain != stable else "")
    out["edges__table"] = splat_numpy.edge_table()
    out["spec"] = np.frombuffer(json.dumps(spec, sort_keys=True).encode(), np.uint8)
    dst = os.path.join(ROOT, "tests", "golden", "splat_ref.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
