"""Generate tests/golden/row_filters_ref.json from the REFERENCE's own DataProcessor (needs the reference checkout; run
here, the fixture travels).  Random sequences of crop_by_bbox / apply_alpha_filter / cap_sh_degree / apply_auto_bbox (the
methods of the eager drop-in class that need no device) on random tables -- bounds as Python floats, ints, numpy float32 /
float64 scalars, coordinates with NaN and +-inf, thresholds at both ends.  For every case: the dtype and sha256 of the
table the reference's class ends with, and the lines it printed.

    python -m oracle.make_golden_rows
"""
from __future__ import annotations

import contextlib
import hashlib
import io
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "row_filters_ref.json")
N_CASES = 40
LOG_PREFIXES = ("Auto-BBox", "Alpha Filter", "After cropping")


def table(n, with_rgb=False, seed=0):
    """a 3DGS vertex table of random finite float32 columns (+ 8-bit colours: 251-byte rows, nothing aligned)"""
    names = ["x", "y", "z", "nx", "ny", "nz"] + ["f_dc_%d" % i for i in range(3)] + ["f_rest_%d" % i for i in range(45)] \
        + ["opacity"] + ["scale_%d" % i for i in range(3)] + ["rot_%d" % i for i in range(4)]
    fields = [(nm, "<f4") for nm in names]
    if with_rgb:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    dt = np.dtype(fields)
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 255, size=(n, dt.itemsize), dtype=np.uint8)
    raw[:, 3::4] &= 0x3F  # keep the float fields finite (exponent < 255)
    return raw.reshape(-1).view(dt)


def cases():
    """-> [(case, table, [(method, args), ...])], the same on every run"""
    rng = np.random.default_rng(77)
    out = []
    for case in range(N_CASES):
        n = int(rng.integers(4096, 60000))
        t = table(n, bool(case % 3 == 0), seed=case)
        for a in "xyz":
            t[a] = (rng.standard_normal(n) * 3).astype(np.float32)
        t["opacity"] = (rng.standard_normal(n) * 3).astype(np.float32)
        if case % 4 == 0:
            t["x"][rng.integers(0, n, 5)] = np.nan
            t["y"][rng.integers(0, n, 5)] = np.inf
            t["opacity"][rng.integers(0, n, 5)] = np.nan
        steps = []
        for _ in range(int(rng.integers(1, 5))):
            kind = int(rng.integers(0, 4))
            if kind == 0:
                lo, hi = sorted(rng.uniform(-6, 6, 2))
                cast = [float, lambda v: int(round(v)), np.float32, np.float64][int(rng.integers(0, 4))]
                steps.append(("crop_by_bbox", tuple(cast(v) for v in (lo, lo - 1, lo, hi, hi + 1, hi))))
            elif kind == 1:
                steps.append(("apply_alpha_filter", (int(rng.choice([0, 1, 17, 128, 200, 254, 255])),)))
            elif kind == 2:
                steps.append(("cap_sh_degree", (int(rng.integers(0, 4)),)))
            else:
                steps.append(("apply_auto_bbox", ()))
        out.append((case, t, steps))
    return out


def run(cls, t, steps):
    """-> {"dtype", "sha256", "log"} of the table `cls` ends with after `steps`"""
    p = cls(t.copy())
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), np.errstate(all="ignore"):
        for name, args in steps:
            getattr(p, name)(*args)
    data = p.data
    return {"dtype": str(data.dtype.descr), "sha256": hashlib.sha256(data.tobytes()).hexdigest(),
            "log": [line for line in buf.getvalue().splitlines() if line.startswith(LOG_PREFIXES)]}


def main():
    from . import refload
    RefDP, _, _ = refload.load()
    out = {"_meta": {"generator": "oracle/make_golden_rows.py run against the reference (v0.8)", "cases": N_CASES}}
    for case, t, steps in cases():
        out[str(case)] = dict(run(RefDP, t, steps), steps=repr(steps))
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", GOLDEN)


if __name__ == "__main__":
    main()
