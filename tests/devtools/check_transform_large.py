"""Run by hand on the GPU box: the scene transform of CHECK_N rows of 248 bytes (default 10M) on the device against the numpy
definition (tests/transform_numpy.py), in slices of a million rows -- bit for bit, a NaN of the definition with any payload.
The table is a random block of a million rows repeated, the edge rows of tests/transform_cases.py at the start of every
repetition (with coordinates of their own behind the first).
    python tests/devtools/check_transform_large.py"""
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import transform_cases as tc  # noqa: E402
import transform_numpy as tn  # noqa: E402

SLICE = 1_000_000


def main():
    n = int(os.environ.get("CHECK_N", 10_000_000))
    lib = importlib.import_module("3dgsconverter_amd._lib")
    tf = importlib.import_module("3dgsconverter_amd.transform")
    lib.require_hip()
    dt = tc.splat_dtype(248)
    rng = np.random.default_rng(99)
    block = tc.random_rows(dt, min(n, SLICE), rng)
    edges = tc.edge_rows(dt)
    block[:min(len(edges), len(block))] = edges[:len(block)]
    table = np.tile(block, (n + len(block) - 1) // len(block))[:n].copy()
    if n > len(edges):                                              # (coordinates of their own behind the first edge rows)
        for a in ("x", "y", "z"):
            table[a][len(edges):] = rng.standard_normal(n - len(edges), dtype=np.float32) * 3
    floats = tc.float_fields(dt)
    failures = 0
    for kind, (R, s, t) in tc.transforms().items():
        t0 = time.perf_counter()
        got = lib.rows_transform_table(table, tf.plan_transform(dt, R, s, t))
        t_dev = time.perf_counter() - t0
        t0 = time.perf_counter()
        for lo in range(0, n, SLICE):
            diff = tn.same_by_class(got[lo:lo + SLICE], tn.transform_table(table[lo:lo + SLICE], R, s, t), floats)
            if diff:
                failures += 1
                print("DIFFERENT", kind, "slice at", lo, diff, flush=True)
                break
        print("%s: %d rows, device path %.2f s, definition and comparison %.1f s" % (kind, n, t_dev, time.perf_counter() - t0), flush=True)
    print("check_transform_large:", "FAILED" if failures else "ok")
    return 1 if failures else 0


if __name__ == "__main__":
    sys.exit(main())
