"""Generate tests/golden/cply_edges_ref.npz from the REFERENCE's compressed-PLY writer (needs the reference checkout; the
fixture travels).  The table is ``oracle.cply.cply_edge_scene()``: a value wherever a packer changes behaviour (its docstring
lists them).  As oracle/make_golden_cply.py: the splat order and the three elements the reference's own
``CompressedPlyFormat.write`` produced, and the same with ``np.argsort`` made stable; here the sh bytes are stored as they are,
and the TABLE ITSELF (``edges__table``), so that nothing which replays the fixture needs the reference or this generator.
For the clouds of ``oracle.cply.edge_morton_clouds()`` the order of the reference's ``_sort_morton_order`` with stable ties.

The reference runs with every numpy warning raised as an error except ``over`` (3e38 * 256, exp(104) and the squared 3e38 of
a quaternion overflow on purpose): an ``invalid`` would mean a NaN reached an integer cast, whose result depends on numpy's
build, and such a row has no place in a bit-for-bit fixture.  No planted row had to leave the table for that.

    python -m oracle.make_golden_cply_edges
"""
from __future__ import annotations

import os
import warnings

import numpy as np

from . import cply, refload

PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "cply_edges_ref.npz")


def reference_runs(table):
    """-> (own, stable): refload.reference_cply with invalid / divide / under raised as errors"""
    with warnings.catch_warnings(), np.errstate(over="ignore", invalid="raise", divide="raise", under="ignore"):
        warnings.simplefilter("error")
        return refload.reference_cply(table), refload.reference_cply(table, stable_ties=True)


def cloud_order(x, y, z):
    """the reference's ``_sort_morton_order`` on a cloud, ties stable (the rest of the table is ``cply_scene``'s)"""
    d = cply.cply_scene(len(x), 5)
    d["x"], d["y"], d["z"] = x, y, z
    with warnings.catch_warnings(), np.errstate(over="ignore", invalid="raise", divide="raise"):
        warnings.simplefilter("error")
        return refload.reference_cply(d, stable_ties=True)["order"]


def build():
    table = cply.cply_edge_scene()
    own, stable = reference_runs(table)
    out = {"edges__table": table}
    for suffix, run in (("ref", own), ("stable", stable)):
        out["edges/order_" + suffix] = run["order"]
        out["edges/chunk_" + suffix] = run["chunk"].view(np.float32).reshape(-1, 18).view(np.uint32)
        out["edges/vertex_" + suffix] = run["vertex"].view(np.uint32).reshape(-1, 4)
        out["edges/sh_" + suffix] = run["sh"].view(np.uint8).reshape(len(table), -1)
    out["edges/sh_names"] = np.array(list(own["sh"].dtype.names))
    for name, (x, y, z) in cply.edge_morton_clouds().items():
        out["clouds/" + name] = cloud_order(x, y, z)
    out["clouds"] = np.array(list(cply.edge_morton_clouds()))
    return out


def main():
    out = build()
    np.savez_compressed(PATH, **out)
    print("wrote", PATH, os.path.getsize(PATH), "bytes; ties differ:", not np.array_equal(out["edges/order_ref"], out["edges/order_stable"]))


if __name__ == "__main__":
    main()
