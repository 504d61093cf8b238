"""Clouds with more than 1024 dense voxels for the device clustering tests (test_density_components_*.py), and what
oracle/density.py -- pinned to the reference -- makes of them.  Points are voxel centres, exact in float32."""
import functools

import numpy as np

from oracle import datasets, density as oden


def block(origin, shape):
    """a full lattice box of voxel keys"""
    g = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), -1).reshape(-1, 3)
    return g + np.asarray(origin, dtype=np.int64)


def snake(origin, w, rows):
    """`rows` full rows of `w` voxels at even y, joined by one connector voxel at odd y, at alternating ends"""
    ox, oy, oz = origin
    out = []
    for r in range(rows):
        out += [(ox + i, oy + 2 * r, oz) for i in range(w)]
        if r + 1 < rows:
            out.append((ox + (w - 1 if r % 2 == 0 else 0), oy + 2 * r + 1, oz))
    return np.array(out, dtype=np.int64)


def centres(keys, voxel, reps=1):
    return np.repeat(((keys + 0.5) * voxel).astype(np.float32), reps, axis=0)


def _snakes():
    return np.concatenate([snake((-30, -7, -3), 64, 32), snake((-30, -7, 0), 64, 31)])


def _bridge(voxel):
    return np.concatenate([centres(block((0, 0, 0), (12, 12, 12)), voxel, 3), centres(block((12, 5, 5), (6, 1, 1)), voxel, 1),
                           centres(block((18, 0, 0), (11, 11, 11)), voxel, 3)])


# name -> (cloud, voxel, threshold %, dense voxels, the largest cluster sizes, tie for the largest)
_CASES = {
    "snakes_v1": (lambda: centres(_snakes(), 1.0), 1.0, 0.0, 4093, [2079, 2014], False),
    "snakes_v0p5": (lambda: centres(_snakes(), 0.5), 0.5, 0.0, 4093, [2079, 2014], False),
    "five_percent": (lambda: centres(np.concatenate([block((0, 0, 0), (20, 10, 10)), block((30, 0, 0), (10, 10, 1)),
                                                     block((50, 0, 0), (11, 9, 1))]), 0.5), 0.5, 0.0, 2199, [2000, 100, 99], False),
    "layers_z": (lambda: centres(np.concatenate([block((0, 0, 4), (40, 40, 1)), block((0, 0, 0), (40, 39, 1))]), 1.0),
                 1.0, 0.0, 3160, [1600, 1560], False),
    "layers_x": (lambda: centres(np.concatenate([block((4, 0, 0), (1, 40, 40)), block((0, 0, 0), (1, 40, 39))]), 1.0),
                 1.0, 0.0, 3160, [1600, 1560], False),
    "small_frame": (lambda: centres(np.concatenate([block((0, 0, 0), (14, 14, 14)), block((15, 0, 0), (1, 14, 14))]), 0.25),
                    0.25, 0.0, 2940, [2744, 196], False),
    "wide": (lambda: centres(np.concatenate([block((-6, -6, -6), (13, 13, 13)), block((3000000,) * 3, (11, 11, 11)),
                                             snake((-3000000, 5, 5), 64, 20)]), 1.0), 1.0, 0.0, 4827, [2197, 1331, 1299], False),
    "bridge": (lambda: _bridge(1.0), 1.0, 0.03, 3059, [1728, 1331], False),
    "bridge_thr0": (lambda: _bridge(1.0), 1.0, 0.0, 3065, [3065], False),
    "tie": (lambda: centres(np.concatenate([block((0, 0, 0), (12, 12, 12)), block((40, 0, 0), (12, 12, 12))]), 1.0),
            1.0, 0.0, 3456, [1728, 1728], True),
    "crowd": (lambda: datasets.uniform(60000, 10.0, 3), 0.3, 0.001, 30231, [30188], False),
    "clustered": (lambda: datasets.make({"kind": "clustered", "n": 100000, "seed": 5}), 0.1, 0.002, 7595, [3059, 905, 213], False),
}
NAMES = list(_CASES)
# what the cases promise beyond the sizes: clusters in all, kept rows (single, multi), kept clusters with keep_multicluster
PROMISES = {"five_percent": {"rows": (2000, 2100), "multi_clusters": 2}, "bridge": {"rows": (5184, 9177), "min_points": 2, "unique": 3065},
            "crowd": {"clusters": 42, "multi_clusters": 1}, "clustered": {"clusters": 2549, "multi_clusters": 3, "min_points": 2}}


def promised(name):
    """-> (voxel, threshold %, dense voxels, largest cluster sizes, tie)"""
    return _CASES[name][1:]


@functools.lru_cache(maxsize=None)
def cloud(name):
    xyz = _CASES[name][0]()
    xyz.setflags(write=False)
    return xyz


@functools.lru_cache(maxsize=None)
def occupancy(name):
    """-> (min_points, unique keys, inverse, dense keys in np.unique's order): data_processor.py:38-52 by the oracle's own steps"""
    _, voxel, thr = _CASES[name][:3]
    keys = oden.voxel_keys(cloud(name), voxel)
    uniq, inverse, counts = np.unique(keys, axis=0, return_inverse=True, return_counts=True)
    min_points = oden.min_points_for(len(keys), thr)
    return min_points, uniq, np.asarray(inverse).reshape(-1), uniq[counts >= min_points]


@functools.lru_cache(maxsize=None)
def expected(name, multi):
    """the oracle's answer -> dict(mask, valid (set of kept voxel keys), kept_clusters, max_len, unique_voxels, min_points, messages)"""
    min_points, uniq, inverse, dense = occupancy(name)
    valid, kept, max_len = oden.cluster_dense_voxels(dense, multi)
    in_cluster = np.fromiter((tuple(k) in valid for k in uniq.tolist()), dtype=bool, count=len(uniq))
    mask = in_cluster[inverse]
    mask.setflags(write=False)
    return {"mask": mask, "valid": valid, "kept_clusters": kept, "max_len": max_len, "unique_voxels": len(uniq), "min_points": min_points,
            # the reference's format strings (data_processor.py:115-116)
            "messages": [f"Density Filter: Kept {kept} clusters (largest: {max_len} voxels).",
                         f"After density filter, retained {int(mask.sum())} out of {len(mask)} vertices."]}


def struct(xyz):
    arr = np.zeros(len(xyz), dtype=[("x", "f4"), ("y", "f4"), ("z", "f4"), ("orig", "i8")])
    arr["x"], arr["y"], arr["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    arr["orig"] = np.arange(len(xyz))
    return arr
