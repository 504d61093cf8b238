"""Shared by the -m gpu tests of the grid KNN (test_sor_gpu, test_brick_plan_gpu, test_knn_variants_gpu): one
gsx_sor_knn_dev call through the device entry point, and the bit-for-bit comparison of mean distances; test_tree_stages_gpu
runs the same call with algo = TREE."""
import numpy as np

BRUTE, GRID, TREE = 1, 2, 3


def differ(a, b):
    """mean distances that are not the same 32 bits"""
    return int(np.count_nonzero(a.view(np.uint32) != b.view(np.uint32)))


def explain(md_gpu, md_ref):
    bad = np.nonzero(md_gpu.view(np.uint32) != md_ref.view(np.uint32))[0]
    if len(bad) == 0:
        return "ok"
    with np.errstate(all="ignore"):
        rel = np.abs(md_gpu[bad].astype(np.float64) - md_ref[bad]) / np.abs(md_ref[bad])
    return "%d / %d mean_dists differ; first %s gpu=%s ref=%s max rel %.3g" % (
        len(bad), len(md_ref), bad[:8], md_gpu[bad[:8]], md_ref[bad[:8]], np.nanmax(rel))


def knn(lib, xyz, k, want_plan=False, ctx=None, window=None, columns=False, algo=GRID, **params):
    """one gsx_sor_knn_dev call with algo = GRID unless another is given (the grid path, adaptive mode off: nothing goes to the tree
    or to brute force) -> (mean distances, info, brick plan or None).  A fresh context unless `ctx` is given (which stays open, `params`
    are set on it); window = (q_begin, q_count): the queries are that index range only; columns: x, y and z as three separate
    arrays instead of interleaved rows"""
    n = len(xyz)
    q0, qc = window if window is not None else (0, n)
    own = ctx is None
    if own:
        ctx = lib.Context(0)
    for name, val in params.items():
        ctx.set_param(name, val)
    if columns:
        bufs = [ctx.alloc(4 * n).upload(np.ascontiguousarray(xyz[:, a])) for a in range(3)]
        px, py, pz, stride = bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, 1
    else:
        bufs = [ctx.alloc(xyz.nbytes).upload(np.ascontiguousarray(xyz))]
        px, py, pz, stride = bufs[0].ptr, bufs[0].ptr + 4, bufs[0].ptr + 8, 3
    out = ctx.alloc(4 * qc)
    info = ctx.sor_knn(px, py, pz, stride, n, q0, qc, k, out.ptr, algo=algo, want_info=True)
    got = out.download(np.float32, qc)
    plan = ctx.debug_brick_plan() if want_plan else None
    for b in bufs + [out]:
        b.free()
    if own:
        ctx.close()
    return got, info, plan
