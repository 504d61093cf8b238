"""-m gpu: the context's work and staging buffers under regrowth and reuse.

Every operation below carves its device workspace out of buffers the context keeps and grows (csrc/gsx_common.h: work, work_sub,
work_leaf, and stage_in / stage_aux / stage_out of the process-wide context behind the host-pointer entry points).  One context
runs each operation at a small size, a larger one (the buffers are freed and re-allocated) and the small one again (the regions
now sit in a buffer larger than they need, with the larger run's bytes still in it); every result must equal, byte for byte, what
a context created for that one call returns.  For the host-pointer entry points the one context is the process's own, and the
fresh one runs the same device entry points on arrays of its own -- which also pins the staging against the direct path.
No tolerance anywhere: every comparison is equality of bytes."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(gsx):
    return gsx._lib


def _same(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, "%s: output %d is %s%s, expected %s%s" % (what, i, g.dtype, g.shape, w.dtype, w.shape)
        assert g.tobytes() == w.tobytes(), "%s: output %d differs" % (what, i)


def _sequence(lib, sizes, op, make):
    """op(ctx, *make(size)) on ONE context for every size in turn, against the same call on a context of its own"""
    fresh = {}
    shared = lib.Context(0)
    try:
        for step, size in enumerate(sizes):
            args = make(size)
            if size not in fresh:
                own = lib.Context(0)
                try:
                    fresh[size] = op(own, *args)
                finally:
                    own.close()
            _same(op(shared, *args), fresh[size], "step %d (size %s)" % (step, size))
    finally:
        shared.close()


def _upload(ctx, arr, slack=16):
    arr = np.ascontiguousarray(arr)
    return ctx.alloc(arr.nbytes + slack).upload(arr)


class _Own:
    """a context for one call: its arrays are freed and it is closed on the way out"""

    def __init__(self, lib):
        self.lib = lib

    def __enter__(self):
        self.ctx, self.bufs = self.lib.Context(0), []
        return self

    def alloc(self, nbytes):
        self.bufs.append(self.ctx.alloc(nbytes))
        return self.bufs[-1]

    def upload(self, arr):
        self.bufs.append(_upload(self.ctx, arr))
        return self.bufs[-1]

    def __exit__(self, *exc):
        for b in self.bufs:
            b.free()
        self.ctx.close()


def _cloud(n, seed=20251):
    """two well separated blobs, interleaved so that every prefix holds both"""
    rng = np.random.default_rng(seed)
    a = rng.normal(0.0, 0.35, (n, 3)) + np.where(np.arange(n)[:, None] % 2 == 0, -3.0, 3.0)
    return a.astype(np.float32)


CLOUD = _cloud(20000)


# ---------------------------------------------------------------- morton_order
def test_morton_order_regrows_and_shrinks(lib):
    rng = np.random.default_rng(7)
    pts = rng.standard_normal((4097, 3)).astype(np.float32)

    def op(ctx, x, y, z):
        order, levels = lib.morton_order(x, y, z, ctx=ctx)
        return order, np.int64(levels)

    _sequence(lib, (1, 65, 4097, 65), op, lambda n: (pts[:n, 0], pts[:n, 1], pts[:n, 2]))


# ---------------------------------------------------------------- batched Lloyd (D = 9, K = 64: the matrix-core path)
def _problems(rows, d=9, k=64, seed=11):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((k, d)).astype(np.float32)) for n in rows]


def _lloyd_batch(lib, ctx, problems, max_iter):
    """kmeans_lloyd_batch's steps, on a context of the caller's"""
    d, k = problems[0][0].shape[1], problems[0][1].shape[0]
    off = np.zeros(len(problems) + 1, dtype=np.int64)
    np.cumsum([len(p[0]) for p in problems], out=off[1:])
    n_total = int(off[-1])
    bufs = [_upload(ctx, np.concatenate([p[0] for p in problems])), _upload(ctx, np.concatenate([p[1] for p in problems])), ctx.alloc(4 * n_total + 16)]
    try:
        lib.check(ctx.lib.gsx_dev_memset(ctx.handle, bufs[2].ptr, 0, 4 * n_total), "gsx_dev_memset")
        lib.check(ctx.lib.gsx_kmeans_lloyd_batch_dev(ctx.handle, bufs[0].ptr, off.ctypes.data, len(problems), d, k, max_iter, bufs[1].ptr, bufs[2].ptr),
                  "gsx_kmeans_lloyd_batch_dev")
        return bufs[1].download(np.float32, len(problems) * k * d), bufs[2].download(np.int32, n_total)
    finally:
        for b in bufs:
            b.free()


def test_lloyd_batch_regrows_and_shrinks(lib):
    max_iter = 4
    small, large = _problems((200, 70, 1)), _problems((3000, 3000, 3000), seed=12)
    ctx = lib.Context(0)
    try:
        for step, problems in enumerate((small, large, small)):
            want = lib.kmeans_lloyd_many(problems, max_iter)   # (a context of its own per call; three problems of one shape: the batch)
            cent, labels = _lloyd_batch(lib, ctx, problems, max_iter)
            _same((cent, labels), (np.concatenate([w[0].reshape(-1) for w in want]), np.concatenate([w[1] for w in want])), "step %d" % step)
    finally:
        ctx.close()


# ---------------------------------------------------------------- density filter, voxel clusters
VOXEL, MIN_POINTS = 0.25, 3


def _info_fields(info):
    return np.array([getattr(info, name) for name, _ in info._fields_], dtype=np.int64)


def _density_filter(lib, ctx, xyz):
    n = len(xyz)
    rows, mask = _upload(ctx, xyz), ctx.alloc(n + 64)
    try:
        info = lib.DensityInfo()
        lib.check(ctx.lib.gsx_density_filter_dev(ctx.handle, rows.ptr, rows.ptr + 4, rows.ptr + 8, 3, n, VOXEL, MIN_POINTS, 1, None, mask.ptr, C.byref(info)),
                  "gsx_density_filter_dev")
        return mask.download(np.uint8, n), _info_fields(info)
    finally:
        rows.free()
        mask.free()


def _voxel_clusters(lib, ctx, keys):
    keep = np.zeros(len(keys), dtype=np.uint8)
    info = lib.DensityInfo()
    lib.check(ctx.lib.gsx_voxel_clusters_dev(ctx.handle, keys.ctypes.data, len(keys), 1, keep.ctypes.data, C.byref(info)), "gsx_voxel_clusters_dev")
    return keep, _info_fields(info)


def test_density_filter_regrows_and_shrinks(lib):
    _sequence(lib, (500, 20000, 500), lambda ctx, xyz: _density_filter(lib, ctx, xyz), lambda n: (CLOUD[:n],))


def test_voxel_clusters_regrow_and_shrink(lib):
    def keys_of(n):
        return (np.ascontiguousarray(np.unique(np.floor(CLOUD[:n] / np.float32(VOXEL)).astype(np.int64), axis=0)),)

    assert len(keys_of(500)[0]) < len(keys_of(20000)[0])
    _sequence(lib, (500, 20000, 500), lambda ctx, keys: _voxel_clusters(lib, ctx, keys), keys_of)


# ---------------------------------------------------------------- k-means++ seeding, the scalar codebook solver
def _kmeans_pp(lib, ctx, data, k, uniforms, trials):
    n, d = data.shape
    rows, cent = _upload(ctx, data), ctx.alloc(4 * k * d + 16)
    try:
        lib.check(ctx.lib.gsx_kmeans_pp_dev(ctx.handle, rows.ptr, n, d, k, uniforms.ctypes.data, trials, cent.ptr), "gsx_kmeans_pp_dev")
        return (cent.download(np.float32, k * d),)
    finally:
        rows.free()
        cent.free()


def _kmeans1d(lib, ctx, vals, k):
    n = len(vals)
    d_vals, cent, labels = _upload(ctx, vals), ctx.alloc(4 * k + 16), ctx.alloc(4 * n + 16)
    try:
        inertia = np.zeros(3, dtype=np.float64)
        lib.check(ctx.lib.gsx_kmeans1d_dev(ctx.handle, d_vals.ptr, n, k, 20, 3, cent.ptr, labels.ptr, inertia.ctypes.data), "gsx_kmeans1d_dev")
        return cent.download(np.float32, k), labels.download(np.int32, n), inertia
    finally:
        for b in (d_vals, cent, labels):
            b.free()


def test_kmeans_pp_regrows_and_shrinks(lib):
    k = 16
    trials = lib.kmeans_pp_trials(k)
    rng = np.random.default_rng(3)
    data = rng.standard_normal((5000, 9)).astype(np.float32)
    uniforms = rng.random(1 + (k - 1) * trials)
    _sequence(lib, (64, 5000, 64), lambda ctx, rows: _kmeans_pp(lib, ctx, rows, k, uniforms, trials), lambda n: (data[:n],))


def test_kmeans1d_regrows_and_shrinks(lib):
    vals = np.random.default_rng(4).standard_normal(5000).astype(np.float32)
    _sequence(lib, (64, 5000, 64), lambda ctx, v: _kmeans1d(lib, ctx, v, 16), lambda n: (vals[:n],))


# ---------------------------------------------------------------- the host-pointer entry points share three staging buffers
K_SOR, FACTOR = 8, 1.0


def _sor_direct(lib, xyz):
    n = len(xyz)
    with _Own(lib) as own:
        ctx = own.ctx
        ctx.set_param("adaptive", 1)   # as the process-wide context behind gsx_sor_filter
        rows, md, st, mask = own.upload(xyz), own.alloc(4 * n + 16), own.alloc(16), own.alloc(n + 16)
        ctx.sor_knn(rows.ptr, rows.ptr + 4, rows.ptr + 8, 3, n, 0, n, K_SOR, md.ptr)
        ctx.sor_stats(md.ptr, n, FACTOR, st.ptr)
        ctx.sor_mask(md.ptr, n, st.ptr + 8, mask.ptr)
        ctx.check()
        return mask.download(np.uint8, n), md.download(np.float32, n), st.download(np.float32, 3)


def _lexsort_direct(lib, cols):
    n = len(cols[0])
    with _Own(lib) as own:
        ctx = own.ctx
        d = [own.upload(c) for c in cols]
        perm = own.alloc(4 * n + 16)
        lib.check(ctx.lib.gsx_lexsort3_dev(ctx.handle, d[0].ptr, d[1].ptr, d[2].ptr, 1, n, perm.ptr), "gsx_lexsort3_dev")
        return (perm.download(np.uint32, n),)


def _rgb_direct(lib, v, cap):
    n = len(v)
    with _Own(lib) as own:
        ctx = own.ctx
        d_v, out, unc, lst, cnt = own.upload(v), own.alloc(n + 16), own.alloc(n + 16), own.alloc(4 * cap + 16), own.alloc(16)
        lib.check(ctx.lib.gsx_rgb_from_sh_dev(ctx.handle, d_v.ptr, n, out.ptr, unc.ptr), "gsx_rgb_from_sh_dev")
        flags = (out.download(np.uint8, n), unc.download(np.uint8, n))
        lib.check(ctx.lib.gsx_dev_memset(ctx.handle, cnt.ptr, 0, 16), "gsx_dev_memset")
        lib.check(ctx.lib.gsx_rgb_from_sh_list_dev(ctx.handle, d_v.ptr, n, out.ptr, lst.ptr, cap, cnt.ptr), "gsx_rgb_from_sh_list_dev")
        count = int(cnt.download(np.uint32, 1)[0])
        return flags, (out.download(np.uint8, n), np.int64(count), np.sort(lst.download(np.uint32, min(count, cap))))


def _rgb_staged(lib, v, cap):
    hip, n = lib.require_hip(), len(v)
    out, unc = np.empty(n, np.uint8), np.empty(n, np.uint8)
    lib.check(hip.gsx_rgb_from_sh(v.ctypes.data, n, out.ctypes.data, unc.ctypes.data), "gsx_rgb_from_sh")
    out2, lst, cnt = np.empty(n, np.uint8), np.empty(cap, np.uint32), C.c_int64(0)
    lib.check(hip.gsx_rgb_from_sh_list(v.ctypes.data, n, out2.ctypes.data, lst.ctypes.data, cap, C.byref(cnt)), "gsx_rgb_from_sh_list")
    return (out, unc), (out2, np.int64(cnt.value), np.sort(lst[:min(cnt.value, cap)]))


def test_host_entry_points_share_their_staging(lib):
    rng = np.random.default_rng(5)
    keys = np.round(rng.standard_normal((3, 5000)) * 4).astype(np.float32)   # (ties: the sort must be the stable lexsort)
    # colours around both clip edges and the rounding boundaries of the power: some elements land in the uncertain list
    f_dc = np.concatenate([rng.uniform(-2.0, 2.0, 4000), np.linspace(-1.7725, 1.7725, 1000)]).astype(np.float32)
    rng.shuffle(f_dc)
    want = {}
    for step, n in enumerate((300, 5000, 300)):
        xyz, cols, v, cap = CLOUD[:n], [np.ascontiguousarray(k[:n]) for k in keys], np.ascontiguousarray(f_dc[:n]), n   # (cap = n: the list never overflows, so its content is determined)
        if n not in want:
            want[n] = (_sor_direct(lib, xyz), _lexsort_direct(lib, cols), _rgb_direct(lib, v, cap))
        # interleaved: each call finds the staging buffers as another entry point left them
        sor = lib.sor_filter(xyz, K_SOR, FACTOR)
        flags, listed = _rgb_staged(lib, v, cap)
        perm = lib.lexsort3(*cols)
        sor_again = lib.sor_filter(xyz, K_SOR, FACTOR)
        what = "step %d (n = %d)" % (step, n)
        for r in (sor, sor_again):
            _same((r["mask"].view(np.uint8), r["mean_dists"], np.array([r["mean"], r["std"], r["threshold"]], np.float32)), want[n][0], what + ": sor_filter")
        _same((perm.astype(np.uint32),), want[n][1], what + ": lexsort3")
        _same(flags, want[n][2][0], what + ": rgb_from_sh")
        _same(listed, want[n][2][1], what + ": rgb_from_sh_list")
