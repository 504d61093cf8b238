"""GPU: the compressed-PLY writer (csrc/cply.hip, _lib.cply_pack_table) where its packers change behaviour -- against the
reference's own output on the edge table (tests/golden/cply_edges_ref.npz) and, at other sizes, against the oracle that
tests/test_cply_edges_host.py certifies on that fixture.  Everything is compared bit for bit; chunk records as uint32."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

from oracle import cply as ocply

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cply_edge_cases as ec  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
SIZES = [1, 63, 64, 65, 255, 256, 257, 511, 512, 513]
NAMES14 = ("x", "y", "z", "scale_0", "scale_1", "scale_2", "f_dc_0", "f_dc_1", "f_dc_2", "opacity", "rot_0", "rot_1", "rot_2", "rot_3")
GUARD = 64


@pytest.fixture(scope="module")
def gold():
    return ec.gold()


@pytest.fixture(scope="module")
def table(gold):
    t = gold["edges__table"]
    t.setflags(write=False)
    return t


@pytest.fixture(scope="module")
def writer():
    return importlib.import_module("3dgsconverter_amd.formats.compressed_ply_writer")


@pytest.fixture(scope="module")
def ctx(gsx):
    c = gsx._lib.Context(0)
    yield c
    c.close()


def columns(t, alpha):
    """(14, n) float32 in the packer's column order; row 9 the opacity, or numpy's sigmoid of it (compressed_ply.py:200-203)"""
    m = np.empty((14, len(t)), dtype=F)
    for i, name in enumerate(NAMES14):
        m[i] = t[name]
    if alpha:
        with np.errstate(over="ignore"):
            m[9] = 1.0 / (1.0 + np.exp(-m[9]))
    return m


class Guarded:
    """a device buffer of `nbytes` with GUARD bytes of 0xAB behind it that a kernel must leave alone"""

    def __init__(self, ctx, nbytes):
        self.nbytes = nbytes
        self.buf = ctx.alloc(nbytes + GUARD).upload(np.full(nbytes + GUARD, 0xAB, np.uint8))
        self.ptr = self.buf.ptr

    def take(self, dtype):
        raw = self.buf.download(np.uint8, self.nbytes + GUARD)
        self.buf.free()
        assert (raw[self.nbytes:] == 0xAB).all(), "the kernel wrote behind its output"
        return raw[:self.nbytes].view(dtype)


def run_pack(gsx, ctx, cols, order, mode, cap=None):
    """one of the three pack entry points on (14, n) columns -> (chunks u32 (nc, 18), verts (n, 4), listed (k, 2) or None, count)
    mode: "pack" | ("strided", element stride) | "opacity" (row 9 is the opacity; list of `cap` entries)"""
    lib = gsx._lib
    hip = lib.require_hip()
    n = cols.shape[1]
    nc = (n + 255) // 256
    bufs = []
    try:
        if isinstance(mode, tuple):
            es = mode[1]
            step = es // 14
            host = np.full((n, es), 7.0, dtype=F)
            for i in range(14):
                host[:, i * step] = cols[i]
            d = ctx.alloc(host.nbytes).upload(host)
            ptrs = (C.c_void_p * 14)(*[d.ptr + 4 * i * step for i in range(14)])
            strides = (C.c_int64 * 14)(*([es] * 14))
        else:
            d = ctx.alloc(cols.nbytes).upload(cols)
            ptrs = (C.c_void_p * 14)(*[d.ptr + 4 * n * i for i in range(14)])
            strides = None
        bufs.append(d)
        d_order = None
        if order is not None:
            d_order = ctx.alloc(4 * n).upload(np.ascontiguousarray(order, dtype=np.uint32))
            bufs.append(d_order)
        optr = d_order.ptr if d_order else None
        g_chunk, g_vert = Guarded(ctx, 72 * nc), Guarded(ctx, 16 * n)
        listed, count = None, None
        if mode == "pack":
            lib.check(hip.gsx_cply_pack_dev(ctx.handle, ptrs, optr, n, g_chunk.ptr, g_vert.ptr), "gsx_cply_pack_dev")
        elif mode == "opacity":
            g_list = Guarded(ctx, 8 * cap)
            d_cnt = ctx.alloc(16).upload(np.full(4, 0xABABABAB, np.uint32))
            bufs.append(d_cnt)
            lib.check(hip.gsx_cply_pack_opacity_dev(ctx.handle, ptrs, None, optr, n, g_chunk.ptr, g_vert.ptr, g_list.ptr, cap, d_cnt.ptr),
                      "gsx_cply_pack_opacity_dev")
            cnt = d_cnt.download(np.uint32, 4)
            assert (cnt[1:] == 0xABABABAB).all()
            count = int(cnt[0])
            listed = g_list.take(np.uint32).reshape(cap, 2)[:min(count, cap)].copy()
        else:
            lib.check(hip.gsx_cply_pack_strided_dev(ctx.handle, ptrs, strides, optr, n, g_chunk.ptr, g_vert.ptr), "gsx_cply_pack_strided_dev")
        return g_chunk.take(np.uint32).reshape(nc, 18), g_vert.take(np.uint32).reshape(n, 4).copy(), listed, count
    finally:
        for b in bufs:
            b.free()


def patch_alpha(verts, listed):
    """cply_pack_table's host patch: numpy's own expression for the listed rows"""
    pos, x = listed[:, 0].astype(np.int64), listed[:, 1].copy().view(F)
    verts[pos, 3] = (verts[pos, 3] & np.uint32(0xffffff00)) | ec.numpy_alpha_byte(x)
    return verts


def oracle_pack(t, order):
    oc, ov, _ = ocply.encode(t, np.arange(len(t)) if order is None else order, [])
    return oc.view(np.uint32), ov


# ---------------------------------------------------------------- end to end
def test_edge_table_end_to_end_is_the_references(gsx, gold, table, writer):
    """writer.encode on the edge table, with the reference's own order and with the device's, on the resident path and on the host
    gather path (a caller's context: numpy's sigmoid): the fixture bit for bit, and the two paths equal each other"""
    lib = gsx._lib
    names = [str(s) for s in gold["edges/sh_names"]]
    n = len(table)
    for suffix, order in (("ref", gold["edges/order_ref"]), ("stable", None)):
        chunk, vertex, sh, got_order = writer.encode(table, order=order)
        assert list(sh.dtype.names) == names
        resident = (chunk.view(np.uint32).reshape(-1, 18), vertex.view(np.uint32).reshape(-1, 4), sh.view(np.uint8).reshape(n, -1), got_order)
        c = lib.Context(0)
        try:
            hc, hv, hs, ho, _ = lib.cply_pack_table(table, names, order, ctx=c)
        finally:
            c.close()
        gather = (hc.view(np.uint32), hv, hs, ho)
        for path, (pc, pv, ps, po) in (("resident", resident), ("gather", gather)):
            np.testing.assert_array_equal(po, gold["edges/order_" + suffix], err_msg=path)
            np.testing.assert_array_equal(pc, gold["edges/chunk_" + suffix], err_msg=path)
            np.testing.assert_array_equal(pv, gold["edges/vertex_" + suffix], err_msg=path)
            np.testing.assert_array_equal(ps, gold["edges/sh_" + suffix], err_msg=path)
        for u, v in zip(resident, gather):
            assert u.tobytes() == v.tobytes()
    lib.release_arenas()


# ---------------------------------------------------------------- pack kernels through the C ABI
@pytest.mark.parametrize("n", SIZES)
def test_pack_entry_points_on_the_head_of_the_edge_table(gsx, ctx, table, n):
    """gsx_cply_pack_dev, gsx_cply_pack_strided_dev (element strides 17 and 62) and gsx_cply_pack_opacity_dev on the first n rows,
    order NULL / identity / a fixed permutation, against oracle.cply.encode with the same order"""
    t = table[:n]
    alpha, opac = columns(t, True), columns(t, False)
    perm = np.random.default_rng(100 + n).permutation(n).astype(np.uint32)
    for oname, order in (("null", None), ("identity", np.arange(n, dtype=np.uint32)), ("permutation", perm)):
        want_c, want_v = oracle_pack(t, order)
        for mode in ("pack", ("strided", 17), ("strided", 62), "opacity"):
            got_c, got_v, listed, count = run_pack(gsx, ctx, opac if mode == "opacity" else alpha, order, mode, cap=n + 8)
            if mode == "opacity":
                assert count == len(listed) <= n
                sure = np.ones(n, bool)
                sure[listed[:, 0]] = False
                np.testing.assert_array_equal(got_v[sure], want_v[sure], err_msg="%s certified" % oname)
                src = np.arange(n) if order is None else order
                np.testing.assert_array_equal(listed[:, 1], t["opacity"][src][listed[:, 0]].view(np.uint32))
                np.testing.assert_array_equal(got_v[:, :3], want_v[:, :3])
                got_v = patch_alpha(got_v, listed)
            np.testing.assert_array_equal(got_c, want_c, err_msg="%s %s" % (oname, mode))
            np.testing.assert_array_equal(got_v, want_v, err_msg="%s %s" % (oname, mode))


def _record_index(col, is_max):
    return (col // 3) * 6 + (3 if is_max else 0) + col % 3


def _extreme(col, is_max):
    """a value outside the body of cply_scene's column (coordinates N(0, 3^2), scales N(-4, 1) -- inside the clip --, f_dc N(0, 1))"""
    return F(((50.0, 19.0, 30.0) if is_max else (-50.0, -19.5, -30.0))[col // 3])


def test_lone_extremes_reach_the_chunk_record(gsx, ctx):
    """the chunk-bound reduction (64-lane shuffles, four waves through LDS): for each of the nine bounded columns ONE row holds the
    maximum (minimum), in lane 0, 63, 64, 191 and 255 of a full chunk, and in the last live row of a 1-, 20- and 65-row chunk"""
    lanes = (0, 63, 64, 191, 255)
    plan = [(lane, col, is_max) for lane in lanes for col in range(9) for is_max in (True, False)]      # one chunk each
    t = ocply.cply_scene(256 * len(plan), 31)
    for ci, (lane, col, is_max) in enumerate(plan):
        t[NAMES14[col]][256 * ci + lane] = _extreme(col, is_max)
    got_c, got_v, _, _ = run_pack(gsx, ctx, columns(t, True), None, "pack")
    want_c, want_v = oracle_pack(t, None)
    for ci, (lane, col, is_max) in enumerate(plan):
        v = _extreme(col, is_max)
        want = ocply._colour(v) if col >= 6 else v
        assert got_c[ci, _record_index(col, is_max)] == np.asarray(want, dtype=F).view(np.uint32), (lane, col, is_max)
    np.testing.assert_array_equal(got_c, want_c)
    np.testing.assert_array_equal(got_v, want_v)
    for live in (1, 20, 65):
        for flip in (False, True):
            t = ocply.cply_scene(256 + live, 32 + live)
            for col in range(9):
                t[NAMES14[col]][-1] = _extreme(col, (col % 2 == 0) != flip)
            for mode in ("pack", ("strided", 17)):
                got_c, got_v, _, _ = run_pack(gsx, ctx, columns(t, True), None, mode)
                want_c, want_v = oracle_pack(t, None)
                for col in range(9):
                    is_max = (col % 2 == 0) != flip
                    want = ocply._colour(_extreme(col, is_max)) if col >= 6 else _extreme(col, is_max)
                    assert got_c[1, _record_index(col, is_max)] == np.asarray(want, dtype=F).view(np.uint32), (live, col, is_max)
                np.testing.assert_array_equal(got_c, want_c)
                np.testing.assert_array_equal(got_v, want_v)


# ---------------------------------------------------------------- SH bytes
def run_sh(gsx, ctx, vals, order, strided):
    """gsx_cply_sh_dev on contiguous columns (column stride n + 3) or gsx_cply_sh_strided_dev on rows (m consecutive fields at
    element 2 of rows of m + 5 floats) -> (n, m) bytes"""
    lib = gsx._lib
    hip = lib.require_hip()
    n, m = vals.shape
    bufs = []
    try:
        if strided:
            host = np.full((n, m + 5), 1e30, dtype=F)
            host[:, 2:2 + m] = vals
        else:
            host = np.full((m, n + 3), 1e30, dtype=F)
            host[:, :n] = vals.T
        d = ctx.alloc(host.nbytes).upload(host)
        bufs.append(d)
        optr = None
        if order is not None:
            d_order = ctx.alloc(4 * n).upload(np.ascontiguousarray(order, dtype=np.uint32))
            bufs.append(d_order)
            optr = d_order.ptr
        out = Guarded(ctx, n * m)
        if strided:
            lib.check(hip.gsx_cply_sh_strided_dev(ctx.handle, d.ptr + 8, m, 1, m + 5, optr, n, out.ptr), "gsx_cply_sh_strided_dev")
        else:
            lib.check(hip.gsx_cply_sh_dev(ctx.handle, d.ptr, m, n + 3, optr, n, out.ptr), "gsx_cply_sh_dev")
        return out.take(np.uint8).reshape(n, m)
    finally:
        for b in bufs:
            b.free()


@pytest.mark.parametrize("m", [1, 9, 24, 45])
def test_sh_bytes_at_every_step_and_at_saturation(gsx, ctx, m):
    """both SH entry points on the edge values (the start of every byte and the float32 below it, +-4, +-1e30, +-3e38, a denormal,
    -0.0) against numpy's expression; 66 and 258 rows join the sizes so that n * m % 4 takes 1, 2 and 3 (the byte tail behind the
    dword stores)"""
    edge = ocply.edge_sh_values()
    tails = set()
    for n in SIZES + [66, 258]:
        tails.add(((n - 1) % 256 + 1) * m % 4)
        idx = (np.arange(n)[:, None] * 3 + np.arange(m)[None, :] * 7 + n) % len(edge)
        vals = edge[idx]
        perm = np.random.default_rng(200 + n).permutation(n).astype(np.uint32)
        for order in (None, perm):
            want = ec.numpy_sh_bytes(vals if order is None else vals[order])
            for strided in (False, True):
                got = run_sh(gsx, ctx, vals, order, strided)
                np.testing.assert_array_equal(got, want, err_msg="n=%d m=%d strided=%s order=%s" % (n, m, strided, order is not None))
    assert tails == ({0} if m % 4 == 0 else {0, 1, 2, 3})


# ---------------------------------------------------------------- the alpha certificate
def test_alpha_certificate_on_the_device(gsx, ctx):
    """gsx_cply_pack_opacity_dev on the edge opacities and on N(0, 4^2), n = 100 000: a row that is not listed carries numpy's byte; a
    row at or beyond +-80 is listed; every entry's payload is its row's own bits; the random column lists at most n / 1000 rows
    (the numpy restatement lists 1 of 100 000: the cap leaves 100x for a device exp that is an ulp off glibc's, and still fails
    a certificate that lists everything); after the host patch the column is numpy's"""
    lib = gsx._lib
    for name, x in (("edges", ocply.edge_opacities()), ("random", ec.random_opacities())):
        n = len(x)
        t = ocply.cply_scene(n, 41)
        t["opacity"] = x
        got_c, got_v, listed, count = run_pack(gsx, ctx, columns(t, False), None, "opacity", cap=n)
        want = ec.numpy_alpha_byte(x)
        assert count == len(listed)
        assert len(set(listed[:, 0].tolist())) == count and (listed[:, 0] < n).all()
        sure = np.ones(n, bool)
        sure[listed[:, 0]] = False
        np.testing.assert_array_equal((got_v[:, 3] & 255)[sure], want[sure], err_msg=name)
        assert not sure[~(np.abs(x) < 80)].any(), name
        np.testing.assert_array_equal(listed[:, 1], x.view(np.uint32)[listed[:, 0]])
        _, cpu_sure = ec.alpha_code(x)
        print("alpha list, %s: device %d of %d rows (%.2e), numpy restatement %d (%.2e)" %
              (name, count, n, count / n, int((~cpu_sure).sum()), float((~cpu_sure).mean())))
        if name == "random":
            assert count <= n // 1000
        np.testing.assert_array_equal(patch_alpha(got_v, listed)[:, 3] & 255, want)
        want_c, want_v = oracle_pack(t, None)
        np.testing.assert_array_equal(got_v, want_v)
        np.testing.assert_array_equal(got_c, want_c)
    # ... and through cply_pack_table's own patch (resident rows)
    t = ocply.cply_scene(100_000, 42)
    t["opacity"] = ec.random_opacities()
    t["opacity"][:779] = ocply.edge_opacities()
    order = np.random.default_rng(5).permutation(len(t)).astype(np.uint32)
    _, verts, _, _, _ = lib.cply_pack_table(t, [], order)
    np.testing.assert_array_equal(verts[:, 3] & 255, ec.numpy_alpha_byte(t["opacity"][order]))
    lib.release_arenas()


def test_uncertain_list_overflow_takes_numpys_whole_column(gsx, ctx):
    """n = 8192: cply_pack_table's list holds n // 64 + 4096 = 4224 rows.  Opacity 90.0 (beyond the |x| < 80 cut: always listed) in
    exactly 4224 rows scattered over all chunks stays on the list path, in 4225 rows takes the whole-column numpy path; both equal
    the oracle, vertices' other three words included.  The rows in between carry 1.0, which the device certifies -- with 0.0 (the
    byte boundary 127 | 128: never certain) all 8192 rows are listed and both tables overflow; that table is checked too.
    Through the C ABI with the same capacity: the counter goes on to 4225, the list stops at 4224 entries."""
    lib = gsx._lib
    n, cap = 8192, 8192 // 64 + 4096
    names = ["f_rest_%d" % i for i in range(45)]
    assert ec.alpha_code(np.array([1.0], F))[1].all() and not ec.alpha_code(np.array([0.0, 90.0], F))[1].any()
    scattered = np.random.default_rng(7).permutation(n)
    for base, planted in ((1.0, cap), (1.0, cap + 1), (0.0, cap)):
        t = ocply.cply_scene(n, 43)
        rows = np.sort(scattered[:planted])
        assert len(set((rows // 256).tolist())) == n // 256
        t["opacity"] = F(base)
        t["opacity"][rows] = F(90.0)
        _, _, listed, count = run_pack(gsx, ctx, columns(t, False), None, "opacity", cap=cap)
        assert count == (planted if base else n) and len(listed) == min(count, cap)
        if base:
            assert set(listed[:, 0].tolist()) <= set(rows.tolist()) and len(set(listed[:, 0].tolist())) == len(listed)
        chunks, verts, sh, order, _ = lib.cply_pack_table(t, names)
        want_order, _ = ocply.morton_order(t["x"], t["y"], t["z"])
        oc, ov, osh = ocply.encode(t, want_order, names)
        np.testing.assert_array_equal(order, want_order)
        np.testing.assert_array_equal(verts, ov, err_msg="%r %d" % (base, planted))
        np.testing.assert_array_equal(chunks.view(np.uint32), oc.view(np.uint32))
        np.testing.assert_array_equal(sh, osh)
    lib.release_arenas()


# ---------------------------------------------------------------- Morton order
def test_morton_order_on_the_edge_clouds(gsx, gold):
    """the lattice k / 1024 (exact products, c == hi clipped to 1023), an extent of 3e38, a child box without extent on one axis, a
    coincident child inside a parent with extent, zeros of both signs: oracle.cply.morton_order, which on these clouds is the
    reference's own sort with stable ties (fixture)"""
    for name, (x, y, z) in ocply.edge_morton_clouds().items():
        want, depth = ocply.morton_order(x, y, z)
        np.testing.assert_array_equal(want, gold["clouds/" + name])
        got, levels = gsx._lib.morton_order(x, y, z)
        np.testing.assert_array_equal(got, want, err_msg=name)
        assert levels >= depth
