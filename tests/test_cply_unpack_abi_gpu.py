"""-m gpu: gsx_cply_unpack_dev (csrc/cply_read.hip) called directly through ctypes -- padded sh rows (sh_stride > n_sh, which no
file has: it takes tile_rows down to 8), row counts on either side of 256 x n_chunks and none at all, and every argument check
with the text of its refusal.  The three element bodies are numpy structured arrays with explicit offsets and itemsize; the
expected rows are tests/cply_read_numpy.py's decode of the same arrays."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cply_read_numpy as crn  # noqa: E402

pytestmark = pytest.mark.gpu
WHO = "gsx_cply_unpack_dev"
GUARD = 64                      # bytes of 0xA5 behind the output rows: the kernel writes none of them


@pytest.fixture(scope="module")
def lib():
    mod = importlib.import_module("3dgsconverter_amd._lib")
    mod.require_hip()
    return mod


@pytest.fixture(scope="module")
def ctx(lib):
    c = lib.Context(0)
    yield c
    c.close()


def tables(n, n_chunks, sh_offsets, sh_stride, seed, chunk_stride=72, vertex_stride=16):
    """-> (chunk, vertex, sh or None): random bytes in every byte of every row, finite random bounds (min <= max); the chunk and
    vertex fields sit at the end of their rows when the strides are wider than 72 and 16"""
    rng = np.random.default_rng(seed)

    def table(rows, names, fmt, offsets, itemsize):
        a = np.zeros(rows, np.dtype({"names": names, "formats": [fmt] * len(names), "offsets": offsets, "itemsize": itemsize}))
        a.view(np.uint8)[:] = rng.integers(0, 256, a.nbytes, dtype=np.uint8)
        return a
    ch = table(n_chunks, crn.CHUNK_FIELDS, "<f4", [chunk_stride - 72 + 4 * i for i in range(18)], chunk_stride)
    for group in (0, 6, 12):
        for k in range(3):
            lo = (rng.standard_normal(n_chunks) * 5).astype(np.float32)
            ch[crn.CHUNK_FIELDS[group + k]] = lo
            ch[crn.CHUNK_FIELDS[group + 3 + k]] = lo + np.abs(rng.standard_normal(n_chunks) * 3).astype(np.float32)
    vt = table(n, crn.VERTEX_FIELDS, "<u4", [vertex_stride - 16 + 4 * i for i in range(4)], vertex_stride)
    sh = table(n, ["f_rest_%d" % i for i in range(len(sh_offsets))], "u1", list(sh_offsets), sh_stride) if len(sh_offsets) else None
    return ch, vt, sh


def layout_of(lib, ch, vt, sh):
    lay = lib.CplyReadLayout()
    lay.chunk_stride, lay.vertex_stride = ch.dtype.itemsize, vt.dtype.itemsize
    for i, f in enumerate(crn.CHUNK_FIELDS):
        lay.chunk_offset[i] = ch.dtype.fields[f][1]
    for i, f in enumerate(crn.VERTEX_FIELDS):
        lay.vertex_offset[i] = vt.dtype.fields[f][1]
    lay.n_sh = len(sh.dtype.names) if sh is not None else 0
    lay.sh_stride = sh.dtype.itemsize if sh is not None else 0
    for i in range(lay.n_sh):
        lay.sh_offset[i] = sh.dtype.fields[sh.dtype.names[i]][1]
    return lay


class Call:
    """the device side of one call: the bodies uploaded at 16-byte aligned addresses with 16 spare bytes behind each (as
    _lib.cply_unpack_table places them), the tables, and an output buffer of `out_rows` rows followed by GUARD bytes"""

    def __init__(self, lib, ctx, ch, vt, sh, out_rows):
        self.lib, self.ctx = lib, ctx
        self.row_words = 17 + (len(sh.dtype.names) if sh is not None else 0)
        self.bufs = {}
        for k, a in (("chunk", ch), ("vertex", vt), ("sh", sh)):
            if a is not None:
                host = np.zeros((a.nbytes + 16 + 15) & ~15, np.uint8)
                host[:a.nbytes] = a.view(np.uint8).reshape(-1)
                self.bufs[k] = ctx.alloc(max(host.nbytes, 16)).upload(host)
                assert self.bufs[k].ptr % 16 == 0
        self.bufs["tables"] = ctx.alloc(lib.cply_read_tables().nbytes).upload(lib.cply_read_tables())
        self.out_bytes = out_rows * self.row_words * 4
        self.bufs["out"] = ctx.alloc(self.out_bytes + GUARD).upload(np.full(self.out_bytes + GUARD, 0xA5, np.uint8))
        self.ptr = {k: b.ptr for k, b in self.bufs.items()}

    def run(self, lay, n_chunks, n_vertices, **ptr):
        """-> rc; `ptr` overrides a pointer (None = null)"""
        p = dict(self.ptr, **ptr)
        rc = self.ctx.lib.gsx_cply_unpack_dev(self.ctx.handle, p["chunk"], int(n_chunks), p["vertex"], int(n_vertices), p.get("sh"),
                                              C.byref(lay) if lay is not None else None, p["tables"], p["out"])
        self.ctx.synchronize()
        return rc

    def rows(self, count):
        """the first `count` output rows as words; the bytes behind them and the guard are still 0xA5"""
        raw = self.bufs["out"].download(np.uint8, self.out_bytes + GUARD)
        used = count * self.row_words * 4
        assert (raw[used:] == 0xA5).all(), "bytes written behind row %d" % count
        return raw[:used].view(np.uint32).reshape(count, self.row_words)

    def free(self):
        for b in self.bufs.values():
            b.free()


def expect(ch, vt, sh, n_dec):
    want, _ = crn.decode(ch, vt, sh)
    return np.ascontiguousarray(want[:n_dec]).view(np.uint32).reshape(n_dec, -1), want.dtype.names


def assert_words(what, got, want, names):
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%s: %d words differ, first at row %d field %s: 0x%08x != 0x%08x" % (
        what, len(bad), bad[0][0], names[bad[0][1]], got[tuple(bad[0])], want[tuple(bad[0])])


def scattered(n_sh, stride, seed):
    """n_sh distinct byte offsets over the whole row, the row's last byte among them, in no order"""
    rng = np.random.default_rng(seed)
    off = rng.choice(stride - 1, n_sh - 1, replace=False).tolist() + [stride - 1]
    return [int(o) for o in rng.permutation(off)]


# tile_rows from the code's formula: halve t from 256 while ((t * sh_stride + 30) // 16 * 16 + 16) + t * (17 + n_sh) * 4 > 65536:
#   (45, 64)     t = 256: 16 416 + 63 488 = 79 904;   t = 128:  8 224 + 31 744 = 39 968              -> 128
#   (45, 257)    t = 256: 65 824 + 63 488;            t = 128: 32 928 + 31 744 = 64 672              -> 128
#   (45, 400)    t = 128: 51 232 + 31 744 = 82 976;   t = 64:  25 632 + 15 872 = 41 504              -> 64
#   (9, 1000)    t = 64:  64 032 +  6 656 = 70 688;   t = 32:  32 032 +  3 328 = 35 360              -> 32
#   (9, 2000)    t = 32:  64 032 +  3 328 = 67 360;   t = 16:  32 032 +  1 664 = 33 696              -> 16
#   (256, 4096)  t = 16:  65 568 + 17 472;            t = 8:   32 800 +  8 736 = 41 536              -> 8
#   (1, 4096)    t = 16:  65 568 +  1 152;            t = 8:   32 800 +    576 = 33 376              -> 8
# (45, 257) still fits a 128-row tile by 864 bytes; (45, 400) and (9, 2000) are here for the 64- and 16-row tiles.
@pytest.mark.parametrize("n_sh,sh_stride", [(45, 64), (45, 257), (45, 400), (9, 1000), (9, 2000), (256, 4096), (1, 4096)])
def test_padded_sh_rows(lib, ctx, n_sh, sh_stride):
    n = 2 * 256 + 11
    ch, vt, sh = tables(n, 3, scattered(n_sh, sh_stride, 7 * sh_stride + n_sh), sh_stride, seed=sh_stride + n_sh)
    lay = layout_of(lib, ch, vt, sh)
    assert lay.sh_stride == sh_stride and lay.n_sh == n_sh and sh_stride - 1 in list(lay.sh_offset[:n_sh])
    call = Call(lib, ctx, ch, vt, sh, n)
    try:
        lib.check(call.run(lay, 3, n), WHO)
        want, names = expect(ch, vt, sh, n)
        assert_words("n_sh=%d stride %d" % (n_sh, sh_stride), call.rows(n), want, names)
    finally:
        call.free()


@pytest.mark.parametrize("n_vertices,n_chunks", [(700, 2), (300, 5), (512, 2), (513, 2), (1, 1)])
def test_row_counts_on_either_side_of_the_chunks(lib, ctx, n_vertices, n_chunks):
    """the first min(n_vertices, 256 n_chunks) rows are written and nothing behind them; chunk and vertex rows wider than
    their fields (strides 81 and 19)"""
    ch, vt, sh = tables(n_vertices, n_chunks, scattered(45, 45, 3), 45, seed=n_vertices, chunk_stride=81, vertex_stride=19)
    n_dec = min(n_vertices, 256 * n_chunks)
    call = Call(lib, ctx, ch, vt, sh, n_dec)
    try:
        lib.check(call.run(layout_of(lib, ch, vt, sh), n_chunks, n_vertices), WHO)
        want, names = expect(ch, vt, sh, n_dec)
        assert_words("%d vertices, %d chunks" % (n_vertices, n_chunks), call.rows(n_dec), want, names)
    finally:
        call.free()


@pytest.mark.parametrize("n_vertices,n_chunks", [(0, 3), (300, 0), (0, 0)])
def test_no_rows_launch_nothing_and_take_null_pointers(lib, ctx, n_vertices, n_chunks):
    ch, vt, sh = tables(300, 3, list(range(45)), 45, seed=1)
    lay = layout_of(lib, ch, vt, sh)
    call = Call(lib, ctx, ch, vt, sh, 4)
    try:
        assert call.run(lay, n_chunks, n_vertices) == 0
        assert call.run(lay, n_chunks, n_vertices, chunk=None, vertex=None, sh=None, tables=None, out=None) == 0
        assert len(call.rows(0)) == 0                                  # (the whole buffer is still 0xA5)
    finally:
        call.free()


def _good():
    return tables(300, 2, scattered(45, 45, 5), 45, seed=9)


def _set(**kw):
    def change(lay):
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(lay, k)[v[0]] = v[1]
            else:
                setattr(lay, k, v)
    return change


STRIDES = WHO + ": row strides chunk %d, vertex %d, sh %d"
ALIGN = WHO + ": output and sh rows must be 16-byte aligned, tables 8-byte aligned"
# (id, change to the layout or None, keyword arguments of Call.run, the refusal's text)
REFUSALS = [
    ("null_layout", None, dict(lay=None), WHO + ": null argument"),
    ("negative_chunks", None, dict(n_chunks=-1), WHO + ": bad row counts"),
    ("negative_vertices", None, dict(n_vertices=-1), WHO + ": bad row counts"),
    ("2_to_the_40_vertices", None, dict(n_vertices=1 << 40), WHO + ": bad row counts"),
    ("n_sh_minus_1", _set(n_sh=-1), {}, WHO + ": -1 sh properties (0 ... 256 are supported)"),
    ("n_sh_257", _set(n_sh=257), {}, WHO + ": 257 sh properties (0 ... 256 are supported)"),
    ("null_chunk_rows", None, dict(chunk=None), WHO + ": null argument"),
    ("null_sh_rows", None, dict(sh=None), WHO + ": null argument"),
    ("chunk_stride_71", _set(chunk_stride=71), {}, STRIDES % (71, 16, 45)),
    ("vertex_stride_15", _set(vertex_stride=15), {}, STRIDES % (72, 15, 45)),
    ("sh_stride_below_n_sh", _set(sh_stride=44), {}, STRIDES % (72, 16, 44)),
    ("sh_stride_4097", _set(sh_stride=4097), {}, STRIDES % (72, 16, 4097)),
    ("chunk_offset_negative", _set(chunk_offset=(17, -1)), {}, WHO + ": chunk field 17 at offset -1"),
    ("chunk_offset_past_the_stride", _set(chunk_offset=(3, 69)), {}, WHO + ": chunk field 3 at offset 69"),
    ("vertex_offset_negative", _set(vertex_offset=(0, -4)), {}, WHO + ": vertex field 0 at offset -4"),
    ("vertex_offset_past_the_stride", _set(vertex_offset=(2, 13)), {}, WHO + ": vertex field 2 at offset 13"),
    ("sh_offset_negative", _set(sh_offset=(7, -1)), {}, WHO + ": sh field 7 at offset -1"),
    ("sh_offset_at_the_stride", _set(sh_offset=(44, 45)), {}, WHO + ": sh field 44 at offset 45"),
    ("out_off_16", None, dict(out=+8), ALIGN),
    ("sh_off_16", None, dict(sh=+4), ALIGN),
    ("tables_off_8", None, dict(tables=+4), ALIGN),
]


@pytest.mark.parametrize("case", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_name_the_argument_and_leave_the_context_usable(lib, ctx, case):
    _, change, kw, message = case
    ch, vt, sh = _good()
    call = Call(lib, ctx, ch, vt, sh, 300)
    try:
        lay = layout_of(lib, ch, vt, sh)
        if change is not None:
            change(lay)
        args = dict(lay=lay, n_chunks=2, n_vertices=300)
        for k, v in kw.items():
            if k in args:
                args[k] = v
            else:
                args[k] = None if v is None else call.ptr[k] + v          # a pointer moved off its alignment
        with pytest.raises(lib.GsxError) as e:
            lib.check(call.run(**args), WHO)
        assert str(e.value) == WHO + " failed: " + message
        assert len(call.rows(0)) == 0                                  # nothing was written
        lib.check(call.run(layout_of(lib, ch, vt, sh), 2, 300), WHO)  # the context still works
        want, names = expect(ch, vt, sh, 300)
        assert_words("after " + case[0], call.rows(300), want, names)
    finally:
        call.free()


def test_fields_that_end_on_the_last_byte_of_their_rows_are_taken(lib, ctx):
    """the accepted side of the offset checks: offset + 4 == stride for chunk and vertex fields, offset == stride - 1 for sh"""
    ch, vt, sh = tables(300, 2, scattered(45, 64, 2), 64, seed=4, chunk_stride=75, vertex_stride=21)
    lay = layout_of(lib, ch, vt, sh)
    assert lay.chunk_offset[17] + 4 == 75 and lay.vertex_offset[3] + 4 == 21 and 63 in list(lay.sh_offset[:45])
    call = Call(lib, ctx, ch, vt, sh, 300)
    try:
        lib.check(call.run(lay, 2, 300), WHO)
        want, names = expect(ch, vt, sh, 300)
        assert_words("fields at the end of their rows", call.rows(300), want, names)
    finally:
        call.free()
