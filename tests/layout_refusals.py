"""The writer entry points' layout checks, called through ctypes with n = 0: a refusal returns before anything is launched, and an
accepted layout has no rows to work on.  Shared by test_spz_gpu.py, test_ksplat_gpu.py and test_splat_gpu.py."""
import ctypes as C

FIELDS = 59          # x y z | rot_0..3 | scale_0..2 | f_dc_0..2 | opacity | f_rest_0..44
ROW_BYTES = 4 * FIELDS
SCALE_2, F_DC, OPACITY, F_REST = 9, 10, 13, 14


def layout(lib, row_bytes=ROW_BYTES, **fields):
    """every field present at 4 * index, then `f<index>=offset` overrides (-1 = absent)"""
    lay = lib.SpzLayout()
    lay.row_bytes = row_bytes
    for f in range(FIELDS):
        lay.offset[f] = 4 * f
    for name, off in fields.items():
        lay.offset[int(name[1:])] = off
    return lay


def absent(*fields):
    return {"f%d" % f: -1 for f in fields}


def call(lib, entry, lay, *args):
    """-> (rc, last_error()) of `entry` on no rows; `args`: the entry point's own scalars (see ENTRY)"""
    ctx = lib.Context(0)
    cnt = ctx.alloc(64)
    try:
        h, p = ctx.handle, (C.byref(lay) if lay is not None else None)
        if entry == "gsx_spz_rest_nonzero_dev":      # args: fields
            word = C.c_uint64(0)
            rc = ctx.lib.gsx_spz_rest_nonzero_dev(h, None, p, 0, *args, C.byref(word))
        elif entry == "gsx_spz_pack_dev":            # args: sh_degree
            rc = ctx.lib.gsx_spz_pack_dev(h, None, p, 0, *args, None, None, 0, cnt.ptr)
        elif entry == "gsx_ksplat_centres_dev":      # args: none
            rc = ctx.lib.gsx_ksplat_centres_dev(h, None, p, 0, 1, None, None, 0, cnt.ptr)
        elif entry == "gsx_ksplat_pack_dev":         # args: sh_count
            rc = ctx.lib.gsx_ksplat_pack_dev(h, None, p, 0, 0, *args, 1, 1.0, None, None, 0, None, 0, cnt.ptr)
        elif entry == "gsx_splat_pack_dev":          # args: red, green, blue
            rc = ctx.lib.gsx_splat_pack_dev(h, None, p, *args, 0, None, None, None)
        else:
            raise KeyError(entry)
        return rc, lib.last_error()
    finally:
        cnt.free()
        ctx.close()


def common_cases(entry, args, first_required_absent):
    """the checks every entry point shares: (id, layout keywords or None, args, message or None = accepted)"""
    return [
        ("null", None, args, entry + ": null layout"),
        ("rows0", dict(row_bytes=0), args, entry + ": rows of 0 bytes (1 ... 512 are supported)"),
        ("rows513", dict(row_bytes=513), args, entry + ": rows of 513 bytes (1 ... 512 are supported)"),
        ("x_absent", absent(0), args, entry + ": field 0 is required"),
        ("last_required_absent", absent(first_required_absent), args, entry + ": field %d is required" % first_required_absent),
        ("field_over_the_end", dict(f0=ROW_BYTES - 3), args, entry + ": field 0 at byte offset 233 of a 236-byte row"),
        ("optional_field_over_the_end", dict(f58=ROW_BYTES - 3), args, entry + ": field 58 at byte offset 233 of a 236-byte row"),
        ("field_at_the_end", dict(f58=ROW_BYTES - 4), args, None),
    ]


def check(lib, entry, kw, args, message):
    lay = None if kw is None else layout(lib, **kw)
    rc, err = call(lib, entry, lay, *args)
    if message is None:
        assert rc == 0, err
    else:
        assert rc != 0
        assert err == message
