"""What tests/test_resident_rows_gpu.py and tests/test_resident_chain_gpu.py share, computed on the CPU: the shapes at which
csrc/resident_rows.hip's kernels take another path, packed dtypes of any stride, the index lists of the take kernel, f_dc values
whose colour byte numpy's own power decides, and small scenes the filters all remove rows from."""
import numpy as np

STRIDES = (12, 68, 71, 251, 256, 257, 512)        # rows of <= 256 bytes: tiles of 128 rows; above: 64
COUNTS = (1, 63, 64, 65, 127, 128, 129, 4097)     # around both tile sizes, and more than one workgroup
FIRST_BYTES = (0, 5, 15)
SH_C0 = 0.28209479177387814


def tile_rows(stride: int) -> int:
    """csrc/row_tile.h spz_tile_rows"""
    return 128 if stride <= 256 else 64


def take_tile_rows(stride_out: int) -> int:
    """csrc/resident_rows.hip take_tile_rows: output rows per workgroup of gsx_rows_take_dev"""
    return tile_rows(stride_out) // 4


def raw_rows(n: int, stride: int, rng) -> np.ndarray:
    """(n, stride) random bytes: NaNs of every payload, infinities, denormals and both zeros occur in any 4 of them"""
    return rng.integers(0, 256, (n, stride), dtype=np.uint8)


def field_view(raw: np.ndarray, offset: int) -> np.ndarray:
    """numpy's view of the '<u4' field at byte `offset` of every row of `raw` (n, stride)"""
    n, stride = raw.shape
    dt = np.dtype({"names": ["f"], "formats": ["<u4"], "offsets": [int(offset)], "itemsize": int(stride)})
    return np.ascontiguousarray(raw).reshape(-1).view(dt)["f"]


def column_offsets(stride: int, m: int):
    """m distinct field offsets inside a row: the row's last 4 bytes first, then unaligned ones, then byte 0"""
    cand = [stride - 4, 1, (stride // 2) | 1, 0, 3, 6]
    out = []
    for o in cand:
        if 0 <= o <= stride - 4 and o not in out:
            out.append(o)
    return out[:m]


def packed_dtype(stride: int, phase: int = 0) -> np.dtype:
    """a packed structured dtype of `stride` bytes without padding: `phase` u1 fields, as many '<f4' fields w0, w1, ... as fit
    behind them (every one at byte phase + 4 j: unaligned for phase 1 ... 3), u1 fields to the row's end"""
    words = (stride - phase) // 4
    fields = [("a%d" % i, "u1") for i in range(phase)] + [("w%d" % j, "<f4") for j in range(words)]
    fields += [("b%d" % i, "u1") for i in range(stride - phase - 4 * words)]
    dt = np.dtype(fields)
    assert dt.itemsize == stride
    return dt


def zero_names(dtype: np.dtype, count: int, rng):
    """`count` (or as many as the row has) of the dtype's '<f4' fields, in random order"""
    names = [nm for nm in dtype.names if nm.startswith("w")]
    rng.shuffle(names)
    return names[:count]


def index_lists(n: int, tr: int):
    """{name: ascending uint32 row indices, or None for the identity}: the lists of the issue's take cases for `n` source rows
    and output tiles of `tr` rows"""
    u = lambda a: np.unique(np.asarray([i for i in a if 0 <= i < n], dtype=np.int64)).astype(np.uint32)   # noqa: E731
    edges = list(range(0, 3)) + [i for t in (tr, 2 * tr) for i in range(t - 3, t + 3)] + list(range(3 * tr - 1, 3 * tr + tr + 2))
    edges += [i for t in (128, 256, 4096) for i in range(t - 2, t + 2)]
    out = {
        "identity": None,
        "empty": np.zeros(0, np.uint32),
        "every_other": np.arange(0, n, 2, dtype=np.uint32),
        "last_row": np.array([n - 1], np.uint32),
        "row_0": np.array([0], np.uint32),
        "runs_over_tile_edges": u(edges),
        "one_per_tile": np.arange(tr // 2, n, tr, dtype=np.uint32) if n > tr // 2 else np.array([n - 1], np.uint32),
        "all_but_one_run": u([i for i in range(n) if i != n // 2]),       # two runs: a tile with a gap takes the slot path
    }
    return out


def numpy_rgb(f_dc: np.ndarray) -> np.ndarray:
    """data_processor.py:316-343 on float32 values, elementwise"""
    with np.errstate(all="ignore"):
        lin = np.clip(0.5 + np.asarray(f_dc, np.float32) * SH_C0, 0.0, 1.0)
        return (np.power(lin, 1.0 / 2.2) * 255).astype(np.uint8)


def near_integer_f_dc(limit: int = 64) -> np.ndarray:
    """float32 f_dc values whose `pow(lin, 1/2.2) * 255`, evaluated in float64 on numpy's float32 `lin`, lies within 1e-6 of an
    integer: a float32 power rounds them to either side, so the device has to leave them to numpy.  Searched on the CPU among the
    +-4096 float32 neighbours of the exact preimage of every byte boundary."""
    e = float(np.float32(1.0 / 2.2))
    found = []
    for k in range(1, 255):
        v0 = np.float32(((k / 255.0) ** (1.0 / e) - 0.5) / SH_C0)
        bits = v0.view(np.uint32).astype(np.int64) + np.arange(-4096, 4097)
        v = bits.astype(np.uint32).view(np.float32)
        lin = np.clip(np.float32(0.5) + v * np.float32(SH_C0), np.float32(0.0), np.float32(1.0))
        t = np.power(lin.astype(np.float64), e) * 255.0
        hit = v[np.abs(t - np.rint(t)) < 1e-6]
        found.extend(hit[:2].tolist())
        if len(found) >= limit:
            break
    return np.array(found, np.float32)


def planted_f_dc() -> np.ndarray:
    """+-0, NaNs, +-inf, the values at and around both clip edges, and near_integer_f_dc()"""
    lo, hi = np.float32(-0.5 / SH_C0), np.float32(0.5 / SH_C0)
    around = lambda x: (x.view(np.uint32).astype(np.int64) + np.arange(-3, 4)).astype(np.uint32).view(np.float32)   # noqa: E731
    special = np.array([0.0, -0.0, np.nan, -np.nan, np.inf, -np.inf, 1.0, -1.0, 1e-30, -1e-30, 3e38, -3e38], np.float32)
    nan_payload = np.array([0x7fc00001, 0xffc12345, 0x7f800001], np.uint32).view(np.float32)
    return np.concatenate([special, nan_payload, around(lo), around(hi), near_integer_f_dc()])


def colour_table(rng, n_random: int = 3000) -> np.ndarray:
    """a packed table whose f_dc_* fields sit at unaligned offsets (a u1 field first), the planted values spread over the three
    channels and random ones behind them"""
    planted = planted_f_dc()
    n = -(-len(planted) // 3) + n_random
    dt = np.dtype([("tag", "u1"), ("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("f_dc_0", "<f4"), ("f_dc_1", "<f4"), ("f_dc_2", "<f4"),
                   ("opacity", "<f4")])
    t = np.zeros(n, dt)
    vals = (rng.standard_normal(3 * n) * 2.0).astype(np.float32)
    vals[:len(planted)] = planted
    for c in range(3):
        t["f_dc_%d" % c] = vals[c::3]
    for nm in ("x", "y", "z", "opacity"):
        t[nm] = rng.standard_normal(n).astype(np.float32)
    return t


SPLAT_FIELDS = (["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"] + ["f_rest_%d" % i for i in range(45)]
                + ["opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"])


def scene(n: int, rng, extra_fields=()) -> np.ndarray:
    """a splat table of 248-byte rows (+ extra_fields): two Gaussian clusters that hold most rows, a thin uniform haze the
    density filter removes and a few far flyers for SOR; opacities on both sides of any alpha threshold; every f_rest field set"""
    dt = np.dtype([(nm, "<f4") for nm in SPLAT_FIELDS] + list(extra_fields))
    t = np.zeros(n, dt)
    for nm in SPLAT_FIELDS:
        t[nm] = rng.standard_normal(n).astype(np.float32)
    n_haze, n_fly = n // 20, min(max(n // 200, 4), n // 2)
    pos = np.concatenate([rng.normal((0, 0, 0), 0.4, (n - n_haze - n_fly - (n - n_haze - n_fly) // 3, 3)),
                          rng.normal((2.5, 0.5, 0), 0.3, ((n - n_haze - n_fly) // 3, 3)),
                          rng.uniform(-9, 9, (n_haze, 3)), rng.uniform(-40, 40, (n_fly, 3))]).astype(np.float32)
    pos = pos[rng.permutation(n)]
    t["x"], t["y"], t["z"] = pos[:, 0], pos[:, 1], pos[:, 2]
    t["opacity"] = rng.uniform(-6, 6, n).astype(np.float32)
    return t
