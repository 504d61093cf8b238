"""A numpy restatement of the .splat file and the deterministic tables the splat tests run on.

The restatement is the checker where the reference is absent (the GPU box: tests/test_splat_gpu.py, and
tests/devtools/check_splat_large.py at 10M and 50M rows).  It states the format from its description -- n records of 32 bytes
(3 float32 position, 3 float32 exp(scale), r g b alpha bytes, 4 rotation bytes), no header, ordered by decreasing visibility
exp(scale_0 + scale_1 + scale_2) * sigmoid(opacity) with equal values in input order -- in numpy's float32 arithmetic with
numpy's own casts, and is itself checked against the reference's files in tests/golden/splat_ref.npz (tests/test_splat_host.py).
"""
from __future__ import annotations

import numpy as np

from spz_numpy import _near_byte_opacities, dtype_3dgs, random_table  # noqa: F401  (the same 3DGS tables)

F = np.float32
SH_C0 = F(0.28209479177387814)
RECORD = np.dtype([("pos", "<f4", (3,)), ("scale", "<f4", (3,)), ("color", "u1", (4,)), ("rot", "u1", (4,))])


# ------------------------------------------------------------------------------------------------------------ format
def _u8(v: np.ndarray) -> np.ndarray:
    with np.errstate(invalid="ignore"):
        return np.clip(v, F(0), F(255)).astype(np.uint8)


def metric(data: np.ndarray) -> np.ndarray:
    """float32 visibility: exp((s0 + s1) + s2) * (1 / (1 + exp(-opacity)))"""
    with np.errstate(all="ignore"):
        total = (data["scale_0"] + data["scale_1"]) + data["scale_2"]
        vis = F(1) / (F(1) + np.exp(-data["opacity"]))
        return np.exp(total) * vis


def order(data: np.ndarray) -> np.ndarray:
    """descending metric, ties (numpy's equality: -0 == +0, NaN == NaN, NaN last) in input order"""
    return np.argsort(-metric(data), kind="stable")


def records(data: np.ndarray) -> np.ndarray:
    """one record per row, in input order"""
    n = len(data)
    out = np.zeros(n, RECORD)
    with np.errstate(all="ignore"):
        out["pos"] = np.stack([data[a] for a in "xyz"], axis=1)
        out["scale"] = np.exp(np.stack([data[f"scale_{a}"] for a in range(3)], axis=1))
        if "f_dc_0" in data.dtype.names:
            for a in range(3):
                out["color"][:, a] = _u8((F(0.5) + SH_C0 * data[f"f_dc_{a}"]) * F(255))
        else:
            for a, c in enumerate(("red", "green", "blue")):
                out["color"][:, a] = data[c]
        out["color"][:, 3] = _u8((F(1) / (F(1) + np.exp(-data["opacity"]))) * F(255))
        q = [data[f"rot_{a}"].astype(F) for a in range(4)]
        length = np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
        for a in range(4):
            out["rot"][:, a] = _u8((q[a] / length) * F(128) + F(128))
    return out


def file_bytes(data: np.ndarray) -> bytes:
    return records(data)[order(data)].tobytes()


def tie_runs(data: np.ndarray) -> np.ndarray:
    """run id, along the sorted order, of every position: equal -metric (numpy's equality) share an id"""
    v = -metric(data)[order(data)]
    v = np.where(v == 0, F(0), v)                              # -0 -> +0
    same = (v[1:] == v[:-1]) | (np.isnan(v[1:]) & np.isnan(v[:-1]))
    return np.concatenate([[0], np.cumsum(~same)]) if len(v) else np.zeros(0, np.int64)


def same_up_to_ties(a: bytes, b: bytes, data: np.ndarray) -> bool:
    """are two files the same records, differing only by a permutation inside runs of equal metric?"""
    if len(a) != len(b) or len(a) != 32 * len(data):
        return False
    runs = tie_runs(data)
    ka, kb = (np.frombuffer(x, "<u8").reshape(-1, 4) for x in (a, b))

    def canon(k):
        return k[np.lexsort((k[:, 3], k[:, 2], k[:, 1], k[:, 0], runs))]
    return np.array_equal(canon(ka), canon(kb))


# ------------------------------------------------------------------------------------------------------------ tables
READ_F4 = ["x", "y", "z", "scale_0", "scale_1", "scale_2", "opacity", "rot_0", "rot_1", "rot_2", "rot_3", "f_dc_0", "f_dc_1", "f_dc_2"]


def minimal_table(n: int, seed: int) -> np.ndarray:
    """only the fields the writer reads"""
    base = random_table(n, seed)
    t = np.zeros(n, [(f, "<f4") for f in READ_F4])
    for f in READ_F4:
        t[f] = base[f]
    return t


def shuffled_table(n: int, seed: int) -> np.ndarray:
    """the read fields in a shuffled order at odd byte offsets, between padding fields"""
    base = random_table(n, seed)
    names = list(READ_F4) + ["nx", "f_rest_0"]
    np.random.default_rng(seed).shuffle(names)
    t = np.zeros(n, [("tag", "u1")] + [(f, "<f4") for f in names] + [("tail", "u2")])
    for f in names:
        t[f] = base[f]
    t["tag"] = np.arange(n) % 251
    return t


def rgb_table(n: int, seed: int) -> np.ndarray:
    """no f_dc fields: the colour comes from u1 red / green / blue, at odd byte offsets"""
    base = random_table(n, seed, rgb=True)
    names = [f for f in READ_F4 if not f.startswith("f_dc_")]
    t = np.zeros(n, [("x", "<f4"), ("red", "u1")] + [(f, "<f4") for f in names[1:5]] + [("green", "u1"), ("blue", "u1")]
                 + [(f, "<f4") for f in names[5:]])
    for f in t.dtype.names:
        t[f] = base[f]
    return t


EXP_HARD = np.array([0xC2781E37], np.uint32).view(np.float32)[0]   # a worst case of numpy's exp


def edge_table() -> np.ndarray:
    """387 rows (not a multiple of 16): a random base with every edge the writer meets, at scattered positions -- NaN / +-inf in
    every field read, zero / huge / tiny quaternions, scale sums past exp's range both ways, metric NaN from inf * 0, -0.0,
    subnormals, alpha and colour bytes near their rounding boundaries"""
    n = 387
    t = random_table(n, 99)
    rng = np.random.default_rng(7)
    spots = iter(rng.permutation(n).tolist())

    def put(**kv):
        i = next(spots)
        for k, v in kv.items():
            t[k][i] = v
        return i
    specials = [np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-45, -1e-45, 1e-40, 3.4e38, -3.4e38, EXP_HARD]
    for f in READ_F4:
        for v in specials:
            put(**{f: v})
    for q in ([0, 0, 0, 0], [-0.0, 0, 0, 0], [1e30, 1e30, 0, 0], [1e20, -1e20, 1e20, 1e20], [1e-30, 0, 0, 0], [1e-25, -1e-25, 0, 0],
              [1e-45, 0, 0, 0], [np.inf, 1, 0, 0], [np.inf, np.inf, 0, 0], [1, 1, 1, 1], [-1, 0, 0, 0], [0.5, -0.5, 0.5, -0.5],
              [np.nan, 0, 0, 0]):
        put(**{f"rot_{a}": q[a] for a in range(4)})
    for s in ([50, 50, 50], [30, 30, 28.8], [-50, -50, -50], [-40, -40, -24], [88.7, 0, 0], [-104, 0, 0], [200, -200, 0],
              [np.inf, -np.inf, 0], [1e38, 1e38, 1e38]):
        put(scale_0=s[0], scale_1=s[1], scale_2=s[2])
    put(scale_0=60.0, scale_1=60.0, scale_2=0.0, opacity=-200.0)     # exp(sum) = inf, sigmoid = 0: metric NaN
    put(scale_0=np.inf, opacity=-np.inf)
    put(scale_0=-60.0, scale_1=-60.0, scale_2=0.0, opacity=5.0)      # metric +0
    put(scale_0=-60.0, scale_1=-60.0, scale_2=0.0, opacity=-200.0)   # +0 * 0
    put(opacity=-120.0)                                               # sigmoid underflows
    for o in _near_byte_opacities()[::11]:
        put(opacity=o)
    for k in range(0, 256, 9):                                        # colour bytes at their boundaries
        v = np.float32((k / 255.0 - 0.5) / 0.28209479177387814)
        put(f_dc_0=v, f_dc_1=np.nextafter(v, F(np.inf)), f_dc_2=np.nextafter(v, F(-np.inf)))
    # the last rows: NaN metric (sorted last, into the partial block of every cast) with NaN colour and rotation too
    for i, (dc, rot) in enumerate((("f_dc_0", "rot_2"), ("f_dc_1", "rot_0"), ("f_dc_2", "rot_3"))):
        t["opacity"][n - 1 - i] = np.nan
        t[dc][n - 1 - i] = np.nan
        t[rot][n - 1 - i] = np.nan
    return t


def ties_table(n: int, seed: int, kind: str) -> np.ndarray:
    """tables whose metric ties often: "all" (every row the same metric), "quant" (scales and opacity from small sets, as
    decoded from quantised formats), "zeros_nans" (many metrics +0 or NaN)"""
    t = random_table(n, seed)
    rng = np.random.default_rng(seed + 1)
    if kind == "all":
        for f in ("scale_0", "scale_1", "scale_2"):
            t[f] = F(-3.25)
        t["opacity"] = F(0.75)
    elif kind == "quant":
        for f in ("scale_0", "scale_1", "scale_2"):
            t[f] = np.log(rng.integers(1, 6, n).astype(F) / F(64))
        t["opacity"] = rng.choice(np.array([-2.0, 0.0, 1.5, 4.0], F), n)
    elif kind == "zeros_nans":
        pick = rng.integers(0, 4, n)
        t["scale_0"][pick == 0] = F(-200)                              # exp underflows: metric +0
        t["opacity"][pick == 1] = np.nan                               # NaN metric
        t["scale_1"][pick == 2] = np.inf
        t["opacity"][pick == 2] = F(-200)                              # inf * 0
    else:
        raise ValueError(kind)
    return t


def case_table(spec: dict) -> np.ndarray:
    kind = spec["kind"]
    if kind == "random":
        t = random_table(spec["n"], spec["seed"], rgb=spec.get("rgb", False))
    elif kind == "minimal":
        t = minimal_table(spec["n"], spec["seed"])
    elif kind == "shuffled":
        t = shuffled_table(spec["n"], spec["seed"])
    elif kind == "rgb":
        t = rgb_table(spec["n"], spec["seed"])
    elif kind == "edges":
        t = edge_table()
    elif kind == "ties":
        t = ties_table(spec["n"], spec["seed"], spec["tie_kind"])
    else:
        raise ValueError(kind)
    drop = spec.get("drop")
    if drop:
        import numpy.lib.recfunctions as rfn
        t = rfn.drop_fields(t, drop, usemask=False)
    return t
