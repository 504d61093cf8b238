"""CPU restatement of the compressed-PLY writer's numeric core -- TEST INFRASTRUCTURE (checker only; nothing under
3dgsconverter_amd/ imports it).

Follows /root/reference/gsconverter/formats/compressed_ply.py:
    morton_order      :245-291   (np.argsort made STABLE: the reference's default sort leaves equal codes in a
                                  build-dependent order; everything else is the reference's arithmetic)
    encode            :193-241   chunk loop
    pack_11_10_11     :293-302
    pack_8888         :304-313
    pack_quaternions  :315-341
PINNED: tests/golden/cply_ref.npz holds what the reference's own ``CompressedPlyFormat.write`` produced
(oracle/make_golden_cply.py, run against /root/reference with only ``_write_ply_file`` intercepted), and its own
``_sort_morton_order`` run with a stable argsort; tests/test_cply_oracle.py checks this restatement against both.
tests/golden/cply_edges_ref.npz (oracle/make_golden_cply_edges.py) holds the same for ``cply_edge_scene()``, the table with a
value wherever a packer changes behaviour, and for ``edge_morton_clouds()``; tests/test_cply_edges_host.py checks that.
"""
from __future__ import annotations

import numpy as np

CHUNK = 256
SH_C0 = 0.28209479177387814


def _part_1_by_2(n):
    n = n & 0x000003ff
    n = (n ^ (n << 16)) & 0xff0000ff
    n = (n ^ (n << 8)) & 0x0300f00f
    n = (n ^ (n << 4)) & 0x030c30c3
    n = (n ^ (n << 2)) & 0x09249249
    return n


def morton_codes(cx, cy, cz):
    """:259-276 for one group; None when the group has no extent"""
    mx, Mx = cx.min(), cx.max()
    my, My = cy.min(), cy.max()
    mz, Mz = cz.min(), cz.max()
    xlen, ylen, zlen = Mx - mx, My - my, Mz - mz
    if xlen == 0 and ylen == 0 and zlen == 0:
        return None
    xmul = 1024.0 / xlen if xlen > 0 else 0
    ymul = 1024.0 / ylen if ylen > 0 else 0
    zmul = 1024.0 / zlen if zlen > 0 else 0
    ix = np.clip((cx - mx) * xmul, 0, 1023).astype(np.uint32)
    iy = np.clip((cy - my) * ymul, 0, 1023).astype(np.uint32)
    iz = np.clip((cz - mz) * zmul, 0, 1023).astype(np.uint32)
    return (_part_1_by_2(iz) << 2) | (_part_1_by_2(iy) << 1) | _part_1_by_2(ix)


def morton_order(x, y, z):
    """-> (uint32 order, recursion depth).  Iterative form of the reference's recursion, stable inside equal codes."""
    x, y, z = (np.ascontiguousarray(v, dtype=np.float32) for v in (x, y, z))
    idx = np.arange(len(x), dtype=np.uint32)
    work = [(0, len(idx), 1)]
    depth = 0
    while work:
        lo, hi, lvl = work.pop()
        if hi - lo <= 1:
            continue
        ids = idx[lo:hi]
        codes = morton_codes(x[ids], y[ids], z[ids])
        if codes is None:
            continue
        depth = max(depth, lvl)
        order = np.argsort(codes, kind="stable")
        idx[lo:hi] = ids[order]
        sc = codes[order]
        diff = np.where(sc[1:] != sc[:-1])[0] + 1
        starts = np.insert(diff, 0, 0)
        ends = np.append(diff, hi - lo)
        for s, e in zip(starts, ends):
            if e - s > CHUNK:
                work.append((lo + s, lo + e, lvl + 1))
    return idx, depth


def _normalize(v, v_min, v_max, t):
    if v_max - v_min < 1e-5:
        return np.zeros_like(v, dtype=np.uint32)
    norm = (v - v_min) / (v_max - v_min)
    return np.clip(np.floor(norm * t + 0.5), 0, t).astype(np.uint32)


def pack_11_10_11(x, y, z, mins, maxs):
    return (_normalize(x, mins[0], maxs[0], 2047) << 21) | (_normalize(y, mins[1], maxs[1], 1023) << 11) | _normalize(z, mins[2], maxs[2], 2047)


def pack_8888(r, g, b, a, mins, maxs):
    na = np.clip(np.floor(a * 255 + 0.5), 0, 255).astype(np.uint32)
    return (_normalize(r, mins[0], maxs[0], 255) << 24) | (_normalize(g, mins[1], maxs[1], 255) << 16) | \
           (_normalize(b, mins[2], maxs[2], 255) << 8) | na


def pack_quaternions(r0, r1, r2, r3):
    quats = np.stack([r0, r1, r2, r3], axis=-1)
    norm = np.linalg.norm(quats, axis=-1, keepdims=True)
    quats /= (norm + 1e-10)
    largest = np.argmax(np.abs(quats), axis=-1)
    signs = np.sign(quats[np.arange(len(quats)), largest])
    quats *= signs[:, None]
    res = largest.astype(np.uint32)
    for i in range(4):
        pc = np.clip(np.floor((quats[:, i] * 0.7071067811865476 + 0.5) * 1023 + 0.5), 0, 1023).astype(np.uint32)
        res = np.where(largest != i, (res << 10) | pc, res)
    return res


def encode(data, order, sh_names):
    """:193-241 -> (chunks (nc, 18) f32, vertices (n, 4) u32, sh (n, m) u8 or None)"""
    sd = data[order]
    n = len(sd)
    nc = (n + CHUNK - 1) // CHUNK
    chunks = np.zeros((nc, 18), dtype=np.float32)
    verts = np.zeros((n, 4), dtype=np.uint32)
    sh = np.zeros((n, len(sh_names)), dtype=np.uint8) if sh_names else None
    r = sd["f_dc_0"] * SH_C0 + 0.5
    g = sd["f_dc_1"] * SH_C0 + 0.5
    b = sd["f_dc_2"] * SH_C0 + 0.5
    with np.errstate(over="ignore"):
        opacity = 1.0 / (1.0 + np.exp(-sd["opacity"]))
    for i in range(nc):
        s, e = i * CHUNK, min((i + 1) * CHUNK, n)
        c = sd[s:e]
        pos = [c["x"], c["y"], c["z"]]
        sc = [np.clip(c["scale_%d" % a], -20, 20) for a in range(3)]
        col = [r[s:e], g[s:e], b[s:e]]
        mins = [[v.min() for v in grp] for grp in (pos, sc, col)]
        maxs = [[v.max() for v in grp] for grp in (pos, sc, col)]
        chunks[i] = [*mins[0], *maxs[0], *mins[1], *maxs[1], *mins[2], *maxs[2]]
        verts[s:e, 0] = pack_11_10_11(*pos, mins[0], maxs[0])
        with np.errstate(over="ignore"):     # (a squared 3e38 in a quaternion's norm: inf, and every component 0)
            verts[s:e, 1] = pack_quaternions(c["rot_0"], c["rot_1"], c["rot_2"], c["rot_3"])
        verts[s:e, 2] = pack_11_10_11(*sc, mins[1], maxs[1])
        verts[s:e, 3] = pack_8888(*col, opacity[s:e], mins[2], maxs[2])
        for j, name in enumerate(sh_names):
            with np.errstate(over="ignore"):     # (3e38 * 256: inf, then clipped)
                sh[s:e, j] = np.clip((c[name] / 8.0 + 0.5) * 256, 0, 255).astype(np.uint8)
    return chunks, verts, sh


def cply_scene(n, seed, kind="plain"):
    """inputs of the fixtures: oracle.datasets.sog_scene plus the geometry that exercises the recursion"""
    from . import datasets
    a = datasets.sog_scene(n, seed)
    rng = np.random.default_rng(seed + 1000)
    if kind == "clustered":
        # a tight clump (> 256 splats inside one level-0 Morton cell), a block of coincident points, and a flat sheet
        m = n // 4
        for ax in "xyz":
            a[ax][:m] = (np.float32(1.25) + rng.standard_normal(m).astype(np.float32) * np.float32(2e-4))
            a[ax][:m // 2] = (np.float32(1.25) + rng.standard_normal(m // 2).astype(np.float32) * np.float32(1.2e-7))   # third level
        a["x"][m:m + 400], a["y"][m:m + 400], a["z"][m:m + 400] = np.float32(-2.0), np.float32(0.5), np.float32(3.0)
        a["z"][m + 400:m + 900] = np.float32(0.75)
        p = rng.permutation(n)
        a = a[p]
    elif kind == "degree1":
        for i in range(9, 45):
            a["f_rest_%d" % i] = 0
    elif kind == "flat_scale":
        a["scale_1"] = np.float32(-3.0)          # range < 1e-5 -> zero field
        a["f_dc_2"] = np.float32(0.25)
    return a


# ---------------------------------------------------------------- the edge table (tests/golden/cply_edges_ref.npz)
EDGE_SEED = 77
EDGE_LANES = (0, 63, 64, 255)          # first / last lane of the first wave, first lane of the second, last lane of the chunk
EDGE_ROTATIONS = (
    (0, 0, 0, 0), (-0.0, 0, 0, 0),                                                   # no direction at all: sign 0, four codes of 512
    (1e-20, 0, 0, 0), (1e-30, -1e-30, 1e-30, 1e-30), (1e-10, 0, 0, 0),               # squares that are denormal / underflow; norm == the 1e-10 guard
    (1e20, 0, 0, 0), (3e38, 3e38, 0, 0),                                             # the norm overflows: every component becomes 0
    (.5, .5, .5, .5), (-.5, .5, .5, .5), (.5, -.5, .5, -.5), (0, 1, -1, 0),          # ties in argmax, some with a negative winner
    (0, 0, 0, -1),                                                                   # negative largest component, the last one
)
EDGE_SCALES_HI = (20.0, float(np.nextafter(np.float32(20), np.float32(np.inf))), np.inf, 3e38)
EDGE_SCALES_LO = (-20.0, float(np.nextafter(np.float32(-20), np.float32(-np.inf))), -np.inf, -3e38)


def edge_opacities():
    """float32: the out-of-range and zero cases first, then the 255 boundaries of the alpha byte (floor(a * 255 + 0.5) steps at
    a = (j + 0.5) / 255), each with its two float32 neighbours"""
    f = np.float32
    aa = (np.arange(255, dtype=np.float64) + 0.5) / 255.0
    mid = np.log(aa / (1 - aa)).astype(f)
    tail = np.array([0.0, -0.0, 79.99999, 80.0, np.nextafter(f(80), f(np.inf)), -79.99999, -80.0, np.nextafter(f(-80), f(-np.inf)),
                     88.8, -88.8, 104.0, -104.0, np.inf, -np.inf], dtype=f)
    return np.concatenate([tail, np.column_stack([np.nextafter(mid, f(-np.inf)), mid, np.nextafter(mid, f(np.inf))]).ravel()])


def edge_sh_values():
    """float32: the value at which every SH byte j begins, 8 * (j / 256 - 0.5), with the float32 below it; saturation, a denormal,
    a negative zero"""
    f = np.float32
    steps = (8.0 * (np.arange(256, dtype=np.float64) / 256.0 - 0.5)).astype(f)
    return np.concatenate([np.column_stack([np.nextafter(steps, f(-np.inf)), steps]).ravel(),
                           np.array([4.0, -4.0, 1e30, -1e30, 3e38, -3e38, 1e-40, -0.0], dtype=f)])


def _colour(fdc):
    return np.asarray(fdc, dtype=np.float32) * SH_C0 + 0.5           # :195-198, float32


def _fdc_pair(near, steps, quantum):
    """two f_dc values around `near` whose linearised colours differ by exactly steps * quantum (float32), first the lower"""
    f = np.float32
    want = f(steps * quantum)
    for d in range(64):
        lo = (np.array([near], dtype=f).view(np.int32) + np.int32(d)).view(f)[0]
        c = _colour(lo)
        target = f(c + want)
        if f(target - c) != want:
            continue
        guess = np.full(33, (np.float64(target) - 0.5) / SH_C0, dtype=f)
        guess = (guess.view(np.int32) + np.arange(-16, 17, dtype=np.int32)).view(f)
        hit = guess[_colour(guess) == target]
        if len(hit):
            return lo, hit[0]
    raise AssertionError("no f_dc pair for %r steps of %r near %r" % (steps, quantum, near))


def cply_edge_scene(seed=EDGE_SEED, with_layout=False):
    """``cply_scene(1300, seed)`` (five full chunks and one of 20 rows) with a value planted wherever a packer of the writer changes
    behaviour.  The rows are laid out IN Morton order (the table's stable Morton order is the identity), so chunk c of the written
    file is rows 256 c ... of the table and a value planted in lane l of chunk c sits there both with ``order = None`` and end to
    end.  No NaN anywhere, no column of a chunk whose minimum or maximum is a zero of both signs.

    coordinates  chunk 0 is the lattice k / 1024 (k = 0 ... 1024 per axis, the corners 0 and 1 among them) inside a parent box
                 of exactly [0, 4]^3: the products (c - lo) * mul are exact, every fourth lattice value sits ON a cell boundary
                 and c == hi is clipped to 1023.  The last two rows (lanes 18 and 19 of the 20-row chunk) are at
                 -+1.5e38: an extent of 3e38, still finite, and everything else inside one level-0 cell.
    scales       chunks 0, 1, 4 and scale_2 of chunk 3: one lone maximum of EDGE_SCALES_HI and one lone minimum of EDGE_SCALES_LO per
                 column, walking over EDGE_LANES (ten columns: every lane and every value on each side, 10 of the 16 pairs --
                 the four values of a side clip to the same +-20, so the value tests the clip of its own row and the lane the
                 reduction, which tests/test_cply_edges_gpu.py also walks lane by lane); chunk 2: ranges of exactly float32(1e-5), one ulp below, one ulp above;
                 chunk 3: scale_0 constant, scale_1 a single ulp wide at -3; chunk 5: its last row carries the extremes.
    f_dc         +-3e38 as lone extremes over EDGE_LANES (chunks 0, 1, 2, 4, and the last row of chunk 5), 0 and -0.0 (their
                 colour is +0.5 both); chunk 3: colour ranges of 335 / 2^25 (below 1e-5) and 336 / 2^25 and 168 / 2^24 (above) --
                 float32(1e-5) itself is not a difference of two colours, whose grid is 2^-25 at best.
    rotations    EDGE_ROTATIONS, every fifth row.
    opacity      edge_opacities() from row 0 on.
    f_rest       edge_sh_values() down every column, shifted by seven rows from one column to the next, rows 0 ... 519."""
    f = np.float32
    n = 1300
    a = cply_scene(n, seed)
    rng = np.random.default_rng(seed + 2000)
    # ---- coordinates first: they decide the order
    big, bigger = f(1.5e38), f(1.5e38) * f(1.0009765625)      # asymmetric: the centre falls into cell 511, below both far points
    lat = rng.integers(0, 1025, (256, 3))
    lat[0], lat[1], lat[2] = (0, 0, 0), (1024, 1024, 1024), (1024, 0, 512)
    xyz = np.empty((n, 3), dtype=f)
    xyz[:256] = lat.astype(f) / f(1024)
    xyz[256:, :2] = rng.random((n - 256, 2), dtype=f) * f(4)
    xyz[256:, 2] = f(2) + rng.random(n - 256, dtype=f) * f(2)
    xyz[256] = (4, 4, 4)
    xyz[-2] = (-big, bigger, -big)
    xyz[-1] = (bigger, -big, bigger)
    a["x"], a["y"], a["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    order, _ = morton_order(a["x"], a["y"], a["z"])
    a = a[order]
    again, _ = morton_order(a["x"], a["y"], a["z"])
    assert np.array_equal(again, np.arange(n)), "the edge table is not in its own Morton order"
    assert np.all(a["z"][:256] <= 1) and np.all(a["z"][256:1298] >= 2) and abs(a["x"][1298]) > 1e38 and abs(a["x"][1299]) > 1e38
    lay = {"lattice_chunk": 0, "far_rows": (1298, 1299), "scale_slots": [], "fdc_slots": []}

    def rows(c):
        return slice(256 * c, min(256 * c + 256, n))

    # ---- scales: lone extremes, walking over the lanes
    t = 0
    for c, cols in ((0, (0, 1, 2)), (1, (0, 1, 2)), (3, (2,)), (4, (0, 1, 2))):
        for k in cols:
            lane_hi, lane_lo = EDGE_LANES[t % 4], EDGE_LANES[(t + 2) % 4]
            v_hi, v_lo = EDGE_SCALES_HI[(t + t // 4) % 4], EDGE_SCALES_LO[(t + t // 4 + 1) % 4]
            a["scale_%d" % k][256 * c + lane_hi] = v_hi
            a["scale_%d" % k][256 * c + lane_lo] = v_lo
            lay["scale_slots"].append((c, k, lane_hi, v_hi, lane_lo, v_lo))
            t += 1
    # chunk 2: ranges at the 1e-5 switch (lo is +0.0 everywhere: no zero of the other sign in the column)
    e = f(1e-5)
    for k, hi in enumerate((e, np.nextafter(e, f(0)), np.nextafter(e, f(1)))):
        col = np.zeros(256, dtype=f)
        col[EDGE_LANES[k]] = hi
        col[100:140] = hi * rng.random(40, dtype=f)
        col[140 + k] = hi
        a["scale_%d" % k][rows(2)] = col
    lay["scale_threshold"] = {"chunk": 2, "at": 0, "below": 1, "above": 2}
    # chunk 3: a constant column, a column one ulp wide
    a["scale_0"][rows(3)] = f(-5.5)
    col = np.full(256, -3.0, dtype=f)
    col[[0, 63, 200]] = np.nextafter(f(-3), f(0))
    a["scale_1"][rows(3)] = col
    # ---- f_dc: lone extremes; zeros of both signs
    t = 0
    for c in (0, 1, 2, 4):
        for k in range(3):
            if (c + k) % 2 == 0:
                lane_hi, lane_lo = EDGE_LANES[t % 4], EDGE_LANES[(t + 1) % 4]
                a["f_dc_%d" % k][256 * c + lane_hi] = f(3e38)
                a["f_dc_%d" % k][256 * c + lane_lo] = f(-3e38)
                lay["fdc_slots"].append((c, k, lane_hi, lane_lo))
                t += 1
        a["f_dc_1"][256 * c + 1], a["f_dc_1"][256 * c + 2] = f(0.0), f(-0.0)
        a["f_dc_2"][256 * c + 65], a["f_dc_2"][256 * c + 66] = f(-0.0), f(0.0)
    # chunk 3: colour ranges at the 1e-5 switch
    near0 = f(-0.5 / SH_C0)
    for k, (near, steps, q) in enumerate(((near0, 335, 2.0 ** -25), (near0, 336, 2.0 ** -25), (f(1e-4), 168, 2.0 ** -24))):
        lo, hi = _fdc_pair(near, steps, q)
        col = np.full(256, lo, dtype=f)
        col[EDGE_LANES[(k + 1) % 4]] = hi
        mids = (lo + (hi - lo) * rng.random(30, dtype=f)).astype(f)
        cm = _colour(mids)
        col[10:40] = np.where((cm >= _colour(lo)) & (cm <= _colour(hi)), mids, lo)
        a["f_dc_%d" % k][rows(3)] = col
    lay["fdc_threshold"] = {"chunk": 3, "below": 0, "above": (1, 2)}
    # ---- the 20-row chunk: its last live row carries the extremes
    a["scale_0"][-1], a["scale_1"][-1], a["scale_2"][-1] = f(np.inf), f(-np.inf), f(3e38)
    a["scale_0"][-20], a["scale_2"][-20] = f(-3e38), EDGE_SCALES_LO[1]
    a["f_dc_0"][-1], a["f_dc_1"][-1], a["f_dc_2"][-20] = f(3e38), f(-3e38), f(3e38)
    # ---- row-local values
    for i in range(0, n, 5):
        q = EDGE_ROTATIONS[(i // 5) % len(EDGE_ROTATIONS)]
        for k in range(4):
            a["rot_%d" % k][i] = q[k]
    op = edge_opacities()
    a["opacity"][:len(op)] = op
    a["opacity"][-1], a["opacity"][-2], a["opacity"][255 + 256 * 3], a["opacity"][64 + 256 * 4] = f(np.inf), f(-np.inf), f(-104), f(80)
    sh = edge_sh_values()
    for k in range(45):
        a["f_rest_%d" % k][:len(sh)] = np.roll(sh, -7 * k)
    return (a, lay) if with_layout else a


def edge_morton_clouds():
    """name -> (x, y, z) float32: the clouds on which the Morton sort is checked at its edges (each <= 5000 rows)"""
    f = np.float32
    rng = np.random.default_rng(EDGE_SEED + 1)
    out = {}
    # every axis on the lattice k / 1024 over an extent of exactly 1: (c - lo) * mul is the integer k, c == hi is clipped to 1023
    k = rng.integers(0, 1025, (4000, 3))
    k[0], k[1] = (0, 0, 0), (1024, 1024, 1024)
    k[2:302] = (517, 3, 1024)                              # > 256 coincident points on the clipped boundary
    lat = k.astype(f) / f(1024)
    out["lattice"] = tuple(np.ascontiguousarray(lat[:, i]) for i in range(3))
    # an extent of 3e38: 1024 / len is tiny but normal, everything else in one level-0 cell and sorted on the next level
    far = (rng.standard_normal((3000, 3)) * 3.0).astype(f)
    far[0], far[1], far[2] = (-1.5e38,) * 3, (1.5e38,) * 3, (0, 0, 0)
    far[1500] = (1.5e38, -1.5e38, 0)
    out["far"] = tuple(np.ascontiguousarray(far[:, i]) for i in range(3))
    # > 256 points in one level-0 cell whose own box has no extent on exactly one axis
    flat = (rng.random((3000, 3), dtype=f) * f(100)).astype(f)
    flat[:700] = f(40.0) + rng.random((700, 3), dtype=f) * f(0.05)
    flat[:700, 1] = f(40.03125)
    out["flat_child"] = tuple(np.ascontiguousarray(flat[:, i]) for i in range(3))
    # > 256 coincident points (and a second, smaller pile) inside a parent group that has an extent
    pile = (rng.random((3000, 3), dtype=f) * f(100)).astype(f)
    pile[100:800] = f(40.0) + rng.random((700, 3), dtype=f) * f(0.05)
    pile[200:600] = (40.01, 40.02, 40.03)
    pile[650:700] = (40.04, 40.0, 40.01)
    out["coincident_child"] = tuple(np.ascontiguousarray(pile[:, i]) for i in range(3))
    # zeros of both signs: equal values, so they share a cell and keep their input order
    z = rng.integers(-2, 3, (2000, 3)).astype(f) * f(0.5)
    z[::3] = np.where(z[::3] == 0, f(-0.0), z[::3])
    z[5:400] = (0.0, -0.0, 0.0)
    z[400:700] = (-0.0, 0.0, -0.0)
    out["signed_zeros"] = tuple(np.ascontiguousarray(z[:, i]) for i in range(3))
    return out
