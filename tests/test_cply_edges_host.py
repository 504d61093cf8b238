"""-m "not gpu": the compressed-PLY writer's edge fixture (tests/golden/cply_edges_ref.npz, written by the reference's own
``CompressedPlyFormat.write`` through oracle/make_golden_cply_edges.py).  The oracle (oracle/cply.py) reproduces it bit for
bit, which certifies the oracle at the edges for the GPU tests that use it at other sizes; the numpy restatement of the
device's alpha certificate never certifies a wrong byte; and the planted rows do what they were planted for."""
import os
import sys

import numpy as np
import pytest

from oracle import cply as ocply, refload

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cply_edge_cases as ec  # noqa: E402


@pytest.fixture(scope="module")
def gold():
    return ec.gold()


@pytest.fixture(scope="module")
def table(gold):
    return gold["edges__table"]


def test_the_stored_table_is_the_generators(table):
    fresh = ocply.cply_edge_scene()
    assert fresh.dtype == table.dtype and fresh.tobytes() == table.tobytes()
    # the contract of the bit-for-bit comparison: no NaN, no column of a chunk whose extreme is a zero of both signs
    for name in table.dtype.names:
        assert not np.isnan(table[name]).any(), name
    for name in ("x", "y", "z", "scale_0", "scale_1", "scale_2"):
        for c in range(6):
            v = table[name][256 * c:256 * c + 256]
            for ext in (v.min(), v.max()):
                if ext == 0:
                    assert len(set(np.signbit(v[v == 0]).tolist())) == 1, (name, c)


def test_oracle_reproduces_the_fixture_bit_for_bit(gold, table):
    names = [str(s) for s in gold["edges/sh_names"]]
    assert names == ["f_rest_%d" % i for i in range(45)]
    order, _ = ocply.morton_order(table["x"], table["y"], table["z"])
    np.testing.assert_array_equal(order, gold["edges/order_stable"])
    np.testing.assert_array_equal(order, np.arange(len(table)))       # the table is laid out in its own Morton order
    assert sorted(gold["edges/order_ref"].tolist()) == list(range(len(table)))
    for suffix in ("ref", "stable"):
        chunks, verts, sh = ocply.encode(table, gold["edges/order_" + suffix], names)
        np.testing.assert_array_equal(chunks.view(np.uint32), gold["edges/chunk_" + suffix])
        np.testing.assert_array_equal(verts, gold["edges/vertex_" + suffix])
        np.testing.assert_array_equal(sh, gold["edges/sh_" + suffix])


def test_oracle_morton_order_on_the_edge_clouds_is_the_references(gold):
    clouds = ocply.edge_morton_clouds()
    assert list(clouds) == [str(s) for s in gold["clouds"]]
    deep = 0
    for name, (x, y, z) in clouds.items():
        assert len(x) <= 5000
        order, depth = ocply.morton_order(x, y, z)
        np.testing.assert_array_equal(order, gold["clouds/" + name], err_msg=name)
        deep = max(deep, depth)
    assert deep >= 2


@pytest.mark.skipif(not refload.available(), reason="reference checkout not present")
def test_fixture_is_reproducible_from_the_reference(gold):
    from oracle import make_golden_cply_edges as gen
    live = gen.build()
    assert sorted(live) == sorted(gold.files)
    for key in gold.files:
        a, b = np.asarray(live[key]), gold[key]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), key


def test_alpha_certificate_never_certifies_a_wrong_byte():
    """cply_alpha_code restated in numpy (float64 exp, +-SOG_ULPS_EXP ulps, numpy's float32 sequence at both ends)"""
    for name, x, cap in (("edges", ocply.edge_opacities(), None), ("N(0, 4^2)", ec.random_opacities(), 2)):
        byte, sure = ec.alpha_code(x)
        want = ec.numpy_alpha_byte(x)
        listed = int((~sure).sum())
        print("%s: %d of %d rows listed" % (name, listed, len(x)))
        assert np.array_equal(byte[sure], want[sure]), name
        assert not sure[~(np.abs(x) < 80)].any()                      # +-80 and beyond, +-inf: numpy decides
        if cap is not None:
            assert listed <= cap                                      # measured with seed 21: 1 row
    # the bytes at the far ends, from numpy itself
    x = ocply.edge_opacities()
    want = ec.numpy_alpha_byte(x)
    assert want[x == np.inf].tolist() == [255] and want[x == -np.inf].tolist() == [0]
    assert want[x >= 80].tolist() == [255] * int((x >= 80).sum()) and want[x <= -80].tolist() == [0] * int((x <= -80).sum())
    near = want[14:].reshape(255, 3).astype(np.int64) - np.arange(255)[:, None]
    assert near.min() == 0 and near.max() == 1 and np.all(np.diff(near, axis=1) >= 0)   # boundary j: byte j below it, j + 1 above


def test_planted_rows_do_what_they_are_for(gold, table):
    _, lay = ocply.cply_edge_scene(with_layout=True)
    chunk = gold["edges/chunk_stable"].view(np.float32)
    vert = gold["edges/vertex_stable"]
    pos, rot, scl, col = (vert[:, i] for i in range(4))
    rows = lambda c: slice(256 * c, min(256 * c + 256, len(table)))   # noqa: E731
    field = {0: lambda w: w >> 21, 1: lambda w: (w >> 11) & 1023, 2: lambda w: w & 2047}
    # ---- the 1e-5 switch of the scale ranges: at and above -> quantised, one ulp below -> all zero
    th = lay["scale_threshold"]
    c = th["chunk"]
    rng_ = chunk[c, 9:12] - chunk[c, 6:9]
    e = np.float32(1e-5)
    assert rng_[th["at"]] == e and rng_[th["below"]] == np.nextafter(e, np.float32(0)) and rng_[th["above"]] == np.nextafter(e, np.float32(1))
    assert not field[th["below"]](scl[rows(c)]).any()
    for k in (th["at"], th["above"]):
        got = field[k](scl[rows(c)])
        assert got.max() == (1023 if k == 1 else 2047) and len(set(got.tolist())) > 10
    # ... of the colour ranges
    th = lay["fdc_threshold"]
    c = th["chunk"]
    rng_ = chunk[c, 15:18] - chunk[c, 12:15]
    byte = lambda k, w: (w >> (24 - 8 * k)) & 255                     # noqa: E731
    assert rng_[th["below"]] < e and not byte(th["below"], col[rows(c)]).any()
    for k in th["above"]:
        assert rng_[k] > e and rng_[k] < np.float32(1.01e-5)
        got = byte(k, col[rows(c)])
        assert got.max() == 255 and len(set(got.tolist())) > 3
    # ---- a constant column and a column one ulp wide: zero fields
    assert chunk[3, 6] == chunk[3, 9] == np.float32(-5.5) and chunk[3, 7] == -3 and chunk[3, 10] == np.nextafter(np.float32(-3), np.float32(0))
    assert not field[0](scl[rows(3)]).any() and not field[1](scl[rows(3)]).any()
    # ---- the clip of the scales: every planted extreme ends as exactly -+20 in its chunk's record and as the end code
    for c, k, lane_hi, v_hi, lane_lo, v_lo in lay["scale_slots"]:
        assert table["scale_%d" % k][256 * c + lane_hi] == np.float32(v_hi) and table["scale_%d" % k][256 * c + lane_lo] == np.float32(v_lo)
        assert chunk[c, 6 + k] == -20 and chunk[c, 9 + k] == 20
        top = 1023 if k == 1 else 2047
        assert field[k](scl[256 * c + lane_hi]) == top and field[k](scl[256 * c + lane_lo]) == 0
        inner = np.delete(field[k](scl[rows(c)]), [lane_hi, lane_lo])
        assert inner.min() > 0 and inner.max() < top                  # the extremes are alone in their lanes
    assert set(l for s in lay["scale_slots"] for l in (s[2], s[4])) == set(ocply.EDGE_LANES)
    assert set(s[3] for s in lay["scale_slots"]) == set(ocply.EDGE_SCALES_HI) and set(s[5] for s in lay["scale_slots"]) == set(ocply.EDGE_SCALES_LO)
    assert chunk[5, 9] == 20 and chunk[5, 7] == -20 and chunk[5, 11] == 20 and field[0](scl[-1]) == 2047 and field[1](scl[-1]) == 0
    # ---- +-3e38 colours: finite records, end codes
    for c, k, lane_hi, lane_lo in lay["fdc_slots"]:
        assert np.isfinite(chunk[c, 12 + k]) and np.isfinite(chunk[c, 15 + k]) and chunk[c, 15 + k] > 8e37 and chunk[c, 12 + k] < -8e37
        assert byte(k, col[256 * c + lane_hi]) == 255 and byte(k, col[256 * c + lane_lo]) == 0
    assert set(l for s in lay["fdc_slots"] for l in s[2:]) == set(ocply.EDGE_LANES)
    # ---- coordinates: the lattice chunk spans exactly [0, 1]^3, the last chunk 3e38
    assert chunk[0, :6].tolist() == [0, 0, 0, 1, 1, 1]
    assert np.all(np.isfinite(chunk[5, :6])) and np.all(chunk[5, 3:6] - chunk[5, :3] > 3e38)
    # ---- rotations
    word = {}
    for i in range(0, len(table), 5):
        word.setdefault(ocply.EDGE_ROTATIONS[(i // 5) % len(ocply.EDGE_ROTATIONS)], set()).add(int(rot[i]))
    assert all(len(v) == 1 for v in word.values())                    # each pattern sits in several rows, one word for all of them
    word = {k: v.pop() for k, v in word.items()}
    mid = (512 << 20) | (512 << 10) | 512
    for q in ((0, 0, 0, 0), (-0.0, 0, 0, 0), (1e20, 0, 0, 0), (3e38, 3e38, 0, 0)):
        assert word[q] == mid, q                                      # largest = 0, three codes of 512
    unpack = lambda w: (w >> 30, (w >> 20) & 1023, (w >> 10) & 1023, w & 1023)   # noqa: E731
    assert unpack(word[(1e-20, 0, 0, 0)]) == (0, 512, 512, 512)       # 1e-20 / 1e-10: too small to move a code
    assert unpack(word[(1e-30, -1e-30, 1e-30, 1e-30)]) == (0, 512, 512, 512)
    assert unpack(word[(1e-10, 0, 0, 0)]) == (0, 512, 512, 512)
    # ties: argmax takes the first component; the winner's sign flips the others
    half = int(np.floor((np.float32(0.5) * 0.7071067811865476 + 0.5) * 1023 + 0.5))
    low = int(np.floor((np.float32(-0.5) * 0.7071067811865476 + 0.5) * 1023 + 0.5))
    assert unpack(word[(.5, .5, .5, .5)]) == (0, half, half, half)
    assert unpack(word[(-.5, .5, .5, .5)]) == (0, low, low, low)
    assert unpack(word[(.5, -.5, .5, -.5)]) == (0, low, half, low)
    assert unpack(word[(0, 1, -1, 0)])[0] == 1 and unpack(word[(0, 1, -1, 0)])[1] == 512 and unpack(word[(0, 1, -1, 0)])[3] == 512
    assert unpack(word[(0, 1, -1, 0)])[2] == 0                        # -1 / (sqrt(2) + 1e-10): the lowest code
    assert unpack(word[(0, 0, 0, -1)]) == (3, 512, 512, 512)
    # ---- opacities and SH bytes are numpy's own expressions on the planted values
    np.testing.assert_array_equal(col & 255, ec.numpy_alpha_byte(table["opacity"]))
    assert (col[-1] & 255) == 255 and (col[-2] & 255) == 0
    sh = gold["edges/sh_stable"]
    vals = ocply.edge_sh_values()
    np.testing.assert_array_equal(sh[:len(vals), 0], ec.numpy_sh_bytes(vals))
    steps = sh[:512, 0].reshape(256, 2)
    assert steps[:, 1].tolist() == list(range(256))                   # byte j begins at 8 * (j / 256 - 0.5) ...
    below = steps[:, 1].astype(int) - steps[:, 0]                     # ... the float32 below it gives j - 1 unless `/ 8 + 0.5` rounds it up
    assert below[0] == 0 and set(below[1:].tolist()) == {0, 1} and below[1:64].all()   # (exact below 0.25)
    assert sh[512:520, 0].tolist() == [255, 0, 255, 0, 255, 0, 128, 128]
    for k in range(45):
        np.testing.assert_array_equal(sh[:len(vals), k], np.roll(sh[:len(vals), 0], -7 * k))
