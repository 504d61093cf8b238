"""-m gpu: csrc/sor_stats.hip (np.mean / np.std / threshold / mask of the SOR filter) at every shape, on bits.

tests/test_sor_gpu.py::test_stats_kernel_matches_numpy runs 13 sizes, i.e. ten ragged last-piece lengths, none of them
behind three full pieces of one workgroup, and crosses the 1024-entry fold tile only inside the 10M-point tests.  Here:
every ragged length 1 ... 8191 at every position of a four-piece workgroup (leaf_of, the "first multiple of 32 inside a
leaf" ownership rule and replay_tree<7> split each length differently), the sequential fold at and around FOLD_TILE through
both entry points, value edges, and the mask at the threshold.  The references are numpy's own reductions."""
import ctypes as C

import numpy as np
import pytest

from oracle import sor as osor

pytestmark = pytest.mark.gpu

NP_BUF = 8192


@pytest.fixture(scope="module")
def lib(gsx):
    gsx._lib.require_hip()
    return gsx._lib


@pytest.fixture(scope="module")
def ctx(lib):
    c = lib.Context(0)
    yield c
    c.close()


def heavy_tail(rng, n):
    """positive float32 with a heavy tail, as in test_stats_kernel_matches_numpy"""
    a = (rng.random(n, dtype=np.float32) * 0.3 + 0.01).astype(np.float32)
    a[rng.integers(0, n, max(5, n // 2000))] *= 40
    return a


def _same_bits(got, want):
    return np.asarray(got, np.float32).view(np.uint32) == np.asarray(want, np.float32).view(np.uint32)


def test_piece_sums_at_every_ragged_length(ctx, lib):
    """gsx_sor_piece_sums_dev on n = 8192 f + r for EVERY r in 1 ... 8191 and f in 0 ... 3 (the ragged piece in each wave
    slot of the four-piece workgroup, the full pieces before it summed by the same workgroup), plain sums and sums of
    (a - mean)^2: 65 528 launches into one buffer, one download; against np.add.reduce per 8192-element piece"""
    rng = np.random.default_rng(41)
    a = heavy_tail(rng, 4 * NP_BUF)
    mean = np.float32(0.2171)
    sq = (a - mean) ** 2
    assert sq.dtype == np.float32
    d_a = ctx.alloc(a.nbytes).upload(a)
    d_mean = ctx.alloc(16).upload(np.array([mean], np.float32))
    slots = np.full((2, 4, NP_BUF - 1, 4), np.nan, np.float32)       # [squares?, f, r - 1, piece]
    d_out = ctx.alloc(slots.nbytes).upload(slots)
    fn, h = ctx.lib.gsx_sor_piece_sums_dev, ctx.handle
    try:
        for s in range(2):
            mp = d_mean.ptr if s else None
            for f in range(4):
                base = d_out.ptr + 4 * slots[s, f].size * (s * 4 + f)
                for r in range(1, NP_BUF):
                    if fn(h, d_a.ptr, f * NP_BUF + r, mp, base + 16 * (r - 1)) != 0:
                        lib.check(1, "gsx_sor_piece_sums_dev")
        got = d_out.download(np.float32, slots.size).reshape(slots.shape)
    finally:
        for x in (d_a, d_mean, d_out):
            x.free()
    for s, src in enumerate((a, sq)):
        full = [np.add.reduce(src[NP_BUF * j:NP_BUF * (j + 1)], dtype=np.float32) for j in range(4)]
        for f in range(4):
            want = np.full((NP_BUF - 1, 4), np.nan, np.float32)
            want[:, :f] = full[:f]
            want[:, f] = [np.add.reduce(src[NP_BUF * f:NP_BUF * f + r], dtype=np.float32) for r in range(1, NP_BUF)]
            bad = np.argwhere(got[s, f].view(np.uint32) != want.view(np.uint32))
            assert len(bad) == 0, "%s, %d full pieces: %d piece sums differ; first (r - 1, piece): %s got %s want %s" % (
                ("plain", "squares")[s], f, len(bad), bad[:5].tolist(), [got[s, f][tuple(i)] for i in bad[:5]],
                [want[tuple(i)] for i in bad[:5]])


FOLD_SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 3001)


def test_fold_of_piece_sums_is_sequential(ctx):
    """gsx_sor_stats_from_pieces_dev on synthetic piece arrays around the 64-entry read batch and the 1024-entry fold tile,
    both modes: the pieces are added one after the other in float32 (np.add.accumulate), then numpy's float64 divide"""
    rng = np.random.default_rng(42)
    factor = 10.5
    d_stats = ctx.alloc(16 * len(FOLD_SIZES))
    d_p = ctx.alloc(4 * 2 * max(FOLD_SIZES))
    want = np.zeros((len(FOLD_SIZES), 4), np.float32)
    try:
        for i, npieces in enumerate(FOLD_SIZES):
            n_total = npieces * NP_BUF - 17 * (npieces > 1) - 3
            p = np.stack([heavy_tail(rng, npieces) * np.float32(NP_BUF), heavy_tail(rng, npieces) * np.float32(300)])
            d_p.upload(np.ascontiguousarray(p))
            for mode in (0, 1):
                rc = ctx.lib.gsx_sor_stats_from_pieces_dev(ctx.handle, d_p.ptr + 4 * npieces * mode, npieces, n_total, mode, factor,
                                                           d_stats.ptr + 16 * i)
                assert rc == 0
            ctx.synchronize()      # d_p is overwritten by the next size
            acc = [np.add.accumulate(p[mode], dtype=np.float32)[-1] for mode in (0, 1)]
            mean = np.float32(np.float64(acc[0]) / n_total)
            std = np.sqrt(np.float32(np.float64(acc[1]) / n_total))
            assert std.dtype == np.float32
            want[i, :3] = mean, std, mean + np.float32(factor) * std
        got = d_stats.download(np.float32, 4 * len(FOLD_SIZES)).reshape(-1, 4)
    finally:
        d_stats.free()
        d_p.free()
    ok = _same_bits(got[:, :3], want[:, :3])
    assert ok.all(), [(FOLD_SIZES[i], got[i, :3].tolist(), want[i, :3].tolist()) for i in np.flatnonzero(~ok.all(axis=1))]


def test_whole_array_stats_across_the_fold_tile(ctx):
    """gsx_sor_stats_dev with 1024, 1025 and 2049 piece sums: the last workgroup to arrive folds them itself, 256 lanes
    staging FOLD_TILE entries at a time; against np.mean / np.std (oracle.sor.threshold_numpy)"""
    rng = np.random.default_rng(43)
    sizes = (NP_BUF * 1024, NP_BUF * 1024 + 1, NP_BUF * 1024 + 8191, NP_BUF * 2048 + 1)
    a = heavy_tail(rng, max(sizes))
    d_a = ctx.alloc(a.nbytes).upload(a)
    d_stats = ctx.alloc(16 * len(sizes))
    try:
        for i, n in enumerate(sizes):
            ctx.sor_stats(d_a.ptr, n, 1.0, d_stats.ptr + 16 * i)
        got = d_stats.download(np.float32, 4 * len(sizes)).reshape(-1, 4)
    finally:
        d_a.free()
        d_stats.free()
    for i, n in enumerate(sizes):
        want = osor.threshold_numpy(a[:n], 1.0)
        assert _same_bits(got[i, :3], want).all(), (n, got[i, :3].tolist(), [float(w) for w in want])


N_EDGE = 3 * NP_BUF + 4465


def _edge_arrays():
    rng = np.random.default_rng(44)
    base = heavy_tail(rng, N_EDGE)
    tiny = base * np.float32(1e-20)             # (a - mean)^2 ~ 1e-42: float32 subnormals
    spike = base.copy()
    spike[N_EDGE // 3] *= np.float32(2.0 ** 60)
    return {"all_equal": np.full(N_EDGE, 0.37, np.float32), "all_zero": np.zeros(N_EDGE, np.float32), "subnormal_squares": tiny,
            "one_value_2^60_times_the_rest": spike}


@pytest.mark.parametrize("name", ["all_equal", "all_zero", "subnormal_squares", "one_value_2^60_times_the_rest"])
def test_stats_value_edges(ctx, name):
    a = _edge_arrays()[name]
    if name == "subnormal_squares":
        m = np.mean(a)
        sq = (a - m) ** 2
        assert 0 < sq.max() < np.finfo(np.float32).tiny            # the case is what its name says
    d_a = ctx.alloc(a.nbytes).upload(a)
    d_stats = ctx.alloc(32)
    try:
        for j, tf in enumerate((1.0, 10.5)):
            ctx.sor_stats(d_a.ptr, len(a), tf, d_stats.ptr + 16 * j)
        got = d_stats.download(np.float32, 8).reshape(2, 4)
    finally:
        d_a.free()
        d_stats.free()
    for j, tf in enumerate((1.0, 10.5)):
        want = osor.threshold_numpy(a, tf)
        assert _same_bits(got[j, :3], want).all(), (name, tf, got[j, :3].tolist(), [float(w) for w in want])


@pytest.mark.parametrize("thr", [0.25, float("nan"), float("inf"), 0.0], ids=["0.25", "nan", "inf", "0"])
def test_mask_at_the_threshold(ctx, thr):
    """mask = md < threshold, strict: entries equal to the threshold are False, one ulp below True, one ulp above False;
    the four-wide body and the 0 ... 3 entries behind it; NaN, +inf and 0 as thresholds"""
    rng = np.random.default_rng(45)
    thr = np.float32(thr)
    for n in (1, 2, 3, 5, 4096, 4097, 4098, 4099):
        a = heavy_tail(rng, n)
        if np.isfinite(thr):
            special = [thr, np.nextafter(thr, np.float32(-np.inf)), np.nextafter(thr, np.float32(np.inf)), -thr]
        else:
            special = [np.float32(np.inf), np.float32(3.4e38), np.float32(0)]
        special += [np.float32(np.nan), np.float32(-0.0), np.float32(1e-45), np.float32(-1e-45)]
        for j, v in enumerate(special * 2):
            a[(n - 1 - j) % n if j < len(special) else (j * 7) % n] = v         # the tail entries and the body
        d_a = ctx.alloc(max(16, a.nbytes)).upload(a)
        d_thr = ctx.alloc(16).upload(np.array([thr], np.float32))
        d_m = ctx.alloc(n + 4)
        try:
            ctx.sor_mask(d_a.ptr, n, d_thr.ptr, d_m.ptr)
            got = d_m.download(np.uint8, n)
        finally:
            for x in (d_a, d_thr, d_m):
                x.free()
        with np.errstate(invalid="ignore"):
            want = a < thr
        assert set(np.unique(got)) <= {0, 1}
        np.testing.assert_array_equal(got.view(np.bool_), want, err_msg="n=%d thr=%r" % (n, thr))
        if np.isfinite(thr) and n >= 4096:
            assert not want[a == thr].any() and want[a == np.nextafter(thr, np.float32(-np.inf))].all()
