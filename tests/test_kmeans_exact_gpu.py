"""-m gpu: the scalar codebook solver (csrc/kmeans1d.hip), the greedy k-means++ seeding (csrc/kmeans_pp.hip) and the codebook
quantiser (csrc/kmeans.hip:quantize_kernel, csrc/sog_math.h:sog_codebook_index) pinned on bits.

The device sums prefixes, tiles and potentials in another order than numpy, which is why tests/test_kmeans_gpu.py compares
them inside a tolerance or on a prefix of the picks.  Here the inputs are chosen so that every sum is exact (values on a
2^-10 grid, rows of small integers: oracle/kmeans.py:exact_values_1d, exact_rows_pp; tests/kmeans_exact_cases.py).  Then the
order cannot matter and the device must equal the float64 restatements step by step, bit for bit: one value in the wrong run,
one early exit too soon, one tile handed over a row late shows.  What the inputs promise is asserted without a GPU in
tests/test_kmeans1d_oracle.py."""
import numpy as np
import pytest

import kmeans_exact_cases as kec
from oracle import kmeans as okm

pytestmark = pytest.mark.gpu


def bits(a) -> bytes:
    return np.ascontiguousarray(a).tobytes()


class K1Device:
    """gsx_kmeans1d_dev (the entry point formats/sog_device.py calls) on values uploaded once, start_mask chosen per call"""

    def __init__(self, gsx, x: np.ndarray):
        self.lib = gsx._lib
        self.ctx = self.lib.Context()
        self.n = len(x)
        self.d_x = self.ctx.alloc(4 * max(self.n, 1))
        if self.n:
            self.d_x.upload(np.ascontiguousarray(x, dtype=np.float32))
        self.d_c = self.ctx.alloc(4 * 1024)
        self.d_l = self.ctx.alloc(4 * max(self.n, 1))

    def run(self, k: int, iters: int, mask: int, labels: bool = False, n=None):
        inertia = np.full(3, np.nan)
        self.lib.check(self.ctx.lib.gsx_kmeans1d_dev(self.ctx.handle, self.d_x.ptr, self.n if n is None else n, int(k), int(iters), int(mask),
                                                     self.d_c.ptr, self.d_l.ptr if labels else None, inertia.ctypes.data), "gsx_kmeans1d_dev")
        cent = self.d_c.download(np.float32, k)
        return cent, inertia, (self.d_l.download(np.int32, self.n) if labels else None)

    def close(self):
        for b in (self.d_x, self.d_c, self.d_l):
            b.free()
        self.ctx.close()


@pytest.fixture
def k1(gsx):
    made = []

    def make(x):
        made.append(K1Device(gsx, x))
        return made[-1]

    yield make
    for d in made:
        d.close()


# The device's inertia is sum_j t_j with t_j = S2 - 2 c S1 + cnt c^2 per run, S1, S2 exact here.  With u = 2^-53 and
# M_j = S2 + 2 |c S1| + cnt c^2: evaluating t_j takes at most 5 rounded operations (c S1, the subtraction, cnt c, times c,
# the addition; a fused multiply-add only removes one), each on a quantity of at most M_j, so the device's t_j and numpy's
# differ from the real t_j by at most 5 u M_j each: 10 u M_j between them.  The device adds the t_j through 6 levels of a
# butterfly and then at most 16 wave totals in turn (k1_block_sum): every t_j passes through at most 22 additions, an error of
# at most 22 u sum |t_j| <= 22 u sum M_j; numpy's pairwise sum of k <= 1024 terms (blocks of at most 128 in 8 lanes: 16 + 3
# additions, then at most 3 levels) stays under 24 u sum M_j in the same way.  10 + 22 + 24 = 56; 64 covers the
# second-order terms.  Not fitted to a run.
INERTIA_ULPS = 64.0


def check_inertia(s, cent, got: float):
    terms, mags = s.inertia_terms(cent)
    want, bound = float(terms.sum()), INERTIA_ULPS * 2.0 ** -53 * float(mags.sum())
    assert abs(got - want) <= bound, (got, want, bound)


def check_start(s, k, mask, start):
    """the device's own start (iters = 0) against _k1_start at the tolerance of tests/test_kmeans_gpu.py (the two cbrt may
    differ in the last bit); ascending"""
    assert np.all(np.diff(start) >= 0)
    ref = okm._k1_start(s.xs, k, mask >> 1)
    err = np.abs(start.astype(np.float64) - ref)
    print("start: max |dev - ref| = %.3g" % err.max())
    assert np.allclose(start, ref, rtol=2e-4, atol=2e-5 * float(s.xs.std()))


def follow(dev, s, k, mask, steps):
    """device centroids after T steps == the restatement's from the device's own start, on bits, for every T in steps(fixed);
    the inertia inside its rounding bound, the other start's slot 0.0, the chosen slot the start's own"""
    start, inertia0, _ = dev.run(k, 0, mask)
    check_start(s, k, mask, start)
    check_inertia(s, start, inertia0[mask])
    traj, fixed = kec.trajectory(s, start)
    for T in steps(fixed, len(traj) - 1):
        cent, inertia, _ = dev.run(k, T, mask)
        assert bits(cent) == bits(traj[T]), "step %d of %d: %d centroids differ" % (T, fixed, np.count_nonzero(cent != traj[T]))
        check_inertia(s, traj[T], inertia[mask])
        assert inertia[3 - mask] == 0.0 and not np.signbit(inertia[3 - mask])
        assert bits(inertia[0]) == bits(inertia[mask])
    last = len(traj) - 1
    ref = okm.kmeans1d_lloyd_from(s, start, last)
    assert bits(ref[0]) == bits(traj[last])
    return traj, fixed


@pytest.mark.parametrize("name,k", [r for r in kec.ONE_D_RUNS if r[0] != "big"], ids=lambda v: str(v))
def test_kmeans1d_trajectory_on_bits(gsx, k1, name, k):
    """every step up to two past the fixed point (so the early exit too), both starts on their own"""
    s = kec.sorted_1d(name)
    dev = k1(kec.values_1d(name))
    for mask in (1, 2):
        traj, fixed = follow(dev, s, k, mask, lambda fixed, last: range(1, last + 1))
        print(name, k, "mask", mask, "fixed after", fixed, "steps; midpoint hits",
              sum(kec.midpoint_hits(s, c) for c in traj), "empty runs", int(np.count_nonzero(np.diff(s.bounds(traj[-1])) == 0)))
        assert fixed < kec.T_CAP


def test_kmeans1d_trajectory_on_bits_257_tiles(gsx, k1):
    """n = 263 169: 257 full prefix tiles and one value more, so the tile scan's carry into its second chunk of 256"""
    s = kec.sorted_1d("big")
    assert (s.n + 1023) // 1024 == 258 and s.n == 257 * 1024 + 1
    dev = k1(kec.values_1d("big"))
    for mask in (1, 2):
        follow(dev, s, 256, mask, lambda fixed, last: sorted({1, 2, 5, min(fixed, last), min(fixed + 1, last)}))


@pytest.mark.parametrize("k", [1, 256])
def test_kmeans1d_constant_input(gsx, k1, k):
    """hi == lo, and wtot == 0 in the equal-count start: every centroid is the value, the inertia exactly 0.0"""
    x = kec.values_1d("constant")
    dev = k1(x)
    for mask in (1, 2, 3, 0):
        for iters in (0, 1, 5):
            cent, inertia, labels = dev.run(k, iters, mask, labels=True)
            assert bits(cent) == bits(np.full(k, x[0], np.float32))
            assert bits(inertia) == bits(np.zeros(3))
            assert not labels.any()


@pytest.mark.parametrize("name,k", sorted(kec.WINNER_RUNS), ids=lambda v: str(v))
def test_kmeans1d_picks_the_winner(gsx, k1, name, k):
    """start_mask 3: each start's inertia is its single run's, start A's centroids unless B's inertia is strictly smaller;
    start_mask 0 and the host entry gsx_kmeans1d return the same bytes, and so does a second call"""
    x = kec.values_1d(name)
    dev = k1(x)
    c1, i1, _ = dev.run(k, 50, 1)
    c2, i2, _ = dev.run(k, 50, 2)
    c3, i3, _ = dev.run(k, 50, 3)
    assert bits(i3[1]) == bits(i1[1]) and bits(i3[2]) == bits(i2[2])
    win = 2 if i3[2] < i3[1] else 1
    print(name, k, "inertia", i3.tolist(), "winner", win)
    assert win == kec.WINNER_RUNS[name, k]
    assert bits(c3) == bits(c2 if win == 2 else c1) and bits(i3[0]) == bits(i3[win])
    for again in (dev.run(k, 50, 0), dev.run(k, 50, 3)):
        assert bits(again[0]) == bits(c3) and bits(again[1]) == bits(i3)
    for _ in range(2):
        hc, hi = gsx._lib.kmeans1d(x, k, iters=50, want_inertia=True)
        assert bits(hc) == bits(c3) and bits(hi) == bits(i3)


def nearest_first(x: np.ndarray, cent: np.ndarray) -> np.ndarray:
    """argmin_j |x - c_j| in float64, numpy's first minimum, in chunks"""
    c = cent.astype(np.float64)
    out = np.empty(len(x), dtype=np.int32)
    for a in range(0, len(x), 4096):
        out[a:a + 4096] = np.abs(x[a:a + 4096].astype(np.float64)[:, None] - c[None, :]).argmin(1)
    return out


def test_kmeans1d_labels_first_minimum(gsx, k1):
    """k1_labels_kernel == argmin with the first minimum: values exactly halfway between two centroids (the lower index),
    duplicate centroids (the first of them), values below the first centroid and above the last"""
    seen = {"halfway": 0, "duplicates": 0, "below": 0, "above": 0}
    for name, k, mask in (("gauss", 1000, 1), ("n1023", 1024, 2), ("n1025", 1000, 1), ("discrete32", 256, 1), ("twovalued", 256, 2),
                          ("twoclose", 256, 1), ("twoclose", 256, 3), ("n63", 64, 2), ("n2", 256, 1)):
        x, s = kec.values_1d(name), kec.sorted_1d(name)
        dev = k1(x)
        start = dev.run(k, 0, mask if mask != 3 else 1)[0]
        traj, fixed = kec.trajectory(s, start)
        hits = [kec.midpoint_hits(s, c) for c in traj]
        steps = sorted({0, int(np.argmax(hits)), 50}) if len(x) * k < 10_000_000 else [int(np.argmax(hits))]
        for T in steps:
            cent, _, labels = dev.run(k, T, mask, labels=True)
            if mask != 3:
                assert bits(cent) == bits(traj[min(T, len(traj) - 1)])
            want = nearest_first(x, cent)
            assert np.array_equal(labels, want), (name, k, T, int(np.count_nonzero(labels != want)))
            seen["halfway"] += kec.midpoint_hits(s, cent)
            same = np.diff(cent) == 0                                        # heads of duplicate runs that some value is nearest to
            heads = np.nonzero(np.concatenate([same, [False]]) & ~np.concatenate([[False], same]))[0]
            seen["duplicates"] += int(np.isin(want, heads).sum())
            seen["below"] += int(np.count_nonzero(x < cent[0]))
            seen["above"] += int(np.count_nonzero(x > cent[-1]))
    print(seen)
    assert all(v > 0 for v in seen.values()), seen


def test_kmeans1d_refusals(gsx, k1):
    """a value that is not finite, or beyond 3.0e38, anywhere in the array; shapes outside 1 <= k <= 1024, iters >= 0, n >= 1"""
    err = gsx._lib.GsxError
    x = kec.values_1d("n4097")[:2049].copy()
    s = okm.K1Sorted(np.sort(x))
    dev = k1(x)
    for bad in (np.nan, np.inf, -np.inf, 3.4e38, -3.4e38):
        for at in (0, 1023, 1024, 2048):
            y = x.copy()
            y[at] = bad
            dev.d_x.upload(y)
            with pytest.raises(err):
                dev.run(256, 5, 3)
    y = x.copy()
    y[1024] = 3.0e38                                                     # the largest magnitude admitted
    dev.d_x.upload(y)
    cent, inertia, _ = dev.run(256, 5, 1)
    assert np.isfinite(cent).all() and np.all(np.diff(cent) >= 0) and cent[-1] > 1e37 and np.isfinite(inertia).all()
    dev.d_x.upload(x)
    for k, iters, n in ((0, 5, None), (1025, 5, None), (-1, 5, None), (256, -1, None), (256, 5, 0), (256, 5, -1)):
        with pytest.raises(err):
            dev.run(k, iters, 3, n=n)
    cent, _, _ = dev.run(256, 3, 1)                                       # and the context still works after every refusal
    assert bits(cent) == bits(okm.kmeans1d_lloyd_from(s, dev.run(256, 0, 1)[0], 3)[0])


# ---- k-means++ ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,k,L,distinct", kec.PP_SHAPES, ids=lambda v: str(v))
def test_kmeans_pp_whole_pick_sequence(gsx, n, d, k, L, distinct):
    """all k centroids == x[the restatement's picks], on exact rows"""
    x = kec.rows_pp(n, d, distinct)
    u = np.random.default_rng(n + k).random(1 + (k - 1) * L)
    st = okm.KmeansPPStepper(x, L)
    picks = st.run(k, u)
    got = gsx._lib.kmeans_pp(x, k, u, L)
    assert got.dtype == np.float32 and got.shape == (k, d)
    assert bits(got) == bits(x[picks]), np.nonzero((got != x[picks]).any(1))[0][:5]
    if distinct:
        assert st.total == 0.0 and len(np.unique(x[picks[:distinct]], axis=0)) == distinct   # the zero-total branch ran after that
    if k == n:
        assert sorted(picks.tolist()) == list(range(n))
    assert bits(gsx._lib.kmeans_pp(x, k, u, L)) == bits(got)


@pytest.mark.parametrize("n,d,k,L", [(4097, 9, 16, 12), (2049, 1024, 6, 12)])
def test_kmeans_pp_planted_uniforms(gsx, n, d, k, L):
    """u = 0, u = 1 - 2^-53, targets exactly ON a cumulative sum (row 0, mid-tile, the last rows of a tile, the first of the
    next), twin trials: every trial of a planted step carries the planted uniform, so the step's pick IS that candidate"""
    x = kec.rows_pp(n, d)
    u, picks, log = kec.planted_run(x, k, L)
    assert sorted(log) == sorted(kec.planted_plan(n))
    got = gsx._lib.kmeans_pp(x, k, u, L)
    wrong = np.nonzero((got != x[picks]).any(1))[0]
    assert bits(got) == bits(x[picks]), [(int(t), log.get(int(t))) for t in wrong[:4]]


def test_kmeans_pp_refusals(gsx):
    kpp, err = gsx._lib.kmeans_pp, gsx._lib.GsxError
    x = kec.rows_pp(6, 3)
    good = np.full(1 + 3 * 2, 0.25)
    assert kpp(x, 4, good, 2).shape == (4, 3)
    with pytest.raises(err):
        kpp(x, 7, np.full(1 + 6 * 2, 0.25), 2)                                  # k > n
    for L in (0, 13):
        with pytest.raises(err):
            kpp(x, 4, np.full(1 + 3 * L, 0.25), L)
    for d, L in ((12289, 1), (1756, 7), (4097, 1), (4097, 3)):                    # L d = 12289 (needs d > 4096: 12289 is prime), 12292; d = 4097
        with pytest.raises(err):
            kpp(np.zeros((2, d), np.float32), 2, np.full(1 + L, 0.25), L)
    assert kpp(np.zeros((2, 4096), np.float32), 2, np.full(1 + 3, 0.25), 3).shape == (2, 4096)   # L d = 12288, d = 4096: admitted
    for bad in (1.0, -2.0 ** -60, np.nan, np.inf):
        for at in (0, 1, 6):
            u = good.copy()
            u[at] = bad
            with pytest.raises(err):
                kpp(x, 4, u, 2)
    u = good.copy()
    u[[0, 6]] = kec.U_LAST, 0.0
    assert kpp(x, 4, u, 2).shape == (4, 3)


def test_kmeans_front_door_use_gpu_false_on_exact_rows(gsx):
    """gpu_ops.kmeans(use_gpu=False): seeds = the restated picks from the same numpy stream, then max_iter Lloyd steps and the
    one-step label call"""
    n, d, k, m = 5000, 45, 64, 3
    x = kec.rows_pp(n, d, seed=1)
    for seed in (0, 7):
        np.random.seed(seed)
        cent, labels = gsx.gpu_ops.kmeans(x, k, max_iter=m, use_gpu=False)
        np.random.seed(seed)
        L = 2 + int(np.log(k))
        u = np.random.random_sample(1 + (k - 1) * L)
        picks = okm.KmeansPPStepper(x, L).run(k, u)
        c_ref, _ = gsx._lib.kmeans_lloyd(x, x[picks], m)
        _, l_ref = gsx._lib.kmeans_lloyd(x, c_ref, 1)
        assert bits(cent) == bits(c_ref) and bits(labels) == bits(l_ref)
        assert labels.dtype == np.int32 and cent.shape == (k, d)


# ---- quantiser --------------------------------------------------------------------------------------------------------------
def _codebooks(kcb: int):
    """sorted dyadic codebooks of kcb entries (multiples of 2^-6, so midpoints and differences are exact in float32) with
    duplicate runs at the front, in the middle, at the end, everywhere, and none"""
    r = np.random.default_rng(kcb)
    base = np.sort(r.choice(np.arange(-4000, 4000), kcb, replace=False)).astype(np.float32) * np.float32(2.0 ** -5)
    out = {"distinct": base}
    for where in ("front", "middle", "end"):
        c = base.copy()
        run = max(1, kcb // 3)
        a = {"front": 0, "middle": (kcb - run) // 2, "end": kcb - run}[where]
        c[a:a + run] = c[a]
        out[where] = np.sort(c)
    out["all_equal"] = np.full(kcb, base[0], np.float32)
    return out


def _quant_values(cb: np.ndarray, n: int) -> np.ndarray:
    mids = (cb[:-1] + cb[1:]) * np.float32(0.5)
    assert np.array_equal(mids.astype(np.float64), (cb[:-1].astype(np.float64) + cb[1:]) * 0.5)   # exact midpoints
    r = np.random.default_rng(n)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, cb[0] - 1, cb[0] - 2.0 ** -6, cb[-1] + 1, cb[-1] + 2.0 ** -6, 3e38, -3e38],
                       dtype=np.float32)
    pool = np.concatenate([special, cb, mids, mids + np.float32(2.0 ** -7), mids - np.float32(2.0 ** -7),
                           (r.integers(-9000, 9000, 64) * 2.0 ** -6).astype(np.float32)])
    if n >= len(pool):
        return np.concatenate([pool, r.choice(pool, n - len(pool))])
    return r.choice(pool, n, replace=False)


@pytest.mark.parametrize("kcb", [1, 2, 3, 255, 256])
def test_quantiser_duplicates_midpoints_and_non_finite(gsx, kcb):
    """quantize_sorted_codebook == the reference's closure (okm.quantize_to_codebook) on bytes"""
    for name, cb in _codebooks(kcb).items():
        for n in (1, 255, 256, 257, 100003):
            vals = _quant_values(cb, n)
            with np.errstate(invalid="ignore"):
                want = okm.quantize_to_codebook(vals, cb)
            got = gsx._lib.quantize_sorted_codebook(vals, cb)
            assert got.dtype == np.uint8 and bits(got) == bits(want), (name, n, np.nonzero(got != want)[0][:5])


def test_quantiser_on_a_codebook_kmeans1d_returned(gsx):
    """the discrete case's codebook: 32 levels and 224 centroids of empty runs left where they started"""
    x = kec.values_1d("discrete32")
    cb = gsx._lib.kmeans1d(x, 256, iters=50)
    assert np.all(np.diff(cb) >= 0) and set(np.unique(x + np.float32(0)).tolist()) <= set(cb.tolist())
    mids = (cb[:-1] + cb[1:]) * np.float32(0.5)
    vals = np.concatenate([x, cb, mids, np.array([0.0, -0.0, -40.0, 40.0, np.inf, -np.inf, np.nan], np.float32)])
    with np.errstate(invalid="ignore"):
        want = okm.quantize_to_codebook(vals, cb)
    assert bits(gsx._lib.quantize_sorted_codebook(vals, cb)) == bits(want)
    assert bits(gsx.gpu_ops.quantize_to_codebook(vals, cb)) == bits(want)
