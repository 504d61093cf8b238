"""not gpu: the scalar-codebook solver that replaces the reference's scikit-learn calls (formats/sog.py:561,
processing/gpu_ops.py:48-52 for D = 1) -- its numpy restatement (oracle/kmeans.py:kmeans1d_sorted, the checker of
csrc/kmeans1d.hip) against scikit-learn itself, the reference's actual arithmetic for these calls.  The reference is
unseeded, so the bar is quality: inertia no worse than MiniBatchKMeans' on the same values.  Below that: the exact-sum
checkers and inputs of tests/test_kmeans_exact_gpu.py (oracle/kmeans.py, tests/kmeans_exact_cases.py) -- what they promise,
asserted here so that the GPU tests cannot pass for want of a hard case."""
import numpy as np
import pytest

import kmeans_exact_cases as kec
from oracle import kmeans as okm

CASES = {
    "scales_50k": lambda r: (r.standard_normal(50000) - 4.0).astype(np.float32),                 # sog.py:396-402 sample
    "dc_50k": lambda r: r.standard_normal(50000).astype(np.float32),                             # sog.py:438-443 sample
    "palette_flat": lambda r: (r.standard_normal(400_000) * 0.1).astype(np.float32),             # sog.py:557-561 (scaled down)
    "bimodal": lambda r: np.concatenate([r.standard_normal(25000) * 0.2 - 3, r.standard_normal(25000) * 2 + 1]).astype(np.float32),
    "outliers": lambda r: np.concatenate([r.standard_normal(49990) * 0.1, r.standard_normal(10) * 50]).astype(np.float32),
    "uniform": lambda r: r.random(50000).astype(np.float32),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_sorted_run_solver_is_at_least_sklearn_quality(name):
    x = CASES[name](np.random.default_rng(7))
    cent, inertia = okm.kmeans1d_sorted(x, 256, 50)
    assert np.all(np.diff(cent) >= 0) and len(cent) == 256
    assert abs(okm.inertia_1d(x, cent) - inertia[0]) <= 1e-6 * inertia[0] + 1e-9   # the prefix-sum inertia is the real one
    assert inertia[0] == min(inertia[1], inertia[2])
    np.random.seed(3)
    sk = min(okm.inertia_1d(x, okm.sklearn_codebook_561(x)) for _ in range(2))
    assert inertia[0] <= 1.0 * sk, (inertia, sk)


def test_fewer_distinct_values_than_centroids():
    x = np.random.default_rng(1).integers(0, 40, 50000).astype(np.float32)
    cent, inertia = okm.kmeans1d_sorted(x, 256, 50)
    assert inertia[0] <= 1e-6 and set(np.unique(x)) <= set(cent.tolist())
    cent, inertia = okm.kmeans1d_sorted(np.full(1000, 2.5, np.float32), 16, 10)
    assert inertia[0] == 0.0 and np.all(cent == np.float32(2.5))


def test_kmeans_pp_restatement_separated_clusters():
    """D^2 sampling must take one row from every cluster when the clusters are tight and far apart"""
    rng = np.random.default_rng(0)
    centers = rng.random((12, 5)) * 1000.0
    which = rng.integers(0, 12, 6000)
    x = (centers[which] + rng.standard_normal((6000, 5)) * 1e-3).astype(np.float32)
    idx = okm.kmeans_pp_restated(x, 12, rng.random(1 + 11 * 4), 4)
    assert sorted(which[idx].tolist()) == list(range(12))
    idx = okm.kmeans_pp_restated(x, 12, rng.random(12), 1)
    assert sorted(which[idx].tolist()) == list(range(12))


# ---- the exact-sum checkers and inputs of tests/test_kmeans_exact_gpu.py: what they promise, asserted without a GPU -----------
@pytest.mark.parametrize("name", sorted(kec.ONE_D))
def test_exact_1d_values_sum_exactly_in_any_order(name):
    """the builder's own integer assertions hold, and so do sums in a scrambled order and in the device's tile order"""
    x = kec.values_1d(name)
    m = np.asarray(kec.ONE_D[name]()[0], dtype=np.int64)
    assert x.dtype == np.float32 and len(x) == len(m) <= okm.EXACT_1D_MAXN and np.abs(m).max() < okm.EXACT_1D_LIMIT
    p = np.random.default_rng(0).permutation(len(x))
    x64 = x.astype(np.float64)
    assert x64[p].sum() * 1024.0 == float(m.sum()) == x64.sum() * 1024.0
    assert (x64[p] ** 2).sum() * 1024.0 ** 2 == float((m * m).sum())
    tiles = [x64[i:i + 1024].sum() for i in range(0, len(x), 1024)]            # tile totals first, then the tiles
    assert float(np.sum(tiles[::-1])) * 1024.0 == float(m.sum())
    if kec.ONE_D[name]()[1]:
        assert np.signbit(x[m == 0]).all() and (m == 0).any()                  # -0.0 is really in there
        assert not np.signbit(kec.sorted_1d(name).xs[kec.sorted_1d(name).xs == 0]).any()


def test_exact_builders_refuse_what_they_cannot_promise():
    for bad in (np.array([1 << 15]), np.array([-(1 << 15)]), np.zeros(0, np.int64), np.zeros((1 << 20) + 1, np.int64)):
        with pytest.raises(AssertionError):
            okm.exact_values_1d(bad)
    with pytest.raises(AssertionError):
        okm.exact_values_1d(np.array([0.5]))
    for bad in (np.full((2, 3), 16), np.full((2, 3), -16), np.zeros((5001, 1), np.int64), np.zeros((1, 1025), np.int64)):
        with pytest.raises(AssertionError):
            okm.exact_rows_pp(bad)
    for n, d, k, L, distinct in kec.PP_SHAPES:
        x = kec.rows_pp(n, d, distinct)
        assert x.shape == (n, d) and x.dtype == np.float32
        assert len(np.unique(x, axis=0)) == (distinct or n) or distinct is None
        # a float32 fma chain over the largest differences stays exact: d * 30^2 < 2^24
        assert np.float32(d * 900.0) == d * 900 and d * 900 < 1 << 24
    assert len(np.unique(kec.rows_pp(257, 5, 10), axis=0)) == 10
    assert len(np.unique(kec.rows_pp(300, 300), axis=0)) == 300               # k == n needs n different rows


@pytest.mark.parametrize("name,k,iters", [("scales_50k", 256, 50), ("bimodal", 64, 7), ("outliers", 256, 0), ("uniform", 1000, 3),
                                          ("dc_50k", 1, 5)])
def test_kmeans1d_sorted_is_its_start_plus_lloyd_from(name, k, iters):
    """kmeans1d_sorted == _k1_start + kmeans1d_lloyd_from on every bit, for both starts, and the winner rule"""
    x = CASES[name](np.random.default_rng(7))
    cent, inertia = okm.kmeans1d_sorted(x, k, iters)
    xs = np.sort(x)
    got = [okm.kmeans1d_lloyd_from(xs, okm._k1_start(xs, k, mode), iters) for mode in (0, 1)]
    for mode in (0, 1):
        assert np.float64(got[mode][2]).tobytes() == np.float64(inertia[1 + mode]).tobytes()
        assert got[mode][1][0] == 0 and got[mode][1][-1] == len(xs) and np.all(np.diff(got[mode][1]) >= 0)
    win = 1 if got[1][2] < got[0][2] else 0
    assert cent.tobytes() == got[win][0].tobytes() and inertia[0] == got[win][2]
    s = okm.K1Sorted(xs)                                                       # a K1Sorted is accepted in place of the values
    assert okm.kmeans1d_lloyd_from(s, okm._k1_start(xs, k, 0), iters)[0].tobytes() == got[0][0].tobytes()
    fixed = okm.kmeans1d_steps_until_fixed(s, okm._k1_start(xs, k, 0))
    a, b = okm.kmeans1d_lloyd_from(s, okm._k1_start(xs, k, 0), fixed), okm.kmeans1d_lloyd_from(s, okm._k1_start(xs, k, 0), fixed + 1)
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])
    if fixed > 1:
        before = okm.kmeans1d_lloyd_from(s, okm._k1_start(xs, k, 0), fixed - 2)
        assert not np.array_equal(before[1], okm.kmeans1d_lloyd_from(s, okm._k1_start(xs, k, 0), fixed - 1)[1])


def test_kmeans_pp_stepper_is_the_restatement():
    rng = np.random.default_rng(4)
    for n, d, k, L in ((3000, 9, 40, 5), (500, 45, 12, 1), (700, 300, 6, 12)):
        y = (rng.standard_normal((n, d)) * 0.1).astype(np.float32)              # generic rows: sums that round
        u = rng.random(1 + (k - 1) * L)
        assert okm.KmeansPPStepper(y, L).run(k, u).tolist() == okm.kmeans_pp_restated(y, k, u, L).tolist()
    for n, d, k, L, distinct in kec.PP_SHAPES:
        if n * d * L > 4_000_000:
            continue                                                            # (the restatement's (L, n, d) temporary)
        x = kec.rows_pp(n, d, distinct)
        u = rng.random(1 + (k - 1) * L)
        st = okm.KmeansPPStepper(x, L)
        assert st.run(k, u).tolist() == okm.kmeans_pp_restated(x, k, u, L).tolist()
        assert np.array_equal(st.mind, np.rint(st.mind)) and st.total == float(int(st.total))
        if distinct:
            assert st.total == 0.0 and len(set(st.idx[:distinct])) == distinct  # then the zero-total branch, k - distinct times
        if k == n:
            assert sorted(st.idx) == list(range(n))


@pytest.mark.parametrize("n,d,k,L", [(4097, 9, 16, 12), (2049, 1024, 6, 12)])
def test_planted_uniforms_land_where_they_are_meant_to(n, d, k, L):
    x = kec.rows_pp(n, d)
    u, picks, log = kec.planted_run(x, k, L)
    assert sorted(log) == sorted(kec.planted_plan(n)) and u.shape == (1 + (k - 1) * L,) and np.all((u >= 0) & (u < 1))
    st = okm.KmeansPPStepper(x, L)
    st.first(u[0])
    for t in range(1, k):
        ut = u[1 + (t - 1) * L: 1 + t * L]
        cs = st.cumsum
        if t in log and log[t][0] == "on":
            i = log[t][1]
            assert np.all(ut * cs[-1] == cs[i]) and cs[-1] < 2 ** 53
            first_above = int(np.searchsorted(cs, cs[i], side="right"))
            assert first_above > i and np.all(st.candidates(ut) == min(first_above, n - 1))
        if t in log and log[t][0] == "const":
            want = int(np.argmax(cs > 0)) if log[t][1] == 0.0 else int(np.nonzero(np.diff(np.concatenate([[0.0], cs])) > 0)[0][-1])
            assert np.all(st.candidates(ut) == want)
        st.step(ut)
    assert st.idx == picks.tolist()
    assert okm.kmeans_pp_restated(x, k, u, L).tolist() == picks.tolist() if n * d * L < 4_000_000 else True


def test_exact_1d_cases_contain_what_they_are_for():
    """long trajectories, midpoints that are a data value, empty runs: conditions on the inputs, from the restated starts"""
    steps, hits, empty = {}, {}, {}
    for name, k in (("gauss", 64), ("gauss", 256), ("gauss", 1000), ("outlier", 256), ("discrete32", 256), ("twovalued", 256)):
        s = kec.sorted_1d(name)
        for mode in (0, 1):
            traj, fixed = kec.trajectory(s, okm._k1_start(s.xs, k, mode))
            steps[name, k, mode] = fixed
            hits[name, k, mode] = sum(kec.midpoint_hits(s, c) for c in traj)
            empty[name, k, mode] = int(np.count_nonzero(np.diff(s.bounds(traj[-1])) == 0))
            assert all(np.all(np.diff(c) >= 0) for c in traj)
    assert min(steps["gauss", 64, 0], steps["gauss", 64, 1]) >= 20 and max(steps["gauss", 256, 0], steps["gauss", 256, 1]) >= 20
    assert max(steps.values()) < kec.T_CAP                                     # every trajectory is followed to its end
    assert hits["gauss", 1000, 0] >= 1 and hits["gauss", 1000, 1] >= 1
    assert empty["gauss", 1000, 1] >= 1 and empty["outlier", 256, 0] >= 1 and empty["outlier", 256, 1] >= 100
    assert empty["discrete32", 256, 0] >= 256 - 32 and empty["twovalued", 256, 1] >= 254
    # duplicate centroids (for the labels' "first of the duplicates" rule) and both outcomes of the winner rule, by a margin
    # that the last bit of a cube root in the start cannot turn
    s = kec.sorted_1d("twoclose")
    assert np.count_nonzero(np.diff(okm._k1_start(s.xs, 256, 0)) == 0) >= 100
    wins = {}
    for name, k in kec.WINNER_RUNS:
        s = kec.sorted_1d(name)
        a, b = (okm.kmeans1d_lloyd_from(s, okm._k1_start(s.xs, k, mode), 50)[2] for mode in (0, 1))
        assert a == b == 0.0 or abs(a - b) > 1e-2 * max(a, b)
        wins[name, k] = 2 if b < a else 1
    assert wins == kec.WINNER_RUNS
