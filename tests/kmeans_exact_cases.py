"""Inputs of tests/test_kmeans_exact_gpu.py: values and rows on which every sum the kernels of csrc/kmeans1d.hip and
csrc/kmeans_pp.hip form is exact, so that the device must equal oracle/kmeans.py's float64 restatements on every bit whatever
its order of summation.  CPU only; tests/test_kmeans1d_oracle.py asserts without a GPU what these inputs promise (exact sums,
long trajectories, midpoints that hit a value, empty runs)."""
import numpy as np

from oracle import kmeans as okm

LIM = okm.EXACT_1D_LIMIT - 1


def _grid(x) -> np.ndarray:
    """to the 2^-10 grid (as integers), clipped inside +-2^5"""
    return np.clip(np.rint(np.asarray(x, dtype=np.float64) * 1024.0), -LIM, LIM).astype(np.int64)


def _gauss(n, seed=11):
    return _grid(np.random.default_rng(seed).standard_normal(n) * 4.0)


def _bimodal(r):
    return _grid(np.concatenate([r.standard_normal(25000) * 0.2 - 3, r.standard_normal(25000) * 2 + 1]))


def _outlier(r):
    return _grid(np.concatenate([r.standard_normal(9990) * 0.1, r.standard_normal(10) * 50]))


# name -> (integers m of the values m * 2^-10, zeros written as -0.0)
ONE_D = {
    "gauss": lambda: (_gauss(50000), False),
    "bimodal": lambda: (_bimodal(np.random.default_rng(12)), False),
    "outlier": lambda: (_outlier(np.random.default_rng(13)), False),
    "discrete32": lambda: ((np.random.default_rng(14).integers(0, 32, 50000) - 16) * 768, True),   # 32 levels, -12 ... 11.25
    "twovalued": lambda: (np.where(np.random.default_rng(15).random(4097) < 0.4, -3 * 1024, 5 * 1024 + 1), False),
    "twoclose": lambda: (np.where(np.random.default_rng(16).random(4097) < 0.5, 8192, 8193), False),   # 8 and 8 + 2^-10: starts
                                                                          # whose neighbours round to one float32 (duplicates)
    "constant": lambda: (np.full(1025, 2560, dtype=np.int64), False),
    "n1": lambda: (_gauss(1, 21), False),
    "n2": lambda: (_gauss(2, 22), False),
    "n63": lambda: (_gauss(63, 23), False),
    "n1023": lambda: (_gauss(1023, 24), False),
    "n1024": lambda: (_gauss(1024, 25), False),
    "n1025": lambda: (np.concatenate([_gauss(1020, 26), np.zeros(5, np.int64)]), True),
    "n4097": lambda: (_gauss(4097, 27), False),
    "big": lambda: (_gauss(263169, 28), False),     # 257 full prefix tiles + 1 value: the tile scan's second chunk of 256
}

# (case, k): every n edge and every k edge at least once, the product's k = 256 on every case
ONE_D_RUNS = [
    ("gauss", 64), ("gauss", 256), ("gauss", 1000),
    ("bimodal", 256), ("bimodal", 65),
    ("outlier", 256), ("outlier", 1024),
    ("discrete32", 256), ("discrete32", 63),
    ("twovalued", 256), ("twovalued", 2),
    ("twoclose", 256),
    ("constant", 256), ("constant", 1),
    ("n1", 256), ("n1", 1),
    ("n2", 256), ("n2", 2),
    ("n63", 256), ("n63", 64),
    ("n1023", 256), ("n1023", 1024),
    ("n1024", 256),
    ("n1025", 256), ("n1025", 1000),
    ("n4097", 256), ("n4097", 1),
    ("big", 256),
]
T_CAP = 120          # no trajectory is followed further than this many steps


def values_1d(name: str) -> np.ndarray:
    m, negz = ONE_D[name]()
    return okm.exact_values_1d(np.asarray(m, dtype=np.int64), negative_zero=negz)


def sorted_1d(name: str) -> "okm.K1Sorted":
    """what the device's sort makes of the values (-0.0 becomes +0.0: csrc/kmeans1d.hip:k1_key)"""
    x = values_1d(name)
    return okm.K1Sorted(np.sort(x + np.float32(0.0)))


def midpoint_hits(s: "okm.K1Sorted", c: np.ndarray) -> int:
    """how many midpoints of neighbouring, different centroids are a data value: where `side="right"` and the device's
    `xs[mid] > t` decide which run a value belongs to"""
    mid = (c[:-1].astype(np.float64) + c[1:].astype(np.float64)) * 0.5
    mid = mid[c[:-1] != c[1:]]
    i = np.searchsorted(s.x64, mid, side="left")
    return int(np.count_nonzero((i < s.n) & (s.x64[np.minimum(i, s.n - 1)] == mid)))


def trajectory(s: "okm.K1Sorted", start: np.ndarray, cap: int = T_CAP):
    """centroids after 0, 1, ... steps up to two past the first step that moves no boundary (or cap), and that step's number"""
    fixed = okm.kmeans1d_steps_until_fixed(s, start, cap)
    out = [np.ascontiguousarray(start, dtype=np.float32)]
    for _ in range(min(fixed + 2, cap)):
        out.append(s.step(out[-1]))
    return out, fixed


# ---- rows of the k-means++ tests: (n, d, k, L, distinct rows or None) ------------------------------------------------
PP_SHAPES = [
    (1, 7, 1, 1, None),
    (1025, 3, 200, 1, None),
    (1024, 1, 64, 6, None),
    (4097, 9, 16, 12, None),
    (5000, 45, 64, 6, None),
    (300, 300, 300, 7, None),
    (2049, 1024, 6, 12, None),
    (257, 5, 40, 4, 10),
]


def rows_pp(n: int, d: int, distinct=None, seed: int = 0) -> np.ndarray:
    r = np.random.default_rng(1000 * n + d + seed)
    if distinct is None:
        return okm.exact_rows_pp(r.integers(-15, 16, (n, d)))
    while True:
        base = r.integers(-15, 16, (distinct, d))
        if len(np.unique(base, axis=0)) == distinct:
            break
    which = np.concatenate([np.arange(distinct), r.integers(0, distinct, n - distinct)])
    return okm.exact_rows_pp(base[r.permutation(which)])


def uniform_on_cumsum(cs: np.ndarray, i: int) -> float:
    """a uniform u in [0, 1) with fl(u * total) == cs[i] exactly: the target lies ON a cumulative sum, where
    searchsorted(side="right") and the device's strict `>` must both move on to the next row with a positive distance"""
    total = float(cs[-1])
    q = float(cs[i]) / total
    for u in (q, float(np.nextafter(q, 0.0)), float(np.nextafter(q, 1.0))):
        if 0.0 <= u < 1.0 and u * total == float(cs[i]):
            return u
    raise AssertionError("no uniform lands on cumsum[%d]" % i)


U_LAST = 1.0 - 2.0 ** -53      # the largest double below 1


def planted_plan(n: int) -> dict:
    """step -> what its L uniforms are: ("on", i) all on cumsum[i], ("const", u) all u, ("twins",) random with trial 0 repeated
    as trials 1 and L - 1.  Steps not named draw from the stream."""
    if n == 4097:
        plan = {1 + j: ("on", i) for j, i in enumerate([0, 511, 1022, 1023, 1024, 2047])}
        plan.update({7: ("const", 0.0), 8: ("const", U_LAST), 9: ("twins",), 10: ("on", 3071)})
        return plan
    if n == 2049:
        return {1: ("on", 1023), 2: ("on", 2047), 3: ("const", 0.0), 4: ("const", U_LAST), 5: ("twins",)}
    return {}


def planted_run(x: np.ndarray, k: int, L: int, seed: int = 5):
    """the stepper's picks with uniforms planted by planted_plan(len(x)) -> (uniforms, picks, what was planted per step)"""
    r = np.random.default_rng(seed)
    st = okm.KmeansPPStepper(x, L)
    u = [float(r.random())]
    st.first(u[0])
    plan, log = planted_plan(len(x)), {}
    for t in range(1, k):
        ut = r.random(L)
        what = plan.get(t)
        if what and st.total > 0:
            if what[0] == "on":
                ut = np.full(L, uniform_on_cumsum(st.cumsum, what[1]))
            elif what[0] == "const":
                ut = np.full(L, what[1])
            else:
                ut[1] = ut[L - 1] = ut[0]
            log[t] = what
        st.step(ut)
        if what and what[0] == "twins" and t in log:
            assert st.cand[0] == st.cand[1] == st.cand[L - 1] and st.pots[0] == st.pots[1] == st.pots[L - 1]
        u.extend(ut.tolist())
    return np.asarray(u), np.asarray(st.idx), log


# (case, k) -> the start that wins after 50 steps (1 = uniform bins, 2 = equal-count bins; equal inertia: the first)
WINNER_RUNS = {("gauss", 256): 2, ("outlier", 256): 1, ("bimodal", 65): 2, ("n63", 64): 1, ("discrete32", 256): 1, ("twovalued", 2): 1}
