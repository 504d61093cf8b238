"""Seeded inputs for the pieces beneath every SOR mean distance (csrc/knn_common.h): the float64 root and the order of the
float64 additions of a row.  CPU only; tests/test_epilogue_cases_host.py checks the generator, tests/test_knn_epilogue_gpu.py
feeds its output to the device functions through gsx_knn_probe_*_dev.

Why crafted inputs: a mean distance is (float)(sum of k float64 roots / k).  A root that is one float64 ulp off, or another
order of the additions, moves the float64 sum by about one ulp, and that moves the float32 result only if the quotient lies
within ~2^-29 (relative) of a float32 rounding boundary -- on an ordinary cloud, a few rows in ten million.  Here EVERY
row's exact sum is k times the midpoint of two adjacent float32 values, to within a fraction of a float64 ulp, so the side
the float32 result falls on is decided by the order of the additions."""
import functools
import math

import numpy as np

# the squared distance of two float32 points is 0 or lies in [2^-298, 2^260): coordinates differ by at least 2^-149 and
# by less than 2^129, three squares are added
ROOT_MIN_EXP, ROOT_MAX_EXP = -298, 260

NET, LIST, LE128, NP = 0, 1, 2, 3                      # gsx_knn_probe_mean_dev forms (include/gsx_hip.h)
NET_LENGTHS = (8, 12, 16, 20, 24, 28, 32, 36, 40, 44, 48, 52, 56, 64)     # TopNet<L>: dispatch_bricks, launch_knn_tree
LIST_CAPS = {9: (1, 8), 17: (9, 16), 26: (17, 25), 33: (17, 26, 32), 51: (33, 50), 65: (33, 51, 64)}   # TopList<KCAP>: the k at
# both edges of the capacity in dispatch_bricks (phase2_net = 0: 9, 17, 26, 33, 51, 65) and launch_knn_brute (9, 17, 33, 65)
LE128_K = (7, 8, 9, 15, 16, 17, 63, 64, 65, 120, 127, 128)
NP_K = (129, 136, 255, 256, 257, 300, 1000)             # 300 and 1000 split irregularly (150 -> 144 + 156, 500 -> 496 + 504)
EXTRA_COLS = 2                                         # further neighbours behind the k a row is summed over


def mean_cases():
    """every (form, cap, k) the GPU test runs"""
    out = [(NET, 8, 2), (NET, 8, 3), (LIST, 9, 2), (LIST, 9, 3), (LE128, 0, 2), (LE128, 0, 3)]    # the k < 8 branches besides k = 1, 7
    prev = 0
    for L in NET_LENGTHS:                                # k = L and the smallest k that selects this L
        out += [(NET, L, prev + 1), (NET, L, L)]
        prev = L
    for cap, ks in LIST_CAPS.items():
        out += [(LIST, cap, k) for k in ks]
    out += [(LE128, 0, k) for k in LE128_K] + [(NP, 0, k) for k in NP_K]
    return out


def _bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def _round_to_double_bits(n: int, scale: int) -> int:
    """bit pattern of RN(n * 2^scale) for a positive integer n (normal range only)"""
    shift = n.bit_length() - 53
    if shift > 0:
        q, rem, half = n >> shift, n & ((1 << shift) - 1), 1 << (shift - 1)
        if rem > half or (rem == half and (q & 1)):
            q += 1
            if q == 1 << 53:
                q >>= 1
                shift += 1
    else:
        q = n << -shift
    e = shift + scale + 52
    assert -1022 <= e <= 1023
    return ((e + 1023) << 52) | (q - (1 << 52))


@functools.lru_cache(maxsize=None)
def hard_root_block(seed: int = 20240607) -> np.ndarray:
    """Roots next to a rounding boundary, as (n, 8) float64 bit patterns.  A square root is never an exact tie, but it comes
    arbitrarily close: for a double y = M * 2^e (M its 53-bit significand) and h half its ulp, (y + h)^2 =
    (2M + 1)^2 * 2^(2e - 2) exactly.  Columns 0 ... 4: that square rounded once, moved by -2 ... +2 ulps; columns 5 ... 7:
    RN(y^2) moved by -1, 0, +1.  1024 draws of y in every binade [2^E, 2^(E+1)) whose squares lie in the domain."""
    rng = np.random.default_rng([seed, 1])
    hard = []
    for E in range(ROOT_MIN_EXP // 2, ROOT_MAX_EXP // 2):
        e = E - 52
        for M in rng.integers(1 << 52, 1 << 53, 1024, dtype=np.uint64).tolist():
            b = _round_to_double_bits((2 * M + 1) ** 2, 2 * e - 2)
            c = _round_to_double_bits(M * M, 2 * e)
            hard.append((b - 2, b - 1, b, b + 1, b + 2, c - 1, c, c + 1))
    return np.array(hard, np.uint64)


def _sqrt_mod_pow2(c: int, nbits: int):
    """the four square roots of c modulo 2^nbits (c = 1 mod 8), by lifting one bit at a time"""
    s = 1
    for j in range(3, nbits):
        if (s * s - c) % (1 << (j + 1)):
            s += 1 << (j - 1)
    mod = 1 << nbits
    return sorted({s % mod, -s % mod, (s + mod // 2) % mod, (-s + mod // 2) % mod})


TIE_RESIDUE_MAX = 1 << 13


@functools.lru_cache(maxsize=None)
def nearest_tie_significands():
    """Odd 54-bit integers s = 2M + 1 whose square lies within TIE_RESIDUE_MAX units of a multiple of the 2^54 or 2^55 that
    rounding to 53 bits cuts off: s^2 = q * 2^shift + c with |c| <= 2^13.  With y + h = s * 2^(e-1) as in hard_root_block,
    x = q * 2^(shift + 2e - 2) is a double whose exact root is (y + h) * (1 - c / (2 s^2)): 2^-55 ... 2^-42 of an ulp from
    the midpoint of two doubles, |c| = 1, 7, 9, 15 ... -- the nearest a root of a double comes to a tie.  (Random draws, as
    in hard_root_block, come no nearer than 2^-19 ulp in 285 000 tries; a root routine whose last correction step is missing
    passes those.)  Returns (s, c) pairs."""
    out = []
    for c in range(1 - TIE_RESIDUE_MAX, TIE_RESIDUE_MAX + 1, 8):       # c = 1 (mod 8), either sign: odd squares are 1 mod 8
        for nbits in (54, 55):
            for s in _sqrt_mod_pow2(c, nbits):
                if (1 << 53) <= s < (1 << 54) and (s * s).bit_length() - 53 == nbits:
                    out.append((s, c))
    return out


@functools.lru_cache(maxsize=None)
def nearest_tie_block() -> np.ndarray:
    """float64 bit patterns (n, binades) of the doubles nearest_tie_significands() describes, at every binade pair of the domain"""
    sig = nearest_tie_significands()
    e0 = -52
    base = np.array([_round_to_double_bits(s * s - c, 2 * e0 - 2) for s, c in sig], np.uint64)     # y in [1, 2)
    E = np.arange(ROOT_MIN_EXP // 2, ROOT_MAX_EXP // 2, dtype=np.int64)
    return (base[:, None].astype(np.int64) + ((2 * E) << 52)[None, :]).astype(np.uint64)


@functools.lru_cache(maxsize=None)
def root_inputs(seed: int = 20240607) -> np.ndarray:
    """float64 inputs of the root, every one 0 or in [2^-298, 2^260) (about 4.3M values)"""
    rng = np.random.default_rng([seed, 0])
    lo_bits = int(_bits(math.ldexp(1.0, ROOT_MIN_EXP)))
    hi_bits = int(_bits(math.ldexp(1.0, ROOT_MAX_EXP)))          # exclusive
    parts = [np.array([0, lo_bits, lo_bits + 1, hi_bits - 1], np.uint64)]
    # every binade: 2048 random mantissas, all zeros, all ones, 1 + ulp
    exps = np.arange(ROOT_MIN_EXP, ROOT_MAX_EXP, dtype=np.int64) + 1023
    mant = rng.integers(0, 1 << 52, (len(exps), 2048), dtype=np.uint64)
    mant = np.concatenate([mant, np.tile(np.array([0, (1 << 52) - 1, 1], np.uint64), (len(exps), 1))], axis=1)
    parts.append(((exps.astype(np.uint64) << np.uint64(52))[:, None] | mant).ravel())
    parts.append(hard_root_block(seed).ravel())
    parts.append(nearest_tie_block().ravel())
    # exact squares of 26-bit values (the root is exact), at every even power of two the domain holds
    v = rng.integers(1 << 25, 1 << 26, 1 << 16, dtype=np.int64)
    s = rng.integers(ROOT_MIN_EXP // 2 - 25, ROOT_MAX_EXP // 2 - 26 + 1, len(v))      # (v 2^s)^2 in [2^-298, 2^260)
    parts.append(_bits(np.ldexp((v * v).astype(np.float64), 2 * s)))
    x = np.concatenate(parts)
    x = x[(x == 0) | ((x >= lo_bits) & (x < hi_bits))]          # the +-ulp moves at the two ends of the domain
    return x.view(np.float64)


# ---- the orders a row's roots can be added in (b: (m, k) float64, one row per query; returns the (m,) float64 sums) ----
def sum_left_to_right(b):
    acc = np.zeros(len(b))
    for j in range(b.shape[1]):
        acc = acc + b[:, j]
    return acc


def sum_right_to_left(b):
    return sum_left_to_right(b[:, ::-1])


def sum_balanced_tree(b):
    n = b.shape[1]
    if n == 1:
        return b[:, 0].copy()
    return sum_balanced_tree(b[:, :n // 2]) + sum_balanced_tree(b[:, n // 2:])


def _sum_accumulators(b, lanes: int, tail: bool):
    """numpy's leaf with `lanes` accumulators; tail=False folds the last n % lanes entries into the accumulators too"""
    n = b.shape[1]
    if n < lanes:
        return sum_left_to_right(b)
    r = [b[:, j].copy() for j in range(lanes)]
    full = n - n % lanes if tail else n
    for j in range(lanes, full):
        r[j % lanes] = r[j % lanes] + b[:, j]
    while len(r) > 1:
        r = [r[i] + r[i + 1] for i in range(0, len(r), 2)]
    res = r[0]
    for j in range(full, n):
        res = res + b[:, j]
    return res


def sum_four_accumulators(b):
    return _sum_accumulators(b, 4, True)


def sum_eight_no_tail(b):
    """numpy's order but for the sequential tail: the last k % 8 entries of a leaf go into the 8 accumulators (what
    mean_from_net's k == L branch would compute if it were taken for a k that is no multiple of 8)"""
    n = b.shape[1]
    if n <= 128:
        return _sum_accumulators(b, 8, False)
    n2 = n // 2
    n2 -= n2 % 8
    return sum_eight_no_tail(b[:, :n2]) + sum_eight_no_tail(b[:, n2:])


def sum_numpy_restated(b):
    """numpy's pairwise order written out (8 accumulators, sequential tail, halves rounded down to a multiple of 8 above 128)"""
    n = b.shape[1]
    if n <= 128:
        return _sum_accumulators(b, 8, True)
    n2 = n // 2
    n2 -= n2 % 8
    return sum_numpy_restated(b[:, :n2]) + sum_numpy_restated(b[:, n2:])


OTHER_ORDERS = (sum_left_to_right, sum_right_to_left, sum_balanced_tree, sum_four_accumulators)


def mean_f32(sums, k):
    out = np.zeros(len(sums), np.float32)
    out[:] = sums / k
    return out


def reference_means(d2, k):
    """the reference's own expression (data_processor.py:172 on cKDTree's distance matrix), evaluated by the running numpy"""
    m = len(d2)
    D = np.zeros((m, k + 1))
    D[:, 1:] = np.sqrt(d2[:, :k])
    out = np.zeros(m, np.float32)
    out[:] = np.mean(D[:, 1:], axis=1)
    return out


def _draw_d2(rng, m, n):
    """squared distances with exponents spread over 2^-40 ... 2^16"""
    return np.ldexp(1.0 + rng.random((m, n)), rng.integers(-40, 16, (m, n)))


def _leading_zeros(rng, head, k):
    """1 ... 3 leading zeros (duplicate points) in every 4th row"""
    m = len(head)
    zeros = rng.integers(1, min(4, k), m)
    for z in range(1, min(4, k)):
        head[(np.arange(m) % 4 == 3) & (zeros >= z), z - 1] = 0.0


def _complete_rows(head, mid, k):
    """the k-th root t = k * mid - sum(roots of head), exact and rounded once, as a squared distance whose np.sqrt is t;
    rows for which no such double exists are dropped.  Returns the sorted (m', k) squared distances."""
    b = np.sqrt(head)
    last = np.zeros(len(head))
    ok = np.zeros(len(head), bool)
    for i in range(len(head)):
        t = math.fsum([k * float(mid[i])] + (-b[i]).tolist())     # k * mid is exact (25 + 10 bits); fsum rounds the exact sum once
        if not t > 0:
            continue
        for cand in (t * t, np.nextafter(t * t, 0.0), np.nextafter(t * t, np.inf)):
            if np.sqrt(cand) == t:
                last[i], ok[i] = cand, True
                break
    return np.sort(np.concatenate([head, last[:, None]], axis=1)[ok], axis=1)


def _midpoint_above(lo):
    """exact midpoint of the float32 lo and the next float32"""
    return (lo.astype(np.float64) + np.nextafter(lo, np.float32(np.inf)).astype(np.float64)) / 2


@functools.lru_cache(maxsize=None)
def rows_for_k(k: int, seed: int = 20240608) -> dict:
    """Candidate rows of length k: d2 (m, k + EXTRA_COLS) ascending float64 squared distances (the last EXTRA_COLS are
    further neighbours that no sum may read), want (m,) float32 = the reference's expression, kept (m,) = numpy's result
    differs from another order's on this row, no_tail (m,) = it differs from sum_eight_no_tail's, level (m,) = the row is
    of the second family.  Every row is a valid input, kept or not; the counts of kept rows are what
    tests/test_epilogue_cases_host.py asserts.

    Two families, interleaved.  Spread rows: k - 1 roots between 2^-20 and 2^8 and a last root near k * 768 that brings the
    sum to k * mid, mid the midpoint of two float32 in [2^9, 2^10) -- the last root dominates, so what shows is where IT
    enters the sum (accumulator, tail, which half of a split).  Level rows: every root in [2^9, 2^10), the completing
    one included, so that one float64 ulp lost anywhere among the k - 1 additions shows."""
    rng = np.random.default_rng([seed, k])
    if k <= 2:       # nothing to reorder (k = 1) or no order that differs (k = 2: one addition): the root, the divide and the cast
        m = 256
        d2 = np.sort(_draw_d2(rng, m, k), axis=1)
        d2[1::8, 0] = 0.0                                       # a duplicate point
        level = np.zeros(m, bool)
    else:
        m = 512 if k < 16 else (256 if k <= 128 else 192)
        head = _draw_d2(rng, m, k - 1)
        _leading_zeros(rng, head, k)
        head.sort(axis=1)
        lo = rng.integers(0x44000000, 0x44800000 - 1, m, dtype=np.int64).astype(np.uint32).view(np.float32)   # [2^9, 2^10)
        spread = _complete_rows(head, _midpoint_above(lo), k)
        # level rows: the float32 pair is the one around (sum of the k - 1 roots + a k-th drawn like them) / k
        head = np.ldexp(1.0 + rng.random((m, k - 1)), 18 + rng.integers(0, 2, (m, k - 1)))      # roots in [2^9, 2^10)
        _leading_zeros(rng, head, k)
        head.sort(axis=1)
        est = (np.sqrt(head).sum(axis=1) + 512.0 * (1.0 + rng.random(m))) / k
        lo = est.astype(np.float32)
        lo = np.where(lo.astype(np.float64) > est, np.nextafter(lo, np.float32(0)), lo)
        lev = _complete_rows(head, _midpoint_above(lo), k)
        n = min(len(spread), len(lev))
        d2 = np.empty((2 * n, k))
        d2[0::2], d2[1::2] = spread[:n], lev[:n]
        m = 2 * n
        level = np.arange(m) % 2 == 1
    further = d2[:, -1:] * (1.0 + np.arange(1, EXTRA_COLS + 1))      # ascending, finite, and ruinous if a sum read them
    d2 = np.ascontiguousarray(np.concatenate([d2, further], axis=1))
    want = reference_means(d2, k)
    b = np.sqrt(d2[:, :k])
    kept = np.zeros(m, bool)
    for order in OTHER_ORDERS:
        kept |= mean_f32(order(b), k).view(np.uint32) != want.view(np.uint32)
    no_tail = mean_f32(sum_eight_no_tail(b), k).view(np.uint32) != want.view(np.uint32)
    return {"k": k, "d2": d2, "want": want, "kept": kept, "no_tail": no_tail, "level": level}
