"""What tests/test_limit_host.py and tests/test_limit_gpu.py share, computed on the CPU: raw u32 key arrays that each exercise one
part of the radix select, the budgets to cut them at, survivor lists, and splat tables whose metrics are NaN, infinite, zero
and denormal."""
import numpy as np

import transform_cases as tc

SIZES = (1, 2, 255, 256, 257, 2047, 2048, 2049, 5000)
KEY_NAN, KEY_POS_INF_METRIC, KEY_NEG_INF_METRIC = 0xffffffff, 0x007fffff, 0xff800000    # sort_key(-m) for m = NaN, +inf, -inf
TIE_FIRST, TIE_LAST = 2038, 2058                        # the block of 21 equal keys: across row 2048, a tile and a workgroup


def key_cases(n: int, seed: int = 0) -> dict:
    """{name: uint32[n]}"""
    rng = np.random.default_rng(977 * n + seed)
    u32 = lambda a: np.asarray(a, dtype=np.uint64).astype(np.uint32)      # noqa: E731
    rand = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    out = {
        "all_equal": u32(np.full(n, 0x3f8ccccd)),                          # the whole answer is the tie rule
        "two_values": u32(np.where(rng.integers(0, 2, n) == 1, 0x80000001, 0x40000000)),
        "low_byte": u32(0xc1d2e300 | (rand & 0xff)),                       # every pass must run
        "top_byte": u32((rand & 0xff) << 24 | 0x00abcdef),
        "random": u32(rand),
        "few_values": u32(rng.choice(np.array([0, 1, 0x00ffffff, 0x01000000, 0x7fffffff, 0x80000000, 0xfffffffe, 0xffffffff], np.uint64), n)),
    }
    special = u32(rand)
    special[rng.integers(0, n, max(1, n // 5))] = KEY_NAN
    special[rng.integers(0, n, max(1, n // 7))] = KEY_POS_INF_METRIC
    special[rng.integers(0, n, max(1, n // 9))] = KEY_NEG_INF_METRIC
    out["nan_and_inf"] = special
    if n > TIE_LAST + 1:
        out["tie_block"] = tie_block(n, rng)
    return out


TIE_KEY, TIE_BELOW = 0x80000000, 1500                   # the block's key; how many other rows have a smaller key


def tie_block(n: int, rng) -> np.ndarray:
    """21 rows with TIE_KEY at rows TIE_FIRST..TIE_LAST; of the other rows exactly TIE_BELOW have a smaller key, the rest a larger"""
    others = n - (TIE_LAST - TIE_FIRST + 1)
    small = rng.integers(0, TIE_KEY, TIE_BELOW, dtype=np.uint64)
    large = rng.integers(TIE_KEY + 1, 1 << 32, others - TIE_BELOW, dtype=np.uint64)
    rest = rng.permutation(np.concatenate([small, large])).astype(np.uint32)
    keys = np.empty(n, np.uint32)
    keys[:TIE_FIRST] = rest[:TIE_FIRST]
    keys[TIE_FIRST:TIE_LAST + 1] = TIE_KEY
    keys[TIE_LAST + 1:] = rest[TIE_FIRST:]
    return keys


def budgets(name: str, n: int):
    """the budgets a key case is cut at; the tie block: the last row kept is row 2047, 2048 and 2049 as well"""
    out = {1, 2, n // 2, n - 1, n}
    if name == "tie_block":
        out |= {TIE_BELOW + (last - TIE_FIRST + 1) for last in (2047, 2048, 2049)}
    return sorted(N for N in out if N >= 1)


def survivor_list(n0: int, n: int, seed: int = 0) -> np.ndarray:
    """a random ascending subset of range(n0) of size n, as the chain's survivor list"""
    return np.sort(np.random.default_rng(31 * n0 + n + seed).choice(n0, n, replace=False)).astype(np.uint32)


# (scale_0, scale_1, scale_2, opacity) and what the row's metric is
PLANTED = [
    ((0.0, 0.0, 0.0, np.inf), "1: the sigmoid of +inf"),
    ((0.0, 0.0, 0.0, -np.inf), "+0: 1 / (1 + inf)"),
    ((0.0, 0.0, 0.0, np.nan), "NaN"),
    ((30.0, 30.0, 30.0, 0.0), "+inf: a scale sum above 88.72"),
    ((30.0, 30.0, 30.0, -np.inf), "NaN: inf * 0"),
    ((-40.0, -40.0, -30.0, 0.0), "+0: a scale sum below -104"),
    ((-30.0, -30.0, -30.0, 0.0), "denormal: exp(-90) / 2"),
    ((-30.0, -30.0, -35.0, 2.0), "denormal: exp(-95) * 0.88"),
    ((1.0, 2.0, 3.0, 100.0), "exp(6): exp(-100) is denormal and vanishes in 1 + e"),
    ((1.0, 2.0, 3.0, -100.0), "+0: exp(100) is inf"),
    ((0.0, 0.0, 0.0, 0.0), "0.5"),
    ((0.25, -0.25, 0.0, 0.0), "0.5 again: a tie"),
    ((-0.0, 0.0, -0.0, -0.0), "0.5 again"),
]


def table(stride: int, n: int, seed: int = 0) -> np.ndarray:
    """transform_cases.table (its edge rows in front: zeros, denormals, huge values, NaN and infinity in every scale field) with
    the PLANTED rows written over the last rows, as many as fit"""
    t = tc.table(stride, n, seed)
    for k, (vals, _) in enumerate(PLANTED[:n]):
        for nm, v in zip(("scale_0", "scale_1", "scale_2", "opacity"), vals):
            t[nm][n - 1 - k] = np.float32(v)
    return t
