"""The splat budget's definition in numpy ("Splat budget"): the metric with the float32 exp of csrc/np_exp.h (its
host twin, _lib.np_exp_host -- not the running numpy's np.exp), the .splat writer's sort key of its negative, and the first N
entries of the stable ascending order of the keys, returned in input order."""
import importlib

import numpy as np

lib = importlib.import_module("3dgsconverter_amd._lib")
F32 = np.float32


def sort_key(v: np.ndarray) -> np.ndarray:
    """csrc/sog_math.h sort_key: float32 -> uint32 whose unsigned order is numpy's sort order (-0 == +0, every NaN last)"""
    v = np.ascontiguousarray(v, dtype=F32).copy()
    v[v == 0] = 0.0                                     # -0.0 -> +0.0
    b = v.view(np.uint32)
    key = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    key[np.isnan(v)] = 0xffffffff
    return key


def sort_unkey(key) -> np.ndarray:
    key = np.asarray(key, dtype=np.uint32)
    return np.where(key & np.uint32(0x80000000), key & np.uint32(0x7fffffff), ~key).astype(np.uint32).view(F32)


def metric(table: np.ndarray) -> np.ndarray:
    """m = E((s0 + s1) + s2) * (1 / (1 + E(-opacity))), every operation float32 in this order"""
    s0, s1, s2, o = (np.ascontiguousarray(table[nm], dtype=F32) for nm in ("scale_0", "scale_1", "scale_2", "opacity"))
    with np.errstate(all="ignore"):
        return lib.np_exp_host((s0 + s1) + s2) * (F32(1) / (F32(1) + lib.np_exp_host(-o)))


def keys(table: np.ndarray) -> np.ndarray:
    with np.errstate(all="ignore"):
        return sort_key(-metric(table))


def kept(key: np.ndarray, N: int) -> np.ndarray:
    """ascending row indices of the N rows a budget of N keeps"""
    return np.sort(np.argsort(key, kind="stable")[:N])


def mask(key: np.ndarray, N: int) -> np.ndarray:
    m = np.zeros(len(key), np.bool_)
    m[kept(key, N)] = True
    return m


def info(key: np.ndarray, N: int):
    """(threshold key, rows with that key that are kept, rows kept) of a non-empty key array"""
    N = min(N, len(key))
    T = np.sort(key, kind="stable")[N - 1]
    return int(T), int(N - np.count_nonzero(key < T)), N


def limit_table(table: np.ndarray, N: int) -> np.ndarray:
    return table[kept(keys(table), N)]
