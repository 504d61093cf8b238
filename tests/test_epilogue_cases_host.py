"""-m "not gpu": the generator of tests/test_knn_epilogue_gpu.py's inputs (tests/epilogue_cases.py).  Its rows are only worth
running if the running numpy's result on them differs from what another order of the float64 additions gives, and its root
inputs only if they stay inside the domain sqrt_rn_dist2 is defined on -- both are asserted here, without a GPU."""
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import epilogue_cases as ec
from oracle import clib

CASES = ec.mean_cases()
ALL_K = sorted({k for _, _, k in CASES})


def test_cases_cover_every_instantiated_form():
    nets = {cap for f, cap, _ in CASES if f == ec.NET}
    lists = {cap for f, cap, _ in CASES if f == ec.LIST}
    assert nets == set(ec.NET_LENGTHS) and lists == set(ec.LIST_CAPS)
    for f, cap, k in CASES:
        if f == ec.NET:     # dispatch_bricks: the list length is the next multiple of 4 (8 at the least), 64 above 56
            assert cap == (64 if k > 56 else max(8, -(-k // 4) * 4)), (cap, k)
        if f == ec.LIST:
            assert 1 <= k <= cap - 1
    assert {k for f, _, k in CASES if f == ec.LE128} == set(ec.LE128_K) | {2, 3}
    assert {k for f, _, k in CASES if f == ec.NP} == set(ec.NP_K)


def test_forms_are_the_ones_the_kernels_instantiate():
    """the list lengths and capacities above, and the ones csrc/knn_probe.hip accepts, read out of the dispatchers: a new
    capacity in dispatch_bricks, launch_knn_tree or launch_knn_brute has to reach the probe and these tests"""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "3dgsconverter_amd", "csrc")
    src = {f: re.sub(r"//[^\n]*", "", open(os.path.join(csrc, f + ".hip")).read()) for f in ("sor_grid", "sor_tree", "sor_brute", "knn_probe")}
    body = src["sor_grid"][src["sor_grid"].index("static int dispatch_bricks"):]
    body = body[:body.index("static int dispatch_ring")]
    net_part, list_part = body.split("#undef GSX_BRICKS")[:2]
    nets = {int(v) - 1 for v in re.findall(r"GSX_BRICKS\((\d+)\)", net_part)} | {int(v) - 1 for v in re.findall(r"launch_bricks<(\d+), true, true, true>", body)}
    nets |= {int(v) - 1 for v in re.findall(r"GSX_LEAVES\((\d+)\)|launch_leaves<(\d+)>", src["sor_tree"]) for v in v if v}
    lists = {int(v) for v in re.findall(r"GSX_BRICKS\((\d+)\)", list_part)} | {int(v) for v in re.findall(r"launch_brute_t<(\d+),", src["sor_brute"])}
    assert nets == set(ec.NET_LENGTHS) and lists == set(ec.LIST_CAPS)
    assert {int(v) for v in re.findall(r"GSX_PROBE_NET\((\d+)\)", src["knn_probe"])} == nets
    assert {int(v) for v in re.findall(r"GSX_PROBE_LIST\((\d+)\)", src["knn_probe"])} == lists


def test_root_inputs_stay_in_the_domain_and_hit_the_hard_cases():
    x = ec.root_inputs()
    assert len(x) > 3_000_000
    lo, hi = math.ldexp(1.0, ec.ROOT_MIN_EXP), math.ldexp(1.0, ec.ROOT_MAX_EXP)
    assert ((x == 0) | ((x >= lo) & (x < hi))).all()
    assert (x == 0).any() and (x == lo).any() and (x == np.nextafter(hi, 0.0)).any()
    _, e = np.frexp(x[x > 0])
    assert set(np.unique(e - 1)) == set(range(ec.ROOT_MIN_EXP, ec.ROOT_MAX_EXP))      # every binade of the domain


def test_hard_root_inputs_lie_next_to_a_rounding_boundary():
    """the construction itself, in rational arithmetic: column 2 of the hard block is the double nearest to the square of
    a midpoint of two adjacent doubles, so its exact root is within about 2^-53 ulp of that midpoint"""
    blk = ec.hard_root_block()
    assert blk.shape == ((ec.ROOT_MAX_EXP - ec.ROOT_MIN_EXP) // 2 * 1024, 8)
    assert (np.diff(blk[:, :5].astype(np.int64), axis=1) == 1).all() and (np.diff(blk[:, 5:].astype(np.int64), axis=1) == 1).all()
    for v in blk[::1117, 2].view(np.float64).tolist():
        r = math.sqrt(v)
        half = Fraction(math.ulp(r)) / 2
        assert min(abs(Fraction(v) - (Fraction(r) + s * half) ** 2) for s in (-1, 1)) <= Fraction(math.ulp(v)) / 2, v
    for v in blk[::1117, 6].view(np.float64).tolist():       # RN(y^2): the root is a double to within ~2^-53 ulp
        r = math.sqrt(v)
        assert abs(Fraction(v) - Fraction(r) ** 2) <= Fraction(math.ulp(v)) / 2, v


def test_nearest_tie_inputs_are_that_near():
    """in rational arithmetic: each double of nearest_tie_block is (midpoint of two adjacent doubles)^2 - c * (one unit of
    the 108-bit square), |c| <= 2^13, so its root is within 2^-42 ulp of that midpoint -- and still in the domain"""
    sig = ec.nearest_tie_significands()
    assert len(sig) > 2000 and {abs(c) for _, c in sig} >= {1, 7, 9, 15}
    blk = ec.nearest_tie_block()
    assert blk.shape == (len(sig), (ec.ROOT_MAX_EXP - ec.ROOT_MIN_EXP) // 2)
    x = blk.view(np.float64)
    assert (x >= math.ldexp(1.0, ec.ROOT_MIN_EXP)).all() and (x < math.ldexp(1.0, ec.ROOT_MAX_EXP)).all()
    col = -(ec.ROOT_MIN_EXP // 2)                                     # the column with y in [1, 2)
    for i in range(0, len(sig), 37):
        s, c = sig[i]
        mid = Fraction(s, 1 << 53)                                   # y + h, y = M 2^-52
        v = Fraction(float(x[i, col]))
        assert v == mid * mid - Fraction(c, 1 << 106), (s, c)
        r = math.sqrt(float(x[i, col]))
        assert abs(Fraction(r) - mid) == Fraction(1, 1 << 53)        # the two doubles on either side of the midpoint
        # first-order distance of the exact root from the midpoint, in ulps of the root
        assert abs(Fraction(c, 1 << 106) / (2 * mid)) * (1 << 52) <= Fraction(1, 1 << 41)
    for j in (0, 1, blk.shape[1] - 1):                               # other binades: the same significands, exponents moved
        m0, e0 = np.frexp(x[:, col])
        mj, ej = np.frexp(x[:, j])
        assert (m0 == mj).all() and (ej - e0 == 2 * (j - col)).all()


@pytest.mark.parametrize("k", ALL_K)
def test_rows_tell_summation_orders_apart(k):
    r = ec.rows_for_k(k)
    d2, want = r["d2"], r["want"]
    assert d2.shape[1] == k + ec.EXTRA_COLS and (np.diff(d2, axis=1) >= 0).all() and (d2 >= 0).all() and np.isfinite(d2).all()
    b = np.sqrt(d2[:, :k])
    # the restatement of numpy's order agrees with the running numpy on every row, kept or not ...
    assert (ec.mean_f32(ec.sum_numpy_restated(b), k).view(np.uint32) == want.view(np.uint32)).all()
    # ... and so does the oracle's C restatement (gsxo_pairwise_sum_f64, the row-mean entry of oracle/gsx_oracle.c)
    lib = clib()
    rows = np.ascontiguousarray(b)
    c_sum = np.array([lib.gsxo_pairwise_sum_f64(rows[i].ctypes.data, k) for i in range(len(rows))])
    assert (ec.mean_f32(c_sum, k).view(np.uint32) == want.view(np.uint32)).all()
    if k <= 2:
        assert len(want) == 256 and not r["kept"].any()         # nothing to reorder: plain rows
        return
    assert int(r["kept"].sum()) >= 32, int(r["kept"].sum())
    if k >= 7:      # ... and as many among the level rows alone (all roots of one size: an ulp lost anywhere in the sum shows)
        assert int((r["kept"] & r["level"]).sum()) >= 32, int((r["kept"] & r["level"]).sum())
        lev = np.sqrt(d2[r["level"], :k])
        lev = np.where(lev == 0, np.nan, lev)
        assert np.nanmin(lev) >= 256 and np.nanmax(lev) < 2048
    if k >= 8 and k % 8:
        assert int((r["kept"] & r["no_tail"]).sum()) >= 8, int((r["kept"] & r["no_tail"]).sum())
    assert (d2[:, 0] == 0).any() and (d2[:, 0] > 0).any()       # duplicate points lead some rows
    # a block of 64 rows holds 64 different rows, with and without leading zeros: lanes diverge in the predicated branches
    head = d2[:64]
    assert len(np.unique(head, axis=0)) == 64 and len(np.unique((head == 0).sum(axis=1))) >= 3


def test_crafted_sum_sits_on_a_float32_boundary():
    """the construction itself: the exact sum of a row's roots is k * (midpoint of two adjacent float32) to within one
    float64 ulp of the sum"""
    for k in (7, 16, 65, 300):
        r = ec.rows_for_k(k)
        b = np.sqrt(r["d2"][:, :k])
        for row in b[:32]:
            exact = sum(Fraction(v) for v in row.tolist()) / k
            f = np.float32(float(exact))
            lo = min(f, np.float32(np.nextafter(f, np.float32(0)))) if Fraction(float(f)) > exact else f
            mid = (Fraction(float(lo)) + Fraction(float(np.nextafter(lo, np.float32(np.inf))))) / 2
            assert abs(exact - mid) * k <= Fraction(math.ulp(float(exact) * k)), (k, float(exact))
