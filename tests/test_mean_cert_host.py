"""csrc/knn_mean_cert.h on the host: tools/check_mean_cert_host.cpp compiled as it stands and driven with float64 sums, every
answer checked against exact rational arithmetic (fractions.Fraction).

The certificate says: with m = S / 16, `certain` only if every real within EPS m of m rounds to the same float32, which is
then f = (float)m.  Rounding is monotone, so "every real in the interval" is decided by its two ends.  What is asserted:

  soundness     where float32(m (1 - EPS)) != float32(m (1 + EPS)) exactly, the flag is false;
  f             is the float32 rounding of the exact m, flag or no flag;
  sharpness     where the ends of the interval widened to EPS + 2^-48 still agree, the flag is true (the header's directed
                slack costs at most 2^-49 on either side): the exact branch is not taken for nothing.

m ranges over [2^-153, 2^127): sixteen roots of which one is 2^-149 and the rest 0, up to the last binade whose float32
neighbours are all finite (the largest mean of finite float32 coordinates lies below 2^130 and overflows float32 in the exact
epilogue as well; a conversion that overflows is left to the device tests)."""
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M_MIN_EXP, M_MAX_EXP = -153, 127


def _compiler():
    for cxx in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if cxx and (shutil.which(cxx) or os.path.exists(cxx)):
            return cxx
    return None


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = _compiler()
    assert cxx, "no C++ compiler found (c++, g++, clang++ or ROCm's clang++)"
    exe = str(tmp_path_factory.mktemp("mean_cert") / "check_mean_cert_host")
    build = subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall",
                            os.path.join(ROOT, "tools", "check_mean_cert_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    assert not build.stderr.strip(), "warnings:\n" + build.stderr
    return exe


@pytest.fixture(scope="module")
def eps(prog):
    out = subprocess.run([prog, "--constants"], capture_output=True, text=True, check=True).stdout.split()
    consts = {out[i]: float.fromhex(out[i + 1]) for i in range(0, len(out), 2)}
    # EPS = the short root's bound + the summation and reordering terms (a small multiple of 2^-53), nothing else
    assert 21 * 2.0 ** -53 <= consts["eps"] - consts["short_root_bound"] <= 64 * 2.0 ** -53, consts
    assert 0 < consts["short_root_bound"] <= 2.0 ** -36, consts
    return Fraction(consts["eps"])


def _run(prog, sums):
    sums = np.ascontiguousarray(sums, np.float64)
    r = subprocess.run([prog], input=sums.tobytes(), capture_output=True, check=True)
    out = np.frombuffer(r.stdout, np.uint32).reshape(-1, 2)
    assert len(out) == len(sums)
    return out[:, 0].copy().view(np.float32), out[:, 1].astype(bool)


def _floor_log2(fr):
    e = fr.numerator.bit_length() - fr.denominator.bit_length()
    return e if Fraction(2) ** e <= fr else e - 1


def f32_rn(fr):
    """the float32 nearest to a positive rational, ties to even, subnormals included, as a Fraction"""
    if fr == 0:
        return Fraction(0)
    q = Fraction(2) ** (max(_floor_log2(fr), -126) - 23)
    return round(fr / q) * q          # round(Fraction): half to even


def _check(sums, f, certain, eps, what):
    wide = eps + Fraction(1, 1 << 48)
    for s, fi, ci in zip(sums.tolist(), f.tolist(), certain.tolist()):
        m = Fraction(s) / 16
        assert Fraction(fi) == f32_rn(m), "%s: S = %s: f = %r is not the float32 of the exact mean" % (what, s.hex(), fi)
        if f32_rn(m * (1 - eps)) != f32_rn(m * (1 + eps)):
            assert not ci, "%s: S = %s: certain, but the ends of the EPS interval round differently" % (what, s.hex())
        if f32_rn(m * (1 - wide)) == f32_rn(m * (1 + wide)):
            assert ci, "%s: S = %s: not certain, though no boundary lies within EPS + 2^-48" % (what, s.hex())
        if ci:   # what the caller relies on
            assert Fraction(fi) == f32_rn(m * (1 - eps)) == f32_rn(m * (1 + eps))


def _f32_points(rng, e):
    """float32 values of the binade [2^e, 2^(e+1)) (of the subnormal range below 2^-126: multiples of 2^-149) as Fractions:
    both ends, two random ones"""
    if e >= -126:
        mant = [0, (1 << 23) - 1] + rng.integers(1, (1 << 23) - 1, 2).tolist()
        return [Fraction((1 << 23) + k) * Fraction(2) ** (e - 23) for k in mant]
    lo, hi = 1 << (e + 149) if e >= -149 else 0, (1 << (e + 150)) - 1 if e >= -149 else 0
    ks = {lo, hi, int(rng.integers(lo, hi + 1))} - {0}
    return [Fraction(k) * Fraction(2) ** -149 for k in ks]


def test_flag_at_float32_values_and_ties_in_every_binade(prog, eps):
    """sums whose mean sits at, just below and just above a float32 value and the tie above it: by one float64 ulp, by
    fractions and small multiples of EPS on either side of the bound, and far away"""
    rng = np.random.default_rng(20250311)
    e = float(eps)
    offs = [0.0]
    for d in (2.0 ** -52, 0.5 * e, e * (1 - 2.0 ** -6), e, e * (1 + 2.0 ** -6), e + 2.0 ** -47, 2 * e, 2.0 ** -30):
        offs += [d, -d]
    sums = []
    for ex in range(M_MIN_EXP, M_MAX_EXP):
        for v in _f32_points(rng, ex):
            ulp = Fraction(2) ** (max(_floor_log2(v), -126) - 23)
            for p in (v, v + ulp / 2):
                for d in offs:
                    s = float(16 * p) * (1.0 + d)      # 16 p has at most 25 significant bits: exact
                    if s > 0.0:
                        sums.append(s)
    sums = np.array(sums)
    f, certain = _run(prog, sums)
    _check(sums, f, certain, eps, "crafted")
    # both outcomes occur, and at the ties themselves the flag is down
    assert 0.2 < certain.mean() < 0.9, certain.mean()


def test_zero_is_certain(prog):
    f, certain = _run(prog, np.zeros(1))
    assert f[0] == 0.0 and certain[0]


def test_the_tie_of_the_device_test(prog, eps):
    """8 roots of exactly 1 and 8 of exactly 1 + 2^-23: the mean is the tie 1 + 2^-24 (tests/test_epilogue_cert_gpu.py), also
    one float64 ulp to either side of it, as short roots leave it -- never certain; 9 and 7 is 2^-27 below the tie and certain"""
    tie = 16.0 + 2.0 ** -20
    sums = np.array([np.nextafter(tie, 0.0), tie, np.nextafter(tie, 32.0), 16.0 + 7 * 2.0 ** -23])
    f, certain = _run(prog, sums)
    assert certain.tolist() == [False, False, False, True]
    assert f[3] == np.float32(1.0)
    _check(sums, f, certain, eps, "tie")


def test_a_million_random_sums(prog, eps):
    """10^6 sums with random binades and mantissas: the flag is up for all but the few whose mean lies next to a float32
    boundary, and wherever it is up f is the float32 of both ends of the interval.  The ends are formed in float64 where
    the mean lies more than 2^-40 (relative) from every boundary -- 2^-53 of rounding cannot reach across -- and exactly
    for the rest, together with 20 000 sums drawn at relative distances 2^-52 ... 2^-36 from a tie"""
    rng = np.random.default_rng(7)
    n = 1_000_000
    sums = np.ldexp(1.0 + rng.random(n), rng.integers(M_MIN_EXP + 4, M_MAX_EXP + 4, n).astype(np.int32))
    f, certain = _run(prog, sums)
    m = sums * 0.0625
    e = float(eps)
    assert np.array_equal(f.view(np.uint32), m.astype(np.float32).view(np.uint32))
    # relative distance of m to the nearest float32 tie, in float64 (error ~2^-52, far below the 2^-40 it is compared with)
    f64 = f.astype(np.float64)
    with np.errstate(over="ignore"):
        up, dn = np.nextafter(f, np.float32(np.inf)).astype(np.float64), np.nextafter(f, np.float32(0)).astype(np.float64)
    dist = np.minimum(np.abs((f64 + up) / 2 - m), np.abs((f64 + dn) / 2 - m)) / m
    far = dist > 2.0 ** -40
    assert far.mean() > 0.999
    assert certain[far].all()
    lo, hi = (m * (1 - e)).astype(np.float32), (m * (1 + e)).astype(np.float32)
    assert np.array_equal(lo[far].view(np.uint32), f[far].view(np.uint32)) and np.array_equal(hi[far].view(np.uint32), f[far].view(np.uint32))
    _check(sums[~far], f[~far], certain[~far], eps, "random, near a boundary")
    # near ties
    k = 20_000
    ex = rng.integers(-126, M_MAX_EXP, k)
    tie = np.ldexp(((1 << 24) + 2 * rng.integers(0, 1 << 23, k) + 1).astype(np.float64), (ex - 24).astype(np.int32))
    rel = np.ldexp(1.0 + rng.random(k), rng.integers(-52, -36, k).astype(np.int32)) * rng.choice([-1.0, 1.0], k)
    near = 16.0 * tie * (1.0 + rel)
    f2, c2 = _run(prog, near)
    _check(near, f2, c2, eps, "random, near a tie")
    assert 0.1 < c2.mean() < 0.9, c2.mean()
