"""-m gpu: sequences of the drop-in DataProcessor's seven methods against the REFERENCE's own runs (tests/golden/chain_ref.json,
oracle/make_golden_chain.py), through the eager class, the lazy class install() binds (device chain, deferred fills, one fused
compaction) and the lazy class with .data read after every step -- same printed lines step by step, same exceptions, same table
bytes.  And gsx_slab_bbox_dev -- the box of the lazy chain, of the device density filter's keys and of the multi-GPU slab
partition -- against numpy at the sizes, strides and values where a reduction goes wrong."""
import importlib
import io
import contextlib
import json
import os

import numpy as np
import pytest

from oracle import make_golden_chain as mgc

pytestmark = pytest.mark.gpu

gsx = importlib.import_module("3dgsconverter_amd")
dp = importlib.import_module("3dgsconverter_amd.processing.data_processor")
L = gsx._lib

# INTEGRATION.md, "Coordinates must be finite": SOR and the density filter raise GsxError on rows that hold a NaN or an infinity
# (the reference's cKDTree raises ValueError; its density filter floors NaN to an arbitrary voxel and goes on).  The only departure
# from the reference these sequences allow.
FINITE_ONLY = ("remove_flyers", "apply_density_filter")

VARIANTS = {
    "eager": lambda d: dp.DataProcessor(d, lazy=False),
    "lazy": dp.ChainedDataProcessor,
    "lazy_read_each_step": dp.ChainedDataProcessor,
}


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(os.path.dirname(__file__), "golden", "chain_ref.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def all_cases():
    return mgc.cases()


def replay(variant, t, steps):
    """like mgc.run; the plain lazy variant never reads .data before its last step (no sha256_in / nonfinite per step)"""
    if variant != "lazy":
        return mgc.run(VARIANTS[variant], t, steps)
    p = VARIANTS[variant](t.copy())
    out = []
    for name, args in steps:
        rec = {"exc": None}
        buf = io.StringIO()
        try:
            with contextlib.redirect_stdout(buf), np.errstate(all="ignore"):
                getattr(p, name)(*args)
        except Exception as e:      # noqa: BLE001
            rec["exc"] = type(e).__name__
        rec["log"] = [line for line in buf.getvalue().splitlines() if line.startswith(mgc.LOG_PREFIXES)]
        out.append(rec)
        if rec["exc"] is not None:
            break
    data = p.data
    return {"dtype": str(data.dtype.descr), "sha256": mgc.sha256(data), "steps": out}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_method_sequences_against_the_reference(variant, gold, all_cases):
    refused = 0
    for case, t, steps in all_cases:
        want = gold[str(case)]
        got = replay(variant, t, steps)
        where = (variant, case)
        for i, w in enumerate(want["steps"]):
            assert i < len(got["steps"]), (where, i, "the drop-in stopped early")
            g = got["steps"][i]
            name = steps[i][0]
            at = (where, i, steps[i])
            if "sha256_in" in g:
                assert g["sha256_in"] == w["sha256_in"] and g["nonfinite"] == w["nonfinite"], at
            if w["nonfinite"] and name in FINITE_ONLY:
                # the finite-coordinates rule: refused, and the table is what it was before the call (the lazy chain included)
                assert g["exc"] == "GsxError", (at, g)
                assert got["sha256"] == w["sha256_in"], at
                assert len(got["steps"]) == i + 1, at
                refused += 1
                break
            if w["exc"] is not None:
                assert g["exc"] in (w["exc"], "GsxError"), (at, g["exc"], w["exc"])
            else:
                assert g["exc"] is None, (at, g["exc"])
            assert g["log"] == w["log"], (at, g["log"], w["log"])
        else:
            assert len(got["steps"]) == len(want["steps"]), where
            assert got["dtype"] == want["dtype"] and got["sha256"] == want["sha256"], (where, steps)
    assert refused > 0      # the fixture reaches the rule


# ------------------------------------------------------------------ gsx_slab_bbox_dev
def _bbox_dev(ctx, xyz, stride):
    """gsx_slab_bbox_dev on (n, 3) float32 coordinates laid out as the first three floats of `stride`-float rows"""
    n = len(xyz)
    rows = np.full((max(n, 1), stride), np.float32(12345.0), dtype=np.float32)
    rows[:n, :3] = xyz
    buf = ctx.alloc(rows.nbytes).upload(rows)
    out = ctx.alloc(32)
    try:
        L.check(ctx.lib.gsx_slab_bbox_dev(ctx.handle, buf.ptr, buf.ptr + 4, buf.ptr + 8, stride, n, out.ptr), "gsx_slab_bbox_dev")
        ctx.synchronize()
        return out.download(np.float32, 7)
    finally:
        buf.free()
        out.free()


def _coords(kind, n, rng):
    xyz = (rng.standard_normal((n, 3)) * 4).astype(np.float32)
    if kind == "inf":
        xyz[rng.integers(0, n, max(1, n // 1000)), 0] = np.inf
        xyz[rng.integers(0, n, 1), 2] = -np.inf
    elif kind == "nan":
        xyz[rng.integers(0, n, max(1, n // 500)), 1] = np.nan
    elif kind == "nan_axis":
        xyz[:, 2] = np.nan
        xyz[rng.integers(0, n, 1), 0] = np.inf
    elif kind == "zeros":
        # x >= 0 with its minimum a zero of either sign, y <= 0 with its maximum a zero of either sign, z only zeros: the
        # device must find each zero by value (-0.0f is INT_MIN as an int: an integer max must not be where it goes)
        xyz[:, 0] = np.abs(xyz[:, 0]) + 1
        xyz[:, 1] = -np.abs(xyz[:, 1]) - 1
        xyz[:, 2] = 0.0
        for a, frac in ((0, 0.001), (1, 0.001), (2, 1.0)):
            at = rng.random(n) < frac
            at[int(rng.integers(0, n))] = True
            xyz[at, a] = np.where(rng.random(int(at.sum())) < 0.5, np.float32(-0.0), np.float32(0.0))
    elif kind == "negzero":
        # the extremes are -0.0 alone: max(y) = -0.0 and min(x) = +0.0 (-x = -0.0)
        xyz[:, 0] = np.abs(xyz[:, 0]) + 1
        xyz[:, 1] = -np.abs(xyz[:, 1]) - 1
        xyz[:, 2] = -0.0
        xyz[int(rng.integers(0, n)), 0] = 0.0
        xyz[int(rng.integers(0, n)), 1] = -0.0
    return xyz


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 4097, 1_000_003])
@pytest.mark.parametrize("stride", [3, 62])
def test_slab_bbox_dev_against_numpy(n, stride):
    rng = np.random.default_rng(n * 7 + stride)
    ctx = L.Context(0)
    try:
        for kind in ("finite", "inf", "nan", "nan_axis", "zeros", "negzero"):
            xyz = _coords(kind, n, rng)
            b = _bbox_dev(ctx, xyz, stride)
            at = (n, stride, kind)
            assert b[6] == (1.0 if (~np.isfinite(xyz)).any() else 0.0), (at, b[6])
            for a in range(3):
                col = xyz[:, a]
                if np.isnan(col).all():
                    assert b[a] == -np.inf and b[3 + a] == -np.inf, (at, a, b)      # no number: the words keep their -inf
                    continue
                # NaNs are dropped (fmaxf); every other value counts by VALUE: -0.0 == 0.0 here, the sign of a zero extreme
                # is not the kernel's to give (apply_auto_bbox takes a zero from numpy, test below)
                assert -b[a] == np.nanmin(col) and b[3 + a] == np.nanmax(col), (at, a, -b[a], b[3 + a], np.nanmin(col), np.nanmax(col))
                if not np.isnan(col).any():
                    assert -b[a] == np.min(col) and b[3 + a] == np.max(col), (at, a)
    finally:
        ctx.close()


@pytest.mark.parametrize("kind", ["zeros", "negzero", "nan", "inf"])
def test_lazy_auto_bbox_prints_the_references_box(kind):
    """the lazy chain's box comes from gsx_slab_bbox_dev; a zero extreme or a non-finite coordinate is the reference's own
    expression, np.min / np.max on the strided field view of the table the reference would hold (data_processor.py:348-353)"""
    rng = np.random.default_rng(len(kind))
    for n in (5000, 70000):
        t = mgc.table(n, 45, False, seed=n)
        xyz = _coords(kind, n, rng)
        for i, a in enumerate("xyz"):
            t[a] = xyz[:, i]
        t["opacity"] = (rng.standard_normal(n) * 3).astype(np.float32)
        p = dp.ChainedDataProcessor(t.copy())
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf), np.errstate(all="ignore"):
            p.apply_alpha_filter(40)
            p.apply_auto_bbox()
        kept = t[t["opacity"] >= np.log((40 / 255.0) / (1 - 40 / 255.0))]
        lo = [np.min(kept[a]) for a in "xyz"]
        hi = [np.max(kept[a]) for a in "xyz"]
        want = f"Auto-BBox Applied: [{lo[0]:.4f}, {lo[1]:.4f}, {lo[2]:.4f}] to [{hi[0]:.4f}, {hi[1]:.4f}, {hi[2]:.4f}]"
        got = [line for line in buf.getvalue().splitlines() if line.startswith("Auto-BBox")]
        assert got == [want], (kind, n, got, want)
        assert p.data.tobytes() == kept.tobytes()
