"""Generate tests/golden/chain_ref.json from the REFERENCE's own DataProcessor (needs the reference checkout; run here, the
fixture travels).  Random sequences of 1-7 calls of all seven methods -- crop_by_bbox, apply_alpha_filter, apply_density_filter,
remove_flyers, cap_sh_degree, add_rgb_from_sh, apply_auto_bbox -- on tables of 248-byte rows, 251-byte rows (u8 colours
already there) and narrower SH layouts, with clustered coordinates plus far flyers, coordinates on a 1/8 grid (exact
duplicates, ties, zeros of both signs at an axis's extremes) and a few NaN / +-inf coordinates and NaN opacities.

remove_flyers: the drop-in implements the reference's Taichi branch (data_processor.py:143-151, which applies the mask) with
the exact mask of its cKDTree branch (which computes that mask and never applies it).  So the reference runs with
``gpu_ops.HAS_TAICHI`` set and ``gpu_ops.filter_sor_gpu`` answering with the mask the reference's own cKDTree branch computes
for the same coordinates (captured by ``refload.reference_sor``'s frame spy); its own code then slices the table and prints.

For every case: the steps' repr; for every step the lines it printed (LOG_PREFIXES), the name of the exception it raised,
whether the rows it started from held a non-finite coordinate and the sha256 of that table; the dtype and sha256 of the table
after the last step that completed.  A case ends at its first exception.

    python -m oracle.make_golden_chain
"""
from __future__ import annotations

import contextlib
import hashlib
import io
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "chain_ref.json")
N_CASES = 48
LOG_PREFIXES = ("Auto-BBox", "Alpha Filter", "After cropping", "After removing flyers", "Density Filter:", "After density filter",
                "Warning:")
HOST_METHODS = ("crop_by_bbox", "apply_alpha_filter", "cap_sh_degree", "apply_auto_bbox")


def table(n, n_rest=45, with_rgb=False, seed=0):
    """a 3DGS vertex table of random finite float32 columns with `n_rest` f_rest fields (45: the 248-byte rows of
    make_golden_rows.table) and, with_rgb, three u8 colours (251-byte rows: nothing aligned)"""
    names = ["x", "y", "z", "nx", "ny", "nz"] + ["f_dc_%d" % i for i in range(3)] + ["f_rest_%d" % i for i in range(n_rest)] \
        + ["opacity"] + ["scale_%d" % i for i in range(3)] + ["rot_%d" % i for i in range(4)]
    fields = [(nm, "<f4") for nm in names]
    if with_rgb:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    dt = np.dtype(fields)
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 255, size=(n, dt.itemsize), dtype=np.uint8)
    raw[:, 3::4] &= 0x3F  # keep the float fields finite (exponent < 255)
    return raw.reshape(-1).view(dt)


def coords(rng, n, grid):
    """(n, 3) float32: 1-4 Gaussian blobs plus 0.5-3 % far flyers.  grid: on a 1/8 grid, one axis shifted so its minimum is 0
    and another so its maximum is 0, the zeros of both signs"""
    centers = rng.uniform(-5, 5, (int(rng.integers(1, 5)), 3))
    sig = rng.uniform(0.3, 1.5, len(centers))
    which = rng.integers(0, len(centers), n)
    xyz = centers[which] + rng.standard_normal((n, 3)) * sig[which, None]
    fly = rng.random(n) < rng.uniform(0.005, 0.03)
    xyz[fly] = rng.uniform(-30, 30, (int(fly.sum()), 3))
    if grid:
        xyz = np.round(xyz * 8) / 8
        lo_axis, hi_axis = rng.permutation(3)[:2]
        xyz[:, lo_axis] -= xyz[:, lo_axis].min()
        xyz[:, hi_axis] -= xyz[:, hi_axis].max()
        xyz = xyz.astype(np.float32)
        for a in range(3):
            z = np.flatnonzero(xyz[:, a] == 0)
            xyz[z, a] = np.where(rng.random(len(z)) < 0.5, np.float32(-0.0), np.float32(0.0))
    return xyz.astype(np.float32)


def tiny_box(rng, xyz):
    """a box around one finite row: a few rows, fewer than SOR's k + 1"""
    fin = np.flatnonzero(np.isfinite(xyz).all(axis=1))
    c = xyz[fin[int(rng.integers(0, len(fin)))]].astype(np.float64)
    w = rng.uniform(0.05, 0.4)
    return c - w, c + w


def step(rng, kind, xyz):
    """one call with random arguments; crop boxes are drawn from the quantiles of the table's coordinates `xyz`"""
    if kind == "crop_by_bbox":
        u = rng.random()
        if u < 0.1:
            lo, hi = tiny_box(rng, xyz)
        elif u < 0.15:                  # an inverted box: nothing left
            lo, hi = np.full(3, 1.0), np.full(3, -1.0)
        else:
            with np.errstate(all="ignore"):
                lo = np.array([np.nanquantile(xyz[:, a], rng.uniform(0.0, 0.4)) for a in range(3)])
                hi = np.array([np.nanquantile(xyz[:, a], rng.uniform(0.6, 1.0)) for a in range(3)])
            lo, hi = np.clip(lo, -1e6, 1e6) - rng.uniform(0, 1), np.clip(hi, -1e6, 1e6) + rng.uniform(0, 1)
        cast = [float, lambda v: int(round(v)), np.float32, np.float64][int(rng.integers(0, 4))]
        return kind, tuple(cast(v) for v in (*lo, *hi))
    if kind == "apply_alpha_filter":
        return kind, (int(rng.choice([0, 1, 254, 255])) if rng.random() < 0.5 else int(rng.integers(2, 254)),)
    if kind == "apply_density_filter":
        keep = bool(rng.random() < 0.5)
        if rng.random() < 0.4:
            return kind, (1.0, 0.32, round(float(rng.uniform(0.1, 0.9)), 3), keep)
        return kind, (round(float(rng.uniform(0.3, 2.0)), 3), round(float(rng.uniform(0.05, 1.5)), 3), None, keep)
    if kind == "remove_flyers":
        if rng.random() < 0.3:
            return kind, (25, 10.5, 50000, int(rng.integers(1, 11)))
        k = int(rng.integers(1, 65)) if rng.random() < 0.9 else 80
        return kind, (k, round(float(rng.uniform(0.3, 4.0)), 3))
    if kind == "cap_sh_degree":
        return kind, (int(rng.integers(0, 4)),)
    return kind, ()


def cases():
    """-> [(case, table, [(method, args), ...])], the same on every run (no reference needed)"""
    rng = np.random.default_rng(20261016)
    methods = ("crop_by_bbox", "apply_alpha_filter", "apply_density_filter", "remove_flyers", "cap_sh_degree", "add_rgb_from_sh",
               "apply_auto_bbox")
    out = []
    for case in range(N_CASES):
        n = int(np.exp(rng.uniform(np.log(2000), np.log(60000))))
        layout = case % 5
        n_rest, with_rgb = [(45, False), (45, True), (0, False), (9, True), (24, False)][layout]
        t = table(n, n_rest, with_rgb, seed=1000 + case)
        grid = case % 3 != 0
        xyz = coords(rng, n, grid)
        for i, a in enumerate("xyz"):
            t[a] = xyz[:, i]
        t["opacity"] = (rng.standard_normal(n) * 3).astype(np.float32)
        if case % 8 == 7:               # non-finite coordinates and opacities
            t["x"][rng.integers(0, n, 3)] = np.nan
            t["y"][rng.integers(0, n, 2)] = np.inf
            t["z"][rng.integers(0, n, 2)] = -np.inf
            t["opacity"][rng.integers(0, n, 4)] = np.nan
        elif case % 8 == 3:             # NaN only: the printed box shows it on that axis
            t["y"][rng.integers(0, n, 2)] = np.nan
        host_only = case % 4 == 1
        pool = HOST_METHODS if host_only else methods
        steps = [step(rng, str(rng.choice(pool)), xyz) for _ in range(int(rng.integers(1, 8)))]
        if case % 6 == 5:               # empty the table part-way, then keep calling methods on it
            steps = steps[:3]
            at = int(rng.integers(0, len(steps) + 1))
            empty = ("apply_alpha_filter", (255,)) if rng.random() < 0.5 else ("crop_by_bbox", (1.0, 1.0, 1.0, -1.0, -1.0, -1.0))
            steps[at:at] = [empty]
            steps += [step(rng, str(rng.choice(pool)), xyz) for _ in range(2)] + [("apply_auto_bbox", ())]
        elif case % 6 == 2 and not host_only:   # SOR on fewer rows than k + 1
            lo, hi = tiny_box(rng, xyz)
            steps = [("crop_by_bbox", tuple(float(v) for v in (*lo, *hi))),
                     ("remove_flyers", (int(rng.integers(8, 65)), 2.0))] + steps[:3]
        if case % 8 == 7:               # the box of a chain whose rows hold NaN and +-inf (the alpha filter keeps them)
            steps[:0] = [("apply_alpha_filter", (int(rng.integers(1, 200)),)), ("apply_auto_bbox", ())]
        elif case % 8 == 3:
            steps[:0] = [("apply_auto_bbox", ())]
        if grid and rng.random() < 0.7 and steps[-1][0] != "apply_auto_bbox":
            steps.append(("apply_auto_bbox", ()))
        out.append((case, t, steps[:7]))
    return out


def has_nonfinite_xyz(data):
    if len(data) == 0:
        return False
    with np.errstate(all="ignore"):
        return not all(np.isfinite(data[a]).all() for a in "xyz")


def sha256(data):
    return hashlib.sha256(np.ascontiguousarray(data).tobytes()).hexdigest()


def run(cls, t, steps, on_step=None):
    """-> {"dtype", "sha256", "steps": [{"log", "exc", "nonfinite", "sha256_in"}]} of `cls` on a copy of `t`; ends at the
    first exception.  on_step(p, i): called after step i completed (the GPU test reads .data there)"""
    p = cls(t.copy())
    out = []
    for i, (name, args) in enumerate(steps):
        data = p.data
        rec = {"nonfinite": has_nonfinite_xyz(data), "sha256_in": sha256(data), "exc": None}
        buf = io.StringIO()
        try:
            with contextlib.redirect_stdout(buf), np.errstate(all="ignore"):
                getattr(p, name)(*args)
        except Exception as e:      # noqa: BLE001 -- recorded, the case ends here
            rec["exc"] = type(e).__name__
        rec["log"] = [line for line in buf.getvalue().splitlines() if line.startswith(LOG_PREFIXES)]
        out.append(rec)
        if rec["exc"] is not None:
            break
        if on_step is not None:
            on_step(p, i)
    data = p.data
    return {"dtype": str(data.dtype.descr), "sha256": sha256(data), "steps": out}


@contextlib.contextmanager
def taichi_branch():
    """the reference's remove_flyers takes its Taichi branch (data_processor.py:143-151) with the exact mask its cKDTree branch
    computes (and drops, :180-182) for the same coordinates"""
    from . import refload
    _, gpu_ops, _ = refload.load()
    saved = gpu_ops.HAS_TAICHI, gpu_ops.filter_sor_gpu
    odd = []

    def filter_sor_gpu(data_np, k=25, threshold_factor=1.0, verbose=False):
        gpu_ops.HAS_TAICHI = False
        try:
            cap = refload.reference_sor(np.asarray(data_np), k, threshold_factor)
        except ValueError:
            raise                       # cKDTree refuses non-finite data: the reference's fallback meets the same error
        except Exception as e:          # anything else would be swallowed by the reference's except: make the run fail
            odd.append(e)
            raise
        finally:
            gpu_ops.HAS_TAICHI = True
        return cap["mask"]

    gpu_ops.HAS_TAICHI, gpu_ops.filter_sor_gpu = True, filter_sor_gpu
    try:
        yield odd
    finally:
        gpu_ops.HAS_TAICHI, gpu_ops.filter_sor_gpu = saved


def main():
    from . import refload
    RefDP, _, _ = refload.load()
    out = {"_meta": {"generator": "oracle/make_golden_chain.py run against the reference (v0.8)", "cases": N_CASES}}
    with taichi_branch() as odd:
        for case, t, steps in cases():
            rec = run(RefDP, t, steps)
            assert not odd, (case, odd)
            out[str(case)] = dict(rec, steps_repr=repr(steps))
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", GOLDEN)


if __name__ == "__main__":
    main()
