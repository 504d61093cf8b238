"""Where does the wave time of knn_brick and knn_ring_fast go?  Needs a diagnostic build of the library:

    GSX_EXTRA_FLAGS=-DGSX_WAVE_STAMPS GSX_VARIANT_TAG=stamps python 3dgsconverter_amd/build.py
    GSX_LIB_PATH=3dgsconverter_amd/variants/libgsx_hip_stamps.so python tools/wave_stamps.py [--n N] [--k K] [--param name=value]

In that build every wave of the two kernels writes one record on exit (csrc/sor_grid_params.h: ws_write): XCC id, workgroup,
wave, start and end on the chip-wide 100 MHz counter, the items it took from its static share and from its group's tail, and (knn_ring_fast) the shader cycles of each phase.  This tool runs the headline cloud (uniform, seed 0) a few
times, takes the records of the last call and prints, per kernel: when the last wave ended, the mean and the spread of the end
times per XCC and per blockIdx % 8 group, the item counts, and the phase shares.  Times are in microseconds after the first
wave's start.  Stamping costs about a tenth of the wave cycles: compare groups and phases, never quote these times."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

PHASES = ("row bounds", "fetch+filter", "hist+select", "exact rank", "epilogue", "queue+rest")


def table(name, rec, out):
    if len(rec) == 0:
        out("%s: no records" % name)
        return
    xcc, blk = rec[:, 0].astype(np.int64), rec[:, 1].astype(np.int64)
    t0 = rec[:, 3].astype(np.int64)
    start = (t0 - t0.min()) / 100.0
    end = (rec[:, 4].astype(np.int64) - t0.min()) / 100.0
    items = rec[:, 5:8].astype(np.int64)
    out("%s: %d waves, last start %.1f us, first end %.1f us, last end %.1f us, mean end %.1f us (%.1f %% of the last)" % (
        name, len(rec), start.max(), end.min(), end.max(), end.mean(), 100.0 * end.mean() / end.max()))
    out("  idle wave time before the last end: %.1f %% (sum over waves of last end - own end, over waves x last end)" % (
        100.0 * (end.max() - end).sum() / (len(rec) * end.max())))
    grp = blk % 8
    pairs = sorted(set(zip(grp.tolist(), xcc.tolist())))
    out("  blockIdx %% 8 -> XCC: %s" % " ".join("%d->%d" % p for p in pairs))
    for label, key in ((("group = XCC", grp),) if all(a == b for a, b in pairs) else (("XCC", xcc), ("group", grp))):
        out("  %s\n        waves   mean_end    min_end    max_end   spread     static       tail   items/wave" % label)
        for v in sorted(set(key.tolist())):
            m = key == v
            e = end[m]
            it = items[m].sum(axis=0)
            out("  %5d %5d %10.1f %10.1f %10.1f %8.1f %10d %10d %12.2f" % (
                v, m.sum(), e.mean(), e.min(), e.max(), e.max() - e.min(), it[0], it[1], it.sum() / m.sum()))
    means = np.array([end[grp == v].mean() for v in sorted(set(grp.tolist()))])
    inside = np.array([end[grp == v].max() - end[grp == v].min() for v in sorted(set(grp.tolist()))])
    out("  between groups: mean end %.1f .. %.1f us (%.1f apart); inside a group: spread %.1f .. %.1f us" % (
        means.min(), means.max(), means.max() - means.min(), inside.min(), inside.max()))
    # inside a group: who ends late?  HW_ID: wave slot [3:0], SIMD [5:4], CU [11:8], shader array [12], shader engine [15:13]
    out("  end time percentiles 0 / 10 / 50 / 90 / 100: " + " / ".join("%.1f" % v for v in np.percentile(end, [0, 10, 50, 90, 100])))
    hw = rec[:, 15].astype(np.int64)
    simd = (hw >> 4) & 3
    cu = (xcc << 8) | (((hw >> 13) & 7) << 5) | (((hw >> 12) & 1) << 4) | ((hw >> 8) & 15)
    # age of a wave on its SIMD: its rank by start stamp among the waves of the same CU and SIMD (0 = the oldest)
    age = np.zeros(len(rec), np.int64)
    key = cu * 4 + simd
    order = np.lexsort((t0, key))
    ks = key[order]
    first = np.r_[0, np.nonzero(ks[1:] != ks[:-1])[0] + 1]
    pos = np.arange(len(rec)) - np.repeat(first, np.diff(np.r_[first, len(rec)]))
    age[order] = pos
    out("  CUs seen %d, waves per (CU, SIMD): min %d max %d" % (len(set(cu.tolist())), np.bincount(np.unique(key, return_inverse=True)[1]).min(),
                                                           np.bincount(np.unique(key, return_inverse=True)[1]).max()))
    for label, k2 in (("SIMD", simd), ("age", age)):
        out("  %-5s waves   mean_end    min_end    max_end  items/wave  of them tail" % label)
        for v in sorted(set(k2.tolist())):
            m = k2 == v
            out("  %5d %5d %10.1f %10.1f %10.1f %11.2f %11.2f" % (v, m.sum(), end[m].mean(), end[m].min(), end[m].max(),
                                                              items[m].sum() / m.sum(), items[m][:, 1:].sum() / m.sum()))
    per_wave = items.sum(axis=1)
    if per_wave.std() > 0:
        out("  correlation of a wave's end time with its item count: %.3f" % np.corrcoef(end, per_wave)[0, 1])
    tot = items.sum(axis=0)
    out("  items: %d static, %d tail (%d in all)" % (tot[0], tot[1], tot.sum()))
    ph = rec[:, 8:14].astype(np.float64).sum(axis=0)
    if ph.sum() > 0:
        out("  phase shares of the stamped cycles: " + ", ".join("%s %.1f %%" % (p, 100.0 * c / ph.sum()) for p, c in zip(PHASES, ph)))
        n_items = max(1, int(tot.sum()))
        out("  shader cycles per query: " + ", ".join("%s %.0f" % (p, c / n_items) for p, c in zip(PHASES, ph)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--extent", type=float, default=5.0)
    ap.add_argument("--calls", type=int, default=5, help="calls before the one whose records are read (clocks and caches warm)")
    ap.add_argument("--param", action="append", default=[], help="name=value library knob, e.g. brick_plan=0")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    import importlib
    L = importlib.import_module("3dgsconverter_amd._lib")
    L.require_hip()
    lines = []

    def out(s):
        print(s)
        lines.append(s)

    ctx = L.Context(0)
    for p in args.param:
        name, val = p.split("=")
        ctx.set_param(name, float(val))
    xyz = np.random.default_rng(0).random((args.n, 3), dtype=np.float32) * np.float32(args.extent)
    buf = ctx.alloc(xyz.nbytes).upload(xyz)
    md = ctx.alloc(4 * args.n)
    for _ in range(args.calls + 1):
        info = ctx.sor_knn(buf.ptr, buf.ptr + 4, buf.ptr + 8, 3, args.n, 0, args.n, args.k, md.ptr, algo=L.KNN_GRID, want_info=True)
    out("# wave stamps: %d uniform points (L=%g, seed 0), k=%d, params %s; bricks %d, fallback queries %d" % (
        args.n, args.extent, args.k, " ".join(args.param) or "(defaults)", info["n_bricks"], info["n_fallback"]))
    out("# a stamped build: compare groups and phases, these are no timings")
    wq = ctx.debug_work_queue()
    for nm, q in wq.items():
        out("# queue %-16s items %8d  workgroups %5d  final counters %s" % (nm, q["items"], q["blocks"], " ".join(str(int(c)) for c in q["ctr"])))
    table("knn_brick", ctx.debug_wave_stamps(0), out)
    table("knn_ring_fast", ctx.debug_wave_stamps(1), out)
    buf.free()
    md.free()
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
