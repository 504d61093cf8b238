"""GPU box: the density stage of BASELINE configs[2] alone (10M uniform splats, L=5, sensitivity 0.5 -> voxel 1.1, 0.55 %), on the
device chain, for `rocprofv3 --kernel-trace --stats` and A/B runs:   python tools/probe_density.py [n] [L] [sensitivity] [cloud]
(cloud: uniform (default) | floaters | blobs -- bench.py's generators; L is ignored for the last two)

The large-dense case:   python tools/probe_density.py large [n] [voxel] [min_points]
bench.py's six blobs + flyers (10M rows), voxel 0.1, min_points 1 -- every occupied voxel is dense, what `--density_voxel_size 0.1
--density_threshold 0` asks for.  Prints the call time and the stage clocks of gsx_density_filter_large_dev, then the wall time of
the host steps the lazy class took above 1024 dense voxels before that call existed (keys down, tuples, BFS, sort, keys up)."""
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

import numpy as np  # noqa: E402

gsx = importlib.import_module("3dgsconverter_amd")
L = gsx._lib


def large_dense(n, voxel, minpts):
    clusters = importlib.import_module("3dgsconverter_amd.processing.clusters")
    xyz = bench.synth_clustered(n, 0)
    ch = L.DeviceChain(xyz, keep_pristine=True)
    res = ch.density_filter_large(voxel, minpts, False)
    print("large-dense: n", n, "voxel", voxel, "min_points", minpts, "-> status", res["status"], "left", res["left"], "unique", res["n_unique"],
          "clusters", res["kept_clusters"], "largest", res["largest"])
    new_left = res["left"]
    ts, stages = [], []
    ch.ctx.set_timing(True)
    for _ in range(5):
        ch.restart()
        ch.ctx.synchronize()
        t0 = time.perf_counter()
        ch.density_filter_large(voxel, minpts, False)
        ch.ctx.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
        stages.append(ch.ctx.density_stage_clocks())
    ch.ctx.set_timing(False)
    print("density_filter_large + compaction, host clock ms:", ["%.3f" % t for t in ts])
    for name in L.DENSITY_STAGES:
        print("  stage %-10s HIP-event ms: %s" % (name, ["%.3f" % s[name] for s in stages]))
    print("  all stages, ms:", ["%.3f" % sum(s.values()) for s in stages])
    # the host steps (DataProcessor._density_lazy below its device calls), timed piece by piece
    ch.restart()
    ch.ctx.synchronize()
    t = [time.perf_counter()]
    occ = ch.density_voxels(voxel, minpts)
    t.append(time.perf_counter())
    comps = clusters.connected_clusters(map(tuple, occ["dense_keys"].tolist()))
    t.append(time.perf_counter())
    kept, kept_clusters, max_len = clusters.select_clusters(comps, False)
    kept_keys = np.array(sorted(kept), dtype=np.int64).reshape(-1, 3)
    t.append(time.perf_counter())
    left = ch.density_keep(voxel, kept_keys)
    ch.ctx.synchronize()
    t.append(time.perf_counter())
    d = [(b - a) * 1e3 for a, b in zip(t, t[1:])]
    print("host steps on the same rows: dense voxels", len(occ["dense_keys"]), "clusters", kept_clusters, "largest", max_len, "left", left)
    print("  occupancy + keys down %.1f ms | tuples + BFS %.1f ms | keep rule + sorted %.1f ms | keys up + mask + compaction %.1f ms | total %.1f ms"
          % (d[0], d[1], d[2], d[3], sum(d)))
    print("same survivors:", left == new_left, "| speed-up of the call: %.0fx" % (sum(d) / min(ts)))
    ch.close()


if len(sys.argv) > 1 and sys.argv[1] == "large":
    large_dense(int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000, float(sys.argv[3]) if len(sys.argv) > 3 else 0.1,
                int(sys.argv[4]) if len(sys.argv) > 4 else 1)
    sys.exit(0)

n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
ext = float(sys.argv[2]) if len(sys.argv) > 2 else 5.0
sens = float(sys.argv[3]) if len(sys.argv) > 3 else 0.5
voxel, thr = max(0.1, 2.0 - 1.8 * sens), 0.1 + 0.9 * sens
cloud = sys.argv[4] if len(sys.argv) > 4 else "uniform"
xyz = bench.synth_uniform(n, ext, 0) if cloud == "uniform" else (bench.synth_scene_with_floaters(n, 0) if cloud == "floaters" else bench.synth_clustered(n, 0))
ch = L.DeviceChain(xyz, keep_pristine=True)
minpts = int(n * (thr / 100.0))
res = ch.density_filter(voxel, minpts, False)
print("status", res["status"], "left", res["left"], "unique", res["n_unique"], "clusters", res["kept_clusters"], "largest", res["largest"])
ts = []
for _ in range(10):
    ch.restart()
    ch._box = ch._box if ch._box is not None else None
    ch.ctx.synchronize()
    t0 = time.perf_counter()
    ch.density_filter(voxel, minpts, False)
    ch.ctx.synchronize()
    ts.append((time.perf_counter() - t0) * 1e3)
print("density_filter + compaction, host clock ms:", ["%.3f" % t for t in ts])
ch.close()
