"""Build box only: run the reference's own ``DataProcessor`` methods and ``CompressedPlyFormat.write`` on the field-dtype cases
(tests/dtypes_cases.py) and record what they gave -> tests/golden/dtypes_ref.npz.

  spec                       JSON: sizes, parameters, the auto-bbox messages, the reference's errors
  <op>/<case>/mask           packed survivor masks of remove_flyers (the mask of :180), apply_density_filter, apply_alpha_filter,
                             crop_by_bbox -- at N rows, and at N_LARGE rows under large/
  sor/<case>/threshold       the float32 threshold's bytes
  rgb/<case>                 sha256 of the colours add_rgb_from_sh appends
  cap/<case>                 sha256 of the fields of the table cap_sh_degree(1) leaves (dtypes_cases.field_bytes)
  cply/<case>/<element>      sha256 of the chunk / vertex / sh elements (stable ties, as tests/golden/cply_ref.npz's *_stable)
  adv_*                      the adversarial tables' reference masks

The archive is written with fixed entry times, so a rerun reproduces the file byte for byte (``--check`` compares instead of
writing).

usage: python tests/devtools/make_golden_dtypes.py [--check]"""
import hashlib
import io
import json
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import refload          # noqa: E402
import dtypes_cases as dc           # noqa: E402

DST = os.path.join(ROOT, "tests", "golden", "dtypes_ref.npz")


def sha(b) -> np.ndarray:
    return np.frombuffer(hashlib.sha256(bytes(b)).digest(), np.uint8)


def npz_bytes(arrays: dict) -> bytes:
    """np.savez_compressed's layout with a fixed entry time (numpy stamps the current time)"""
    bio = io.BytesIO()
    with zipfile.ZipFile(bio, "w", zipfile.ZIP_DEFLATED) as zf:
        for key in sorted(arrays):
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[key]), allow_pickle=False)
            zf.writestr(info, buf.getvalue())
    return bio.getvalue()


def main(check=False):
    DataProcessor, _, dpmod = refload.load()
    msgs = []
    dpmod.status_print = lambda *a, **kw: msgs.append(" ".join(map(str, a)))
    out, spec = {}, {"N": dc.N, "N_LARGE": dc.N_LARGE, "sor": [dc.SOR_K, dc.SOR_SIGMA], "density": dc.DENSITY_KW,
                     "alpha_min": dc.ALPHA_MIN, "box": dc.BOX, "bbox_message": {}, "cply_error": {}, "numpy": np.__version__}

    def sor(prefix, t):
        cap = refload.reference_sor_table(t, dc.SOR_K, dc.SOR_SIGMA)
        out[prefix + "/mask"] = np.packbits(cap["mask"])
        out[prefix + "/threshold"] = np.frombuffer(np.float32(cap["threshold"]).tobytes(), np.uint8)

    def density(prefix, t):
        rows = DataProcessor(t.copy()).apply_density_filter(**dc.DENSITY_KW)
        out[prefix + "/mask"] = np.packbits(dc.masks_from_rows(rows, len(t)))

    with np.errstate(all="ignore"):
        for case in dc.CASES:
            t = dc.table(case)
            n = len(t)
            sor("sor/" + case, t)
            density("density/" + case, t)
            out["alpha/%s/mask" % case] = np.packbits(dc.masks_from_rows(DataProcessor(t.copy()).apply_alpha_filter(dc.ALPHA_MIN), n))
            out["crop/%s/mask" % case] = np.packbits(dc.masks_from_rows(DataProcessor(t.copy()).crop_by_bbox(*dc.BOX), n))
            p = DataProcessor(t.copy())
            p.add_rgb_from_sh()
            out["rgb/" + case] = sha(np.column_stack([p.data[c] for c in ("red", "green", "blue")]).tobytes())
            p = DataProcessor(np.array(t))
            p.cap_sh_degree(1)
            out["cap/" + case] = sha(dc.field_bytes(p.data))
            del msgs[:]
            DataProcessor(t).apply_auto_bbox()
            spec["bbox_message"][case] = msgs[-1]
            try:
                got = refload.reference_cply(t, stable_ties=True)
            except Exception as e:                       # (recorded: a refused dtype need not be writable by the reference)
                spec["cply_error"][case] = "%s: %s" % (type(e).__name__, e)
            else:
                for el in ("chunk", "vertex", "sh"):
                    out["cply/%s/%s" % (case, el)] = sha(b"" if got[el] is None else got[el].tobytes())
            print(case, "done")
        for case in dc.LARGE_CASES:
            t = dc.table(case, dc.N_LARGE, seed=2)
            sor("large/sor/" + case, t)
            if case in dc.ACCEPT["density"]:
                density("large/density/" + case, t)
            print("large", case, "done")

        t = dc.adv_sor_table()
        cap = refload.reference_sor_table(t, dc.ADV_SOR["k"], dc.ADV_SOR["sigma"])
        out["adv_sor/mask"] = np.packbits(cap["mask"])
        out["adv_sor/mean_dists"] = cap["mean_dists"]
        t = dc.adv_density_table()
        rows = DataProcessor(t.copy()).apply_density_filter(dc.ADV_DENSITY["voxel_size"], dc.ADV_DENSITY["threshold_percentage"])
        out["adv_density/mask"] = np.packbits(dc.masks_from_rows(rows, len(t)))
        t = dc.adv_div_table()
        coords = np.column_stack((t["x"], t["y"], t["z"]))
        out["adv_div/keys"] = np.floor(coords / dc.ADV_DIV["voxel_size"]).astype(np.int64)   # :38-39 as written
    out["spec"] = np.frombuffer(json.dumps(spec, sort_keys=True).encode(), np.uint8)
    blob = npz_bytes(out)
    if check:
        with open(DST, "rb") as f:
            same = f.read() == blob
        print("identical" if same else "DIFFERENT", DST)
        return 0 if same else 1
    with open(DST, "wb") as f:
        f.write(blob)
    print("wrote", DST, len(blob), "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main("--check" in sys.argv[1:]))
