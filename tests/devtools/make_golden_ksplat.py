"""Build box only: run the reference's own ``KSplatFormat.write`` (gsconverter/formats/ksplat.py) on every .ksplat case and record
what it wrote -> tests/golden/ksplat_ref.npz.

  spec         JSON: one recipe per case (tests/ksplat_numpy.py: case_table / case_kwargs, "level"), with "error" = [exception
               type, message] for the cases the reference refuses (it then creates no file)
  <case>       the whole file (edge and small cases) -- or <case>__sha256, the file's sha256 (random tables of 500+ rows)
  edges__table the explicit edge rows themselves

usage: python tests/devtools/make_golden_ksplat.py"""
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import refload          # noqa: E402
import ksplat_numpy                  # noqa: E402

R = dict(kind="random")
CASES = {}
for lv in (0, 1, 2, 7):
    CASES[f"d3_248_l{lv}"] = dict(R, n=4096, seed=1, level=lv)
CASES["d3_251_rgb_l1"] = dict(R, n=4096, seed=2, rgb=True, level=1)
CASES["d3_251_rgb_l0"] = dict(R, n=4096, seed=2, rgb=True, level=0)
for lv in (0, 1, 2):
    CASES[f"deg2_l{lv}"] = dict(R, n=700, seed=3, sh_upto=24, level=lv)
    CASES[f"deg1_l{lv}"] = dict(R, n=700, seed=4, sh_upto=9, level=lv)
    CASES[f"sh0_l{lv}"] = dict(R, n=700, seed=5, sh_scale=0.0, level=lv)
    CASES[f"c9_l{lv}"] = dict(R, n=600, seed=6, n_rest=9, level=lv)
    CASES[f"c24_l{lv}"] = dict(R, n=600, seed=7, n_rest=24, level=lv)
    CASES[f"nosh_l{lv}"] = dict(R, n=600, seed=8, n_rest=0, level=lv)
    CASES[f"shlevel0_l{lv}"] = dict(R, n=500, seed=9, level=lv, kw=dict(sh_level=0))
    CASES[f"shlevel1_l{lv}"] = dict(R, n=500, seed=10, level=lv, kw=dict(sh_level=1))
    CASES[f"edges_l{lv}"] = dict(kind="edges", level=lv)
    CASES[f"edges_b7_l{lv}"] = dict(kind="edges", level=lv, kw=dict(bucket_size=7))
    for n in (0, 1, 255, 256, 257):
        CASES[f"n{n}_l{lv}"] = dict(R, n=n, seed=20 + n, level=lv)
for bs in (1, 7, 256, 1000, 5000):
    CASES[f"bucket{bs}_l1"] = dict(R, n=3001, seed=11, level=1, kw=dict(bucket_size=bs))
CASES["bucket7_l2"] = dict(R, n=3001, seed=12, level=2, kw=dict(bucket_size=7))
for blk in (5.0, 0.37, -2.0):
    CASES[f"block{blk}_l1"] = dict(R, n=1500, seed=13, level=1, kw=dict(block_size=blk))
CASES["block0.37_b7_l2"] = dict(R, n=1500, seed=14, level=2, kw=dict(block_size=0.37, bucket_size=7))
CASES["ties_l1"] = dict(kind="ties", level=1, kw=dict(block_size=63.998046875))
CASES["level3_shlevel1"] = dict(R, n=300, seed=15, level=3, kw=dict(sh_level=1, bucket_size=100))
CASES["edges_l7"] = dict(kind="edges", level=7)           # levels >= 3 cast SH values to u8 without the quantiser
# the reference's errors
CASES["err_bucket0_l0"] = dict(R, n=10, seed=30, level=0, kw=dict(bucket_size=0))
CASES["err_bucket0_l1"] = dict(R, n=10, seed=30, level=1, kw=dict(bucket_size=0))
CASES["err_bucket_neg_l1"] = dict(R, n=10, seed=30, level=1, kw=dict(bucket_size=-4))
CASES["err_block0_l1"] = dict(R, n=10, seed=30, level=1, kw=dict(block_size=0.0))
CASES["err_shlevel_neg"] = dict(R, n=10, seed=30, level=0, kw=dict(sh_level=-1))
CASES["err_level_neg"] = dict(R, n=10, seed=30, level=-1)
CASES["err_level_65536"] = dict(R, n=10, seed=30, level=65536)
CASES["err_bucket_neg_l0"] = dict(R, n=10, seed=30, level=0, kw=dict(bucket_size=-4))
HASH_ONLY = {k for k, v in CASES.items() if v.get("n", 0) >= 500}   # the larger random tables: sha256 only
MISSING = {"err_no_opacity": ("opacity", 0), "err_no_y_l1": ("y", 1), "err_no_rest5_l0": ("f_rest_5", 0)}


def main():
    refload.load()
    from gsconverter.formats.ksplat import KSplatFormat
    out, spec = {}, {}
    cases = dict(CASES)
    for name, (field, lv) in MISSING.items():
        cases[name] = dict(R, n=10, seed=31, level=lv, drop=field)
    with tempfile.TemporaryDirectory() as tmp:
        for name, rec in cases.items():
            t = ksplat_numpy.case_table(rec)
            path = os.path.join(tmp, name + ".ksplat")
            rec = dict(rec)
            try:
                with np.errstate(all="ignore"):
                    KSplatFormat().write(t, path, compression_level=rec["level"], **rec.get("kw", {}))
            except Exception as e:                   # noqa: BLE001  (the reference's own exception, recorded)
                rec["error"] = [type(e).__name__, str(e)]
                assert not os.path.exists(path), name
                spec[name] = rec
                print(name, type(e).__name__, e)
                continue
            with open(path, "rb") as f:
                data = f.read()
            rec["bytes"] = len(data)
            if name in HASH_ONLY:
                out[name + "__sha256"] = np.frombuffer(hashlib.sha256(data).digest(), np.uint8)
            else:
                out[name] = np.frombuffer(data, np.uint8)
            spec[name] = rec
            print(name, "bytes", len(data))
    out["edges__table"] = ksplat_numpy.edge_table()
    out["spec"] = np.frombuffer(json.dumps(spec, sort_keys=True).encode(), np.uint8)
    dst = os.path.join(ROOT, "tests", "golden", "ksplat_ref.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
