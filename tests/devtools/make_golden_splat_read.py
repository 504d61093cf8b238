"""Build tests/golden/splat_read_ref.npz from the REFERENCE's own .splat reader (build box only: needs the reference).

The reference's ``SplatFormat().read`` (formats/splat.py:9-80) runs unchanged on every case.  The input files come from
tests/splat_read_numpy.py's builders and are stored whole, except the 12.6 MB pattern file, which the builder makes again (its
sha256 is recorded).  Per case the spec records the reference's dtype names / types / itemsize and its rows (whole for small
cases, sha256 of the row bytes for larger ones).

    python tests/devtools/make_golden_splat_read.py
"""
import hashlib
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import splat_read_numpy as sn  # noqa: E402
from oracle import refload  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "splat_read_ref.npz")
WHOLE_BELOW = 24000          # row bytes up to this are stored whole


def reference_read(path):
    refload.load()
    import gsconverter.formats.splat as mod  # type: ignore
    with np.errstate(all="ignore"):
        return mod.SplatFormat().read(path)


def cases():
    """-> [(name, file bytes, stored whole?)]"""
    rng = np.random.default_rng(20261019)
    out = [("random_small", sn.random_records(257, rng), True),
           ("random", sn.random_records(3001, rng), True),
           ("realistic", sn.realistic_records(1500, rng), True),
           ("pattern", sn.pattern_records(), False),
           ("edge_scales", sn.edge_scale_records(), True),
           ("all_128", sn.all_128_records(100, rng), True)]
    for n in (0, 1, 127, 128, 129):
        out.append(("n%d" % n, sn.random_records(n, rng), True))
    for k in (1, 31):
        out.append(("trailing%d" % k, sn.random_records(130, rng) + bytes(range(1, k + 1)), True))
    out.append(("trailing_only", bytes(range(1, 32)), True))
    return out


def main():
    import tempfile
    spec, arrays = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, data, whole in cases():
            path = os.path.join(tmp, name + ".splat")
            with open(path, "wb") as f:
                f.write(data)
            rec = {"file_bytes": len(data), "file_sha256": hashlib.sha256(data).hexdigest()}
            if whole:
                arrays[name + "__file"] = np.frombuffer(data, np.uint8)
            rows = reference_read(path)
            rec["names"] = list(rows.dtype.names)
            rec["rows"] = len(rows)
            rec["dtype"] = [rows.dtype[f].str for f in rows.dtype.names]
            rec["itemsize"] = rows.dtype.itemsize
            raw = np.ascontiguousarray(rows).view(np.uint8).reshape(-1)
            if raw.nbytes <= WHOLE_BELOW:
                arrays[name + "__rows"] = raw.copy()
            else:
                arrays[name + "__sha256"] = np.frombuffer(sn.sha(rows), np.uint8)
            rec["nan_words"] = int(sum(np.isnan(rows[f]).sum() for f in rows.dtype.names if rows.dtype[f].kind == "f"))
            spec[name] = rec
            print(name, "%d rows, %d NaN words" % (rec["rows"], rec["nan_words"]))
    arrays["spec"] = np.frombuffer(json.dumps(spec, sort_keys=True).encode(), np.uint8)
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    with open(OUT, "wb") as f:
        f.write(buf.getvalue())
    print(OUT, len(buf.getvalue()), "bytes")


if __name__ == "__main__":
    main()
