"""The stored runs of the reference's own ``Converter.run`` and ``report_info`` (tests/golden/converter_ref.npz, written by
tests/devtools/make_golden_converter.py) as the two converter tests read them."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "converter_ref.npz")
REFERENCE_VERSION = "0.8"
# The reference's wording where it names the backend that did the work, and this package's (processing/data_processor.py,
# formats/sog_writer.py): the reference ran without Taichi, this package runs on the device.  Everything else in a line is equal.
BACKEND_WORDING = (("[SOR] Building KDTree (CPU Fallback)...", "[SOR] Determining outliers on GPU (HIP gfx950, exact KNN, device-resident chain)..."),
                   ("After removing flyers, retained ", "After removing flyers (GPU), retained "),
                   ("Strategy: CPU (Fallback)", "Strategy: GPU (HIP gfx950)"))


class Case:
    def __init__(self, name, rec, g):
        self.name, self.input_name, self.target, self.kwargs = name, rec["input"], rec["target"], rec["kwargs"]
        self.lines, self.info_in, self.info_out, self.record = rec["lines"], rec["info_in"], rec["info_out"], rec["record"]
        self.input = bytes(g[rec["blobs"]["input"]])
        self.output = {k: g[v] for k, v in rec["blobs"].items() if k != "input"}

    def __repr__(self):
        return self.name


def load_cases():
    with np.load(GOLD) as g:
        spec = json.loads(bytes(g["spec"]))
        return [Case(name, spec[name], g) for name in sorted(spec)]


def expected_lines(lines, tmp, version):
    """the reference's stdout lines as this package prints them: its temporary directory, its version, its backend's name"""
    out = []
    for ln in lines:
        ln = ln.replace("<TMP>", tmp)
        if ln == f"3D Gaussian Splatting Converter: {REFERENCE_VERSION}":
            ln = f"3D Gaussian Splatting Converter: {version}"
        for ref, here in BACKEND_WORDING:
            ln = ln.replace(ref, here)
        out.append(ln)
    return out
