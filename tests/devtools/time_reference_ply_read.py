"""Build box: the reference's own Ply3DGSFormat.read and PlyCCFormat.read (CPU) on PROBE_N-row files of the three layouts of
tools/probe_ply_read.py, three runs each -- the figures profiles/ply_reader_10m.txt sets the device reader's call against.
plyfile is not installed here: ``PlyData.read`` is the stub of tests/devtools/make_golden_ply_read.py, made to hand the
reference a memory map of the file as plyfile does (np.memmap of the vertex rows), so the clock is the reference's mapping loop
with its page faults, not a parser's copy.
    python tests/devtools/time_reference_ply_read.py            # PROBE_N=1000000"""
import json, os, sys, tempfile, time, types
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ply_read_numpy as pn        # noqa: E402
import probe_ply_read as probe     # noqa: E402
from oracle import refload         # noqa: E402


class MappedPlyData(pn.PlyData):
    """the stub's PlyData over a memory map of a single-element file"""

    @staticmethod
    def read(path):
        with open(path, "rb") as f:
            head = f.read(1 << 16)
        end = head.index(b"end_header\n") + len(b"end_header\n")
        name, count, props = None, 0, []
        for line in head[:end].decode("ascii").splitlines():
            w = line.split()
            if w[0] == "element":
                name, count = w[1], int(w[2])
            elif w[0] == "property":
                t = pn.TYPES[w[1]]
                props.append((w[2], "<" + t if t[1] != "1" else "|" + t))
        return pn.PlyData([(name, np.memmap(path, np.dtype(props), "r", end, (count,)))])


def main(tmp):
    stub = types.ModuleType("plyfile")
    stub.PlyData, stub.PlyElement = MappedPlyData, object
    sys.modules["plyfile"] = stub
    refload.load()
    import gsconverter.formats.ply_3dgs as m3  # type: ignore
    import gsconverter.formats.ply_cc as mcc   # type: ignore
    n = int(os.environ.get("PROBE_N", 1_000_000))
    for name, fields, dialect in probe.probe_files():
        path = probe.write_repeated(os.path.join(tmp, name + ".ply"), fields, n)
        fmt = m3.Ply3DGSFormat() if dialect == "3dgs" else mcc.PlyCCFormat()
        runs = []
        for _ in range(3):
            t = time.perf_counter()
            with np.errstate(all="ignore"):
                rows = fmt.read(path)
            runs.append(round(time.perf_counter() - t, 3))
        assert len(rows) == n
        print(json.dumps({"file": name, "reference_read_s": runs, "reader": dialect, "n": n}), flush=True)
        os.remove(path)


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as tmp:
        main(tmp)
