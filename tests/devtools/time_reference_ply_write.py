"""Build box: the reference's own Ply3DGSFormat.write and PlyCCFormat.write (CPU) on PROBE_N-row tables of the five layouts of
tools/probe_ply_write.py, three runs each -- the figures profiles/ply_writer_10m.txt sets the device writer's call against.
plyfile is not installed here: ``PlyElement.describe`` keeps the array and ``PlyData(...).write`` does nothing, so the clock is
the reference's numpy part -- the crop_sh scans, the zeroed output table and the column copies -- which is what the device
path replaces; the container's own write is not in it.
    python tests/devtools/time_reference_ply_write.py            # PROBE_N=1000000"""
import json, os, sys, time, types
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ply_write_numpy as pw       # noqa: E402
import probe_ply_write as probe    # noqa: E402
from oracle import refload         # noqa: E402


class NoWritePlyData:
    def __init__(self, elements, text=False, byte_order="<"):
        self.elements = list(elements)

    def write(self, path):
        pass


def main():
    stub = types.ModuleType("plyfile")
    stub.PlyData, stub.PlyElement = NoWritePlyData, pw.StandInElement
    sys.modules["plyfile"] = stub
    refload.load()
    import gsconverter.formats.ply_3dgs as m3  # type: ignore
    import gsconverter.formats.ply_cc as mcc   # type: ignore
    for m in (m3, mcc):
        m.PlyData, m.PlyElement = NoWritePlyData, pw.StandInElement
        m.status_print = lambda *a, **k: None
    n = int(os.environ.get("PROBE_N", 1_000_000))
    for name, fields, zero_rest, dialect, crop in probe.probe_tables():
        table = probe.repeated_table(fields, n, zero_rest)
        fmt = m3.Ply3DGSFormat() if dialect == "3dgs" else mcc.PlyCCFormat()
        runs = []
        for _ in range(3):
            t = time.perf_counter()
            with np.errstate(all="ignore"):
                fmt.write(table, os.devnull, crop_sh=crop)
            runs.append(round(time.perf_counter() - t, 3))
        print(json.dumps({"table": name, "reference_write_numpy_s": runs, "writer": dialect, "crop_sh": crop, "n": n}), flush=True)


if __name__ == "__main__":
    main()
