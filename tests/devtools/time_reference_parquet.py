"""Build box: the reference's own ParquetFormat.write and ParquetFormat.read (CPU, pandas and pyarrow) on the PROBE_N-row table
of tools/probe_parquet.py, three runs each -- the figures profiles/parquet_10m.txt sets the device path's calls against.  Beside
them the codec alone on the same file: pq.read_table, and pq.write_table of the table pq.read_table returned.
    python tests/devtools/time_reference_parquet.py            # PROBE_N=1000000"""
import contextlib, io, json, os, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import probe_parquet as probe      # noqa: E402
from oracle import refload         # noqa: E402


def clock(fn, runs=3):
    out = []
    for _ in range(runs):
        t = time.perf_counter()
        with np.errstate(all="ignore"), contextlib.redirect_stdout(io.StringIO()):
            res = fn()
        out.append(round(time.perf_counter() - t, 3))
    return out, res


def main(tmp):
    import pyarrow.parquet as pq
    refload.load()
    from gsconverter.formats.parquet import ParquetFormat  # type: ignore
    n = int(os.environ.get("PROBE_N", 1_000_000))
    t = probe.table(n)
    path = os.path.join(tmp, "ref.parquet")
    fmt = ParquetFormat()
    w, _ = clock(lambda: fmt.write(t, path))
    r, rows = clock(lambda: fmt.read(path))
    assert len(rows) == n
    c, tab = clock(lambda: pq.read_table(path))
    e, _ = clock(lambda: pq.write_table(tab, os.path.join(tmp, "again.parquet"), compression="snappy"))
    print(json.dumps({"n": n, "file_bytes": os.path.getsize(path), "reference_write_s": w, "reference_read_s": r, "pq_read_table_s": c, "pq_write_table_s": e}), flush=True)


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as tmp:
        main(tmp)
