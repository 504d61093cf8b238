"""GPU box: every rotation byte triple through the SOG reader's kernel against numpy's own statements (sog.py:108-142): all
2^24 triples with each alpha byte class -- 252, 253, 254, 255 (the four slots) and one byte below 252 (no slot: zeros).
usage: python tests/devtools/check_sog_read_quat.py"""
import importlib, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sog_read_numpy as srn        # noqa: E402
lib = importlib.import_module("3dgsconverter_amd._lib")
CHUNK = 1 << 22


def run_chunk(first, alpha, tables, dtype):
    i = np.arange(first, first + CHUNK, dtype=np.uint32)
    quats = np.stack([i & 0xFF, (i >> 8) & 0xFF, (i >> 16) & 0xFF, np.full_like(i, alpha)], axis=1).astype(np.uint8)

    def fill(host, place):
        host[:] = 0
        off, nb = place["quats"]
        host[off:off + nb] = quats.reshape(-1)
    rows = lib.sog_unpack_table(fill, CHUNK, 0, 0, tables, dtype)
    q_rest = srn.quat_component_of(quats[:, :3])
    max_comp_idx = quats[:, 3] - 252
    q_missing = np.sqrt(np.maximum(1.0 - np.sum(q_rest ** 2, axis=1), 0.0))
    ok = True
    for mc in range(4):
        want = np.zeros(CHUNK, np.float32)
        m = max_comp_idx == mc
        want[m] = q_missing[m]
        for other in range(4):
            if other != mc:
                k = max_comp_idx == other
                want[k] = q_rest[k, mc - (mc > other)]
        bad = np.nonzero(rows["rot_%d" % mc].view(np.uint32) != want.view(np.uint32))[0]
        if len(bad):
            ok = False
            print("check_sog_read_quat: alpha %d rot_%d: %d rows differ, first triple %s: %r != %r"
                  % (alpha, mc, len(bad), quats[bad[0], :3].tolist(), rows["rot_%d" % mc][bad[0]], want[bad[0]]), flush=True)
    return ok


if __name__ == "__main__":
    tables = lib.sog_read_tables(srn.MINS, srn.MAXS, [0.0] * 256, [0.0] * 256)
    dtype = srn.define_dtype(0)
    t, ok = time.perf_counter(), True
    for alpha in (252, 253, 254, 255, 7):
        for first in range(0, 1 << 24, CHUNK):
            ok &= run_chunk(first, alpha, tables, dtype)
        print("check_sog_read_quat: alpha %d, all 2^24 triples done (%.0f s) %s" % (alpha, time.perf_counter() - t, "ok" if ok else "DIFFER"), flush=True)
    print("check_sog_read_quat: %s" % ("EQUAL" if ok else "DIFFER"))
    sys.exit(0 if ok else 1)
