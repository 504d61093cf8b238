"""Prove csrc/np_log.h against this process's numpy over ALL 2^32 float32 bit patterns.

  host    a C++ twin of the header, compiled here with a real fma (-mfma -ffp-contract=off), called through ctypes, against
          np.log on the same inputs
  device  (--device, GPU box) gsx_np_log_math_dev over all 2^32 inputs in chunks: np_logf of csrc/np_log.h as the .splat
          reader's kernel runs it, against np.log

usage: python tests/devtools/check_np_log.py [--device] [--chunk-log2 24] [--threads 8]      (exit 0 = no mismatch)"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HEADER_DIR = os.path.join(ROOT, "3dgsconverter_amd", "csrc")

TWIN = r"""
#include "np_log.h"
extern "C" void np_logf_range(uint32_t start, int64_t n, uint32_t *out)
{
    for (int64_t i = 0; i < n; ++i) out[i] = gsx::np_f32_bits(gsx::np_logf(gsx::np_bits_f32(start + (uint32_t)i)));
}
"""


def host_twin(tmp):
    src, so = os.path.join(tmp, "twin.cpp"), os.path.join(tmp, "twin.so")
    with open(src, "w") as f:
        f.write(TWIN)
    cxx = os.environ.get("CXX", "g++")
    subprocess.run([cxx, "-O2", "-mfma", "-ffp-contract=off", "-fno-math-errno", "-shared", "-fPIC", "-I", HEADER_DIR, src, "-o", so],
                   check=True)
    lib = C.CDLL(so)
    lib.np_logf_range.argtypes = [C.c_uint32, C.c_int64, C.c_void_p]
    lib.np_logf_range.restype = None
    return lib


def chunk_inputs(start, n):
    return np.arange(start, start + n, dtype=np.uint64).astype(np.uint32).view(np.float32)


def compare(start, x, got):
    with np.errstate(all="ignore"):
        want = np.log(x).view(np.uint32)
    bad = np.nonzero(got != want)[0]
    return len(bad), [(hex(start + int(i)), hex(int(got[i])), hex(int(want[i]))) for i in bad[:4]]


def run_host(chunk, threads):
    with tempfile.TemporaryDirectory() as tmp:
        lib = host_twin(tmp)

        def one(start):
            got = np.empty(chunk, np.uint32)
            lib.np_logf_range(start, chunk, got.ctypes.data)
            return compare(start, chunk_inputs(start, chunk), got)
        return sweep(one, chunk, threads, "host twin")


def run_device(chunk):
    sys.path.insert(0, ROOT)
    import importlib
    lib = importlib.import_module("3dgsconverter_amd._lib")
    ctx = lib.Context(0)
    d_in, d_log = ctx.alloc(4 * chunk), ctx.alloc(4 * chunk)

    def one(start):
        x = chunk_inputs(start, chunk)
        d_in.upload(x)
        lib.check(ctx.lib.gsx_np_log_math_dev(ctx.handle, d_in.ptr, chunk, d_log.ptr), "gsx_np_log_math_dev")
        return compare(start, x, d_log.download(np.uint32, chunk))
    try:
        return sweep(one, chunk, 1, "device log")
    finally:
        for b in (d_in, d_log):
            b.free()
        ctx.close()


def sweep(one, chunk, threads, what):
    t = time.perf_counter()
    starts = list(range(0, 1 << 32, chunk))
    total, examples = 0, []
    with ThreadPoolExecutor(max(1, threads)) as ex:
        for k, (n_bad, ex_bad) in enumerate(ex.map(one, starts)):
            total += n_bad
            examples += ex_bad[:4 - len(examples)] if len(examples) < 4 else []
            if k % 16 == 15:
                print("  %s: %d / %d chunks, %d mismatches so far" % (what, k + 1, len(starts), total), flush=True)
    print("check_np_log: %s vs numpy %s over all 2^32 float32 inputs: %d mismatches (%.1f s)%s"
          % (what, np.__version__, total, time.perf_counter() - t, "" if not examples else "; first: %r" % examples), flush=True)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--chunk-log2", type=int, default=24)
    ap.add_argument("--threads", type=int, default=min(8, os.cpu_count() or 1))
    a = ap.parse_args()
    chunk = 1 << a.chunk_log2
    bad = run_device(chunk) if a.device else run_host(chunk, a.threads)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
