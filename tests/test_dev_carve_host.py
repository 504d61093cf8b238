"""csrc/dev_carve.h on the host: tools/check_dev_carve_host.cpp, compiled as it stands (no sanitizer flags here; its header says
how to run it under them) and run as a program.  It checks, for the layouts the library carves its context buffers with, that
the measured size is the last region's end, that regions neither overlap nor miss their alignment, that a region of count 0 is
valid and that measuring does not depend on the base."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compiler():
    for cxx in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if cxx and (shutil.which(cxx) or os.path.exists(cxx)):
            return cxx
    return None


def test_check_dev_carve_host(tmp_path):
    cxx = _compiler()
    assert cxx, "no C++ compiler found (c++, g++, clang++ or ROCm's clang++)"
    exe = str(tmp_path / "check_dev_carve_host")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tools", "check_dev_carve_host.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    assert not build.stderr.strip(), "warnings:\n" + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
