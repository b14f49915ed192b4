"""csrc/gcm_dispatch.h, the helper every launcher picks its kernel instantiation with, as plain host C++:
tests/dispatch_check.cpp is compiled with the host compiler and run; its exit status says whether f was called exactly
once with the matching constants, and not at all on a miss.  No GPU, no HIP."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_compiler():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for cxx in (os.environ.get("CXX"), "c++", "g++", "clang++", os.path.join(rocm, "llvm", "bin", "clang++")):
        path = cxx and shutil.which(cxx)
        if path:
            return path
    return None


def test_pick_calls_once_with_the_matching_constants(tmp_path):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "dispatch_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror",
                            "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "graph-conv-memory_amd", "csrc"),
                            os.path.join(ROOT, "tests", "dispatch_check.cpp"), "-o", exe],
                           capture_output=True, timeout=120)
    assert build.returncode == 0, build.stderr.decode()[-4000:]
    run = subprocess.run([exe], capture_output=True, timeout=60)
    assert run.returncode == 0, run.stdout.decode()[-2000:]
