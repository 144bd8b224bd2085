"""The shared steps of the host-pointer batch searches (vectordb-from-scratch_amd/csrc/vdb_hostio.h: the batch-shape check,
the id-mask stager, the copy-out) on the CPU: a stand-alone program whose own fakes stand in for the few runtime calls the
header makes, built with AddressSanitizer and UBSan.  It links no HIP runtime and needs no GPU; what it checks is listed in
tests/cpp/hostio_test.cpp."""
import os
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "hostio_test.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "hostio_test")


def test_host_io_under_sanitizers():
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", EXE]
    subprocess.check_call(cmd)
    out = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "host io ok" in out.stdout
