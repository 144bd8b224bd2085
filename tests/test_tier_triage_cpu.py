"""The tier hand-over of a search and the flag-block structs (vectordb-from-scratch_amd/csrc/vdb_flags.h) on the CPU: a
stand-alone program built with AddressSanitizer and UBSan.  The header includes nothing of HIP, so the program links no HIP
runtime and needs no GPU; what it checks is listed in tests/cpp/tier_triage_test.cpp."""
import os
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "tier_triage_test.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "tier_triage_test")


def test_tier_triage_under_sanitizers():
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", EXE]
    subprocess.check_call(cmd)
    out = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "tier triage ok" in out.stdout
