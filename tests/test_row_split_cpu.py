"""The codec of the SPLIT row layout (csrc/row_split.h) on the CPU: tests/cpp/row_split_test.cpp walks the listed edge patterns,
10^7 random ones and -- for the rounding claim the certificate rests on -- every finite f32 pattern."""
import os
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "row_split_test.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "row_split_test")


def _build():
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-pthread", "-I", os.path.join(ROOT, "vectordb-from-scratch_amd", "csrc"), SRC, "-o", EXE]
    subprocess.check_call(cmd)
    return EXE


def test_row_split_codec_round_trips_and_rounds_within_half_an_ulp():
    out = subprocess.run([_build()], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "row split ok" in out.stdout
