"""The numeric range predicates of the C++ host mirror (host/vdb_host.hpp parse_number, MetadataFilter::lt / le / gt / ge):
tests/cpp/numeric_filter_test.cpp is a stand-alone program that creates no index and touches no device, built the way
test_cpp_host.py builds its program plus -fsanitize=address,undefined, and run here, on the host.  It reads the same fixture as
test_numeric_filter_cpu.py.  (It uses no symbol of the shared library, so it is not linked against it: the sanitizers then watch
this program's code and nothing else.)"""
import os
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "numeric_filter_test.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "numeric_filter_test")
FIXTURE = os.path.join(ROOT, "tests", "golden", "numeric_strings.tsv")


def test_cpp_numeric_filters_under_the_sanitizers():
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-static-libubsan",                    # the runtimes inside the program: nothing to load, no load order to get wrong
           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "vectordb-from-scratch_amd", "host"), SRC, "-o", EXE]
    subprocess.check_call(cmd)
    out = subprocess.run([EXE, FIXTURE], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    assert "numeric filter ok" in out.stdout and "runtime error" not in out.stderr
