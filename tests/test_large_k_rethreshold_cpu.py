"""VDB_TIERS_FORCE_RETHRESHOLD at the boundary (include/vdb_flat.h, index.py), no GPU needed.  That vdb_flat_set_tiers refuses
flag 32 needs a handle, and a handle needs a device: tests/test_gpu_large_k_rethreshold.py checks it."""
import ctypes
import os
import re

from conftest import ROOT, load_package


def _header():
    return open(os.path.join(ROOT, "include", "vdb_flat.h")).read()


def test_the_header_defines_the_flag_as_16_and_python_agrees():
    flags = {name: int(val) for name, val in re.findall(r"#define\s+(VDB_TIERS_[A-Z0-9_]+)\s+(\d+)u", _header())}
    assert flags["VDB_TIERS_FORCE_RETHRESHOLD"] == 16
    assert sorted(flags.values()) == [1, 2, 4, 8, 16]              # one bit each: vdb_flat_set_tiers accepts flags & ~31u == 0
    ix = load_package().GpuFlatIndex
    for name, val in flags.items():
        assert getattr(ix, name[len("VDB_"):]) == val, name


def test_the_library_exports_what_the_header_declares():
    vdb = load_package()
    L = ctypes.CDLL(vdb.build())
    header = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = set(re.findall(r"\b(vdb_[a-z0-9_]+)\s*\(", header)) - {"vdb_status", "vdb_metric"}
    assert "vdb_flat_set_tiers" in declared and "vdb_flat_last_stats_ex" in declared
    for name in sorted(declared):
        assert hasattr(L, name), name
