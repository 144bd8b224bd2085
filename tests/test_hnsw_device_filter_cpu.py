"""HNSW search under a filter compiled on the device (include/vdb_hnsw.h vdb_hnsw_search_batch_filtered): what can be checked
without a GPU -- the built library exports the call and its test hook, the header declares them, the Python binding names them,
and the ABI version did not move."""
import ctypes
import os
import re

from conftest import ROOT, load_package

NEW = ("vdb_hnsw_search_batch_filtered", "vdb_hnsw_debug_present_mask")


def test_library_exports_and_binding_declares_the_filtered_search():
    vdb = load_package()
    L = ctypes.CDLL(vdb.build())
    for name in NEW:
        assert hasattr(L, name), f"{name} is not exported"
        assert name in vdb._ffi.SYMBOLS
    assert L.vdb_abi_version() == 1


def test_header_declares_the_filtered_search():
    with open(os.path.join(ROOT, "include", "vdb_hnsw.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)          # declarations only, not the prose
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    assert re.search(r"vdb_hnsw_search_batch_filtered\s*\([^)]*const\s+vdb_meta_mask\s*\*\s*mask", header)


def test_python_index_takes_a_compiled_mask():
    import inspect
    vdb = load_package()
    for fn in (vdb.GpuHnswIndex.search_batch_arrays, vdb.GpuHnswIndex.search_batch):
        assert inspect.signature(fn).parameters["compiled_mask"].default is None
    assert callable(vdb.GpuHnswIndex.debug_present_mask)
