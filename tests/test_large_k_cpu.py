"""The large-k range's row floor (vdb_flat_large_k_min_rows, include/vdb_flat.h), host arithmetic only: no GPU needed."""
from conftest import load_package


def test_large_k_row_floor():
    L = load_package()._ffi.lib()
    f = L.vdb_flat_large_k_min_rows
    assert f(0) == 0 and f(10) == 0 and f(112) == 0 and f(1025) == 0 and f(1 << 40) == 0
    assert f(113) > 70_000                                   # 70 000 rows at k = 113 stay on the exact scan
    assert f(300) <= 125_000                                 # one eighth of a 1M-row index at k <= 300
    assert f(1024) <= 1_000_000
    prev = 0
    for k in range(113, 1025):
        assert f(k) >= max(prev, 65536)
        prev = f(k)
    assert f(113) == 240 * (113 + 192) and f(1024) == 240 * (1024 + 192)
