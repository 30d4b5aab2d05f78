"""The wide QR fill's host-side surface (no GPU): the compiled limits, the cache size and the
Python width-class helper."""
import os

import pytest

from gflownet_spai_amd import _lib

pytestmark = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libspai_hip.so not built (run build())")


def test_wide_limits_cover_the_issue():
    from gflownet_spai_amd import kernels
    mw, mwa, mrows = kernels.qr_wide_limits()
    assert mw >= 32 and mwa >= 32 and mrows >= 256
    lib = _lib.load()
    assert lib.spai_qr_wide_limits(None, None, None) == _lib.SPAI_ERR_INVALID


def test_wide_cache_bytes():
    lib = _lib.load()
    assert lib.spai_qr_wide_cache_bytes(0, 25) == 0 and lib.spai_qr_wide_cache_bytes(-3, 25) == 0
    assert lib.spai_qr_wide_cache_bytes(100, 0) == 0 and lib.spai_qr_wide_cache_bytes(100, 33) == 0
    # one record per line: packed R, Q^T e, the tail
    assert lib.spai_qr_wide_cache_bytes(100, 25) == 100 * (25 * 26 // 2 + 25 + 1) * 8
    sizes = [lib.spai_qr_wide_cache_bytes(n, W) for n, W in ((100, 9), (100, 25), (100, 32), (1000, 32))]
    assert sizes == sorted(sizes) and len(set(sizes)) == 4


def test_wide_entry_points_reject_widths_past_the_limits_before_any_device_access():
    lib = _lib.load()
    p = 4096  # never dereferenced
    rc = lib.spai_qr_wide_max_rows(10, 33, p, 7, p, p, None)
    assert rc == _lib.SPAI_ERR_UNSUPPORTED and b"32" in lib.spai_last_error()
    rc = lib.spai_qr_wide_factor(10, 25, p, 7, p, p, _lib.DTYPE_F64, 257, p, 1 << 30, None)
    assert rc == _lib.SPAI_ERR_UNSUPPORTED and b"256" in lib.spai_last_error()
    rc = lib.spai_qr_wide_factor(10, 25, p, 7, p, p, _lib.DTYPE_F64, 60, p, 8, None)
    assert rc == _lib.SPAI_ERR_INVALID and b"rcache too small" in lib.spai_last_error()
    rc = lib.spai_fill_lines_qr_wide(10, 0, 10, 33, p, p, 1 << 30, 1, p, 1, 0, None, _lib.DTYPE_F64, p, 1 << 20, None)
    assert rc == _lib.SPAI_ERR_UNSUPPORTED
    rc = lib.spai_fill_lines_qr_wide(10, 0, 10, 25, p, p, 8, 1, p, 1, 0, None, _lib.DTYPE_F64, p, 1 << 20, None)
    assert rc == _lib.SPAI_ERR_INVALID and b"rcache too small" in lib.spai_last_error()


def test_width_class_of_wide_lines_is_not_13():
    from gflownet_spai_amd import kernels
    assert [kernels.qr_class(*w) for w in ((5, 5), (7, 7), (13, 7))] == [5, 7, 13]
    for w in ((25, 7), (9, 9), (27, 27), (10, 10), (14, 7), (13, 8), (32, 32)):
        assert kernels.qr_class(*w) == kernels.QR_WIDE_CLASS != 13, w
    assert kernels.qr_class(33, 7) == 0 and kernels.qr_class(5, 33) == 0
