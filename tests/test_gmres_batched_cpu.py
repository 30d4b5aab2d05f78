"""Batched GMRES without a device: argument validation of the new entry points through the loaded
library (every check runs before any device access: the pointers below are never dereferenced),
the workspace size, and the row view of a column-oriented pattern against lines_to_coo."""
import os

import numpy as np
import pytest
import torch

from gflownet_spai_amd import _lib

needs_lib = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libspai_hip.so not built (run build())")
P = 4096  # a non-null address that is never read
F32, F64 = _lib.DTYPE_F32, _lib.DTYPE_F64


def _spmv(n=100, W=5, B=2, idx=P, ibs=0, val=P, dt=F64, vbs=0, src=None, x=P, y=P, active=None):
    return (n, W, B, idx, ibs, val, dt, vbs, src, x, y, active, None)


def _init(n=100, B=2, restart=20, maxiter=50, rtol=1e-5, atol=0.0, W=5, idx=P, ibs=0, val=P, dt=F64, vbs=0, src=None,
          rhs=P, x=P, report=P, ws=P, ws_bytes=1 << 40):
    return (n, B, restart, maxiter, rtol, atol, W, idx, ibs, val, dt, vbs, src, rhs, x, report, ws, ws_bytes, None)


def _cycle(n=100, B=2, restart=20, maxiter=50, aW=5, aidx=P, aval=P, adt=F64, W=5, idx=P, ibs=0, val=P, dt=F64, vbs=0,
           src=None, rhs=P, x=P, report=P, ws=P, ws_bytes=1 << 40):
    return (n, B, restart, maxiter, aW, aidx, aval, adt, W, idx, ibs, val, dt, vbs, src, rhs, x, report, ws, ws_bytes,
            None)


@needs_lib
def test_batched_spmv_argument_validation():
    lib = _lib.load()
    name = b"spai_ell_spmv_batched"
    for kw in (dict(idx=None), dict(val=None), dict(x=None), dict(y=None)):
        assert lib.spai_ell_spmv_batched(*_spmv(**kw)) == _lib.SPAI_ERR_INVALID
        assert name in lib.spai_last_error() and b"null pointer" in lib.spai_last_error()
    for kw in (dict(B=0), dict(B=-2), dict(n=0), dict(W=0), dict(dt=7), dict(ibs=3), dict(vbs=-1),
               dict(src=P, ibs=500)):
        assert lib.spai_ell_spmv_batched(*_spmv(**kw)) == _lib.SPAI_ERR_INVALID, kw
        assert name in lib.spai_last_error(), kw


@needs_lib
@pytest.mark.parametrize("fn,args", [("spai_gmres_batched_init", _init), ("spai_gmres_batched_cycle", _cycle)])
def test_gmres_entry_points_argument_validation(fn, args):
    lib = _lib.load()
    call = getattr(lib, fn)
    bad = [dict(B=0), dict(n=0), dict(restart=0), dict(maxiter=0), dict(dt=5), dict(W=0), dict(idx=None),
           dict(val=None), dict(rhs=None), dict(x=None), dict(report=None), dict(ws=None), dict(ws_bytes=64),
           dict(ibs=7), dict(src=P, ibs=500)]
    if fn.endswith("init"):
        bad += [dict(rtol=-1.0), dict(atol=-1.0)]
    else:
        bad += [dict(aidx=None), dict(aval=None), dict(adt=9), dict(aW=0)]
    for kw in bad:
        assert call(*args(**kw)) == _lib.SPAI_ERR_INVALID, kw
        assert fn.encode() in lib.spai_last_error(), (kw, lib.spai_last_error())
    rc = call(*args(restart=65))
    assert rc == _lib.SPAI_ERR_UNSUPPORTED and fn.encode() in lib.spai_last_error()
    assert b"restart 65" in lib.spai_last_error()
    with pytest.raises(NotImplementedError):
        _lib.check(rc, fn)


@needs_lib
def test_gmres_workspace_bytes_positive_and_monotone():
    lib = _lib.load()
    ws = lib.spai_gmres_workspace_bytes
    base = ws(1000, 4, 20)
    assert base >= 4 * 21 * 1000 * 8  # at least the Krylov bases
    assert ws(1, 1, 1) > 0
    assert ws(0, 4, 20) == 0 and ws(1000, 0, 20) == 0 and ws(1000, 4, 0) == 0
    for n0, n1 in ((1, 2), (255, 256), (256, 257), (1000, 1001), (65536, 300000), (300000, 1300000)):
        assert ws(n0, 4, 20) <= ws(n1, 4, 20)
    assert ws(1000, 4, 20) < ws(2000, 4, 20) and ws(1000, 4, 20) < ws(1000, 5, 20) < ws(1000, 8, 20)
    sizes = [ws(1000, 4, r) for r in range(1, 65)]
    assert all(a < b for a, b in zip(sizes, sizes[1:]))


@pytest.mark.parametrize("seed,n,density", [(0, 40, 0.1), (1, 300, 0.02), (2, 7, 0.6)])
def test_row_view_of_column_lines_rebuilds_m(seed, n, density):
    """M rebuilt from (idx, src, values) of the row view equals lines_to_coo of the column lines."""
    import scipy.sparse as sp
    from gflownet_spai_amd.gmres import row_view
    from gflownet_spai_amd.layout import build_lines, lines_to_coo
    Pm = (sp.random(n, n, density=density, random_state=seed, format="coo") + sp.identity(n)).tocoo()
    rows, cols = torch.from_numpy(Pm.row.astype(np.int64)), torch.from_numpy(Pm.col.astype(np.int64))
    L = build_lines(rows, cols, torch.ones(rows.numel()), n, "col", "cpu", torch.float32)
    idx, src = row_view(L)
    assert idx.dtype == torch.int32 and src.dtype == torch.int32 and idx.shape == src.shape
    assert int(src.min()) >= 0 and int(src.max()) < n * L.width
    g = torch.Generator().manual_seed(seed)
    vals = torch.randn(n, L.width, generator=g, dtype=torch.float64)
    vals[L.idx < 0] = 0.0
    vals[torch.rand(n, L.width, generator=g) < 0.2] = 0.0  # removed entries hold 0
    ref = lines_to_coo(L, vals, n).to_dense()
    ok = idx.reshape(-1) >= 0
    ri = torch.arange(n).repeat_interleave(idx.shape[1])[ok]
    got = torch.zeros(n, n, dtype=torch.float64)
    got[ri, idx.reshape(-1)[ok].long()] = vals.reshape(-1)[src.reshape(-1)[ok].long()]
    assert torch.equal(got, ref)
    assert int(ok.sum()) == int((L.idx >= 0).sum())
    cols_sorted = idx.long().clone()
    cols_sorted[idx < 0] = n
    assert bool((cols_sorted[:, 1:] >= cols_sorted[:, :-1]).all())  # slot order = column order, padding last


def test_gmres_batched_rejects_host_callables():
    from gflownet_spai_amd.gmres import DeviceOperator, gmres_batched
    A = object.__new__(DeviceOperator)  # no device here: the type check comes before any device work
    A.n, A.shape, A.device = 4, (4, 4), torch.device("cpu")
    with pytest.raises(TypeError, match="solve_with_gmres"):
        gmres_batched(A, np.ones(4), M=lambda v: v)
    with pytest.raises(TypeError, match="solve_with_gmres"):
        gmres_batched(A, np.ones(4), M=[None, lambda v: v])
