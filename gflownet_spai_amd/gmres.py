"""GMRES evaluation of a preconditioner on the MI355X.

Reference: GFlowNet100.py:61-93 ``solve_with_gmres(A, b, M=None)`` =
``scipy.sparse.linalg.gmres(A, b, x0=0, M=M, maxiter=10260, callback=callback)`` (restart 20,
rtol 1e-5, left preconditioning, legacy callback = preconditioned relative residual per inner
iteration), and GFlowNet100.py:126-132 (the spilu baseline as a LinearOperator).

``_gmres`` restates scipy 1.15's ``gmres`` (scipy/sparse/linalg/_isolve/iterative.py) step for
step: Arnoldi with modified Gram-Schmidt, LAPACK ``lartg`` Givens rotations, the gh-8400 inner
tolerance control, the same breakdown and exit rules.  The Krylov basis and every length-n
vector live on the GPU; A v and M v run on ``spai_ell_spmv`` (row-ELL, fp64); the dot products
and axpys of the Gram-Schmidt are device ops; only the (restart+1)-sized Hessenberg column
crosses to the host once per inner iteration, where the rotations run in fp64 exactly as scipy
runs them.  Preconditioners: None, a sparse matrix (SPAI M: applied on the GPU) or a host
callable / LinearOperator (e.g. the spilu baseline: applied on the host, copied each way).

``gmres_batched`` / ``evaluate_candidates`` run the same algorithm for B samples in lock step
entirely on the device (csrc/krylov_batched.hip): one shared A, a different M per sample
(``BatchedOperator``: the env's ``last_m`` read in place, or a list of sparse matrices), classical
Gram-Schmidt with one re-orthogonalisation instead of the modified one, 8 launches per inner
iteration whatever B and the iteration, and one host read per restart cycle.
"""
from __future__ import annotations

import time
from dataclasses import dataclass
from typing import Callable

import numpy as np
import torch

from . import _lib, kernels
from .layout import Lines, build_lines


class DeviceOperator:
    """y = A x on the GPU for a square sparse A held as row-ELL lines (values fp32 or fp64)."""

    def __init__(self, A, device=None, dtype=None):
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if isinstance(A, Lines):
            if A.orient != "row":
                raise ValueError("DeviceOperator needs row lines")
            self.lines, self.n = A, A.n
        else:
            rows, cols, vals, n = _coo_of(A)
            vd = dtype or (torch.float64 if vals.dtype == torch.float64 else torch.float32)
            self.lines = build_lines(rows, cols, vals, n, "row", dev, vd)
            self.n = n
        self.shape = (self.n, self.n)
        self.device = self.lines.idx.device
        _lib.require_device(self.lines.idx)

    def matvec_into(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        L = self.lines
        dt = 1 if L.val.dtype == torch.float64 else 0  # SPAI_DTYPE_F64 / SPAI_DTYPE_F32
        st = kernels._l().spai_ell_spmv(self.n, L.width, _lib.ptr(L.idx), _lib.ptr(L.val), dt, _lib.ptr(x),
                                        _lib.ptr(y), _lib.stream_ptr(self.device))
        _lib.check(st, "spai_ell_spmv")
        return y

    def matvec(self, x: torch.Tensor) -> torch.Tensor:
        if x.dtype != torch.float64 or not x.is_contiguous() or x.device != self.device:
            raise ValueError("DeviceOperator.matvec takes a contiguous fp64 vector on its device")
        return self.matvec_into(x, torch.empty_like(x))


def _coo_of(A):
    """(rows, cols, vals, n) of a scipy sparse matrix or a torch sparse tensor, duplicates summed."""
    if isinstance(A, torch.Tensor):
        if not A.is_sparse:
            raise ValueError("A must be sparse")
        c = A.coalesce()
        return c.indices()[0], c.indices()[1], c.values(), int(A.shape[0])
    import scipy.sparse as sp
    if not sp.issparse(A):
        raise ValueError("A must be a scipy sparse matrix, a torch sparse tensor or Lines")
    c = sp.coo_matrix(A)
    c.sum_duplicates()
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt))  # noqa: E731
    vdt = np.float64 if c.dtype == np.float64 else np.float32
    return t(c.row, np.int64), t(c.col, np.int64), t(c.data, vdt), int(c.shape[0])


def _host_psolve(fn, device) -> Callable[[torch.Tensor], torch.Tensor]:
    def apply(v: torch.Tensor) -> torch.Tensor:
        out = np.asarray(fn(v.detach().cpu().numpy()), dtype=np.float64).reshape(-1)
        return torch.from_numpy(out).to(device)
    return apply


def _gmres(matvec, psolve, b: torch.Tensor, x0: torch.Tensor | None = None, *, rtol=1e-5, atol=0.0, restart=None,
           maxiter=None, callback=None):
    """scipy.sparse.linalg.gmres (legacy callback semantics) on torch vectors; returns (x, info).
    ``matvec``/``psolve`` map a length-n fp64 tensor to one on the same device."""
    from scipy.linalg import get_lapack_funcs

    n = b.numel()
    x = torch.zeros_like(b) if x0 is None else x0.clone()
    bnrm2 = float(torch.linalg.vector_norm(b))
    if atol is None or atol < 0:
        raise ValueError("atol must be a real, non-negative number")
    atol = max(float(atol), float(rtol) * bnrm2)
    if bnrm2 == 0:
        return b.clone(), 0
    eps = np.finfo(np.float64).eps
    if maxiter is None:
        maxiter = n * 10
    restart = min(20 if restart is None else restart, n)
    Mb_nrm2 = float(torch.linalg.vector_norm(psolve(b)))
    ptol_max_factor = 1.0
    ptol = Mb_nrm2 * min(ptol_max_factor, atol / bnrm2)
    presid = 0.0
    lartg = get_lapack_funcs("lartg", dtype=np.float64)
    v = torch.empty(restart + 1, n, dtype=torch.float64, device=b.device)
    h = np.zeros([restart, restart + 1], dtype=np.float64)
    givens = np.zeros([restart, 2], dtype=np.float64)
    hcol = torch.empty(restart + 3, dtype=torch.float64, device=b.device)
    inner_iter = 0
    rnorm = float("inf")
    for iteration in range(maxiter):
        if iteration == 0:
            r = b - matvec(x) if bool(x.any()) else b.clone()
            if float(torch.linalg.vector_norm(r)) < atol:
                return x, 0
        v[0] = psolve(r)
        tmp = float(torch.linalg.vector_norm(v[0]))
        v[0] *= 1 / tmp
        S = np.zeros(restart + 1, dtype=np.float64)
        S[0] = tmp
        breakdown = False
        for col in range(restart):
            w = psolve(matvec(v[col]))
            hcol[0] = torch.linalg.vector_norm(w)
            for k in range(col + 1):  # modified Gram-Schmidt, on the device
                t = torch.dot(v[k], w)
                hcol[1 + k] = t
                w -= t * v[k]
            hcol[col + 2] = torch.linalg.vector_norm(w)
            hh = hcol[:col + 3].cpu().numpy()  # the one host round trip of the inner iteration
            h0, h1 = hh[0], hh[col + 2]
            h[col, :col + 1] = hh[1:col + 2]
            h[col, col + 1] = h1
            v[col + 1] = w
            if h1 <= eps * h0:
                h[col, col + 1] = 0
                breakdown = True
            else:
                v[col + 1] *= 1 / h1
            for k in range(col):
                c, s = givens[k, 0], givens[k, 1]
                n0, n1 = h[col, [k, k + 1]]
                h[col, [k, k + 1]] = [c * n0 + s * n1, -np.conj(s) * n0 + c * n1]
            c, s, mag = lartg(h[col, col], h[col, col + 1])
            givens[col, :] = [c, s]
            h[col, [col, col + 1]] = mag, 0
            tmp = -np.conjugate(s) * S[col]
            S[[col, col + 1]] = [c * S[col], tmp]
            presid = np.abs(tmp)
            inner_iter += 1
            if callback is not None:
                callback(presid / bnrm2)
            if callback is not None and inner_iter == maxiter:
                break
            if presid <= ptol or breakdown:
                break
        if h[col, col] == 0:
            S[col] = 0
        y = np.zeros([col + 1], dtype=np.float64)
        y[:] = S[:col + 1]
        for k in range(col, 0, -1):
            if y[k] != 0:
                y[k] /= h[k, k]
                tmp = y[k]
                y[:k] -= tmp * h[k, :k]
        if y[0] != 0:
            y[0] /= h[0, 0]
        x += torch.from_numpy(y).to(b.device) @ v[:col + 1]
        r = b - matvec(x)
        rnorm = float(torch.linalg.vector_norm(r))
        if callback is not None and inner_iter == maxiter:
            return x, 0 if rnorm <= atol else maxiter
        if rnorm <= atol:
            break
        elif breakdown:
            break
        elif presid <= ptol:
            ptol_max_factor = max(eps, 0.25 * ptol_max_factor)
        else:
            ptol_max_factor = min(1.0, 1.5 * ptol_max_factor)
        ptol = presid * min(ptol_max_factor, atol / rnorm)
    info = 0 if rnorm <= atol else maxiter
    return x, info


def gmres(A, b, x0=None, *, M=None, rtol=1e-5, atol=0.0, restart=None, maxiter=None, callback=None, device=None):
    """scipy.sparse.linalg.gmres on the GPU: A (scipy / torch sparse, Lines or DeviceOperator),
    M None | sparse (applied on the GPU) | host callable or LinearOperator.  Returns (x, info)
    with x an fp64 device tensor."""
    Aop = A if isinstance(A, DeviceOperator) else DeviceOperator(A, device=device)
    dev = Aop.device
    bt = torch.as_tensor(np.asarray(b, dtype=np.float64).reshape(-1) if not isinstance(b, torch.Tensor) else b,
                         dtype=torch.float64).reshape(-1).to(dev).contiguous()
    if bt.numel() != Aop.n:
        raise ValueError(f"Shape mismatch: A is {Aop.shape}, but b is {tuple(bt.shape)}")
    if M is None:
        psolve = lambda v: v.clone()  # noqa: E731  (scipy's IdentityOperator returns a copy)
    elif isinstance(M, DeviceOperator):
        psolve = M.matvec
    elif isinstance(M, torch.Tensor) or hasattr(M, "tocoo") and not hasattr(M, "matvec"):
        psolve = DeviceOperator(M, device=dev).matvec
    else:
        import scipy.sparse as sp
        if sp.issparse(M):
            psolve = DeviceOperator(M, device=dev).matvec
        else:
            fn = M.matvec if hasattr(M, "matvec") else M
            psolve = _host_psolve(fn, dev)
    x0t = None if x0 is None else torch.as_tensor(np.asarray(x0, np.float64)).to(dev)
    return _gmres(lambda v: Aop.matvec(v.contiguous()), lambda v: psolve(v.contiguous()), bt, x0t, rtol=rtol,
                  atol=atol, restart=restart, maxiter=maxiter, callback=callback)


def solve_with_gmres(A, b, M=None, *, verbose: bool = True, device=None, maxiter: int = 10260):
    """GFlowNet100.py:61-93: (x, residuals, num_iterations, elapsed_time) of GMRES from x0 = 0
    with maxiter = 10260 (the driver's; a keyword lowers it for large evaluations), recording the
    legacy callback's preconditioned relative residual of every inner iteration; x is returned
    as a host numpy array like the reference's."""
    b = np.asarray(b, dtype=np.float64).reshape(-1) if not isinstance(b, torch.Tensor) else b.reshape(-1)
    n = A.n if isinstance(A, DeviceOperator) else A.shape[0]
    if b.shape[0] != n:
        raise ValueError(f"Shape mismatch: A is {tuple(A.shape)}, but b is {tuple(b.shape)}")
    residuals: list = []
    start = time.time()
    x, exit_code = gmres(A, b, M=M, maxiter=maxiter, callback=residuals.append, device=device)
    torch.cuda.synchronize(x.device)
    elapsed = time.time() - start
    if verbose:
        print("GMRES converged successfully." if exit_code == 0 else f"GMRES did not converge. Exit code: {exit_code}")
    return x.cpu().numpy(), residuals, len(residuals), elapsed


def spai_power_pattern(A, power: int = 1, device=None, fill: str | None = None):
    """The power-pattern SPAI baseline: M with the sparsity of A^power,
    each column the least-squares solution of min ||A m_j - e_j|| (the env's LSQ fill, AM side,
    nothing removed).  ``fill``: "lsq" (normal equations of the Gram cache) or "qr" (Householder
    QR); None = "lsq" where the Gram fill applies (pattern columns <= 13 entries over A columns
    <= 7) and "qr" otherwise (up to 32 / 32: A^2 of a 3-D stencil, 9- and 27-point stencils).
    Returns M as a sparse COO tensor on the device (A's dtype)."""
    import scipy.sparse as sp

    from .preconditioner import PreconditionerEnv
    rows, cols, vals, n = _coo_of(A)
    Acsr = sp.csr_matrix((vals.double().numpy(), (rows.numpy(), cols.numpy())), shape=(n, n))
    P = sp.csr_matrix(Acsr, copy=True)
    P.data[:] = 1.0
    Pk = P
    for _ in range(power - 1):
        Pk = Pk @ P
    if fill is None:  # widths of the AM side's lines: the columns
        w, wa = int(np.diff(Pk.tocsc().indptr).max()), int(np.diff(Acsr.tocsc().indptr).max())
        fill = "lsq" if w <= 13 and wa <= 7 else "qr"
    Pk = Pk.tocoo()
    pat = torch.sparse_coo_tensor(torch.from_numpy(np.vstack([Pk.row, Pk.col]).astype(np.int64)),
                                  torch.ones(Pk.nnz, dtype=torch.float32), (n, n))
    orig = torch.sparse_coo_tensor(torch.stack([rows, cols]), vals, (n, n))
    env = PreconditionerEnv(n, pat, orig, side="AM", fill=fill, keep_m=True, device=device)
    words = (env.init_nnz + 31) // 32
    removed = torch.zeros(1, words, dtype=torch.int32, device=env.device)
    counts = torch.zeros(1, dtype=torch.int32, device=env.device)
    env.rewards_from_removed(removed, counts, torch.tensor(0.5))
    return env.assemble(0)


# ---------------------------------------------------------------------- batched, on the device
MAX_RESTART = 64  # krylov_batched.hip kMaxRestart


def row_view(lines: Lines):
    """Row gather view of column lines: (idx [n, Wr] int32 column of each row slot, -1 padded;
    src [n, Wr] int32 flat position line * W + slot of that entry in the column lines, 0 in the
    padding).  With it M = values[src] over idx is applied row by row (no scatter); depends on
    the pattern only.  Works on any device."""
    n, W = lines.n, lines.width
    flat = lines.idx.reshape(-1).long()
    pos = torch.nonzero(flat >= 0).reshape(-1)
    rows, cols = flat[pos], pos // W
    order = torch.argsort(rows * n + cols, stable=True)
    rows, cols, pos = rows[order], cols[order], pos[order]
    counts = torch.bincount(rows, minlength=n)
    wr = max(int(counts.max()) if pos.numel() else 0, 1)
    start = torch.cumsum(counts, 0) - counts
    slot = torch.arange(pos.numel(), device=flat.device) - start[rows]
    idx = torch.full((n * wr,), -1, dtype=torch.int32, device=flat.device)
    src = torch.zeros(n * wr, dtype=torch.int32, device=flat.device)
    idx[rows * wr + slot] = cols.to(torch.int32)
    src[rows * wr + slot] = pos.to(torch.int32)
    return idx.view(n, wr), src.view(n, wr)


def _keep_mask(env) -> torch.Tensor:
    """[B, n, W] bool: the pattern slots the last batch's removal bitmaps keep (assemble's rule)."""
    if env.last_removed is None:
        raise ValueError("no removal bitmaps: run update / rewards_from_removed first or pass removed")
    act = env.pattern.act.long()
    a = act.clamp(min=0)
    bits = env.last_removed.to(env.pattern.act.device)
    return (act >= 0).unsqueeze(0) & (((bits[:, a >> 5] >> (a & 31).unsqueeze(0)) & 1) == 0)


class BatchedOperator:
    """y[b] = Op_b x[b] for B samples on the GPU (spai_ell_spmv_batched): row-ELL ``idx`` shared
    ([n, W]) or per sample ([B, n, W]); values shared (``val_bstride`` 0) or per sample, read in
    place or through the int32 indirection ``src`` [n, W] (a column-oriented pattern's values)."""

    def __init__(self, n: int, B: int, idx: torch.Tensor, val: torch.Tensor, *, val_bstride: int,
                 src: torch.Tensor | None = None, nnz=None):
        if idx.dtype != torch.int32 or val.dtype not in (torch.float32, torch.float64):
            raise ValueError("BatchedOperator takes int32 indices and fp32 / fp64 values")
        if src is not None and (idx.dim() != 2 or src.shape != idx.shape or src.dtype != torch.int32):
            raise ValueError("src needs a shared [n, W] pattern and its shape")
        _lib.require_device(idx)
        self.n, self.B, self.width = n, B, int(idx.shape[-1])
        self.idx, self.val, self.src = idx.contiguous(), val.contiguous(), None if src is None else src.contiguous()
        self.idx_bstride = 0 if idx.dim() == 2 else n * self.width
        self.val_bstride = int(val_bstride)
        self.nnz = nnz
        self.device = idx.device
        self.shape = (B, n, n)

    @classmethod
    def identity(cls, n: int, B: int, device) -> "BatchedOperator":
        idx = torch.arange(n, dtype=torch.int32, device=device).view(n, 1)
        return cls(n, B, idx, torch.ones(n, 1, dtype=torch.float64, device=device), val_bstride=0)

    @classmethod
    def from_matrices(cls, mats, n: int | None = None, device=None) -> "BatchedOperator":
        """One operator per entry of ``mats`` (scipy / torch sparse; None = the identity, stored
        as a diagonal), padded to the widest row."""
        mats = list(mats)
        if not mats:
            raise ValueError("from_matrices needs at least one matrix")
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        coos = [None if m is None else _coo_of(m) for m in mats]
        sizes = {c[3] for c in coos if c is not None} | ({int(n)} if n is not None else set())
        if len(sizes) != 1:
            raise ValueError(f"from_matrices needs one matrix size, got {sorted(sizes)}")
        n = sizes.pop()
        vd = torch.float64 if any(c is None or c[2].dtype == torch.float64 for c in coos) else torch.float32
        lines = []
        for c in coos:
            if c is None:
                d = torch.arange(n)
                c = (d, d, torch.ones(n, dtype=vd), n)
            lines.append(build_lines(c[0], c[1], c[2], n, "row", dev, vd))
        W = max(L.width for L in lines)
        pad = torch.nn.functional.pad
        idx = torch.stack([pad(L.idx, (0, W - L.width), value=-1) for L in lines])
        val = torch.stack([pad(L.val, (0, W - L.width)) for L in lines])
        nnz = [int((L.idx >= 0).sum()) for L in lines]
        return cls(n, len(lines), idx, val, val_bstride=n * W, nnz=nnz)

    @classmethod
    def from_env(cls, env) -> "BatchedOperator":
        """The M of every sample of the env's last batch, read where the fill left it
        (``env.last_m``; fill="copy": the pattern's values masked by ``env.last_removed``)."""
        if env._lsq and env.last_m is None:
            raise ValueError("construct with keep_m=True to keep M")
        keep = _keep_mask(env)
        pat = env.pattern
        n, W, B = pat.n, pat.width, keep.shape[0]
        if env._lsq:
            if env.last_m.shape[0] != B:
                raise ValueError("env.last_m and env.last_removed are of different batches")
            val = env.last_m.reshape(B, n * W)
        else:
            val = torch.where(keep, pat.val.unsqueeze(0), torch.zeros((), dtype=pat.val.dtype, device=pat.val.device))
            val = val.reshape(B, n * W)
        nnz = keep.reshape(B, -1).sum(1)
        if pat.orient == "row":
            return cls(n, B, pat.idx, val, val_bstride=n * W, nnz=nnz)
        if getattr(env, "_row_view", None) is None:  # env-constant: all samples share the pattern
            env._row_view = row_view(pat)
        idx, src = env._row_view
        return cls(n, B, idx, val, val_bstride=n * W, src=src, nnz=nnz)

    def _args(self):
        dt = _lib.DTYPE_F64 if self.val.dtype == torch.float64 else _lib.DTYPE_F32
        return (self.width, _lib.ptr(self.idx), self.idx_bstride, _lib.ptr(self.val), dt, self.val_bstride,
                _lib.ptr(self.src))

    def matvec_into(self, x: torch.Tensor, y: torch.Tensor, active: torch.Tensor | None = None) -> torch.Tensor:
        for t in (x, y):
            if t.dtype != torch.float64 or not t.is_contiguous() or t.device != self.device or \
                    tuple(t.shape) != (self.B, self.n):
                raise ValueError("BatchedOperator.matvec_into takes contiguous fp64 [B, n] tensors on its device")
        if active is not None and (active.dtype != torch.int32 or active.numel() != self.B or
                                   active.device != self.device or not active.is_contiguous()):
            raise ValueError("active must be a contiguous int32 [B] tensor on the operator's device")
        W, idx, ibs, val, dt, vbs, src = self._args()
        st = kernels._l().spai_ell_spmv_batched(self.n, W, self.B, idx, ibs, val, dt, vbs, src, _lib.ptr(x),
                                                _lib.ptr(y), _lib.ptr(active), _lib.stream_ptr(self.device))
        _lib.check(st, "spai_ell_spmv_batched")
        return y

    def matvec(self, x: torch.Tensor) -> torch.Tensor:
        return self.matvec_into(x, torch.empty_like(x))


@dataclass
class BatchedGmresResult:
    x: torch.Tensor          # [B, n] fp64, on the device
    info: np.ndarray         # [B] int64: 0 = converged, maxiter otherwise (scipy's exit code)
    iterations: np.ndarray   # [B] int64 inner iterations
    residuals: list          # B lists: the legacy callback's values, one per inner iteration
    nnz: np.ndarray | None = None  # evaluate_candidates: nnz(M) per sample


def gmres_batched(A, b, M=None, *, rtol=1e-5, atol=0.0, restart=None, maxiter=None, device=None) -> BatchedGmresResult:
    """``_gmres`` with a callback, for B samples at once on the device: A as for ``gmres`` (shared),
    b [n] (shared) or [B, n], M None | BatchedOperator | list of sparse matrices / None (identity).
    x0 = 0, left preconditioning, ``maxiter`` counts inner iterations, a zero right-hand side gives
    x = 0 and info 0 for that sample.  Host-callable preconditioners are not batched."""
    Aop = A if isinstance(A, DeviceOperator) else DeviceOperator(A, device=device)
    dev, n = Aop.device, Aop.n
    if M is not None and not isinstance(M, (BatchedOperator, list, tuple)):
        raise TypeError("gmres_batched takes M = None, a BatchedOperator or a list of sparse matrices; a host "
                        "callable / LinearOperator (or one matrix) goes through solve_with_gmres")
    if isinstance(M, (list, tuple)):
        if any(m is not None and (callable(m) or hasattr(m, "matvec")) and not hasattr(m, "tocoo") and
               not isinstance(m, torch.Tensor) for m in M):
            raise TypeError("gmres_batched cannot batch host callables / LinearOperators: use solve_with_gmres")
        M = BatchedOperator.from_matrices(M, n=n, device=dev)
    bt = torch.as_tensor(np.asarray(b, dtype=np.float64) if not isinstance(b, torch.Tensor) else b, dtype=torch.float64)
    if bt.dim() not in (1, 2) or bt.shape[-1] != n:
        raise ValueError(f"Shape mismatch: A is {Aop.shape}, but b is {tuple(bt.shape)}")
    B = M.B if M is not None else (bt.shape[0] if bt.dim() == 2 else 1)
    if M is None:
        M = BatchedOperator.identity(n, B, dev)
    if M.n != n or M.device != dev:
        raise ValueError("M and A differ in size or device")
    if bt.dim() == 2 and bt.shape[0] != B:
        raise ValueError(f"b has {bt.shape[0]} right-hand sides for {B} preconditioners")
    rhs = (bt.to(dev).expand(B, n) if bt.dim() == 1 else bt.to(dev)).contiguous()
    if atol is None or atol < 0:
        raise ValueError("atol must be a real, non-negative number")
    if maxiter is None:
        maxiter = n * 10
    if maxiter < 1:
        raise ValueError("maxiter must be at least 1")
    restart = min(20 if restart is None else int(restart), n)
    lib = kernels._l()
    nbytes = lib.spai_gmres_workspace_bytes(n, B, min(restart, MAX_RESTART))
    ws = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)
    x = torch.empty(B, n, dtype=torch.float64, device=dev)
    report = torch.zeros(B, 8 + restart, dtype=torch.int64, device=dev)
    stream = _lib.stream_ptr(dev)
    margs = M._args()
    tail = (_lib.ptr(rhs), _lib.ptr(x), _lib.ptr(report), _lib.ptr(ws), ws.numel(), stream)
    _lib.check(lib.spai_gmres_batched_init(n, B, restart, int(maxiter), float(rtol), float(atol), *margs, *tail),
               "spai_gmres_batched_init")
    L = Aop.lines
    adt = _lib.DTYPE_F64 if L.val.dtype == torch.float64 else _lib.DTYPE_F32
    residuals = [[] for _ in range(B)]
    done = np.zeros(B, dtype=np.int64)
    rep = report.cpu()  # the one host read per cycle
    while bool(rep[:, 0].any()):
        _lib.check(lib.spai_gmres_batched_cycle(n, B, restart, int(maxiter), L.width, _lib.ptr(L.idx), _lib.ptr(L.val),
                                                adt, *margs, *tail), "spai_gmres_batched_cycle")
        rep = report.cpu()
        its = rep[:, 2].numpy()
        hist = rep[:, 8:].view(torch.float64)
        for s in np.nonzero(its > done)[0]:
            residuals[s].extend(hist[s, :its[s] - done[s]].tolist())
        done = its.copy()
    return BatchedGmresResult(x, rep[:, 3].numpy().copy(), done, residuals)


def evaluate_candidates(env, b, **kw) -> BatchedGmresResult:
    """GMRES on the env's A for every candidate M of the env's last batch at once (after
    ``sample_states`` / ``rewards_from_removed`` with ``keep_m=True``): ``gmres_batched`` with
    ``BatchedOperator.from_env(env)``, plus each sample's nnz(M)."""
    M = BatchedOperator.from_env(env)
    if getattr(env, "_a_operator", None) is None:
        env._a_operator = DeviceOperator(env.original_matrix, device=env.device)
    res = gmres_batched(env._a_operator, b, M, **kw)
    res.nnz = M.nnz.cpu().numpy()
    return res
