"""Timing of the wide QR fill (csrc/qr_wide.hip) on one GPU.

Workload: the 3-D 7-point Laplacian on a grid^3 lattice (default 64, as config C3) with the FULL
A^2 pattern (25 slots per interior line; the narrow kernels stop at 13), fp64, B = 8 removal sets
at fraction 0.2.  The solve kernel (spai_fill_lines_qr_wide, M stored) is timed alone with events
after a warm-up; the factor kernel (spai_qr_wide_factor) once.  Reported for the solve: the median
ms per fill, the bytes it has to move (the R cache once + the action ids + the bitmap words + M)
and the fraction of 8 TB/s those bytes imply.

The one comparison that exists on the parent's kernels: C3's own 13-wide axial pattern at the same
size, the narrow cached solve (the default) against the wide kernels forced onto it (qr_wide=True).

  python scripts/bench_qr_wide.py [--grid 64] [--batch 8] [--iters 20] [--warmup 3]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import scipy.sparse as sp
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gflownet_spai_amd import PreconditionerEnv, _lib, axial_pattern_3d, kernels, poisson_3d  # noqa: E402

HBM_BYTES_PER_S = 8e12


def squared_pattern(A: torch.Tensor) -> torch.Tensor:
    c = A.coalesce()
    P = sp.csr_matrix((np.ones(c._nnz()), tuple(c.indices().numpy())), shape=tuple(c.shape))
    P = sp.csr_matrix(P @ P)
    P.sort_indices()
    P = P.tocoo()
    ind = torch.from_numpy(np.vstack([P.row, P.col]).astype(np.int64))
    return torch.sparse_coo_tensor(ind, torch.ones(P.nnz, dtype=torch.float64), tuple(c.shape)).coalesce()


def removal_bitmaps(E: int, B: int, frac: float, dev) -> torch.Tensor:
    words = (E + 31) // 32
    bits = np.random.default_rng(7).random((B, words, 32)) < frac
    w = (bits.astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(2).astype(np.uint32)
    return torch.from_numpy(w.view(np.int32)).to(dev)


def time_events(fn, iters: int, warmup: int) -> list:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def time_solve(env, removed, iters, warmup):
    """ms per launch of the env's QR solve kernel alone (M stored in A's dtype, no reduce)."""
    B, n, W = removed.shape[0], env.matrix_size, env.pattern.width
    dt = env.a_lines.val.dtype
    m = torch.empty(B, n, W, dtype=dt, device=removed.device)
    nb = _lib.load().spai_fill_workspace_bytes(n, B)
    if isinstance(env.rcache, kernels.QrDict):
        nb = max(nb, kernels.qr_table_offset(n, B) + env.rcache.entries * 32 * 6 * 8)
    ws = _lib.workspace(nb, removed.device, "fill")
    ms = time_events(lambda: kernels._fill_lines_qr(env.pattern, env.a_lines, env.qr_rows, removed, 0, n, m, dt, 0,
                                                    ws, env.rcache), iters, warmup)
    return ms, m.numel() * m.element_size()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frac", type=float, default=0.2)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    A = poisson_3d(args.grid)
    n, B = A.shape[0], args.batch

    # ---- the A^2 pattern: only the wide kernels run it
    env = PreconditionerEnv(n, squared_pattern(A), A, side="AM", fill="qr", device=dev)
    assert env.qr_wide
    W = env.pattern.width
    removed = removal_bitmaps(env.init_nnz, B, args.frac, dev)
    ms, m_bytes = time_solve(env, removed, args.iters, args.warmup)
    cache_bytes = kernels.cache_nbytes(env.rcache)
    moved = cache_bytes + n * W * 4 + removed.numel() * 4 + m_bytes
    med = statistics.median(ms)
    print(json.dumps({"workload": f"poisson_3d({args.grid}) A^2 pattern", "n": n, "W": W, "WA": env.a_lines.width,
                      "rows": env.qr_rows, "B": B, "dtype": "fp64", "removed_frac": args.frac,
                      "kernel": "k_qrw_solve", "iters": args.iters, "median_ms": med, "min_ms": min(ms),
                      "max_ms": max(ms), "cache_bytes": cache_bytes, "act_bytes": n * W * 4,
                      "bitmap_bytes": removed.numel() * 4, "m_bytes": m_bytes, "bytes_moved": moved,
                      "frac_of_8TBs": moved / (med * 1e-3) / HBM_BYTES_PER_S}), flush=True)
    fac = time_events(lambda: kernels.qr_cache(env.pattern, env.a_lines, env.qr_rows, wide=True), 1, 0)
    print(json.dumps({"workload": f"poisson_3d({args.grid}) A^2 pattern", "kernel": "k_qrw_factor", "rows": env.qr_rows,
                      "launches": 1, "ms": fac[0]}), flush=True)
    del env
    torch.cuda.empty_cache()

    # ---- C3's 13-wide axial pattern: the narrow cached solve against the wide kernels forced onto it
    P13 = axial_pattern_3d(args.grid)
    res = {}
    for name, kw in (("narrow", {}), ("wide", {"qr_wide": True})):
        e = PreconditionerEnv(n, P13, A, side="AM", fill="qr", device=dev, **kw)
        rm = removal_bitmaps(e.init_nnz, B, args.frac, dev)
        t, _ = time_solve(e, rm, args.iters, args.warmup)
        res[name] = statistics.median(t)
        del e
        torch.cuda.empty_cache()
    print(json.dumps({"workload": f"poisson_3d({args.grid}) axial 13-wide pattern (C3)", "n": n, "B": B, "dtype": "fp64",
                      "narrow_median_ms": res["narrow"], "wide_median_ms": res["wide"],
                      "wide_over_narrow": res["wide"] / res["narrow"]}), flush=True)


if __name__ == "__main__":
    main()
