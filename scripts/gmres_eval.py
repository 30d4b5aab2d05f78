"""Preconditioner quality by GMRES (GFlowNet100.py:61-93, 126-132) on one
MI355X: iterations and time of solve_with_gmres(A, b, M) for M = none, the driver's spilu
baseline (host LinearOperator), the power-pattern SPAI baselines (pattern of A, A^2; LSQ fill
on the GPU) and GFlowNet-sampled SPAI patterns (throughput rollout of the bench policy, LSQ
fill), plus the spai_ell_spmv roofline (HIP events over repeated products).
usage: python scripts/gmres_eval.py [--matrix poisson|thermal] [--grid 256] [--maxiter 10260] [--no-spilu]
                                    [--batched [--repeats 3]] [--out gmres.json]
--batched: beside the loop, the --samples GFlowNet candidates in one evaluate_candidates call (timed
against the loop env.assemble(s) + solve_with_gmres per sample: warm-up, synchronised, median of
--repeats), candidate 0 alone (B = 1) against solve_with_gmres, and "none" + the power-pattern baselines
+ the candidates in one gmres_batched call; both sets of iteration counts and timings are written.
(--matrix thermal --grid 1108: the C5 stand-in, utils.thermal_like, 1.23 M unknowns, fp64)"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from gflownet_spai_amd import BackwardPolicy, GFlowNet, PreconditionerEnv, poisson_2d, thermal_like  # noqa: E402
from gflownet_spai_amd.gmres import (BatchedOperator, DeviceOperator, evaluate_candidates, gmres_batched,  # noqa: E402
                                     solve_with_gmres, spai_power_pattern)


def spmv_roofline(op: DeviceOperator, reps=200):
    n, W = op.n, op.lines.width
    x = torch.randn(n, dtype=torch.float64, device=op.device)
    y = torch.empty_like(x)
    for _ in range(5):
        op.matvec_into(x, y)
    s = torch.cuda.current_stream(op.device)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(reps):
        op.matvec_into(x, y)
    e1.record(s)
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / reps
    vb = op.lines.val.element_size()
    algo = n * W * (4 + vb) + 8 * n + 8 * n  # lines + y + x once
    return {"n": n, "W": W, "avg_us": us, "algorithmic_bytes": algo, "GB_s": algo / us / 1e3,
            "frac_of_8TBs": algo / us / 1e3 / 8000.0}


def timed(fn, warm, repeats):
    """(last result, seconds {median, min, max, all}) of fn(): one warm-up call, then `repeats`
    calls timed between device synchronisations."""
    warm()
    ts, r = [], None
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return r, {"median": float(np.median(ts)), "min": min(ts), "max": max(ts), "all": ts}


def batched_section(args, env, Aop, b, baselines, runs, restart=20):
    """The batched evaluation beside the loop (see the module docstring)."""
    B, n, mi = args.samples, Aop.n, args.maxiter

    def loop(maxiter=mi, samples=range(B)):
        return [solve_with_gmres(Aop, b, env.assemble(s), verbose=False, maxiter=maxiter)[2] for s in samples]

    res, t_b = timed(lambda: evaluate_candidates(env, b, maxiter=mi), lambda: evaluate_candidates(env, b, maxiter=2),
                     args.repeats)
    it_loop, t_l = timed(loop, lambda: loop(2), args.repeats)
    it_b = [int(i) for i in res.iterations]
    sec = {"B": B, "repeats": args.repeats, "maxiter": mi, "evaluate_candidates_seconds": t_b,
           "loop_assemble_plus_solve_with_gmres_seconds": t_l, "loop_over_batched": t_l["median"] / t_b["median"],
           "iterations_batched": it_b, "iterations_loop": it_loop, "iterations_equal": it_b == it_loop,
           "info_batched": [int(i) for i in res.info], "nnz_M": [int(z) for z in res.nnz]}
    # lock step: the batch runs as many inner-iteration steps as its slowest sample's cycles hold
    cycles = max(-(-it // restart) for it in it_b) if max(it_b) else 0
    steps = max(cycles * restart, 1)
    W_a, W_m = Aop.lines.width, env.pattern.width
    vb_a, vb_m = Aop.lines.val.element_size(), env.last_m.element_size()
    src = 4 if env.pattern.orient == "col" else 0
    avg_cols = (restart + 1) / 2.0  # mean of col + 1 over a cycle
    per_sample = (n * W_a * (4 + vb_a) + 16 * n) + (n * W_m * (4 + src + vb_m) + 16 * n)  # t = A v, w = M t
    per_sample += 4 * avg_cols * 8 * n  # V[:, :col+1] read by k_dots, twice by k_upd_dots, by k_upd_norm
    per_sample += 6 * 8 * n             # w in / v_col written back; w in / out; w in / v_{col+1} out
    us = t_b["median"] / steps * 1e6
    sec["inner_iteration"] = {"launches": 8, "lockstep_steps": steps, "us_per_step": us,
                              "algorithmic_bytes_all_samples_active": B * per_sample,
                              "GB_s_if_all_active": B * per_sample / us / 1e3,
                              "frac_of_8TBs_if_all_active": B * per_sample / us / 1e3 / 8000.0,
                              "sample_steps_active": sum(it_b)}
    # B = 1: candidate 0 alone
    keep_m, keep_r = env.last_m, env.last_removed
    env.last_m, env.last_removed = keep_m[:1].contiguous(), keep_r[:1].contiguous()
    r1, t1 = timed(lambda: evaluate_candidates(env, b, maxiter=mi), lambda: evaluate_candidates(env, b, maxiter=2),
                   args.repeats)
    env.last_m, env.last_removed = keep_m, keep_r
    M0 = env.assemble(0).coalesce()
    s1, ts1 = timed(lambda: solve_with_gmres(Aop, b, M0, verbose=False, maxiter=mi)[2],
                    lambda: solve_with_gmres(Aop, b, M0, verbose=False, maxiter=2), args.repeats)
    sec["b1"] = {"batched_seconds": t1, "solve_with_gmres_seconds": ts1, "iterations_batched": int(r1.iterations[0]),
                 "iterations_solve_with_gmres": s1, "sequential_over_batched": ts1["median"] / t1["median"]}
    # everything in one call: the baselines (None = identity) and the candidates as a list of matrices
    names = list(baselines) + [f"GFlowNet sample {s} LSQ" for s in range(B)]
    mats = list(baselines.values()) + [env.assemble(s).coalesce() for s in range(B)]
    op = BatchedOperator.from_matrices(mats, n=n, device=Aop.device)
    ra, ta = timed(lambda: gmres_batched(Aop, b, op, maxiter=mi), lambda: gmres_batched(Aop, b, op, maxiter=2),
                   args.repeats)
    sec["one_call"] = {"names": names, "seconds": ta, "iterations_batched": [int(i) for i in ra.iterations],
                       "iterations_loop": [runs[k]["iterations"] for k in names],
                       "loop_seconds_sum": sum(runs[k]["seconds"] for k in names)}
    sec["one_call"]["iterations_equal"] = sec["one_call"]["iterations_batched"] == sec["one_call"]["iterations_loop"]
    print("batched", json.dumps(sec), flush=True)
    return sec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--matrix", default="poisson", choices=["poisson", "thermal"])
    ap.add_argument("--maxiter", type=int, default=10260)
    ap.add_argument("--no-spilu", action="store_true")
    ap.add_argument("--powers", default="1,2")
    ap.add_argument("--samples", type=int, default=2)
    ap.add_argument("--batched", action="store_true")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    if args.matrix == "poisson":
        A32 = poisson_2d(args.grid, torch.float32)
        A64 = poisson_2d(args.grid, torch.float64).coalesce()
    else:
        A64 = thermal_like(args.grid).coalesce()
        A32 = torch.sparse_coo_tensor(A64.indices(), A64.values().float(), A64.shape)
    n = A64.shape[0]
    Acsr = sp.csr_matrix((A64.values().numpy(), tuple(A64.indices().numpy())), shape=(n, n))
    b = np.random.default_rng(0).standard_normal(n)
    Aop = DeviceOperator(Acsr, device=dev)
    out = {"matrix": (f"{args.grid}^2 5-pt Poisson" if args.matrix == "poisson" else
                      f"thermal2-like synthetic (utils.thermal_like({args.grid}))") + f" (n={n}, nnz={Acsr.nnz}), fp64",
           "b": "N(0,1), seed 0",
           "gmres": f"restart 20, rtol 1e-5, maxiter {args.maxiter} (GFlowNet100.py:81 uses 10260)", "runs": {}}

    def run(name, M, nnz=None):
        solve_with_gmres(Aop, b, M, verbose=False, maxiter=2) if name == "warmup" else None
        x, res, it, el = solve_with_gmres(Aop, b, M, verbose=False, maxiter=args.maxiter)
        rel = float(np.linalg.norm(b - Acsr @ x) / np.linalg.norm(b))
        out["runs"][name] = {"iterations": it, "seconds": el, "true_rel_residual": rel, "nnz_M": nnz}
        print(name, out["runs"][name], flush=True)

    run("warmup", None)
    out["runs"].pop("warmup")
    run("none", None)
    if not args.no_spilu:
        t0 = time.perf_counter()
        ilu = spla.spilu(Acsr.tocsc())
        out["spilu_seconds"] = time.perf_counter() - t0
        run("spilu (host LinearOperator, GFlowNet100.py:126-132)", spla.LinearOperator(Acsr.shape, ilu.solve),
            int(ilu.L.nnz + ilu.U.nnz))
    baselines = {"none": None}
    for p in (int(x) for x in args.powers.split(",") if x):
        M = spai_power_pattern(A64, p, device=dev).coalesce()
        run(f"SPAI pattern(A^{p}) LSQ", M, int(M._nnz()))
        baselines[f"SPAI pattern(A^{p}) LSQ"] = M
        if p == 1:
            out["spmv_A"] = spmv_roofline(Aop)
            out["spmv_M"] = spmv_roofline(DeviceOperator(M, device=dev))
    # GFlowNet-sampled patterns of A (bench policy: ~20% of the entries removed), LSQ fill
    env = PreconditionerEnv(n, A32, A64, side="AM", fill="lsq", keep_m=True, device=dev)
    fwd = bench.make_policy(env, A32, dev)
    torch.manual_seed(0)
    bwd = BackwardPolicy(1, 4, env.num_actions).to(dev)
    g = GFlowNet(fwd, bwd, env, mode="throughput", seed=1234)
    with torch.no_grad():
        log = g.sample_states([A32] * args.samples, return_log=True)
    for s in range(args.samples):
        M = env.assemble(s).coalesce()
        run(f"GFlowNet sample {s} LSQ", M, int((M.values() != 0).sum()))
    if args.batched:
        out["batched"] = batched_section(args, env, Aop, b, baselines, out["runs"])
    line = json.dumps(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
