#!/usr/bin/env python
"""Record the bits of every per-rollout fill path into tests/golden/fill_bits.json.

tests/test_fill_bits_gpu.py recomputes each case with ``run_case`` below and compares with ``==``:
the other tests compare the fill paths with each other and with the oracle to ~1e-11, which a
reordered sum inside code they all share would pass.  Re-record deliberately (on the MI355X, from
a commit whose fills are known good) only when a toolchain change moves the bits:

    python scripts/record_fill_bits.py

Only PreconditionerEnv's public keywords are used.  Per case: res2 of fill_partial over all lines,
the exact limbs of the last line shard [256, n), the SHA-256 of last_m after the whole-matrix
call, the env's qr_rows and the cache form it actually got.
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURE = os.path.join(ROOT, "tests", "golden", "fill_bits.json")
B, SEED, PROBS = 11, 11, (0.0, 0.2, 0.5, 1.0)  # one full chunk of 8 + 3; sample groups of 4 + 3; an odd last pair
SHARD_BEGIN = 256                              # the last shard: lines [256, n)
GRIDS = {"2d": 18, "3d": 9, "3d13": 9}         # 3d13: main() raises it until the caches come out as dictionaries

# geometry -> (A, pattern or None for A itself, side)
GEOMETRIES = ("2d_f32", "2d_f64", "3d7", "3d13", "2d_ma")
# fill id -> PreconditionerEnv keywords
FILLS = {
    "copy": dict(fill="copy"),
    "lsq": dict(fill="lsq"),
    "lsq_nodict": dict(fill="lsq", cache_dict=False),
    "lsq_fp64gram": dict(fill="lsq", compact_gram=False),
    "lsq_fp64gram_nodict": dict(fill="lsq", compact_gram=False, cache_dict=False),
    "qr": dict(fill="qr"),  # rcache=True, cache_dict=True: must come out as a CacheDict
    "qr_nodict": dict(fill="qr", rcache=True, cache_dict=False),
    "qr_fused": dict(fill="qr", rcache=False),
    "qr_wide": dict(fill="qr", qr_wide=True),
}
CASES = [f"{g}-{f}" for g in GEOMETRIES for f in FILLS]


def geometry(name, grids):
    from gflownet_spai_amd import axial_pattern_3d, poisson_2d, poisson_3d
    if name == "2d_f32":
        A = poisson_2d(grids["2d"])
        return A, A, "AM"
    if name == "2d_f64":
        A = poisson_2d(grids["2d"], torch.float64)
        return A, A, "AM"
    if name == "2d_ma":
        A = poisson_2d(grids["2d"])
        return A, A, "MA"
    if name == "3d7":
        A = poisson_3d(grids["3d"])
        return A, A, "AM"
    if name == "3d13":
        return poisson_3d(grids["3d13"]), axial_pattern_3d(grids["3d13"]), "AM"
    raise KeyError(name)


def removal_bits(E, device):
    """[B, ceil(E/32)] int32 removal bitmaps: sample b removes each action with probability PROBS[b % 4]."""
    rng = np.random.default_rng(SEED)
    removed = rng.random((B, E)) < np.array([PROBS[b % len(PROBS)] for b in range(B)])[:, None]
    words = (E + 31) // 32
    pad = np.zeros((B, words * 32), bool)
    pad[:, :E] = removed
    w = (pad.reshape(B, words, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(2).astype(np.uint32)
    return torch.from_numpy(w.view(np.int32)).to(device)


def cache_form(env):
    """Which cache the env's fill reads: "none", or full / dict / wide with the element type."""
    from gflownet_spai_amd import kernels
    c = env.rcache if env.fill == "qr" else env.gram
    if c is None:
        return "none"
    if isinstance(c, kernels.CacheDict):
        return "dict:" + str(c.dtype).replace("torch.", "")
    if isinstance(c, kernels.WideRCache):
        return "wide:" + str(c.tensor.dtype).replace("torch.", "")
    return "full:" + str(c.dtype).replace("torch.", "")


def make_env(case, grids):
    from gflownet_spai_amd import PreconditionerEnv
    g, f = case.split("-")
    A, P, side = geometry(g, grids)
    return PreconditionerEnv(A.shape[0], P, A, side=side, keep_m=True, **FILLS[f])


def run_case(case, grids, env=None):
    env = make_env(case, grids) if env is None else env
    n = env.matrix_size
    bits = removal_bits(env.init_nnz, env.device)
    res2 = env.fill_partial(bits)
    m = env.last_m.contiguous().cpu().numpy()
    limbs = env.fill_partial(bits, SHARD_BEGIN, n, limbs=True)
    return {
        "cache": cache_form(env),
        "qr_rows": env.qr_rows,
        "n": n,
        "res2": res2.cpu().numpy().tobytes().hex(),
        "limbs": limbs.cpu().numpy().tobytes().hex(),
        "m_sha256": hashlib.sha256(m.tobytes()).hexdigest(),
    }


def main():
    grids = dict(GRIDS)
    # the dictionary paths of the 13-wide geometry need at most n / 4 distinct lines: the smallest
    # grid (with n no multiple of 64) at which both caches come out as dictionaries
    while True:
        g = grids["3d13"]
        if g ** 3 % 64 and all(cache_form(make_env(c, grids)).startswith("dict") for c in ("3d13-qr", "3d13-lsq")):
            break
        if g >= 20:
            raise SystemExit("no dictionary up to grid 20")
        grids["3d13"] = g + 1
    out = {"B": B, "seed": SEED, "probs": list(PROBS), "shard_begin": SHARD_BEGIN, "grids": grids, "cases": {}}
    for case in CASES:
        out["cases"][case] = r = run_case(case, grids)
        print(case, r["cache"], r["qr_rows"], r["n"], r["m_sha256"][:12], flush=True)
        if case.endswith("-qr") and not r["cache"].startswith("dict"):
            raise SystemExit(f"{case}: the env's defaults gave {r['cache']}, not a dictionary")
    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
