"""Batched on-device GMRES (csrc/krylov_batched.hip, gmres.gmres_batched) against the existing
sequential solver (gmres.gmres, the function solve_with_gmres wraps: scipy's algorithm with the
Krylov loop on the host) and scipy products.  The new code is never compared with itself, except
in the bitwise batch-independence check.

Tolerances: the batched SpMV forms the same fp64 products as scipy and differs only in summation
order, so |y - ref| <= 1e-13 (|Op| |x|) elementwise (W <= 25 terms, 25 eps = 2.8e-15).  Against the
sequential solver the bars are test_device_gmres_matches_scipy's: histories rtol 1e-8 / atol 1e-15,
x rtol 1e-8 / atol 1e-11 max|x|; iteration counts, exit codes and history lengths are equal.
Measured: histories within 3e-12 on the CASES matrices; 2e-9 on the slowest env candidate (nonsym300,
10 % removed, 215 iterations over 11 restart cycles), which is that problem's rounding sensitivity (on
the CPU scipy and _gmres differ by 5e-9 there, and scipy by 4e-9 from itself when b is scaled by 1 + 2e-16)."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 12345.0


# ------------------------------------------------------------------ helpers
def poisson_csr(g):
    from gflownet_spai_amd.utils import poisson_2d
    A = poisson_2d(g, torch.float64).coalesce()
    return sp.csr_matrix((A.values().numpy(), tuple(A.indices().numpy())), shape=A.shape)


def nonsym(n, seed):
    rng = np.random.default_rng(seed)
    R = sp.random(n, n, density=4.0 / n, random_state=seed, format="csr")
    return (sp.identity(n) * 4 + R - R.T * 0.5 + sp.diags(rng.random(n))).tocsr()


CASES = [("poisson16", lambda: poisson_csr(16), None), ("poisson16-jacobi", lambda: poisson_csr(16), "jacobi"),
         ("nonsym300", lambda: nonsym(300, 1), None), ("nonsym300-jacobi", lambda: nonsym(300, 2), "jacobi")]


def jacobi(A):
    return sp.diags(1.0 / A.diagonal()).tocsr()


def sequential(A, b, M=None, **kw):
    """(x, info, residuals) of the existing one-at-a-time device solver."""
    from gflownet_spai_amd.gmres import gmres
    res = []
    x, info = gmres(A, b, M=M, callback=res.append, **kw)
    return x.cpu().numpy(), int(info), res


def torch_coo(M, dtype=torch.float64):
    M = sp.csr_matrix(M)
    M.sort_indices()
    c = M.tocoo()
    ind = torch.from_numpy(np.vstack([c.row, c.col]).astype(np.int64))
    return torch.sparse_coo_tensor(ind, torch.from_numpy(c.data.astype(np.float64)).to(dtype), M.shape).coalesce()


def to_scipy(M):
    M = M.coalesce()
    return sp.csr_matrix((M.values().double().cpu().numpy(), tuple(M.indices().cpu().numpy())), shape=tuple(M.shape))


def bits_of(removed_bool):
    K, E = removed_bool.shape
    words = (E + 31) // 32
    pad = np.zeros((K, words * 32), bool)
    pad[:, :E] = removed_bool
    w = (pad.reshape(K, words, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(2).astype(np.uint32)
    return torch.from_numpy(w.view(np.int32)).to(DEV)


def assert_sample_matches(res, s, ref, label=""):
    x0, i0, r0 = ref
    x1 = res.x[s].cpu().numpy()
    print(label, "sample", s, "iterations", int(res.iterations[s]), "ref", len(r0), "info", int(res.info[s]), "ref", i0)
    assert int(res.iterations[s]) == len(r0) and len(res.residuals[s]) == len(r0), label
    assert int(res.info[s]) == i0, label
    if r0:
        diff = np.abs(np.array(res.residuals[s]) - r0) / np.maximum(np.abs(r0), 1e-300)
        print(label, "  max rel history diff", float(diff.max()))
    np.testing.assert_allclose(res.residuals[s], r0, rtol=1e-8, atol=1e-15)
    np.testing.assert_allclose(x1, x0, rtol=1e-8, atol=1e-11 * max(np.abs(x0).max(), 1e-300))


# ------------------------------------------------------------------ 1. batched SpMV
def random_ell(rng, n, W):
    """idx [n, W] (-1 padded, sorted distinct columns, row 0 full) of a random row-ELL pattern."""
    idx = np.full((n, W), -1, np.int32)
    for i in range(n):
        k = min(W, n) if i == 0 else int(rng.integers(0, min(W, n) + 1))
        idx[i, :k] = np.sort(rng.choice(n, size=k, replace=False))
    return idx


def csr_of(idx, val):
    n, W = idx.shape
    ok = idx >= 0
    rows = np.repeat(np.arange(n), W).reshape(n, W)[ok]
    return sp.csr_matrix((val[ok].astype(np.float64), (rows, idx[ok])), shape=(n, n))


@pytest.mark.parametrize("n", [100, 300, 9216])
@pytest.mark.parametrize("shape", ["shared", "indirect", "per-sample"])
def test_batched_spmv_matches_scipy(shape, n):
    from gflownet_spai_amd.gmres import BatchedOperator
    rng = np.random.default_rng(n)
    worst = 0.0
    for W in (1, 5, 7, 13, 25):
        shared_idx = random_ell(rng, n, W)
        for vdt in (np.float32, np.float64):
            for B in (1, 3, 8):
                tdt = torch.float32 if vdt == np.float32 else torch.float64
                if shape == "shared":  # A: one pattern, one set of values
                    val = rng.standard_normal((n, W)).astype(vdt)
                    op = BatchedOperator(n, B, torch.from_numpy(shared_idx).to(DEV), torch.from_numpy(val).to(DEV),
                                         val_bstride=0)
                    mats = [csr_of(shared_idx, val)] * B
                elif shape == "indirect":  # the env's M: shared pattern, per-sample values through src
                    src = rng.permutation(n * W).astype(np.int32).reshape(n, W)
                    src[shared_idx < 0] = 0
                    vals = rng.standard_normal((B, n * W)).astype(vdt)
                    vals[rng.random((B, n * W)) < 0.2] = 0.0
                    op = BatchedOperator(n, B, torch.from_numpy(shared_idx).to(DEV), torch.from_numpy(vals).to(DEV),
                                         val_bstride=n * W, src=torch.from_numpy(src).to(DEV))
                    mats = [csr_of(shared_idx, vals[b][src]) for b in range(B)]
                else:  # unrelated matrices padded to a common width
                    idxs = np.stack([random_ell(rng, n, W) if b else shared_idx for b in range(B)])
                    vals = rng.standard_normal((B, n, W)).astype(vdt)
                    op = BatchedOperator(n, B, torch.from_numpy(idxs).to(DEV), torch.from_numpy(vals).to(DEV),
                                         val_bstride=n * W)
                    mats = [csr_of(idxs[b], vals[b]) for b in range(B)]
                assert op.val.dtype == tdt and op.width == W
                x = rng.standard_normal((B, n))
                xd = torch.from_numpy(x).to(DEV)
                masks = [None] if B == 1 else []
                m = np.ones(B, np.int32)
                m[B - 1] = 0  # one inactive sample (B = 1: the only one)
                masks.append(m)
                for mask in masks:
                    y = torch.full((B, n), SENTINEL, dtype=torch.float64, device=DEV)
                    op.matvec_into(xd, y, None if mask is None else torch.from_numpy(mask).to(DEV))
                    y = y.cpu().numpy()
                    for b in range(B):
                        if mask is not None and not mask[b]:
                            assert np.all(y[b] == SENTINEL), (W, vdt, B, b)
                            continue
                        ref = mats[b] @ x[b]
                        bound = abs(mats[b]) @ np.abs(x[b])
                        err = np.abs(y[b] - ref)
                        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
                        assert np.all(err <= 1e-13 * bound), (W, vdt, B, b, float(err.max()))
    print(shape, n, "worst |y - ref| / (|Op| |x|)", worst)


# ------------------------------------------------------------------ 2. against the sequential solver
@pytest.mark.parametrize("kw", [dict(maxiter=10260), dict(restart=5, maxiter=400), dict(maxiter=7)],
                         ids=["default", "restart5", "maxiter7"])
@pytest.mark.parametrize("name,mk,mkind", CASES)
def test_batched_matches_sequential(name, mk, mkind, kw):
    from gflownet_spai_amd.gmres import gmres_batched
    A = mk()
    n = A.shape[0]
    J = jacobi(A)
    Ms = [None, J, None]
    b = np.random.default_rng(0).standard_normal((3, n))
    res = gmres_batched(A, b, Ms, **kw)
    assert res.x.shape == (3, n) and res.x.dtype == torch.float64 and res.x.is_cuda
    for s in range(3):
        assert_sample_matches(res, s, sequential(A, b[s], Ms[s], **kw), f"{name} {kw}")


# ------------------------------------------------------------------ 3-5. an env's batch of candidates
SEEDS = {"poisson16": 11, "nonsym300": 11}


@functools.lru_cache(maxsize=None)
def env_batch(name):
    """AM-side LSQ env, B = 4 removal bitmaps (about 0 / 10 / 30 / 60 % removed), one right-hand side;
    the sequential solver's result per sample (computed once, shared by the tests below)."""
    from gflownet_spai_amd import PreconditionerEnv
    A = poisson_csr(16) if name == "poisson16" else nonsym(300, 1)
    n = A.shape[0]
    At = torch_coo(A)
    env = PreconditionerEnv(n, At, At, side="AM", fill="lsq" if name == "poisson16" else "qr", keep_m=True, device=DEV)
    rng = np.random.default_rng(SEEDS[name])
    removed = rng.random((4, env.init_nnz)) < np.array([0.0, 0.1, 0.3, 0.6])[:, None]
    bits = bits_of(removed)
    env.fill_partial(bits)
    b = rng.standard_normal(n)
    refs = [sequential(A, b, env.assemble(s), maxiter=300) for s in range(4)]
    return A, env, bits, b, refs


@pytest.mark.parametrize("name", ["poisson16", "nonsym300"])
def test_samples_that_stop_at_different_times(name):
    from gflownet_spai_amd.gmres import evaluate_candidates
    A, env, bits, b, refs = env_batch(name)
    env.fill_partial(bits)
    its, infos = [len(r[2]) for r in refs], [r[1] for r in refs]
    print(name, "sequential iterations", its, "info", infos)
    # the condition of the test: early exits, late exits and samples that run into the cap
    assert len(set(its)) > 1 and any(i == 0 for i in infos) and any(i != 0 for i in infos)
    res = evaluate_candidates(env, b, maxiter=300)
    for s in range(4):
        assert_sample_matches(res, s, refs[s], name)
    assert res.nnz.tolist() == [int(env.assemble(s)._nnz()) for s in range(4)]


@pytest.mark.parametrize("name", ["poisson16", "nonsym300"])
def test_true_residual_of_converged_samples(name):
    """The solver's own stopping rule re-evaluated in numpy fp64: ||b - A x|| <= rtol ||b|| (1 + 1e-9)."""
    from gflownet_spai_amd.gmres import evaluate_candidates, gmres_batched
    A, env, bits, b, _ = env_batch(name)
    env.fill_partial(bits)
    res = evaluate_candidates(env, b, maxiter=300)
    plain = gmres_batched(A, np.stack([b, 2.0 * b[::-1]]), [None, jacobi(A)])
    checked = 0
    for r, rhs in ((res, [b] * 4), (plain, [b, 2.0 * b[::-1]])):
        for s in range(len(rhs)):
            if r.info[s] != 0:
                continue
            true = np.linalg.norm(rhs[s] - A @ r.x[s].cpu().numpy())
            print(name, s, "true residual / ||b||", true / np.linalg.norm(rhs[s]))
            assert true <= 1e-5 * np.linalg.norm(rhs[s]) * (1 + 1e-9)
            checked += 1
    assert checked >= 3


@pytest.mark.parametrize("name", ["poisson16", "nonsym300"])
def test_batch_independence_bitwise(name):
    """Whole batch, each sample alone (B = 1) and the samples permuted: identical bits."""
    from gflownet_spai_amd.gmres import BatchedOperator, gmres_batched
    A, env, bits, b, _ = env_batch(name)
    env.fill_partial(bits)
    whole = gmres_batched(A, b, BatchedOperator.from_env(env), maxiter=300)
    assert len(set(whole.iterations.tolist())) > 1
    for s in range(4):
        env.fill_partial(bits[s:s + 1].contiguous())
        one = gmres_batched(A, b, BatchedOperator.from_env(env), maxiter=300)
        assert one.x.shape[0] == 1
        assert torch.equal(one.x[0], whole.x[s]) and one.residuals[0] == whole.residuals[s]
        assert one.iterations[0] == whole.iterations[s] and one.info[0] == whole.info[s]
    perm = [2, 0, 3, 1]
    env.fill_partial(bits[perm].contiguous())
    mixed = gmres_batched(A, b, BatchedOperator.from_env(env), maxiter=300)
    for k, s in enumerate(perm):
        assert torch.equal(mixed.x[k], whole.x[s]) and mixed.residuals[k] == whole.residuals[s]
        assert mixed.iterations[k] == whole.iterations[s] and mixed.info[k] == whole.info[s]


# ------------------------------------------------------------------ 6. edge cases
def test_identity_breaks_down_happily():
    from gflownet_spai_amd.gmres import gmres_batched
    n = 50
    A = sp.identity(n, format="csr")
    b = np.random.default_rng(1).standard_normal((2, n))
    res = gmres_batched(A, b)
    for s in range(2):
        assert res.info[s] == 0 and res.iterations[s] == 1
        assert_sample_matches(res, s, sequential(A, b[s]), "identity")
        np.testing.assert_allclose(res.x[s].cpu().numpy(), b[s], rtol=1e-14)


def test_zero_rhs_inside_a_batch():
    from gflownet_spai_amd.gmres import gmres_batched
    A = poisson_csr(8)
    b = np.random.default_rng(2).standard_normal((3, 64))
    b[1] = 0.0
    res = gmres_batched(A, b, [None, jacobi(A), jacobi(A)])
    assert res.info[1] == 0 and res.iterations[1] == 0 and res.residuals[1] == []
    assert not res.x[1].any()
    for s in (0, 2):
        assert_sample_matches(res, s, sequential(A, b[s], [None, None, jacobi(A)][s]), "zero-rhs batch")


def test_exact_inverse_takes_one_iteration():
    from gflownet_spai_amd.gmres import gmres_batched
    n = 300
    d = np.random.default_rng(3).uniform(0.5, 4.0, n)
    A, Minv = sp.diags(d).tocsr(), sp.diags(1.0 / d).tocsr()
    b = np.random.default_rng(4).standard_normal(n)
    res = gmres_batched(A, b, [Minv, None])
    assert res.iterations[0] == 1 and res.info[0] == 0
    np.testing.assert_allclose(res.x[0].cpu().numpy(), b / d, rtol=1e-12)
    assert_sample_matches(res, 0, sequential(A, b, Minv), "exact inverse")
    assert_sample_matches(res, 1, sequential(A, b), "diagonal, no M")


def test_restart_64_and_65():
    from gflownet_spai_amd.gmres import gmres_batched
    A = poisson_csr(32)  # more than 64 iterations at restart 64: every column of a full cycle, then a second one
    b = np.random.default_rng(5).standard_normal((2, 1024))
    res = gmres_batched(A, b, [None, jacobi(A)], restart=64, maxiter=150)
    assert res.iterations.max() > 64
    for s, M in enumerate([None, jacobi(A)]):
        assert_sample_matches(res, s, sequential(A, b[s], M, restart=64, maxiter=150), "restart 64")
    with pytest.raises(NotImplementedError, match="restart 65"):
        gmres_batched(A, b, restart=65)


def test_one_unknown():
    from gflownet_spai_amd.gmres import gmres_batched
    A = sp.csr_matrix(np.array([[2.0]]))
    res = gmres_batched(A, np.array([[3.0], [-5.0]]))
    assert res.info.tolist() == [0, 0] and res.iterations.tolist() == [1, 1]
    np.testing.assert_allclose(res.x.cpu().numpy().ravel(), [1.5, -2.5], rtol=1e-15)
    assert_sample_matches(res, 0, sequential(A, np.array([3.0])), "n = 1")


# ------------------------------------------------------------------ 7. from_env on both orientations
def nine_point(g):
    T = sp.diags([np.ones(g - 1), np.ones(g), np.ones(g - 1)], [-1, 0, 1])
    return sp.csr_matrix(9.0 * sp.identity(g * g) - sp.kron(T, T))


@pytest.mark.parametrize("side,fill,case", [("MA", "lsq", "poisson"), ("AM", "lsq", "poisson"), ("AM", "qr", "poisson"),
                                            ("MA", "copy", "poisson"), ("AM", "copy", "poisson"),
                                            ("AM", "qr", "nine")])
def test_from_env_matvec_matches_assemble(side, fill, case):
    from gflownet_spai_amd import PreconditionerEnv, kernels
    from gflownet_spai_amd.gmres import BatchedOperator
    A = poisson_csr(12) if case == "poisson" else nine_point(12)
    n = A.shape[0]
    At = torch_coo(A, torch.float32 if fill == "copy" else torch.float64)
    env = PreconditionerEnv(n, At, At, side=side, fill=fill, keep_m=fill != "copy", device=DEV)
    if case == "nine":
        assert env.pattern.width == 9 and env.qr_wide and isinstance(env.rcache, kernels.WideRCache)
    rng = np.random.default_rng(7)
    removed = rng.random((3, env.init_nnz)) < np.array([0.0, 0.25, 0.6])[:, None]
    env.fill_partial(bits_of(removed))
    op = BatchedOperator.from_env(env)
    assert (op.src is None) == (side == "MA")
    v = rng.standard_normal((3, n))
    y = op.matvec(torch.from_numpy(v).to(DEV)).cpu().numpy()
    for s in range(3):
        M = to_scipy(env.assemble(s))
        assert int(op.nnz[s]) == M.nnz == int((~removed[s]).sum())
        err = np.abs(y[s] - M @ v[s])
        assert np.all(err <= 1e-13 * (abs(M) @ np.abs(v[s]))), (s, float(err.max()))


def test_from_env_needs_kept_m():
    from gflownet_spai_amd import PreconditionerEnv
    from gflownet_spai_amd.gmres import BatchedOperator
    At = torch_coo(poisson_csr(6))
    env = PreconditionerEnv(36, At, At, side="AM", fill="lsq", keep_m=False, device=DEV)
    env.fill_partial(bits_of(np.zeros((1, env.init_nnz), bool)))
    with pytest.raises(ValueError, match="construct with keep_m=True to keep M"):
        BatchedOperator.from_env(env)


# ------------------------------------------------------------------ 8. end to end
def test_evaluate_candidates_after_a_rollout():
    from gflownet_spai_amd import GFlowNet, PreconditionerEnv, evaluate_candidates, poisson_2d

    class Fixed(torch.nn.Module):
        def __init__(self, l):
            super().__init__()
            self.l = l

        def logits(self, data):
            return self.l.to(DEV), torch.tensor(0.5, device=DEV)

    A32, A = poisson_2d(16), poisson_csr(16)
    env = PreconditionerEnv(256, A32, A32, side="AM", fill="lsq", keep_m=True, device=DEV)
    E = env.num_actions - 1
    l = torch.randn(E + 1, generator=torch.Generator().manual_seed(1))
    l[E] = 5.0
    with torch.no_grad():
        GFlowNet(Fixed(l), None, env, mode="throughput", seed=5).sample_states([A32] * 4, return_log=True)
    b = np.random.default_rng(8).standard_normal(256)
    res = evaluate_candidates(env, b, maxiter=300)
    A_env = to_scipy(env.original_matrix)
    for s in range(4):
        M = env.assemble(s)
        ref = sequential(A_env, b, M, maxiter=300)
        assert int(res.iterations[s]) == len(ref[2]) and int(res.info[s]) == ref[1]
        assert int(res.nnz[s]) == int(M._nnz())
    print("iterations", res.iterations.tolist(), "nnz", res.nnz.tolist())
