"""The least-squares QR fill for wide lines (csrc/qr_wide.hip: pattern widths up to 32 over A
lines up to 32 entries, row unions up to 256; PreconditionerEnv(fill="qr") past the 5 / 7 / 13
width classes) against the oracle's stacked Householder QR and numpy lstsq, against the narrow
kernels where both apply (qr_wide=True), across line shards and bitmap windows, and through the
public API (spai_power_pattern, GFlowNet.sample_states).

Bars: fp64 M within 1e-11 (relative Frobenius) of the oracle, the bar the narrow kernels meet in
test_qr_gpu.py — the stencils here have block condition numbers 19-34 and the oracle's two fp64
solvers agree to 9e-15; fp32 storage of the fp64 solve 1e-6; the ill-conditioned blocks (1e6-2e7)
1e-6 against lstsq (the oracle's own QR and lstsq differ by 8.2e-10 there).
"""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from oracle import spai_oracle as O

from .test_qr_gpu import _bits, _lines, _sp

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _coo(M, dtype=torch.float64):
    """scipy matrix -> coalesced torch COO in row-major order (action id = CSR position)."""
    M = sp.csr_matrix(M)
    M.sort_indices()
    c = M.tocoo()
    ind = torch.from_numpy(np.vstack([c.row, c.col]).astype(np.int64))
    return torch.sparse_coo_tensor(ind, torch.from_numpy(c.data.astype(np.float64)).to(dtype), M.shape).coalesce()


def _tri(g):
    return sp.diags([np.ones(g - 1), np.ones(g), np.ones(g - 1)], [-1, 0, 1])


def _square(A):
    P = sp.csr_matrix(A, copy=True)
    P.data[:] = 1.0
    P = sp.csr_matrix(P @ P)
    P.data[:] = 1.0
    return P


def _case(name):
    """(A, pattern) scipy CSR of the stencil cases past the narrow classes."""
    if name == "lap3d_sq":  # 3-D 7-point Laplacian, pattern A^2: W 25, WA 7
        from gflownet_spai_amd import poisson_3d
        A = _sp(poisson_3d(6))
        return A, _square(A)
    if name in ("nine", "nine_sq"):  # 2-D 9-point 9 I - kron(T, T): W 9 / 25, WA 9
        g = 12 if name == "nine" else 10
        A = sp.csr_matrix(9.0 * sp.identity(g * g) - sp.kron(_tri(g), _tri(g)))
        return A, (A if name == "nine" else _square(A))
    g = 6  # 3-D 27-point 27 I - kron(T, T, T): W = WA = 27, 125 rows (more than one row per lane)
    A = sp.csr_matrix(27.0 * sp.identity(g ** 3) - sp.kron(sp.kron(_tri(g), _tri(g)), _tri(g)))
    return A, A


def _removed(E, fracs, seed):
    return np.random.default_rng(seed).random((len(fracs), E)) < np.array(fracs)[:, None]


def _oracle_m(idx, act, a_idx, a_val, removed_row, lines=None):
    keep = (idx >= 0) & ~removed_row[np.clip(act, 0, None)]
    return keep, O.lsq_fill(idx, keep, a_idx, a_val, lines)


@pytest.mark.parametrize("name,n,W,WA,rows", [("lap3d_sq", 216, 25, 7, 60), ("nine", 144, 9, 9, 25),
                                               ("nine_sq", 100, 25, 9, 49), ("twentyseven", 216, 27, 27, 125)])
def test_wide_stencils_vs_oracle(name, n, W, WA, rows):
    """Stencils past the narrow classes: M within 1e-11 of the oracle's QR, removed and padding
    slots exactly 0, res^2 within 1e-11 of scipy's ||A M - I||_F^2, at removal fractions 0, 0.2, 0.5."""
    from gflownet_spai_amd import PreconditionerEnv, kernels
    A_sp, P_sp = _case(name)
    env = PreconditionerEnv(n, _coo(P_sp), _coo(A_sp), side="AM", fill="qr", keep_m=True)
    assert (env.pattern.width, env.a_lines.width) == (W, WA)
    assert env.qr_wide and isinstance(env.rcache, kernels.WideRCache)
    assert env.qr_rows == rows
    idx, act, a_idx, a_val = _lines(A_sp, P_sp, n)
    removed = _removed(env.init_nnz, [0.0, 0.2, 0.5], 7)
    res2 = env.fill_partial(_bits(removed))
    m = env.last_m.cpu().numpy()
    assert m.dtype == np.float64
    for b in range(3):
        keep, m_ref = _oracle_m(idx, act, a_idx, a_val, removed[b])
        rel = np.linalg.norm(m[b] - m_ref) / np.linalg.norm(m_ref)
        print(name, b, "rel M err", rel)
        assert rel < 1e-11, (b, rel)
        assert np.all(m[b][~keep] == 0)
        ref = O.residual_fro_fp64(A_sp.tocsc(), O.m_to_csc(idx, m[b], n, np.float64)) ** 2
        print(name, b, "res2", float(res2[b]), ref)
        assert float(res2[b]) == pytest.approx(ref, rel=1e-11)


@pytest.mark.parametrize("kind", ["2d", "3d13"])
def test_wide_equals_narrow_where_both_apply(kind):
    """qr_wide=True on a class-5 and a class-13 pattern against the narrow kernels: residuals 1e-12,
    M 1e-11 / 1e-13 (the tolerances between two correct fills), with an all-removed sample (M = 0,
    res^2 = n exactly) and a nothing-removed one."""
    from gflownet_spai_amd import PreconditionerEnv, axial_pattern_3d, kernels, poisson_2d, poisson_3d
    if kind == "2d":
        A = poisson_2d(40, torch.float64)
        P = A
    else:
        A, P = poisson_3d(12), axial_pattern_3d(12)
    n = A.shape[0]
    envn = PreconditionerEnv(n, P, A, side="AM", fill="qr", keep_m=True)
    envw = PreconditionerEnv(n, P, A, side="AM", fill="qr", keep_m=True, qr_wide=True)
    assert not envn.qr_wide and not isinstance(envn.rcache, kernels.WideRCache)
    assert envw.qr_wide and isinstance(envw.rcache, kernels.WideRCache) and envw.qr_rows == envn.qr_rows
    removed = _removed(envn.init_nnz, [0.3] * 5 + [1.0, 0.0], 3)
    bits = _bits(removed)
    rn, rw = envn.fill_partial(bits), envw.fill_partial(bits)
    mn, mw = envn.last_m.cpu().numpy(), envw.last_m.cpu().numpy()
    np.testing.assert_allclose(rw.cpu().numpy(), rn.cpu().numpy(), rtol=1e-12)
    np.testing.assert_allclose(mw, mn, rtol=1e-11, atol=1e-13)
    print(kind, "all removed: res2 - n =", float(rw[5]) - n, "(narrow:", float(rn[5]) - n, ")")
    assert float(rw[5]) == float(n) and not mw[5].any()


@pytest.fixture(scope="module")
def sharded():
    """The 3-D A^2 pattern at grid 10 (n = 1000: four 256-line blocks, the last partial), its env,
    five removal sets and the single launch's squared residuals."""
    from gflownet_spai_amd import PreconditionerEnv, poisson_3d
    A = _sp(poisson_3d(10))
    n = A.shape[0]
    env = PreconditionerEnv(n, _coo(_square(A)), _coo(A), side="AM", fill="qr")
    removed = _removed(env.init_nnz, [0.3] * 5, 11)
    bits = _bits(removed)
    return env, n, removed, bits, env.fill_partial(bits).clone()


@pytest.mark.parametrize("P", [2, 3])
def test_wide_shards_sum_exactly(sharded, P):
    from gflownet_spai_amd import kernels
    from gflownet_spai_amd.distributed import LINE_ALIGN, shard_lines
    env, n, _, bits, whole = sharded
    lb = sum(env.fill_partial(bits, *shard_lines(n, q, P, LINE_ALIGN), limbs=True) for q in range(P))
    assert torch.equal(kernels.res2_from_limbs(lb), whole)


def test_wide_rewards_and_bitmap_window(sharded):
    """fill_rewards (one launch) gives the residuals of rewards_from_res2(fill_partial); a shard
    evaluated from its bitmap word window (word_base) equals the shard from whole bitmaps."""
    from gflownet_spai_amd.distributed import LINE_ALIGN, shard_lines
    env, n, removed, bits, whole = sharded
    counts = torch.from_numpy(removed.sum(1).astype(np.int32)).to(DEV)
    alpha = torch.tensor(0.5)
    rw = env.fill_rewards(bits, counts, alpha)
    res_one = env.last_residual.clone()
    rw2 = env.rewards_from_res2(env.fill_partial(bits), counts, alpha)
    assert torch.equal(res_one, env.last_residual) and torch.equal(rw, rw2)
    assert torch.equal(res_one.double(), whole.sqrt())
    P, q = 3, 1
    b, e = shard_lines(n, q, P, LINE_ALIGN)
    w0, w1 = env.word_spans(P)[q]
    assert 0 < w0 and w1 < bits.shape[1]  # a real window
    full = env.fill_partial(bits, b, e, limbs=True)
    win = env.fill_partial(bits[:, w0:w1].contiguous(), b, e, word_base=w0, limbs=True)
    assert torch.equal(win, full)


@pytest.mark.parametrize("B", [1, 3])
def test_wide_fp32_and_small_batches(B):
    """Case nine_sq with fp32 A: M comes back fp32, within 1e-6 of the oracle on the fp32-rounded A
    (fp32 storage of an fp64 solve); rcache=False (a scratch cache per call) gives the same bits."""
    from gflownet_spai_amd import PreconditionerEnv
    A_sp, P_sp = _case("nine_sq")
    n = A_sp.shape[0]
    A32 = _coo(A_sp, torch.float32)
    env = PreconditionerEnv(n, _coo(P_sp), A32, side="AM", fill="qr", keep_m=True)
    envf = PreconditionerEnv(n, _coo(P_sp), A32, side="AM", fill="qr", keep_m=True, rcache=False)
    assert env.qr_wide and envf.qr_wide and envf.rcache is None
    A_r = sp.csr_matrix(A_sp.astype(np.float32).astype(np.float64))
    idx, act, a_idx, a_val = _lines(A_r, P_sp, n)
    removed = _removed(env.init_nnz, [0.3] * B, 9)
    bits = _bits(removed)
    res2 = env.fill_partial(bits)
    assert env.last_m.dtype == torch.float32 and env.last_m.shape == (B, n, 25)
    m = env.last_m.cpu().numpy().astype(np.float64)
    for b in range(B):
        keep, m_ref = _oracle_m(idx, act, a_idx, a_val, removed[b])
        rel = np.linalg.norm(m[b] - m_ref) / np.linalg.norm(m_ref)
        print("fp32", B, b, "rel M err", rel)
        assert rel < 1e-6, (b, rel)
        assert np.all(m[b][~keep] == 0)
    res2f = envf.fill_partial(bits)
    assert torch.equal(res2f, res2) and torch.equal(envf.last_m, env.last_m)


def test_wide_ill_conditioned_matches_lstsq():
    """Block-diagonal A of 20 dense 10 x 10 blocks 1 + 1e-5 randn (W = WA = 10: wide because
    WA > 7), block conditions 1e6 - 2e7: every line within 1e-6 of numpy lstsq."""
    from gflownet_spai_amd import PreconditionerEnv
    nb, w = 20, 10
    n = nb * w
    g = torch.Generator().manual_seed(5)
    blocks = 1.0 + 1e-5 * torch.randn(nb, w, w, generator=g, dtype=torch.float64)
    bi = torch.arange(nb).view(nb, 1, 1) * w
    rows = (bi + torch.arange(w).view(1, w, 1)).expand(nb, w, w).reshape(-1)
    cols = (bi + torch.arange(w).view(1, 1, w)).expand(nb, w, w).reshape(-1)
    A = torch.sparse_coo_tensor(torch.stack([rows, cols]), blocks.reshape(-1), (n, n))
    env = PreconditionerEnv(n, A, A, side="AM", fill="qr", keep_m=True)
    assert env.qr_wide and env.qr_rows == w
    env.fill_partial(_bits(np.zeros((1, env.init_nnz), bool)))
    A_sp = _sp(A)
    idx, act, a_idx, a_val = _lines(A_sp, A_sp, n)
    keep = idx >= 0
    A_csc = A_sp.tocsc()
    m = env.last_m[0].cpu().numpy()
    err = 0.0
    for j in range(n):
        mj, _ = O.lsq_fill_lstsq(idx, keep, A_csc, j)
        slots = [p for p in range(idx.shape[1]) if keep[j, p]]
        err = max(err, np.linalg.norm(m[j, slots] - mj) / np.linalg.norm(mj))
    print("ill-conditioned: worst line rel err", err)
    assert err < 1e-6, err


def test_wide_limits_raise_at_construction():
    """A 33-wide pattern, and widths inside the limits with a row union past the cap, raise
    NotImplementedError when the env is built."""
    from gflownet_spai_amd import PreconditionerEnv, kernels
    mw, mwa, mrows = kernels.qr_wide_limits()
    n = 64
    i = np.arange(n)
    band = sp.csr_matrix(sum(sp.diags(np.ones(n - abs(k)), k) for k in range(-16, 17)) + 40.0 * sp.identity(n))
    assert np.diff(band.tocsc().indptr).max() == 33 > mw
    I = _coo(sp.identity(n, format="csr"))
    with pytest.raises(NotImplementedError, match=str(mw)):
        PreconditionerEnv(n, _coo(band), I, side="AM", fill="qr")
    n = 2000
    rng = np.random.default_rng(2)
    rows = np.concatenate([rng.choice(n, 20, replace=False) for _ in range(n)] + [np.arange(n)])
    cols = np.concatenate([np.repeat(np.arange(n), 20), np.arange(n)])
    R = sp.csr_matrix((np.ones(rows.size), (rows, cols)), shape=(n, n))
    R.data[:] = rng.standard_normal(R.nnz)
    R = sp.csr_matrix(R + 25.0 * sp.identity(n))
    Rc = R.tocsc()
    assert np.diff(Rc.indptr).max() <= min(mw, mwa)
    union = max(np.unique(np.concatenate([Rc[:, k].indices for k in Rc[:, j].indices])).size for j in range(0, n, 50))
    assert union > mrows
    with pytest.raises(NotImplementedError, match=str(mrows)):
        PreconditionerEnv(n, _coo(R), _coo(R), side="AM", fill="qr")


def test_power_pattern_squared_3d_through_gmres():
    """spai_power_pattern(A, 2) on a 3-D stencil (25-wide lines: the QR fill by default): sampled
    columns match lstsq, and GMRES with that M needs fewer iterations than without."""
    from gflownet_spai_amd import poisson_3d
    from gflownet_spai_amd.gmres import solve_with_gmres, spai_power_pattern
    A = _sp(poisson_3d(6))
    n = A.shape[0]
    M = spai_power_pattern(A, 2).coalesce()
    Mcsc = sp.csc_matrix((M.values().double().cpu().numpy(), tuple(M.indices().cpu().numpy())), shape=(n, n))
    P = _square(A).tocsc()
    for j in range(0, n, 7):
        J = P[:, j].indices
        m, *_ = np.linalg.lstsq(A[:, J].toarray(), np.eye(n)[:, j], rcond=None)
        np.testing.assert_allclose(Mcsc[J, j].toarray().ravel(), m, rtol=1e-6, atol=1e-9)
    b = np.random.default_rng(3).standard_normal(n)
    _, _, it_m, _ = solve_with_gmres(A, b, M, verbose=False)
    _, _, it_0, _ = solve_with_gmres(A, b, None, verbose=False)
    assert it_m < it_0, (it_m, it_0)


def test_throughput_rollout_on_a_wide_env():
    """GFlowNet(mode="throughput").sample_states on the 3-D A^2 env with fixed logits: the logged
    removal sets' residuals match the oracle's fill at 1e-10."""
    from gflownet_spai_amd import GFlowNet, PreconditionerEnv
    A_sp, P_sp = _case("lap3d_sq")
    n = A_sp.shape[0]
    P = _coo(P_sp)
    env = PreconditionerEnv(n, P, _coo(A_sp), side="AM", fill="qr", keep_m=True)
    E = env.init_nnz

    class Fixed(torch.nn.Module):
        def __init__(self, l):
            super().__init__()
            self.l = l

        def logits(self, data):
            return self.l.to(DEV), torch.tensor(0.5, device=DEV)

    l = torch.randn(E + 1, generator=torch.Generator().manual_seed(1))
    l[E] = 3.0
    log = GFlowNet(Fixed(l), None, env, mode="throughput", seed=5).sample_states([P] * 4, return_log=True)
    words = log.removed.cpu().numpy().view(np.uint32)
    removed = ((words[:, np.arange(E) >> 5] >> (np.arange(E) & 31).astype(np.uint32)) & 1).astype(bool)
    assert removed.any()
    idx, act, a_idx, a_val = _lines(A_sp, P_sp, n)
    got = env.last_residual.cpu().numpy()
    for b in range(4):
        _, m_ref = _oracle_m(idx, act, a_idx, a_val, removed[b])
        ref = O.residual_fro_fp64(A_sp.tocsc(), O.m_to_csc(idx, m_ref, n, np.float64))
        assert float(got[b]) == pytest.approx(ref, rel=1e-10)
