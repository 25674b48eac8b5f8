"""gcge_amd.eigsh(method="chebyshev"): Chebyshev-filtered subspace iteration (GCGE_RunChFSI) behind the same face as the GCG solve —
matrices, start vectors and results as torch device tensors, check_result of tests/test_eigsh.py unchanged (1e-8 on eigenvalues, 1e-6 on
the recomputed residuals and on residual_norms), warm starts, NoConvergence, the refusals, and the gradient of the eigenvalues."""
import numpy as np
import pytest

from gcge_amd.lib import cheb_stats, csr_arrays, csr_to_scipy, make_problem
from test_eigsh import K, check_result, problem, to_torch_csr, to_triple


@pytest.fixture(scope="module")
def first(hip):
    """the cold solve the other tests compare with"""
    from gcge_amd import eigsh
    return eigsh(to_torch_csr(problem("lap3d", 12)[0]), K, method="chebyshev", backend=hip)


@pytest.mark.gpu
def test_standard_problem(first):
    A, _, SA, _, ref = problem("lap3d", 12)
    print("outer iterations:", first.iterations)
    assert first.iterations >= 1
    check_result(first, SA, None, ref)


@pytest.mark.gpu
def test_triple_and_handle(hip):
    from gcge_amd import eigsh
    A, _, SA, _, ref = problem("lap3d", 12)
    check_result(eigsh(to_triple(A), K, method="chebyshev", backend=hip), SA, None, ref)
    m = hip.matrix(A)
    try:
        check_result(eigsh(m, K, method="chebyshev", backend=hip), SA, None, ref)
        check_result(eigsh(m, K, method="chebyshev", degree=12, upper_bound=12.0, backend=hip), SA, None, ref)      # (12 bounds the 7-point stencil's spectrum)
    finally:
        hip.free_matrix(m)


@pytest.mark.gpu
def test_warm_start(hip, first):
    from gcge_amd import eigsh
    A, _, SA, _, ref = problem("lap3d", 12)
    r = eigsh(to_torch_csr(A), K, X0=first.eigenvectors, method="chebyshev", backend=hip)
    print("iterations: cold %d, warm %d" % (first.iterations, r.iterations))
    assert r.iterations <= 1 and r.iterations < first.iterations
    check_result(r, SA, None, ref)


@pytest.mark.gpu
def test_sio2_on_the_sweep_path_agrees_with_gcg(hip):
    """make_problem("sio2", 12), nev_max = 2 k, with k among 4 .. 8 where scipy's spectrum has its widest gap (k = 6: lambda_7 - lambda_6 =
    0.19 lambda_6): converges within maxiter = 60 (13 outer iterations over the CPU oracle's table) with every filter step taken as
    product + sweep, and gives GCG's eigenvalues to 1e-8 relative."""
    from gcge_amd import eigsh
    A, _ = make_problem("sio2", 12)
    S = csr_to_scipy(A)
    lam = np.linalg.eigvalsh(S.toarray())
    k = max(range(4, 9), key=lambda j: (lam[j] - lam[j - 1]) / abs(lam[j - 1]))
    assert lam[k] - lam[k - 1] > 1e-3 * abs(lam[k - 1])                      # the premise: k ends at a gap
    T = to_torch_csr(A)
    s0 = cheb_stats()
    r = eigsh(T, k, nev_max=2 * k, maxiter=60, method="chebyshev", backend=hip)
    s1 = cheb_stats()
    print("k = %d, outer iterations %d, steps fused / swept: %d / %d" % (k, r.iterations, s1[0] - s0[0], s1[1] - s0[1]))
    assert r.converged >= k and r.iterations <= 60
    assert s1[0] == s0[0] and s1[1] - s0[1] >= 20 * r.iterations and s1[2] == s0[2]
    g = eigsh(T, k, nev_max=2 * k, backend=hip)
    a, b = r.eigenvalues.cpu().numpy(), g.eigenvalues.cpu().numpy()
    assert np.max(np.abs(a - b) / np.abs(b)) <= 1e-8
    assert np.max(np.abs(a - lam[:k]) / np.abs(lam[:k])) <= 1e-8


@pytest.mark.gpu
def test_fused_steps_inside_a_solve(hip):
    """lap3d 16, the smallest size whose handle takes the fused step (tests/test_cheb_step.py): the filter's steps behind the first one
    run fused while the locked count is even, and the eigenvalues are the closed form's to 1e-8"""
    from gcge_amd import eigsh
    from helpers import lap3d_exact
    A, _ = make_problem("lap3d", 16)
    s0 = cheb_stats()
    r = eigsh(to_torch_csr(A), K, method="chebyshev", backend=hip)
    s1 = cheb_stats()
    print("outer iterations %d, steps fused / swept: %d / %d" % (r.iterations, s1[0] - s0[0], s1[1] - s0[1]))
    assert r.converged >= K and s1[0] - s0[0] >= 19 and s1[1] - s0[1] >= r.iterations and s1[2] == s0[2]
    assert (s1[0] - s0[0]) + (s1[1] - s0[1]) == 20 * r.iterations
    lam, ref = r.eigenvalues.cpu().numpy(), lap3d_exact(16, K)
    assert np.max(np.abs(lam - ref) / ref) <= 1e-8


@pytest.mark.gpu
def test_slot_path_over_the_hip_table(hip, first, monkeypatch):
    """GCGE_NO_CHEB_STEP: every filter step is MatDotMultiVec and two MultiVecAxpby of the HIP table; the same eigenvalues to 1e-10"""
    from gcge_amd import eigsh
    A = problem("lap3d", 12)[0]
    monkeypatch.setenv("GCGE_NO_CHEB_STEP", "1")
    s0 = cheb_stats()
    r = eigsh(to_torch_csr(A), K, method="chebyshev", backend=hip)
    assert cheb_stats() == s0
    a, b = r.eigenvalues.cpu().numpy(), first.eigenvalues.cpu().numpy()
    assert np.max(np.abs(a - b) / np.abs(b)) <= 1e-10


@pytest.mark.gpu
def test_refusals(hip):
    from gcge_amd import eigsh
    A, B = problem("fe3d", 8)[:2]
    TA, TB = to_torch_csr(A), to_torch_csr(B)
    for kw in (dict(M=TB), dict(amg_levels=3), dict(block_size=8)):
        with pytest.raises(ValueError):
            eigsh(TA, K, method="chebyshev", backend=hip, **kw)
    with pytest.raises(ValueError):
        eigsh(TA, K, method="lanczos", backend=hip)


@pytest.mark.gpu
def test_one_filter_pass_raises_no_convergence_with_a_result(hip):
    import torch
    from gcge_amd import NoConvergence, eigsh
    A = problem("lap3d", 12)[0]
    with pytest.raises(NoConvergence) as e:
        eigsh(to_torch_csr(A), K, maxiter=1, method="chebyshev", backend=hip)
    r = e.value.result
    assert r.converged < K and r.iterations == 1
    assert tuple(r.eigenvalues.shape) == (K,) and tuple(r.eigenvectors.shape) == (A.nrows, K) and tuple(r.residual_norms.shape) == (K,)
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in (r.eigenvalues, r.eigenvectors, r.residual_norms))


@pytest.mark.gpu
def test_chebyshev_filter_on_a_tensor(hip):
    """HipBackend.chebyshev_filter against the eigen-decomposition: p(A) x = V p(Lambda) V^T x, with p from the recurrence on the
    eigenvalues.  Every iterate is bounded by |x|; 1e-10 |x| as tests/test_chfsi_host.py derives it."""
    import torch
    A, _, SA, _, _ = problem("lap3d", 12)
    lam, V = np.linalg.eigh(SA.toarray())
    n, m, degree = SA.shape[0], 6, 10
    lower, upper, lowest = float(lam[40]), float(lam[-1]), float(lam[0])
    X = np.random.default_rng(3).random((n, m)) - 0.5
    e, c = 0.5 * (upper - lower), 0.5 * (upper + lower)
    s1 = e / (lowest - c)
    tau, sg, pp, p = 2.0 / s1, s1, np.ones(n), (s1 / e) * (lam - c)
    for _ in range(2, degree + 1):
        s2 = 1.0 / (tau - sg)
        pp, p = p, (2.0 * s2 / e) * (lam - c) * p - sg * s2 * pp
        sg = s2
    ref = V @ (p[:, None] * (V.T @ X))
    mat = hip.matrix(A)
    try:
        s0 = cheb_stats()
        Y = hip.chebyshev_filter(mat, torch.from_numpy(X).cuda(), degree, lower, upper, lowest)
        assert sum(cheb_stats()[:2]) - sum(s0[:2]) == degree
        with pytest.raises(ValueError):
            hip.chebyshev_filter(mat, torch.from_numpy(X).cuda(), 0, lower, upper, lowest)
    finally:
        hip.free_matrix(mat)
    assert Y.is_cuda and tuple(Y.shape) == (n, m) and Y.dtype == torch.float64
    err = np.linalg.norm(Y.cpu().numpy() - ref, axis=0) / np.linalg.norm(X, axis=0)
    print("max column error / |X|:", err.max())
    assert np.all(err <= 1e-10)


@pytest.mark.gpu
def test_eigenvalue_gradient(hip):
    """lap3d 12, k = 7 (multiplicities 1, 3, 3: k ends the second cluster), loss = the sum of the eigenvalues: d loss / d A_ij = (V V^T)_ij
    on the stored entries, V the 7 lowest eigenvectors of numpy's eigh, within 1e-6 absolute.  The invariant subspace is off by at
    most |r| / gap with |r| <= 1e-8 lambda_7, and V V^T by twice that: 2 * 1e-8 * lambda_7 / (lambda_8 - lambda_7) = 1.0033e-7 from
    numpy's eigenvalues (0.51629226 and 0.61921123) — the premise, asserted as <= 1.1e-7: a tenth of the bound."""
    import torch
    from gcge_amd import eigsh
    A, _, SA, _, _ = problem("lap3d", 12)
    lam, V = np.linalg.eigh(SA.toarray())
    k = 7
    assert lam[7] - lam[6] > 0.1 * lam[6] and abs(lam[6] - lam[4]) < 1e-12 and abs(lam[3] - lam[1]) < 1e-12
    assert 2 * 1e-8 * lam[6] / (lam[7] - lam[6]) <= 1.1e-7
    rp, ci, va = csr_arrays(A)
    crow, col = torch.from_numpy(rp.astype(np.int64)).cuda(), torch.from_numpy(ci.astype(np.int64)).cuda()
    val = torch.from_numpy(va.copy()).cuda().requires_grad_()
    r = eigsh((crow, col, val), k, method="chebyshev", backend=hip)
    assert r.eigenvalues.requires_grad and r.converged >= k
    r.eigenvalues.sum().backward()
    rows = np.repeat(np.arange(A.nrows), np.diff(rp))
    want = np.einsum("ec,ec->e", V[rows, :k], V[ci, :k])
    got = val.grad.cpu().numpy()
    print("max gradient error:", np.abs(got - want).max())
    assert np.abs(got - want).max() <= 1e-6
