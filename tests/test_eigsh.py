"""gcge_amd.eigsh: matrices, start vectors and results as torch device tensors, the solve by the harness in between.

Bounds.  Eigenvalues: for a symmetric problem |lambda~ - lambda| <= ||r|| / ||x||, and the harness stops a pair at ||r|| <= tol |lambda|
with tol = 1e-8 and ||x||_B = 1: 1e-8 relative against the dense solver.  Residuals recomputed in numpy from the returned tensors:
< 1e-6 relative to |lambda| ||B x||, the bound tests/test_warm_start.py::_check uses for the same quantity (the solver tested the Ritz
vectors of its last iteration by its own sums; 1e-6 leaves two digits for the recomputation).  residual_norms against those numpy
residuals: the same 1e-6 |lambda| and no tighter, because the back-end's residual_sq may form ||A x - lambda x||^2 from expanded sums
(x.A A x - 2 lambda x.A x + lambda^2 x.x inside the product sweep), whose cancellation error is of the order eps |lambda|^2 ||x||^2
under the square root, i.e. about 1e-8 |lambda| in the norm — far above the rounding of a residual formed entry by entry."""
import ctypes as C

import numpy as np
import pytest

from gcge_amd.lib import csr_arrays, csr_to_scipy, make_problem, mat_device_stats

K = 8


def to_torch_csr(A):
    import torch
    rp, ci, va = csr_arrays(A)
    return torch.sparse_csr_tensor(torch.from_numpy(rp.astype(np.int64)).cuda(), torch.from_numpy(ci.astype(np.int64)).cuda(),
                                   torch.from_numpy(va).cuda(), size=(A.nrows, A.ncols))


def to_triple(A):
    import torch
    return tuple(torch.from_numpy(a).cuda() for a in csr_arrays(A))


_cache = {}


def problem(kind, size):
    """(A struct, B struct or None, scipy A, scipy B or None, reference eigenvalues or None): built once per module"""
    if (kind, size) not in _cache:
        A, B = make_problem(kind, size)
        SA, SB = csr_to_scipy(A), (csr_to_scipy(B) if B is not None else None)
        ref = None
        if A.nrows <= 2000:
            import scipy.linalg
            ref = np.linalg.eigvalsh(SA.toarray())[:K] if SB is None else scipy.linalg.eigh(SA.toarray(), SB.toarray(), eigvals_only=True)[:K]
        _cache[(kind, size)] = (A, B, SA, SB, ref)
    return _cache[(kind, size)]


def check_result(r, SA, SB, ref, k=K):
    import torch
    n = SA.shape[0]
    for t, shape in ((r.eigenvalues, (k,)), (r.eigenvectors, (n, k)), (r.residual_norms, (k,))):
        assert isinstance(t, torch.Tensor) and t.is_cuda and tuple(t.shape) == shape and t.dtype == torch.float64
    assert r.converged >= k and r.iterations >= 0 and r.seconds > 0.0
    lam, V, rn = r.eigenvalues.cpu().numpy(), r.eigenvectors.cpu().numpy(), r.residual_norms.cpu().numpy()
    err = np.abs(lam - ref) / np.abs(ref)
    BV = SB @ V if SB is not None else V
    R = SA @ V - BV * lam
    res = np.linalg.norm(R, axis=0)
    rel = res / (np.abs(lam) * np.linalg.norm(BV, axis=0))
    print("eigenvalue error %.2e, relative residual %.2e, residual_norms against numpy %.2e |lambda|" %
          (err.max(), rel.max(), (np.abs(rn - res) / np.abs(lam)).max()))
    assert err.max() <= 1e-8, err
    assert rel.max() < 1e-6, rel
    assert np.all(np.abs(rn - res) <= 1e-6 * np.abs(lam)), (rn, res)


def test_residual_norms_through_the_slots(oracle):
    """GCGE_ResidualNorms over a table whose back-end offers no residual_sq (the CPU oracle): CheckConvergence's slot sequence on
    blocks of its own.  The residual is formed entry by entry there: a row's error is at most about (7 + 2) eps max|a| max|x| < 2e-14
    and the norm over n = 512 rows at most sqrt(n) times that, so 1e-11 holds with room."""
    from gcge_amd.lib import host_lib, run_gcg
    A, B, SA, SB, _ = problem("fe3d", 8)
    mA, mB = oracle.matrix(A), oracle.matrix(B)
    ev, res, evec = run_gcg(oracle.ops_handle, mA, mB, ["-nevConv", 4], keep_evec=True)
    assert res.nevConv >= 4
    h = host_lib()
    lam, rn = np.ascontiguousarray(ev[1:4]), np.zeros(3)
    dp = C.POINTER(C.c_double)
    assert h.GCGE_ResidualNorms(mA, mB, evec, 1, 4, lam.ctypes.data_as(dp), rn.ctypes.data_as(dp), oracle.ops_handle) == 0
    assert h.GCGE_ResidualNorms(mA, mB, evec, 2, 1, lam.ctypes.data_as(dp), rn.ctypes.data_as(dp), oracle.ops_handle) == -1
    V = oracle.mv_to_numpy(evec, A.nrows, 1, 4)
    oracle.ops.mv_destroy(evec, 8)
    want = np.linalg.norm(SA @ V - (SB @ V) * lam, axis=0)
    assert np.all(np.abs(rn - want) <= 1e-11), (rn, want)
    assert np.all(rn <= 1e-6 * np.abs(lam))


@pytest.fixture(scope="module")
def first(hip):
    """the cold standard solve the other tests compare with"""
    from gcge_amd import eigsh
    A, _, SA, _, ref = problem("lap3d", 12)
    return eigsh(to_torch_csr(A), K, backend=hip)


@pytest.mark.gpu
def test_standard_problem(first):
    A, _, SA, _, ref = problem("lap3d", 12)
    assert SA.shape[0] == 1728
    check_result(first, SA, None, ref)


@pytest.mark.gpu
def test_generalised_problem(hip):
    from gcge_amd import eigsh
    A, B, SA, SB, ref = problem("fe3d", 8)
    s0 = mat_device_stats()
    r = eigsh(to_torch_csr(A), K, M=to_torch_csr(B), backend=hip)
    assert mat_device_stats()[0] == s0[0] + 2
    check_result(r, SA, SB, ref)


@pytest.mark.gpu
def test_warm_second_call(hip, first):
    from gcge_amd import eigsh
    A, _, SA, _, ref = problem("lap3d", 12)
    r = eigsh(to_torch_csr(A), K, X0=first.eigenvectors, backend=hip)
    print("iterations: cold %d, warm %d" % (first.iterations, r.iterations))
    assert r.converged >= K and r.iterations < first.iterations
    a, b = r.eigenvalues.cpu().numpy(), first.eigenvalues.cpu().numpy()
    assert np.max(np.abs(a - b) / np.abs(b)) <= 1e-8
    check_result(r, SA, None, ref)


@pytest.mark.gpu
def test_block_amg(hip):
    from gcge_amd import eigsh
    A = to_torch_csr(problem("lap3d", 16)[0])
    plain, amg = eigsh(A, K, amg_levels=0, backend=hip), eigsh(A, K, amg_levels=3, backend=hip)
    a, b = amg.eigenvalues.cpu().numpy(), plain.eigenvalues.cpu().numpy()
    print("iterations: block CG %d, BlockAMG %d" % (plain.iterations, amg.iterations))
    assert np.max(np.abs(a - b) / np.abs(b)) <= 1e-8


@pytest.mark.gpu
def test_handles_stay_and_created_matrices_are_counted(hip):
    """handles: the caller's before and after (a product on each succeeds); a triple of device arrays and the process's own default
    back-end: one matrix analysed on the device per matrix given"""
    from gcge_amd import eigsh
    A, B, SA, SB, ref = problem("fe3d", 8)
    n = A.nrows
    mA, mB = hip.matrix(A), hip.matrix(B)
    try:
        s0 = mat_device_stats()
        r = eigsh(mA, K, M=mB, backend=hip)
        assert mat_device_stats()[0] == s0[0]
        check_result(r, SA, SB, ref)
        X = np.ones((n, 2))
        for m, S in ((mA, SA), (mB, SB)):
            x, y = hip.mv_from_numpy(m, X), hip.mv_from_numpy(m, np.zeros((n, 2)))
            hip.ops.spmm(m, x, y, (0, 0), (2, 2))
            Y = hip.mv_to_numpy(y, n, 0, 2)
            hip.ops.mv_destroy(x, 2)
            hip.ops.mv_destroy(y, 2)
            assert np.allclose(Y, S @ X, rtol=1e-13, atol=1e-13 * np.abs(S).sum(axis=1).max())
    finally:
        hip.free_matrix(mA)
        hip.free_matrix(mB)
    L, _, SL, _, refL = problem("lap3d", 12)
    s0 = mat_device_stats()
    r = eigsh(to_triple(L), K)                                     # (crow, col, val), the default back-end
    assert mat_device_stats()[0] == s0[0] + 1
    check_result(r, SL, None, refL)


@pytest.mark.gpu
def test_no_convergence_carries_the_partial_result(hip):
    import torch
    from gcge_amd import NoConvergence, eigsh
    A = problem("lap3d", 12)[0]
    with pytest.raises(NoConvergence) as info:
        eigsh(to_torch_csr(A), K, maxiter=1, backend=hip)
    r = info.value.result
    assert isinstance(info.value, RuntimeError) and r.converged < K
    assert tuple(r.eigenvectors.shape) == (A.nrows, K) and r.eigenvectors.is_cuda and r.eigenvalues.dtype == torch.float64
