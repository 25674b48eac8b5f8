"""gcge_amd.solve / HipBackend.linear_solver on the GPU: the back-end's three sweeps against the same driver over the slots, the
true residual of every solve recomputed with torch.sparse in float64, the SCF shape of use (new values, refresh, warm start), a
star + dense-block handle, a re-ordered handle, and the interface.

The residual bound S_j = 16 eps (|A|_inf |x_j| + |b_j|) / |b_j| is the rounding of a row sum for two evaluations (the library's
and torch's): the reported relative residual equals torch's within S_j, and torch's is <= tol + S_j."""
import ctypes as C

import numpy as np
import pytest

from gcge_amd.lib import csr_to_scipy, make_problem, mat_device_stats

EPS = np.finfo(np.float64).eps
TOL = 1e-8


def device_csr(S):
    import torch
    S = S.tocsr()
    S.sort_indices()
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data.astype(np.float64)))


def rhs(n, m, seed):
    import torch
    return torch.from_numpy(np.random.default_rng(seed).random((n, m)) - 0.5).cuda()


def check_residual(S, b, r, tol=TOL, converged=True):
    """r.residual_norms against torch.sparse's |b - A x| / |b| within S_j; with converged: torch's value <= tol + S_j"""
    import torch
    t = device_csr(S)
    A = torch.sparse_csr_tensor(t[0].long(), t[1].long(), t[2], size=S.shape)
    b2, x2 = b.reshape(S.shape[0], -1).double(), r.x.reshape(S.shape[0], -1)
    nb = torch.linalg.norm(b2, dim=0)
    true = torch.linalg.norm(b2 - A @ x2, dim=0) / nb
    slack = 16 * EPS * (abs(S).sum(axis=1).max() * torch.linalg.norm(x2, dim=0) + nb) / nb
    print("residuals", r.residual_norms.cpu().numpy(), "torch", true.cpu().numpy(), "iterations", r.iterations, "%.1f ms" % (1e3 * r.seconds))
    assert r.x.dtype == torch.float64 and r.x.is_cuda and tuple(r.x.shape) == tuple(b.shape)
    assert r.residual_norms.is_cuda and r.converged.dtype == torch.bool and r.converged.shape == r.residual_norms.shape == true.shape
    assert torch.all(torch.abs(r.residual_norms - true) <= slack), (r.residual_norms, true, slack)
    if converged:
        assert torch.all(r.converged) and torch.all(true <= tol + slack), (true, slack)


@pytest.fixture(scope="module")
def lap16():
    return csr_to_scipy(make_problem("lap3d", 16)[0]).tocsr()


@pytest.mark.gpu
def test_hook_path_equals_slot_path(hip, lap16, monkeypatch):
    """the three sweeps of pcg_sweeps.hip against the slot sequences they replace, in the same driver"""
    import torch
    from gcge_amd import solve
    b = rhs(lap16.shape[0], 8, 3)
    r = solve(device_csr(lap16), b, tol=TOL, amg_levels=3, backend=hip)
    monkeypatch.setenv("GCGE_NO_PCG_SWEEPS", "1")
    s = solve(device_csr(lap16), b, tol=TOL, amg_levels=3, backend=hip)
    monkeypatch.delenv("GCGE_NO_PCG_SWEEPS")
    check_residual(lap16, b, r)
    check_residual(lap16, b, s)
    dx = (torch.linalg.norm(r.x - s.x, dim=0) / torch.linalg.norm(s.x, dim=0)).cpu().numpy()
    print("hooks against slots: relative difference of x", dx, "iterations", r.iterations, s.iterations)
    assert np.all(dx <= 1e-12)
    assert r.iterations == s.iterations and 1 <= r.iterations <= 16
    assert torch.all(torch.abs(r.residual_norms - s.residual_norms) <= 1e-12 * TOL + 1e-3 * s.residual_norms)


@pytest.mark.gpu
def test_live_handle_hierarchy_and_solver_through_an_scf_step(hip, lap16):
    """a handle, a kept hierarchy, a kept solver; then new values in place (a shifted diagonal), refresh(), and a second solve
    warm-started from the first x, which needs no more iterations than a cold one"""
    import scipy.sparse as sp
    import torch
    n = lap16.shape[0]
    b = rhs(n, 8, 5)
    m = hip.matrix_from_device(*device_csr(lap16), updatable=True)
    h = None
    try:
        h = hip.multigrid(m, levels=3, block_size=8)
        s0 = mat_device_stats()
        with hip.linear_solver(m, amg=h, max_cols=8) as ls:
            r1 = ls.solve(b, tol=TOL)
            check_residual(lap16, b, r1)
            plain = hip.linear_solver(m, max_cols=8)
            try:
                rp = plain.solve(b, tol=TOL)
            finally:
                plain.close()
            check_residual(lap16, b, rp)
            print("V-cycle preconditioner:", r1.iterations, "outer iterations; plain fused CG:", rp.iterations)
            assert 4 * r1.iterations <= rp.iterations
            S2 = (lap16 + 0.05 * sp.identity(n)).tocsr()
            S2.sort_indices()
            assert S2.nnz == lap16.nnz
            assert hip.matrix_update_values(m, torch.from_numpy(S2.data).cuda())
            assert h.refresh() is True
            warm = ls.solve(b, x0=r1.x, tol=TOL)
            cold = ls.solve(b, tol=TOL)
            check_residual(S2, b, warm)
            check_residual(S2, b, cold)
            print("after the update: warm", warm.iterations, "cold", cold.iterations)
            assert warm.iterations <= cold.iterations
        s1 = mat_device_stats()
        assert s1[0] == s0[0] and s1[3] == s0[3]                     # no matrix created, nothing downloaded
    finally:
        if h is not None:
            h.close()
        hip.free_matrix(m)


@pytest.mark.gpu
def test_star_and_dense_block_handle(hip):
    S = csr_to_scipy(make_problem("sio2", 16)[0]).tocsr()
    b = rhs(S.shape[0], 4, 7)
    m = hip.matrix_from_device(*device_csr(S), updatable=True)
    try:
        print("form:", hip.g.gcge_hip_mat_spmm_form(m).decode())
        with hip.multigrid(m, levels=3, block_size=4) as h, hip.linear_solver(m, amg=h, max_cols=4) as ls:
            check_residual(S, b, ls.solve(b, tol=TOL))
    finally:
        hip.free_matrix(m)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [16, 23])
def test_reordered_handle_returns_x_in_the_callers_order(hip, N):
    """A randomly permuted Lap3D N^3 under reorder mode 1: the handle keeps P A P^T, b goes in and x comes back in the caller's row
    order.  The back-end keeps ONE row order per problem size while a matrix of that size is alive, so in a process where an earlier
    test left a 16^3 matrix in the caller's order behind, the 16^3 handle here follows it and stays "as given" (alone, this file
    re-orders it); 23^3 is a size no other test uses, and there the handle must be re-ordered."""
    S0 = csr_to_scipy(make_problem("lap3d", N)[0]).tocsr()
    n = S0.shape[0]
    p = np.random.default_rng(11).permutation(n)
    S = S0[p][:, p].tocsr()
    S.sort_indices()
    b = rhs(n, 4, 9)
    hip.g.gcge_hip_spmm_reorder_mode(1)
    try:
        m = hip.matrix_from_device(*device_csr(S), updatable=True)
    finally:
        hip.g.gcge_hip_spmm_reorder_mode(0)
    try:
        order = hip.g.gcge_hip_mat_row_order(m).decode()
        print("N", N, "row order:", order)
        assert order != "as given" or N == 16
        with hip.multigrid(m, levels=3, block_size=4) as h, hip.linear_solver(m, amg=h, max_cols=4) as ls:
            check_residual(S, b, ls.solve(b, tol=TOL))
    finally:
        hip.free_matrix(m)
        hip.g.gcge_hip_bpcg_release(hip.ops_handle)      # (the fused CG's blocks of this size live in the handle's order)


class Foreign:
    """an object that has __cuda_array_interface__ and nothing else (it keeps its tensor alive)"""

    def __init__(self, t):
        self._t = t
        self.__cuda_array_interface__ = t.__cuda_array_interface__


@pytest.mark.gpu
def test_interface(hip, lap16):
    import torch
    from gcge_amd import NoConvergence, SolveResult, solve
    n = lap16.shape[0]
    b = rhs(n, 4, 13)
    m = hip.matrix_from_device(*device_csr(lap16))
    other = hip.matrix_from_device(*device_csr(lap16))
    free0 = None
    try:
        with hip.multigrid(m, levels=3, block_size=4) as h:
            for rep in range(2):                                         # the second round: nothing is left behind by the first
                s0 = mat_device_stats()
                r = solve(m, b[:, 0].contiguous(), amg=h, backend=hip)   # (n,)
                assert isinstance(r, SolveResult) and r.x.dim() == 1
                check_residual(lap16, b[:, 0].contiguous(), r)
                r = solve(m, Foreign(b), amg=h)                          # __cuda_array_interface__; the back-end is the hierarchy's
                check_residual(lap16, b, r)
                bc = b.t().contiguous().t()                              # column-major
                assert bc.stride() == (1, n)
                r2 = solve(m, bc, amg=h, backend=hip)
                check_residual(lap16, bc, r2)
                assert torch.equal(r2.x, r.x)
                r = solve(m, b, x0=Foreign(r.x), amg=h, backend=hip)     # a start that is the solution: no iteration
                assert r.iterations == 0
                assert mat_device_stats() == s0                          # a handle given: nothing created, nothing downloaded
                with pytest.raises(NoConvergence) as e:
                    solve(m, b, maxiter=1, amg=h, backend=hip)
                res = e.value.result
                assert not torch.any(res.converged) and res.iterations == 1
                check_residual(lap16, b, res, converged=False)
                assert torch.all(res.residual_norms > TOL)
                free = torch.cuda.mem_get_info()[0] + hip.g.gcge_hip_pool_cached_bytes()
                if rep == 0:
                    free0 = free
            assert free >= free0 - (1 << 20), "a round of solves left device memory behind"
            # what is refused
            with pytest.raises(ValueError):
                solve(other, b, amg=h, backend=hip)                      # not the handle the hierarchy was built on
            with pytest.raises(ValueError):
                hip.linear_solver(other, amg=h)
            with pytest.raises(ValueError):
                solve(device_csr(lap16), b, amg=h, backend=hip)
            with pytest.raises(ValueError):
                solve(m, b, amg=h, amg_levels=3, backend=hip)

            class AnotherBackend:
                pass
            with pytest.raises(ValueError):
                solve(m, b, amg=h, backend=AnotherBackend())
            with hip.linear_solver(m, amg=h, max_cols=2) as ls:
                with pytest.raises(ValueError):
                    ls.solve(b)                                          # 4 columns, created for 2
                with pytest.raises(ValueError):
                    ls.solve(b[:-1, :2])                                 # another row count
                with pytest.raises(TypeError):
                    ls.solve(b[:, :2].cpu())                             # a host tensor
                with pytest.raises(TypeError):
                    ls.solve(np.zeros((n, 2)))
                with pytest.raises(ValueError):
                    ls.solve(b[:, :2], x0=b[:, :1])
                check_residual(lap16, b[:, :2], ls.solve(b[:, :2]))      # and the solver still works
        s0 = mat_device_stats()
        r = solve(device_csr(lap16), b, amg_levels=3)                    # a triple, the default back-end, a hierarchy built inside
        check_residual(lap16, b, r)
        assert mat_device_stats()[0] >= s0[0] + 1
        r = solve(device_csr(lap16), b, backend=hip)                     # no preconditioner: the fused block CG
        check_residual(lap16, b, r)
        assert r.iterations > 30
    finally:
        hip.free_matrix(m)
        hip.free_matrix(other)
