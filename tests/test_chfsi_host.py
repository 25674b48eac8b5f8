"""Chebyshev-filtered subspace iteration (csrc/host/chfsi.c) over the CPU oracle's table, which offers no cheb_step: every filter
step is MatDotMultiVec and two MultiVecAxpby.  GCGE_ChebFilter against the same recurrence in numpy; GCGE_RunChFSI against numpy's
dense eigenvalues, its upper bound, a given bound (no Lanczos product: counted through a wrapped MatDotMultiVec slot), a warm start,
bad arguments."""
import ctypes as C

import numpy as np
import pytest

from gcge_amd.lib import csr_to_scipy, make_problem, run_chfsi
from gcge_amd.ops_struct import SIGNATURES
from helpers import bits, uniform

EPS = np.finfo(np.float64).eps


def cheb_filter_numpy(S, X, degree, lower, upper, lowest):
    """the scaled three-term recurrence of GCGE_ChebFilter (include/gcge_solver.h)"""
    e, c = 0.5 * (upper - lower), 0.5 * (upper + lower)
    sigma1 = e / (lowest - c)
    tau, sigma = 2.0 / sigma1, sigma1
    Yp, Y = X, (sigma1 / e) * (S @ X - c * X)
    for _ in range(2, degree + 1):
        s2 = 1.0 / (tau - sigma)
        Yp, Y = Y, (2.0 * s2 / e) * (S @ Y - c * Y) - (sigma * s2) * Yp
        sigma = s2
    return Y


@pytest.fixture(scope="module")
def lap8(oracle):
    A, _ = make_problem("lap3d", 8)
    S = csr_to_scipy(A)
    return A, S, oracle.matrix(A), np.linalg.eigvalsh(S.toarray())


@pytest.fixture(scope="module")
def lap12(oracle):
    A, _ = make_problem("lap3d", 12)
    S = csr_to_scipy(A)
    return A, S, oracle.matrix(A), np.linalg.eigvalsh(S.toarray())


@pytest.mark.parametrize("degree", [1, 2, 3, 8])
def test_filter_equals_the_recurrence_in_numpy(oracle, lap8, degree):
    """Degree 8 on lap3d 8 (and 1, 2, 3: the result ends in each of the three blocks): column-wise |Y - Y_np| <= 1e-10 |X|.  On the
    scaled recurrence every iterate is bounded by |X| and an error of step i reaches the end times at most (degree - i + 1), about
    degree^2 (nnz_row + 3) (2 |A|_inf / e + 2) eps ~ 1e-12 in all; 1e-10 is that with two digits to spare.  Observed maximum at
    degree 8: 2.2e-17 |X| (profiles/chfsi/README.md)."""
    A, S, mA, lam = lap8
    n, m = S.shape[0], 4
    upper, lower, lowest = lam[-1], float(np.median(lam)), lam[0] - 0.1
    X = np.asfortranarray(uniform(7, (n, m)) - 0.5)
    ref = cheb_filter_numpy(S, X, degree, lower, upper, lowest)
    assert np.all(np.linalg.norm(ref, axis=0) <= 1.0001 * np.linalg.norm(X, axis=0))            # the premise: bounded by |X|
    mx = oracle.mv_from_numpy(mA, np.column_stack([np.full(n, 3.0), X, np.full(n, 5.0)]))       # the window [1, 1 + m) of a wider block
    w1, w2 = oracle.ops.mv_create(m, mA), oracle.ops.mv_create(m + 1, mA)
    try:
        rc = oracle.h.GCGE_ChebFilter(mA, mx, 1, m, degree, lower, upper, lowest, w1, w2, oracle.ops_handle)
        got = oracle.mv_to_numpy(mx, n, 0, m + 2)
    finally:
        oracle.ops.mv_destroy(mx, m + 2); oracle.ops.mv_destroy(w1, m); oracle.ops.mv_destroy(w2, m + 1)
    assert rc == 0
    assert np.all(got[:, 0] == 3.0) and np.all(got[:, -1] == 5.0)                               # the columns round the window
    err = np.linalg.norm(got[:, 1:1 + m] - ref, axis=0) / np.linalg.norm(X, axis=0)
    print("degree", degree, "max column error / |X|:", err.max())
    assert np.all(err <= 1e-10)


def test_filter_refuses_bad_arguments(oracle, lap8):
    A, S, mA, lam = lap8
    n, m = S.shape[0], 2
    X = np.asfortranarray(uniform(9, (n, m)) - 0.5)
    mx, w1, w2 = oracle.mv_from_numpy(mA, X), oracle.ops.mv_create(m, mA), oracle.ops.mv_create(m, mA)
    f = lambda *a: oracle.h.GCGE_ChebFilter(mA, *a, oracle.ops_handle)
    try:
        assert f(mx, 0, m, 0, 6.0, 12.0, 0.0, w1, w2) == -1            # degree < 1
        assert f(mx, 0, m, 4, 12.0, 12.0, 0.0, w1, w2) == -1           # lower >= upper
        assert f(mx, 0, m, 4, 6.0, 12.0, 6.0, w1, w2) == -1            # lowest >= lower
        assert f(mx, 0, m, 4, 6.0, 12.0, 0.0, mx, w2) == -1            # aliased blocks
        assert f(mx, 0, m, 4, 6.0, 12.0, 0.0, w1, w1) == -1
        assert np.array_equal(bits(oracle.mv_to_numpy(mx, n, 0, m)), bits(X))
    finally:
        oracle.ops.mv_destroy(mx, m); oracle.ops.mv_destroy(w1, m); oracle.ops.mv_destroy(w2, m)


ARGS = ["-nevConv", 8, "-nevMax", 16, "-chfsi_degree", 20, "-gcge_rel_tol", "1e-8", "-gcge_max_niter", 30]


def solve(oracle, mA, n, args, start=None):
    """(eval, result, return code, eigenvector block as numpy) of one GCGE_RunChFSI with 16 columns"""
    evec = oracle.ops.mv_create(16, mA) if start is None else oracle.mv_from_numpy(mA, np.column_stack([start, np.zeros((n, 16 - start.shape[1]))]))
    try:
        ev, res, rc = run_chfsi(oracle.ops_handle, mA, args, evec, given=0 if start is None else start.shape[1])
        V = oracle.mv_to_numpy(evec, n, 0, 16)
    finally:
        oracle.ops.mv_destroy(evec, 16)
    return ev, res, rc, V


@pytest.fixture(scope="module")
def cold(oracle, lap12):
    A, S, mA, lam = lap12
    return solve(oracle, mA, S.shape[0], ARGS)


def test_run_converges_to_the_dense_eigenvalues(lap12, cold):
    """lap3d 12, 8 of 16 columns, degree 20, 1e-8: all 8 within 30 outer iterations (the C run needs 6, a numpy prototype
    of the plain algorithm 5), eigenvalues within 1e-8 relative of eigvalsh, the Lanczos bound inside [lambda_max, 2 lambda_max]."""
    A, S, mA, lam = lap12
    ev, res, rc, V = cold
    print("outer iterations:", res.numIter, "upper bound:", res.upper, "lambda_max:", lam[-1])
    assert rc == 0 and res.nevConv == 8 and 1 <= res.numIter <= 30 and res.degree == 20
    assert np.all(np.abs(ev[:8] - lam[:8]) <= 1e-8 * np.abs(lam[:8]))
    assert lam[-1] <= res.upper <= 2 * lam[-1]
    R = S @ V[:, :8] - V[:, :8] * ev[:8]
    assert np.all(np.linalg.norm(R, axis=0) <= 1.01e-8 * np.abs(ev[:8]))
    assert np.abs(V[:, :8].T @ V[:, :8] - np.eye(8)).max() <= 1e-12


def test_given_upper_bound_makes_no_lanczos_product(oracle, lap12, cold):
    """-chfsi_upper_bound: res.upper is that value and the 10 single-column products of the Lanczos steps are not made (counted through
    a wrapped MatDotMultiVec slot); the start block is the same, so everything else is"""
    A, S, mA, lam = lap12
    n = S.shape[0]
    res, proto = SIGNATURES["MatDotMultiVec"]
    real = C.CFUNCTYPE(res, *proto)(oracle.ops.struct.MatDotMultiVec)
    calls = []

    def counted(mat, x, y, s, e, ops):
        calls.append(e[0] - s[0])
        real(mat, x, y, s, e, ops)
    wrapper = C.CFUNCTYPE(res, *proto)(counted)
    before = oracle.ops.struct.MatDotMultiVec
    oracle.ops.struct.MatDotMultiVec = C.cast(wrapper, C.c_void_p).value
    try:
        ev0, r0, rc0, _ = solve(oracle, mA, n, ARGS)
        with_lanczos = list(calls)
        del calls[:]
        ev1, r1, rc1, _ = solve(oracle, mA, n, ARGS + ["-chfsi_upper_bound", repr(float(cold[1].upper))])
        given = list(calls)
    finally:
        oracle.ops.struct.MatDotMultiVec = before
    assert rc0 == 0 and rc1 == 0 and r1.upper == cold[1].upper and r0.upper == cold[1].upper
    assert r1.numIter == r0.numIter == cold[1].numIter and r1.nevConv == 8
    assert with_lanczos.count(1) - given.count(1) == 10 and len(with_lanczos) - len(given) == 10, (len(with_lanczos), len(given))
    assert np.array_equal(bits(ev0), bits(ev1))


def test_warm_start_from_converged_vectors_needs_at_most_one_iteration(oracle, lap12, cold):
    A, S, mA, lam = lap12
    ev, res, rc, V = cold
    ev2, res2, rc2, _ = solve(oracle, mA, S.shape[0], ARGS, start=V)
    print("warm start: outer iterations", res2.numIter, "cold:", res.numIter)
    assert rc2 == 0 and res2.nevConv == 8 and res2.numIter <= 1 and res2.numIter < res.numIter
    assert np.all(np.abs(ev2[:8] - lam[:8]) <= 1e-8 * np.abs(lam[:8]))


def test_run_refuses_bad_arguments_and_leaves_evec(oracle, lap12):
    A, S, mA, lam = lap12
    n = S.shape[0]
    X = np.asfortranarray(uniform(11, (n, 16)) - 0.5)
    for args, given in ((["-nevConv", 8, "-nevMax", 4], 0), (["-nevConv", 0, "-nevMax", 16], 0),
                        (["-nevConv", 8, "-nevMax", 16, "-chfsi_degree", 0], 0), (ARGS, 17), (ARGS, -1),
                        (["-nevConv", 8, "-nevMax", 16, "-gcge_max_niter", -1], 0)):
        evec = oracle.mv_from_numpy(mA, X)
        try:
            ev, res, rc = run_chfsi(oracle.ops_handle, mA, args, evec, given=given)
            assert rc == -1, (args, given, rc)
            assert np.array_equal(bits(oracle.mv_to_numpy(evec, n, 0, 16)), bits(X))
        finally:
            oracle.ops.mv_destroy(evec, 16)
    evec = oracle.mv_from_numpy(mA, X)
    try:
        assert oracle.h.GCGE_RunChFSI(None, 0, None, oracle.ops_handle, None, evec, 0, None) == -1
    finally:
        oracle.ops.mv_destroy(evec, 16)


def test_table_is_left_as_found(oracle, lap12, cold):
    """ops->MultiVecOrth and its workspace are what they were before the run"""
    A, S, mA, lam = lap12
    st = oracle.ops.struct
    before = (st.MultiVecOrth, st.orth_workspace)
    ev, res, rc, _ = solve(oracle, mA, S.shape[0], ["-nevConv", 2, "-nevMax", 6, "-gcge_max_niter", 2])
    assert rc == 0 and (st.MultiVecOrth, st.orth_workspace) == before
