"""Eigenpairs inside an interval (GCGE_ChebBandCoefficients, GCGE_ChebBandFilter, GCGE_RunChFSIBand, csrc/host/chfsi.c) over the CPU
oracle's table, which offers no cheb_step: every filter step is MatDotMultiVec and two MultiVecAxpby, every accumulation of a pair of
iterates two MultiVecAxpby.

The case: make_problem("lap3d", 12), n = 1728, the integer stencil 6 / -1, interval [1.0, 1.55]: 23 eigenvalues below it, 25 inside,
none within 0.015 of an end (test_the_premise).  Bounds: the spectrum widened by 5 % of its width at each end.  Degree 60, 48
columns; a numpy prototype of the algorithm converges in 13 outer iterations, the runs here get -gcge_max_niter 40."""
import ctypes as C

import numpy as np
import pytest

from gcge_amd.lib import ChFSIBandResult, band_coefficients, csr_to_scipy, make_problem, run_chfsi_band
from helpers import bits, uniform

LO, HI = 1.0, 1.55
INSIDE, BELOW = 25, 23
SHIFT = 1.3
DEGREE, NEVMAX = 60, 48


def coefficients_numpy(degree, a, b, lmin, lmax):
    """the Jackson-damped expansion of the indicator of [a, b], as include/gcge_solver.h states it"""
    c, e = 0.5 * (lmax + lmin), 0.5 * (lmax - lmin)
    tha, thb = np.arccos(max(-1.0, (a - c) / e)), np.arccos(min(1.0, (b - c) / e))
    j = np.arange(1, degree + 1)
    gamma = np.concatenate([[(tha - thb) / np.pi], 2.0 * (np.sin(j * tha) - np.sin(j * thb)) / (j * np.pi)])
    j = np.arange(degree + 1)
    al = np.pi / (degree + 2)
    return gamma * ((degree + 2 - j) * np.cos(j * al) + np.sin(j * al) / np.tan(al)) / (degree + 2)


def poly(mu, lmin, lmax, lam):
    """p(lam) = sum_j mu_j T_j((lam - c) / e)"""
    c, e = 0.5 * (lmax + lmin), 0.5 * (lmax - lmin)
    return np.polynomial.chebyshev.chebval((np.asarray(lam) - c) / e, mu)


def band_filter_numpy(S, X, mu, lmin, lmax):
    c, e = 0.5 * (lmax + lmin), 0.5 * (lmax - lmin)
    Tp, T = X, (S @ X - c * X) / e
    Y = mu[0] * Tp + mu[1] * T
    for j in range(2, len(mu)):
        Tp, T = T, (2.0 / e) * (S @ T - c * T) - Tp
        Y = Y + mu[j] * T
    return Y


def bounds_of(lam):
    w = lam[-1] - lam[0]
    return float(lam[0] - 0.05 * w), float(lam[-1] + 0.05 * w)


@pytest.fixture(scope="module")
def lap12(oracle):
    A, _ = make_problem("lap3d", 12)
    S = csr_to_scipy(A)
    lam, V = np.linalg.eigh(S.toarray())
    return A, S, oracle.matrix(A), lam, V


@pytest.fixture(scope="module")
def lap12_shifted(oracle):
    """the same matrix with -SHIFT on the diagonal: indefinite"""
    A, _ = make_problem("lap3d", 12)
    val = np.ctypeslib.as_array(A.val, (int(A.nnz),))
    assert np.count_nonzero(val == 6.0) == A.nrows
    val[val == 6.0] -= SHIFT
    return A, csr_to_scipy(A), oracle.matrix(A)


def test_the_premise(lap12):
    A, S, mA, lam, V = lap12
    assert S.shape[0] == 1728 and np.count_nonzero(lam < LO) == BELOW and np.count_nonzero((lam >= LO) & (lam <= HI)) == INSIDE
    assert np.abs(lam - LO).min() > 0.015 and np.abs(lam - HI).min() > 0.015
    assert lam[0] - SHIFT < 0.0 < lam[-1] - SHIFT                                      # the shifted matrix is indefinite


@pytest.mark.parametrize("degree", [2, 3, 60, 61])
def test_coefficients_equal_the_formula(lap12, degree):
    lmin, lmax = bounds_of(lap12[3])
    for a, b in ((LO, HI), (lmin - 1.0, HI), (LO, lmax + 1.0)):                       # (an end outside the bounds is clipped)
        assert np.abs(band_coefficients(degree, a, b, lmin, lmax) - coefficients_numpy(degree, a, b, lmin, lmax)).max() <= 1e-14


def test_coefficients_refuse_bad_arguments():
    for args in ((1, 1.0, 2.0, 0.0, 12.0), (8, 2.0, 1.0, 0.0, 12.0), (8, 1.0, 1.0, 0.0, 12.0), (8, 1.0, 2.0, 12.0, 0.0),
                 (8, 1.0, 2.0, 3.0, 12.0), (8, 13.0, 14.0, 0.0, 12.0)):
        with pytest.raises(ValueError):
            band_coefficients(*args)


def test_edge_values_are_about_one_half(lap12):
    lmin, lmax = bounds_of(lap12[3])
    mu = band_coefficients(DEGREE, LO, HI, lmin, lmax)
    pa, pb = poly(mu, lmin, lmax, LO), poly(mu, lmin, lmax, HI)
    print("p(a) =", pa, "p(b) =", pb)
    assert 0.45 <= pa <= 0.55 and 0.45 <= pb <= 0.55


@pytest.mark.parametrize("degree", [2, 3, 4, 9])
def test_band_filter_equals_the_recurrence_in_numpy(oracle, lap12, degree):
    """Column-wise |Y - Y_np| <= 1e-10 |X|: the unscaled iterates T_j((A - c) / e) X are bounded by |X| (|T_j| <= 1 on the bounds), an
    error of step i reaches T_j times at most (j - i + 1) (the U_{j-i} growth), and sum |mu_j| <= 1 + (2 / pi) sum_j 1 / j < 3 at these
    degrees; as in tests/test_chfsi_host.py that is degree^2 (nnz_row + 3) (2 |A|_inf / e + 2) eps times 3, about 1e-12."""
    A, S, mA, lam, V = lap12
    n, m = S.shape[0], 4
    lmin, lmax = bounds_of(lam)
    X = np.asfortranarray(uniform(17, (n, m)) - 0.5)
    mu = coefficients_numpy(degree, LO, HI, lmin, lmax)
    assert np.abs(mu).sum() <= 1.0 + (2.0 / np.pi) * np.sum(1.0 / np.arange(1, degree + 1))
    ref = band_filter_numpy(S, X, mu, lmin, lmax)
    mx = oracle.mv_from_numpy(mA, np.column_stack([np.full(n, 3.0), X, np.full(n, 5.0)]))
    w1, w2, acc = oracle.ops.mv_create(m, mA), oracle.ops.mv_create(m + 1, mA), oracle.ops.mv_create(m, mA)
    try:
        rc = oracle.h.GCGE_ChebBandFilter(mA, mx, 1, m, degree, LO, HI, lmin, lmax, w1, w2, acc, oracle.ops_handle)
        got = oracle.mv_to_numpy(mx, n, 0, m + 2)
        kept = oracle.mv_to_numpy(acc, n, 0, m)
    finally:
        oracle.ops.mv_destroy(mx, m + 2); oracle.ops.mv_destroy(w1, m); oracle.ops.mv_destroy(w2, m + 1); oracle.ops.mv_destroy(acc, m)
    assert rc == 0
    assert np.all(got[:, 0] == 3.0) and np.all(got[:, -1] == 5.0)
    err = np.linalg.norm(got[:, 1:1 + m] - ref, axis=0) / np.linalg.norm(X, axis=0)
    print("degree", degree, "max column error / |X|:", err.max())
    assert np.all(err <= 1e-10)
    assert np.array_equal(bits(kept), bits(np.asfortranarray(got[:, 1:1 + m])))          # acc keeps the result


def test_band_filter_refuses_bad_arguments(oracle, lap12):
    A, S, mA, lam, V = lap12
    n, m = S.shape[0], 2
    X = np.asfortranarray(uniform(19, (n, m)) - 0.5)
    mx, w1, w2, acc = (oracle.mv_from_numpy(mA, X),) + tuple(oracle.ops.mv_create(m, mA) for _ in range(3))
    f = lambda *a: oracle.h.GCGE_ChebBandFilter(mA, *a, oracle.ops_handle)
    try:
        assert f(mx, 0, m, 1, LO, HI, 0.0, 12.0, w1, w2, acc) == -1           # degree < 2
        assert f(mx, 0, m, 4, HI, LO, 0.0, 12.0, w1, w2, acc) == -1           # a >= b
        assert f(mx, 0, m, 4, LO, HI, 12.0, 0.0, w1, w2, acc) == -1           # lmin >= lmax
        assert f(mx, 0, m, 4, 13.0, 14.0, 0.0, 12.0, w1, w2, acc) == -1       # the interval misses the bounds
        assert f(mx, 0, m, 4, LO, HI, 0.0, 12.0, w1, w2, mx) == -1            # aliased blocks
        assert f(mx, 0, m, 4, LO, HI, 0.0, 12.0, w1, w2, w1) == -1
        assert f(mx, 0, m, 4, LO, HI, 0.0, 12.0, w1, w1, acc) == -1
        assert f(mx, 0, m, 4, LO, HI, 0.0, 12.0, w1, w2, None) == -1
        assert np.array_equal(bits(oracle.mv_to_numpy(mx, n, 0, m)), bits(X))
    finally:
        for v in (mx, w1, w2, acc):
            oracle.ops.mv_destroy(v, m)


def band_args(lo, hi, nev_max=NEVMAX, bounds=None, degree=DEGREE):
    args = ["-chfsi_band_lo", repr(lo), "-chfsi_band_hi", repr(hi), "-nevMax", nev_max, "-chfsi_degree", degree, "-gcge_rel_tol", "1e-8",
            "-gcge_max_niter", 40]
    if bounds is not None:
        args += ["-chfsi_lower_bound", repr(bounds[0]), "-chfsi_upper_bound", repr(bounds[1])]
    return args


def solve(oracle, mA, n, args, nev_max=NEVMAX, start=None):
    """(eval, result, return code, eigenvector block as numpy) of one GCGE_RunChFSIBand"""
    evec = oracle.ops.mv_create(nev_max, mA) if start is None else \
        oracle.mv_from_numpy(mA, np.column_stack([start, np.zeros((n, nev_max - start.shape[1]))]))
    try:
        ev, res, rc = run_chfsi_band(oracle.ops_handle, mA, args, evec, given=0 if start is None else start.shape[1])
        V = oracle.mv_to_numpy(evec, n, 0, nev_max)
    finally:
        oracle.ops.mv_destroy(evec, nev_max)
    return ev, res, rc, V


def check_pairs(S, want, ev, res, rc, V):
    k = len(want)
    assert rc == 0 and res.converged == 1 and res.nevConv == k, (rc, res.converged, res.nevConv, res.numIter)
    assert np.all(np.abs(ev[:k] - want) <= 1e-8 * np.abs(want))
    R = S @ V[:, :k] - V[:, :k] * ev[:k]
    assert np.all(np.linalg.norm(R, axis=0) <= 1.01e-8 * np.abs(ev[:k]))
    assert np.abs(V[:, :k].T @ V[:, :k] - np.eye(k)).max() <= 1e-12


@pytest.fixture(scope="module")
def cold(oracle, lap12):
    A, S, mA, lam, V = lap12
    return solve(oracle, mA, S.shape[0], band_args(LO, HI, bounds=bounds_of(lam)))


def test_run_with_given_bounds_finds_the_25_pairs(lap12, cold):
    A, S, mA, lam, V = lap12
    ev, res, rc, X = cold
    lmin, lmax = bounds_of(lam)
    print("outer iterations:", res.numIter, "spurious at the end:", res.spurious, "edge:", res.edge)
    check_pairs(S, lam[BELOW:BELOW + INSIDE], ev, res, rc, X)
    assert 1 <= res.numIter <= 40 and res.degree == DEGREE and res.lmin == lmin and res.lmax == lmax
    mu = coefficients_numpy(DEGREE, LO, HI, lmin, lmax)
    assert abs(res.edge - min(poly(mu, lmin, lmax, LO), poly(mu, lmin, lmax, HI))) <= 1e-12


def test_run_with_lanczos_bounds_finds_the_25_pairs(oracle, lap12):
    A, S, mA, lam, V = lap12
    ev, res, rc, X = solve(oracle, mA, S.shape[0], band_args(LO, HI))
    print("outer iterations:", res.numIter, "bounds:", res.lmin, res.lmax, "spectrum:", lam[0], lam[-1])
    assert res.lmin <= lam[0] and lam[-1] <= res.lmax
    check_pairs(S, lam[BELOW:BELOW + INSIDE], ev, res, rc, X)
    mu = coefficients_numpy(DEGREE, LO, HI, res.lmin, res.lmax)
    assert abs(res.edge - min(poly(mu, res.lmin, res.lmax, LO), poly(mu, res.lmin, res.lmax, HI))) <= 1e-12


def test_indefinite_matrix_same_eigenvectors(oracle, lap12, lap12_shifted, cold):
    """A - 1.3 I with the interval [-0.3, 0.25]: the same 25 eigenvectors, the eigenvalues shifted"""
    A, S, mA, lam, V = lap12
    A2, S2, mA2 = lap12_shifted
    lmin, lmax = bounds_of(lam)
    ev, res, rc, X = solve(oracle, mA2, S.shape[0], band_args(LO - SHIFT, HI - SHIFT, bounds=(lmin - SHIFT, lmax - SHIFT)))
    want = lam[BELOW:BELOW + INSIDE] - SHIFT
    print("outer iterations:", res.numIter, "smallest |lambda|:", np.abs(want).min())
    check_pairs(S2, want, ev, res, rc, X)
    P, P0 = X[:, :INSIDE] @ X[:, :INSIDE].T, cold[3][:, :INSIDE] @ cold[3][:, :INSIDE].T      # the same invariant subspace
    assert np.abs(P - P0).max() <= 1e-6


def test_a_block_of_20_columns_is_too_small(oracle, lap12):
    A, S, mA, lam, V = lap12
    ev, res, rc, X = solve(oracle, mA, S.shape[0], band_args(LO, HI, nev_max=20, bounds=bounds_of(lam)), nev_max=20)
    print("outer iterations:", res.numIter)
    assert rc == -6 and res.nevConv == 20 and res.converged == 0


def test_warm_start_needs_fewer_iterations(oracle, lap12, cold):
    A, S, mA, lam, V = lap12
    ev, res, rc, X = cold
    ev2, res2, rc2, X2 = solve(oracle, mA, S.shape[0], band_args(LO, HI, bounds=bounds_of(lam)), start=X[:, :INSIDE])
    print("warm start: outer iterations", res2.numIter, "cold:", res.numIter)
    check_pairs(S, lam[BELOW:BELOW + INSIDE], ev2, res2, rc2, X2)
    assert res2.numIter < res.numIter


def test_run_refuses_bad_arguments_and_leaves_evec(oracle, lap12):
    A, S, mA, lam, V = lap12
    n = S.shape[0]
    X = np.asfortranarray(uniform(23, (n, 8)) - 0.5)
    good = ["-chfsi_band_lo", LO, "-chfsi_band_hi", HI, "-nevMax", 8]
    for args, given in ((good[2:], 0), (good[:2] + good[4:], 0), (good[:4], 0), (["-chfsi_band_lo", HI, "-chfsi_band_hi", LO, "-nevMax", 8], 0),
                        (good + ["-chfsi_degree", 1], 0), (good + ["-gcge_max_niter", -1], 0), (good, 9), (good, -1),
                        (good + ["-chfsi_lower_bound", 12.0, "-chfsi_upper_bound", 0.0], 0),
                        (good + ["-chfsi_lower_bound", 2.0, "-chfsi_upper_bound", 12.0], 0)):
        evec = oracle.mv_from_numpy(mA, X)
        try:
            ev, res, rc = run_chfsi_band(oracle.ops_handle, mA, args if "-nevMax" in args else args + ["-nevConv", 4], evec, given=given)
            assert rc == -1, (args, given, rc)
            assert np.array_equal(bits(oracle.mv_to_numpy(evec, n, 0, 8)), bits(X))
        finally:
            oracle.ops.mv_destroy(evec, 8)
    evec = oracle.mv_from_numpy(mA, X)
    try:
        assert oracle.h.GCGE_RunChFSIBand(None, 0, None, oracle.ops_handle, None, evec, 0, None) == -1
    finally:
        oracle.ops.mv_destroy(evec, 8)


def test_table_is_left_as_found(oracle, lap12):
    A, S, mA, lam, V = lap12
    st = oracle.ops.struct
    before = (st.MultiVecOrth, st.orth_workspace)
    ev, res, rc, _ = solve(oracle, mA, S.shape[0], band_args(LO, HI, nev_max=6, degree=4)[:-2] + ["-gcge_max_niter", 1], nev_max=6)
    assert rc == 0 and (st.MultiVecOrth, st.orth_workspace) == before
    assert isinstance(res, ChFSIBandResult)
