"""Chebyshev moments and eigenvalue counts (GCGE_ChebMoments, GCGE_ChebCountFromMoments, csrc/host/chfsi.c) over the CPU oracle's table,
which offers no cheb_step_dots and no cheb_step: every step is MatDotMultiVec and two MultiVecAxpby, followed by two
MultiVecLocalInnerProd('D').

The case: make_problem("lap3d", 12), n = 1728, bounds = the spectrum widened by 5 % of its width at each end, as in
tests/test_chfsi_band_host.py.  The interval (0.3, 1.1) has both ends in gaps of the spectrum — 0.174 .. 0.345 (width 0.17) and
1.064 .. 1.151 (width 0.087) — and holds 25 eigenvalues; sum_i p(lambda_i) = 24.95 at degree 60 and 24.75 at degree 120 (numpy).  As a
contrast, (1.0, 1.55) of that file also holds 25, but its ends sit 0.020 and 0.028 from eigenvalues of high multiplicity, where p is still
near 1/2: sum_i p(lambda_i) = 29.2 there, so the trace of p is a biased count however many probes are taken.  Only that premise is
asserted for it, not an estimate."""
import ctypes as C

import numpy as np
import pytest

from gcge_amd.lib import count_from_moments, csr_to_scipy, make_problem
from helpers import bits, uniform
from test_chfsi_band_host import bounds_of, coefficients_numpy, poly

LO, HI, INSIDE = 0.3, 1.1, 25
CLUSTER_LO, CLUSTER_HI = 1.0, 1.55
PROBES, SEED, DEGREE = 64, 0, 60


@pytest.fixture(scope="module")
def lap12(oracle):
    A, _ = make_problem("lap3d", 12)
    S = csr_to_scipy(A)
    lam = np.linalg.eigvalsh(S.toarray())
    return A, S, oracle.matrix(A), lam


def moments_numpy(S, V, degree, lmin, lmax):
    """mu[j, col] = v^T T_j((S - c) / e) v directly: every iterate of the recurrence against v"""
    c, e = 0.5 * (lmax + lmin), 0.5 * (lmax - lmin)
    Tp, T = V, (S @ V - c * V) / e
    out = [np.sum(V * Tp, axis=0), np.sum(V * T, axis=0)]
    for _ in range(2, degree + 1):
        Tp, T = T, (2.0 / e) * (S @ T - c * T) - Tp
        out.append(np.sum(V * T, axis=0))
    return np.array(out[:degree + 1])


def moments(oracle, mA, V, degree, lmin, lmax, v0=1):
    """GCGE_ChebMoments on the window [v0, v0 + m) of a block of m + 2 columns: (return code, moments, the block after)"""
    n, m = V.shape
    block = np.asfortranarray(np.column_stack([np.full(n, 3.0)] * v0 + [V, np.full(n, 5.0)]))
    mv = oracle.mv_from_numpy(mA, block)
    w = [oracle.ops.mv_create(m, mA), oracle.ops.mv_create(m + 1, mA), oracle.ops.mv_create(m, mA)]
    mom = np.full((degree + 1, m), np.nan)
    try:
        rc = oracle.h.GCGE_ChebMoments(mA, mv, v0, m, degree, lmin, lmax, w[0], w[1], w[2], mom.ctypes.data_as(C.c_void_p), oracle.ops_handle)
        after = oracle.mv_to_numpy(mv, n, 0, block.shape[1])
    finally:
        oracle.ops.mv_destroy(mv, block.shape[1])
        for k, b in enumerate(w):
            oracle.ops.mv_destroy(b, m + (k == 1))
    return rc, mom, after, block


def rademacher(n, m, seed):
    return np.asfortranarray(2.0 * np.random.default_rng(seed).integers(0, 2, (n, m)) - 1.0)


def test_the_premise(lap12):
    A, S, mA, lam = lap12
    lmin, lmax = bounds_of(lam)
    assert S.shape[0] == 1728 and np.count_nonzero((lam >= LO) & (lam <= HI)) == INSIDE
    # both ends in gaps: the neighbours of 0.3 are 0.174 and 0.345, those of 1.1 are 1.064 and 1.151
    assert abs(lam[lam < LO].max() - 0.1743) < 1e-3 and abs(lam[lam > LO].min() - 0.3453) < 1e-3
    assert abs(lam[lam < HI].max() - 1.0641) < 1e-3 and abs(lam[lam > HI].min() - 1.1511) < 1e-3
    for degree, want in ((60, 24.95), (120, 24.75)):
        got = poly(coefficients_numpy(degree, LO, HI, lmin, lmax), lmin, lmax, lam).sum()
        print("degree", degree, "sum p(lambda_i) =", got)
        assert abs(got - want) <= 0.005
    # the contrast: as many inside, the ends within 0.03 of eigenvalues, and a trace of p that is 4 too large
    assert np.count_nonzero((lam >= CLUSTER_LO) & (lam <= CLUSTER_HI)) == INSIDE
    assert np.abs(lam - CLUSTER_LO).min() < 0.03 and np.abs(lam - CLUSTER_HI).min() < 0.03
    got = poly(coefficients_numpy(60, CLUSTER_LO, CLUSTER_HI, lmin, lmax), lmin, lmax, lam).sum()
    print("(1.0, 1.55), degree 60: sum p(lambda_i) =", got)
    assert abs(got - 29.2) <= 0.05


@pytest.mark.parametrize("degree", [1, 2, 3, 60, 61])
def test_moments_equal_the_recurrence_in_numpy(oracle, lap12, degree):
    """|mu_j - v^T T_j v| <= 1e-10 |v|^2 per column.  tests/test_chfsi_band_host.py derives about 1e-12 |v| for the error of every
    iterate t_k = T_k v, and |t_k| <= |v| (|T_k| <= 1 on the bounds).  A product t_k . t_l inherits |dt_k| |t_l| + |t_k| |dt_l| <=
    2e-12 |v|^2 from the iterates and n eps |v|^2 = 4e-13 |v|^2 from its own n = 1728 roundings; the doubling identity
    mu_2k = 2 t_k . t_k - mu_0 doubles that and adds the rounding of mu_0: about 5e-12 |v|^2.  The numpy reference carries the same
    iterate error.  An even and an odd degree of each size: the last step writes one moment or two."""
    A, S, mA, lam = lap12
    n, m = S.shape[0], 4
    lmin, lmax = bounds_of(lam)
    V = np.asfortranarray(uniform(29, (n, m)) - 0.5)
    rc, mom, after, block = moments(oracle, mA, V, degree, lmin, lmax)
    assert rc == 0 and not np.isnan(mom).any()
    assert np.array_equal(bits(after), bits(block))                                      # v is read only
    ref = moments_numpy(S, V, degree, lmin, lmax)
    err = np.abs(mom - ref).max(axis=0) / np.sum(V * V, axis=0)
    print("degree", degree, "max |mu - ref| / |v|^2 per column:", err)
    assert np.all(err <= 1e-10)
    assert np.all(np.abs(mom[0] - np.sum(V * V, axis=0)) <= 1e-12 * np.sum(V * V, axis=0))      # mu_0 = v . v


def test_window_origin_zero_gives_the_same_moments(oracle, lap12):
    A, S, mA, lam = lap12
    lmin, lmax = bounds_of(lam)
    V = np.asfortranarray(uniform(29, (S.shape[0], 4)) - 0.5)
    rc0, mom0, _, _ = moments(oracle, mA, V, 9, lmin, lmax, v0=0)
    rc1, mom1, _, _ = moments(oracle, mA, V, 9, lmin, lmax, v0=1)
    assert rc0 == 0 and rc1 == 0 and np.array_equal(bits(mom0), bits(mom1))


def test_moments_refuse_bad_arguments(oracle, lap12):
    A, S, mA, lam = lap12
    n, m = S.shape[0], 2
    V = np.asfortranarray(uniform(31, (n, m)) - 0.5)
    mv = oracle.mv_from_numpy(mA, V)
    w1, w2, w3 = (oracle.ops.mv_create(m, mA) for _ in range(3))
    mom = np.full((5, m), np.nan)
    f = lambda *a: oracle.h.GCGE_ChebMoments(mA, *a, mom.ctypes.data_as(C.c_void_p), oracle.ops_handle)
    try:
        assert f(mv, 0, m, 0, 0.0, 12.0, w1, w2, w3) == -1                      # degree < 1
        assert f(mv, 0, 0, 4, 0.0, 12.0, w1, w2, w3) == -1                      # m < 1
        assert f(mv, 0, m, 4, 12.0, 0.0, w1, w2, w3) == -1                      # lmin >= lmax
        assert f(mv, 0, m, 4, 12.0, 12.0, w1, w2, w3) == -1
        assert f(mv, 0, m, 4, 0.0, 12.0, mv, w2, w3) == -1                      # aliased blocks
        assert f(mv, 0, m, 4, 0.0, 12.0, w1, w1, w3) == -1
        assert f(mv, 0, m, 4, 0.0, 12.0, w1, w2, w1) == -1
        assert f(mv, 0, m, 4, 0.0, 12.0, w1, w2, w2) == -1
        assert f(mv, 0, m, 4, 0.0, 12.0, w1, w2, None) == -1
        assert oracle.h.GCGE_ChebMoments(mA, mv, 0, m, 4, 0.0, 12.0, w1, w2, w3, None, oracle.ops_handle) == -1
        assert np.isnan(mom).all()                                               # nothing written
        assert np.array_equal(bits(oracle.mv_to_numpy(mv, n, 0, m)), bits(V))
    finally:
        for v in (mv, w1, w2, w3):
            oracle.ops.mv_destroy(v, m)


@pytest.mark.parametrize("degree", [2, 3, 60])
def test_count_from_moments_equals_numpy(lap12, degree):
    """per_probe = mu @ moments to 1e-12 n (sum |mu_j| < 3 and |moments| <= n: the products' roundings stay below 61 * 3 eps n),
    count their mean, stderr the sample standard deviation / sqrt(m)"""
    A, S, mA, lam = lap12
    n, m = S.shape[0], 5
    lmin, lmax = bounds_of(lam)
    mom = moments_numpy(S, rademacher(n, m, 3), degree, lmin, lmax)
    count, err, per = count_from_moments(mom, lmin, lmax, (LO, HI))
    ref = coefficients_numpy(degree, LO, HI, lmin, lmax) @ mom
    assert np.all(np.abs(per - ref) <= 1e-12 * n)
    assert abs(count - ref.mean()) <= 1e-12 * n and abs(err - ref.std(ddof=1) / np.sqrt(m)) <= 1e-12 * n
    c1, e1, p1 = count_from_moments(mom[:, :1], lmin, lmax, (LO, HI))
    assert e1 == 0.0 and c1 == p1[0]                                             # one probe: no scatter to report


def test_count_from_moments_refuses_bad_arguments():
    mom = np.ones((5, 2))
    for args in ((mom, 0.0, 12.0, (2.0, 1.0)), (mom, 12.0, 0.0, (1.0, 2.0)), (mom, 0.0, 12.0, (13.0, 14.0)), (mom[:2], 0.0, 12.0, (1.0, 2.0))):
        with pytest.raises(ValueError):
            count_from_moments(*args)


def test_count_on_an_interval_with_both_ends_in_gaps(oracle, lap12):
    """64 seeded +-1 probes at degree 60 on (0.3, 1.1): the estimate lies within 4 standard errors of sum_i p(lambda_i) = 24.95 (a
    4-sigma band about the estimator's own mean), and the standard error is at most 1.5.  The path is deterministic for a given V;
    this seed gives count 25.35, stderr 0.83."""
    A, S, mA, lam = lap12
    n = S.shape[0]
    lmin, lmax = bounds_of(lam)
    V = rademacher(n, PROBES, SEED)
    rc, mom, _, _ = moments(oracle, mA, V, DEGREE, lmin, lmax, v0=0)
    assert rc == 0 and np.all(mom[0] == n)                                       # v^T v = n exactly
    count, err, per = count_from_moments(mom, lmin, lmax, (LO, HI))
    trace = poly(coefficients_numpy(DEGREE, LO, HI, lmin, lmax), lmin, lmax, lam).sum()
    print("count", count, "stderr", err, "sum p(lambda_i)", trace, "inside", INSIDE)
    assert abs(count - trace) <= 4.0 * err and err <= 1.5
