"""gcge_amd.eigenvalue_count, count_from_moments, spectral_density and HipBackend.chebyshev_moments: counting before solving, behind the
torch face.  The case is that of tests/test_kpm_host.py: lap3d 12 (n = 1728), the interval (0.3, 1.1) with both ends in gaps and 25
eigenvalues inside, bounds = the spectrum widened by 5 %, degree 60, 64 seeded +-1 probes — as a sparse_csr tensor and as a handle.

With the same V the count equals the CPU oracle's to 1e-9 n: both run GCGE_ChebMoments, whose moments tests/test_kpm_host.py bounds by
1e-10 |v|^2 = 1e-10 n against the recurrence in numpy, so two tables differ by at most 2e-10 n in every moment, and
sum_j |mu_j| < 3 turns that into 6e-10 n in a count.  GCGE_NO_CHEB_STEP_DOTS=1 (the step, then two inner products) gives moments
within 1e-10 n of the slot's: the steps write the same bits either way, so the iterates are the same, and the two routes add the same n
products, each bounded in sum by |v|^2 = n, in different orders: n eps n = 4e-13 n per sum, doubled by the identities."""
import numpy as np
import pytest

from gcge_amd.lib import cheb_stats, cheb_step_dots_stats, count_from_moments as count_c, csr_to_scipy, make_problem
from test_chfsi_band_host import bounds_of, coefficients_numpy, poly
from test_eigsh import to_torch_csr
from test_kpm_host import DEGREE, HI, INSIDE, LO, PROBES, SEED, moments as oracle_moments, rademacher

_lap12 = {}


def lap12():
    if not _lap12:
        A, _ = make_problem("lap3d", 12)
        S = csr_to_scipy(A)
        lam = np.linalg.eigvalsh(S.toarray())
        _lap12.update(A=A, S=S, lam=lam, bounds=bounds_of(lam))
    return _lap12["A"], _lap12["S"], _lap12["lam"], _lap12["bounds"]


def test_refusals_need_no_device():
    """raised before anything imports torch or touches a back-end"""
    from gcge_amd import count_from_moments, eigenvalue_count
    ok = dict(interval=(LO, HI), lower_bound=-0.4, upper_bound=12.4)
    for kw in (dict(ok, interval=(HI, LO)), dict(ok, interval=(LO, LO)), dict(ok, interval=(LO, float("inf"))), dict(ok, interval=(float("nan"), HI)),
               dict(ok, interval=3.0), dict(ok, interval=(1.0, 2.0, 3.0)), dict(ok, probes=0), dict(ok, degree=1), dict(ok, lower_bound=12.4, upper_bound=-0.4),
               dict(ok, lower_bound=float("nan")), dict(ok, upper_bound=float("inf")), dict(ok, upper_bound=0.2), dict(ok, lower_bound=1.2),
               dict(ok, V=object())):
        with pytest.raises(ValueError) as e:
            eigenvalue_count(None, **kw)
        assert str(e.value).startswith("eigenvalue_count:"), (kw, str(e.value))
    for args in ((None, -0.4, 12.4, (HI, LO)), (None, 12.4, -0.4, (LO, HI)), (None, None, 12.4, (LO, HI)), (None, -0.4, 12.4, (13.0, 14.0))):
        with pytest.raises(ValueError) as e:
            count_from_moments(*args)
        assert str(e.value).startswith("count_from_moments:"), (args, str(e.value))


@pytest.fixture(scope="module")
def counted(hip):
    """eigenvalue_count on the sparse_csr tensor with a given V and with the seeded probes, and how the stats moved"""
    import torch
    from gcge_amd import eigenvalue_count
    A, S, lam, (lmin, lmax) = lap12()
    Vh = rademacher(S.shape[0], PROBES, SEED)
    V = torch.from_numpy(np.ascontiguousarray(Vh)).cuda()
    V0 = V.clone()
    d0, s0 = cheb_step_dots_stats(), cheb_stats()
    r = eigenvalue_count(to_torch_csr(A), (LO, HI), degree=DEGREE, lower_bound=lmin, upper_bound=lmax, V=V, backend=hip)
    d1, s1 = cheb_step_dots_stats(), cheb_stats()
    assert torch.equal(V, V0)                                                        # V is unchanged
    return r, Vh, V, tuple(b - a for a, b in zip(d0, d1)), tuple(b - a for a, b in zip(s0, s1))


@pytest.mark.gpu
def test_count_agrees_with_the_cpu_oracle(oracle, counted):
    import torch
    r, Vh, V, dd, ds = counted
    A, S, lam, (lmin, lmax) = lap12()
    n = S.shape[0]
    rc, mom, _, _ = oracle_moments(oracle, oracle.matrix(A), Vh, DEGREE, lmin, lmax, v0=0)
    assert rc == 0
    count, err, per = count_c(mom, lmin, lmax, (LO, HI))
    for t, shape in ((r.moments, (DEGREE + 1, PROBES)), (r.per_probe, (PROBES,))):
        assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == shape
    print("count", r.count, "oracle", count, "stderr", r.stderr, "max moment difference / n", np.abs(r.moments.cpu().numpy() - mom).max() / n)
    assert abs(r.count - count) <= 1e-9 * n and abs(r.stderr - err) <= 1e-9 * n
    assert np.all(np.abs(r.per_probe.cpu().numpy() - per) <= 1e-9 * n)
    assert r.degree == DEGREE and r.lower_bound == lmin and r.upper_bound == lmax
    assert r.suggested_nev_max == int(np.ceil(1.5 * (r.count + 3.0 * r.stderr))) + 4
    assert sum(dd[:2]) == (DEGREE + 1) // 2 and dd[2] == 0 and ds == (0, 0, 0)       # one slot call per step, 30 steps, none through cheb_step
    trace = poly(coefficients_numpy(DEGREE, LO, HI, lmin, lmax), lmin, lmax, lam).sum()
    assert abs(r.count - trace) <= 4.0 * r.stderr and r.stderr <= 1.5               # the host test's check, on the device's numbers


@pytest.mark.gpu
def test_handle_and_seeded_probes(hip):
    """a handle for A, the probes drawn on the device: the same count for the same seed, +-1 columns (mu_0 = n), Lanczos bounds that
    enclose the spectrum, and the driver's degree rule when none is given"""
    from gcge_amd import eigenvalue_count
    A, S, lam, (lmin, lmax) = lap12()
    n = S.shape[0]
    mat = hip.matrix(A)
    try:
        r1 = eigenvalue_count(mat, (LO, HI), probes=16, seed=5, lower_bound=lmin, upper_bound=lmax, backend=hip)
        r2 = eigenvalue_count(mat, (LO, HI), probes=16, seed=5, lower_bound=lmin, upper_bound=lmax, backend=hip)
        r3 = eigenvalue_count(mat, (LO, HI), probes=16, seed=6, degree=20, backend=hip)
    finally:
        hip.free_matrix(mat)
    want = min(max(int(np.ceil(6.0 * (lmax - lmin) / (HI - LO))), 20), 1000)
    assert r1.degree == want and tuple(r1.moments.shape) == (want + 1, 16)
    assert r1.count == r2.count and r1.stderr == r2.stderr
    assert np.all(r1.moments[0].cpu().numpy() == n) and np.all(r3.moments[0].cpu().numpy() == n)
    assert r3.count != r1.count and r3.degree == 20
    assert r3.lower_bound <= lam[0] and lam[-1] <= r3.upper_bound
    trace = poly(coefficients_numpy(want, LO, HI, lmin, lmax), lmin, lmax, lam).sum()
    print("16 probes, degree", want, ": count", r1.count, "stderr", r1.stderr, "trace of p", trace)
    assert abs(r1.count - trace) <= 4.0 * r1.stderr


@pytest.mark.gpu
def test_count_from_moments_equals_a_fresh_call(hip, counted):
    from gcge_amd import count_from_moments, eigenvalue_count
    r, Vh, V, _, _ = counted
    A, S, lam, (lmin, lmax) = lap12()
    second = (2.0, 3.0)
    again = count_from_moments(r.moments, lmin, lmax, second)
    fresh = eigenvalue_count(to_torch_csr(A), second, degree=DEGREE, lower_bound=lmin, upper_bound=lmax, V=V, backend=hip)
    inside = np.count_nonzero((lam >= second[0]) & (lam <= second[1]))
    print("interval", second, ":", inside, "inside, count", again.count, "stderr", again.stderr)
    assert again.count == fresh.count and again.stderr == fresh.stderr and again.suggested_nev_max == fresh.suggested_nev_max
    assert np.array_equal(again.per_probe.cpu().numpy(), fresh.per_probe.cpu().numpy())
    assert again.degree == DEGREE and again.moments is r.moments
    same = count_from_moments(r.moments.cpu().numpy(), lmin, lmax, (LO, HI))          # a host array of moments counts the same
    assert same.count == r.count and same.stderr == r.stderr


@pytest.mark.gpu
def test_spectral_density_integrates_to_n(counted):
    import torch
    from gcge_amd import spectral_density
    r, _, _, _, _ = counted
    A, S, lam, (lmin, lmax) = lap12()
    n = S.shape[0]
    pts = torch.linspace(lmin, lmax, 2002, dtype=torch.float64)[1:-1]                 # 2000 points inside the bounds
    rho = spectral_density(r.moments, lmin, lmax, pts)
    assert rho.is_cuda and tuple(rho.shape) == (2000,) and float(rho.min()) >= -1e-9 * n
    total = float(torch.trapezoid(rho.cpu(), pts))
    print("integral of the density:", total, "n:", n)
    assert abs(total - n) <= 0.01 * n
    outside = spectral_density(r.moments, lmin, lmax, [lmin - 1.0, lmin, lmax, lmax + 1.0])
    assert torch.all(outside == 0.0)
    host = spectral_density(r.moments.cpu().numpy(), lmin, lmax, pts.numpy())       # host moments and points: the same density, on the host
    assert not host.is_cuda and torch.allclose(host, rho.cpu(), rtol=0.0, atol=1e-9 * n)


@pytest.mark.gpu
def test_suggested_nev_max_holds_the_25_pairs(hip, counted):
    from gcge_amd import eigsh
    r, _, _, _, _ = counted
    A, S, lam, (lmin, lmax) = lap12()
    assert r.suggested_nev_max > INSIDE
    e = eigsh(to_torch_csr(A), interval=(LO, HI), nev_max=r.suggested_nev_max, method="chebyshev", degree=DEGREE, lower_bound=lmin, upper_bound=lmax,
              maxiter=40, backend=hip)
    got = e.eigenvalues.cpu().numpy()
    want = lam[(lam >= LO) & (lam <= HI)]
    print("nev_max", r.suggested_nev_max, "pairs", e.converged, "iterations", e.iterations)
    assert e.converged == INSIDE and got.shape == (INSIDE,) and np.all(np.abs(got - want) <= 1e-8 * np.abs(want))


@pytest.mark.gpu
def test_without_the_slot_the_same_moments(hip, counted, monkeypatch):
    import torch
    r, Vh, V, _, _ = counted
    A, S, lam, (lmin, lmax) = lap12()
    n = S.shape[0]
    mat = hip.matrix(A)
    try:
        with_slot = hip.chebyshev_moments(mat, V, DEGREE, lmin, lmax)
        again = hip.chebyshev_moments(mat, V, DEGREE, lmin, lmax)
        monkeypatch.setenv("GCGE_NO_CHEB_STEP_DOTS", "1")
        d0, s0 = cheb_step_dots_stats(), cheb_stats()
        without = hip.chebyshev_moments(mat, V, DEGREE, lmin, lmax)
        d1, s1 = cheb_step_dots_stats(), cheb_stats()
    finally:
        hip.free_matrix(mat)
    assert d1 == d0 and sum(s1[:2]) - sum(s0[:2]) == (DEGREE + 1) // 2                 # every step through cheb_step, none through the slot
    assert torch.equal(with_slot, again)                                              # the same bits on every run
    assert float((with_slot - r.moments).abs().max()) <= 1e-10 * n                    # (another handle of the same matrix)
    diff = float((with_slot - without).abs().max())
    print("max |moments with the slot - without| / n:", diff / n)
    assert diff <= 1e-10 * n
