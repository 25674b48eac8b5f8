"""gcge_amd.eigsh(interval=(a, b), method="chebyshev", nev_max=N): every eigenpair inside an interval (GCGE_RunChFSIBand) behind the torch
face — matrices, start vectors and results as device tensors — and HipBackend.chebyshev_band_filter.

The cases are those of tests/test_chfsi_band_host.py (lap3d 12, [1.0, 1.55]: 25 pairs inside, 23 below), lap3d 16 with [0.437, 0.824]
(n = 4096, the smallest handle that takes the fused filter step: 27 inside, 11 below), make_problem("sio2", 12) (no pattern table) and
the indefinite lap3d 12 - 1.3 I.  Bounds on the pairs: eigenvalues 1e-8 relative (the driver stops a pair at |r| <= tol |lambda| with
tol = 1e-8, and |lambda~ - lambda| <= |r|), residuals recomputed in numpy <= 1.01e-8 |lambda| and V^T V - I <= 1e-12, as the host
test has them.  The iteration caps keep a stalled run from hiding; they are no performance claims."""
import numpy as np
import pytest

from gcge_amd.lib import band_coefficients, cheb_accum_stats, cheb_stats, csr_arrays, csr_to_scipy, make_problem
from helpers import lap3d_exact
from test_chfsi_band_host import BELOW, HI, INSIDE, LO, SHIFT, bounds_of
from test_eigsh import to_torch_csr

DEGREE, NEVMAX = 60, 48
LO16, HI16, INSIDE16, BELOW16 = 0.437, 0.824, 27, 11

_lap12 = {}


def lap12():
    """(A struct, scipy A, eigenvalues, eigenvectors) of lap3d 12, computed once"""
    if not _lap12:
        A, _ = make_problem("lap3d", 12)
        S = csr_to_scipy(A)
        lam, V = np.linalg.eigh(S.toarray())
        _lap12.update(A=A, S=S, lam=lam, V=V)
    return _lap12["A"], _lap12["S"], _lap12["lam"], _lap12["V"]


def band_kw(lam=None, **kw):
    out = dict(nev_max=NEVMAX, degree=DEGREE, method="chebyshev", maxiter=40)
    if lam is not None:
        out["lower_bound"], out["upper_bound"] = bounds_of(lam)
    out.update(kw)
    return out


def check_pairs(r, S, want):
    import torch
    n, k = S.shape[0], len(want)
    for t, shape in ((r.eigenvalues, (k,)), (r.eigenvectors, (n, k)), (r.residual_norms, (k,))):
        assert isinstance(t, torch.Tensor) and t.is_cuda and tuple(t.shape) == shape and t.dtype == torch.float64, (tuple(t.shape), shape)
    assert r.converged == k and r.iterations >= 0 and r.seconds > 0.0
    lam, V, rn = r.eigenvalues.cpu().numpy(), r.eigenvectors.cpu().numpy(), r.residual_norms.cpu().numpy()
    assert np.all(np.diff(lam) >= 0.0)
    err = np.abs(lam - want) / np.abs(want)
    res = np.linalg.norm(S @ V - V * lam, axis=0)
    orth = np.abs(V.T @ V - np.eye(k)).max()
    print("iterations %d, eigenvalue error %.2e, residual / |lambda| %.2e, orthogonality %.2e" % (r.iterations, err.max(), (res / np.abs(lam)).max(), orth))
    assert err.max() <= 1e-8, err
    assert np.all(res <= 1.01e-8 * np.abs(lam)), res / np.abs(lam)
    assert orth <= 1e-12
    assert np.all(np.abs(rn - res) <= 1e-6 * np.abs(lam)), (rn, res)      # (tests/test_eigsh.py: residual_sq may use expanded sums)


def test_the_premises():
    A, S, lam, V = lap12()
    assert np.count_nonzero(lam < LO) == BELOW and np.count_nonzero((lam >= LO) & (lam <= HI)) == INSIDE
    l16 = np.sort(lap3d_exact(16, 16 ** 3))
    assert l16.size == 4096 and np.count_nonzero(l16 < LO16) == BELOW16 and np.count_nonzero((l16 >= LO16) & (l16 <= HI16)) == INSIDE16
    assert np.abs(l16 - LO16).min() > 0.031 and np.abs(l16 - HI16).min() > 0.031


def test_refusals_need_no_device():
    """raised before eigsh imports torch or touches a back-end (a CPU process that has loaded the HIP library must not load torch's own
    runtime beside it)"""
    from gcge_amd import eigsh
    iv = dict(interval=(LO, HI), nev_max=NEVMAX, method="chebyshev")
    for kw in (dict(iv, method="gcg"), dict(iv, k=5), dict(interval=(LO, HI), method="chebyshev"), dict(iv, interval=(HI, LO)),
               dict(iv, interval=(LO, LO)), dict(iv, interval=(LO, float("inf"))), dict(iv, interval=(float("nan"), HI)), dict(iv, degree=1),
               dict(iv, eigenvector_grad=True), dict(iv, M=object()), dict(iv, block_size=8), dict(iv, amg_levels=3),
               dict(method="chebyshev"), dict(), dict(k=4, lower_bound=0.0, method="chebyshev")):
        with pytest.raises(ValueError) as e:
            eigsh(None, **kw)
        assert str(e.value).startswith("eigsh:"), (kw, str(e.value))
    with pytest.raises(ValueError) as e:
        eigsh(None, interval=(LO, HI), method="chebyshev")
    assert "nev_max" in str(e.value)


@pytest.fixture(scope="module")
def cold(hip):
    from gcge_amd import eigsh
    A, S, lam, V = lap12()
    return eigsh(to_torch_csr(A), interval=(LO, HI), backend=hip, **band_kw(lam))


@pytest.mark.gpu
def test_given_bounds_find_the_25_pairs(cold):
    A, S, lam, V = lap12()
    check_pairs(cold, S, lam[BELOW:BELOW + INSIDE])
    assert 1 <= cold.iterations <= 40


@pytest.mark.gpu
def test_lanczos_bounds_find_the_25_pairs(hip):
    from gcge_amd import eigsh
    A, S, lam, V = lap12()
    r = eigsh(to_torch_csr(A), interval=(LO, HI), backend=hip, **band_kw(maxiter=80))
    check_pairs(r, S, lam[BELOW:BELOW + INSIDE])


@pytest.mark.gpu
def test_lap3d_16_takes_the_fused_step_and_the_two_term_sums(hip):
    from gcge_amd import eigsh
    A, _ = make_problem("lap3d", 16)
    S = csr_to_scipy(A)
    l16 = np.sort(lap3d_exact(16, 16 ** 3))
    assert np.count_nonzero(l16 < LO16) == BELOW16 and np.count_nonzero((l16 >= LO16) & (l16 <= HI16)) == INSIDE16
    assert np.abs(l16 - LO16).min() > 0.031 and np.abs(l16 - HI16).min() > 0.031
    s0, a0 = cheb_stats(), cheb_accum_stats()
    r = eigsh(to_torch_csr(A), interval=(LO16, HI16), backend=hip, **band_kw(l16, maxiter=60))
    s1, a1 = cheb_stats(), cheb_accum_stats()
    check_pairs(r, S, l16[BELOW16:BELOW16 + INSIDE16])
    fused, swept, two, one = s1[0] - s0[0], s1[1] - s0[1], a1[0] - a0[0], a1[1] - a0[1]
    print("steps fused / swept: %d / %d, sums of two / one: %d / %d" % (fused, swept, two, one))
    assert fused > 0 and s1[2] == s0[2] and fused + swept == DEGREE * (r.iterations + 1)
    assert two == 30 * (r.iterations + 1) and one == r.iterations + 1 and a1[2] == a0[2]


def sio2_interval(lam):
    """(first index, count, a, b): 8 to 20 interior eigenvalues with the widest gaps on either side relative to the interval they span,
    a and b in the middle of those gaps"""
    best = None
    for i0 in range(8, 200):
        for c in range(8, 21):
            glo, ghi = lam[i0] - lam[i0 - 1], lam[i0 + c] - lam[i0 + c - 1]
            score = min(glo, ghi) / (lam[i0 + c - 1] - lam[i0] + glo + ghi)
            if best is None or score > best[0]:
                best = (score, i0, c)
    _, i0, c = best
    return i0, c, float(0.5 * (lam[i0 - 1] + lam[i0])), float(0.5 * (lam[i0 + c - 1] + lam[i0 + c]))


@pytest.mark.gpu
def test_sio2_on_the_sweep_path(hip):
    """make_problem("sio2", 12) has no pattern table: every filter step is product + sweep.  The interval holds 8 to 20 eigenvalues
    between the two widest gaps relative to its width (each end at least a tenth of the width from the nearest eigenvalue; the driver's own degree, 1000 here, converges in 6 outer iterations over the CPU oracle)."""
    from gcge_amd import eigsh
    A, _ = make_problem("sio2", 12)
    S = csr_to_scipy(A)
    lam = np.linalg.eigvalsh(S.toarray())
    i0, c, a, b = sio2_interval(lam)
    assert 8 <= c <= 20 and i0 >= 8 and np.count_nonzero((lam >= a) & (lam <= b)) == c
    assert min(lam[i0] - a, a - lam[i0 - 1], lam[i0 + c] - b, b - lam[i0 + c - 1]) >= 0.1 * (b - a)                # the gaps
    s0 = cheb_stats()
    r = eigsh(to_torch_csr(A), interval=(a, b), nev_max=2 * c, method="chebyshev", maxiter=40, lower_bound=bounds_of(lam)[0],
              upper_bound=bounds_of(lam)[1], backend=hip)
    s1 = cheb_stats()
    print("interval [%.6f, %.6f], %d inside from index %d, outer iterations %d, steps swept %d" % (a, b, c, i0, r.iterations, s1[1] - s0[1]))
    assert r.converged == c and s1[0] == s0[0] and s1[1] > s0[1] and s1[2] == s0[2]
    got = r.eigenvalues.cpu().numpy()
    assert np.max(np.abs(got - lam[i0:i0 + c]) / np.abs(lam[i0:i0 + c])) <= 1e-8


@pytest.mark.gpu
def test_indefinite_matrix(hip):
    from gcge_amd import eigsh
    _, S, lam, V = lap12()
    A, _ = make_problem("lap3d", 12)
    val = np.ctypeslib.as_array(A.val, (int(A.nnz),))
    assert np.count_nonzero(val == 6.0) == A.nrows
    val[val == 6.0] -= SHIFT
    S2 = csr_to_scipy(A)
    assert lam[0] - SHIFT < 0.0 < lam[-1] - SHIFT
    lmin, lmax = bounds_of(lam)
    m = hip.matrix(A)
    try:
        r = eigsh(m, interval=(LO - SHIFT, HI - SHIFT), backend=hip, **band_kw(lower_bound=lmin - SHIFT, upper_bound=lmax - SHIFT))
    finally:
        hip.free_matrix(m)
    check_pairs(r, S2, lam[BELOW:BELOW + INSIDE] - SHIFT)


@pytest.mark.gpu
def test_warm_start_needs_fewer_iterations(hip, cold):
    from gcge_amd import eigsh
    A, S, lam, V = lap12()
    r = eigsh(to_torch_csr(A), interval=(LO, HI), X0=cold.eigenvectors, backend=hip, **band_kw(lam))
    print("iterations: cold %d, warm %d" % (cold.iterations, r.iterations))
    check_pairs(r, S, lam[BELOW:BELOW + INSIDE])
    assert r.iterations < cold.iterations


@pytest.mark.gpu
def test_a_block_of_20_columns_is_too_small(hip):
    from gcge_amd import NoConvergence, eigsh
    A, S, lam, V = lap12()
    with pytest.raises(NoConvergence) as e:
        eigsh(to_torch_csr(A), interval=(LO, HI), backend=hip, **band_kw(lam, nev_max=20))
    assert "nev_max" in str(e.value) and e.value.result.converged == 20
    assert tuple(e.value.result.eigenvectors.shape) == (S.shape[0], 20)


@pytest.mark.gpu
def test_one_iteration_raises_no_convergence_with_a_result(hip):
    import torch
    from gcge_amd import NoConvergence, eigsh
    A, S, lam, V = lap12()
    with pytest.raises(NoConvergence) as e:
        eigsh(to_torch_csr(A), interval=(LO, HI), backend=hip, **band_kw(lam, maxiter=1))
    r = e.value.result
    j = r.converged
    assert 0 <= j < NEVMAX and r.iterations == 1
    assert tuple(r.eigenvalues.shape) == (j,) and tuple(r.eigenvectors.shape) == (S.shape[0], j) and tuple(r.residual_norms.shape) == (j,)
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in (r.eigenvalues, r.eigenvectors, r.residual_norms))


@pytest.mark.gpu
def test_chebyshev_band_filter_on_a_tensor(hip):
    """HipBackend.chebyshev_band_filter against V p(Lambda) V^T X with p by chebval on band_coefficients; 1e-10 |X| as
    tests/test_chfsi_band_host.py derives it"""
    import torch
    A, S, lam, V = lap12()
    n, m, degree = S.shape[0], 6, 10
    lmin, lmax = bounds_of(lam)
    X = np.random.default_rng(5).random((n, m)) - 0.5
    mu = band_coefficients(degree, LO, HI, lmin, lmax)
    p = np.polynomial.chebyshev.chebval((lam - 0.5 * (lmax + lmin)) / (0.5 * (lmax - lmin)), mu)
    ref = V @ (p[:, None] * (V.T @ X))
    mat = hip.matrix(A)
    try:
        a0 = cheb_accum_stats()
        Y = hip.chebyshev_band_filter(mat, torch.from_numpy(X).cuda(), degree, LO, HI, lmin, lmax)
        a1 = cheb_accum_stats()
        with pytest.raises(ValueError):
            hip.chebyshev_band_filter(mat, torch.from_numpy(X).cuda(), 1, LO, HI, lmin, lmax)
        with pytest.raises(ValueError):
            hip.chebyshev_band_filter(mat, torch.from_numpy(X).cuda(), degree, HI, LO, lmin, lmax)
    finally:
        hip.free_matrix(mat)
    assert (a1[0] - a0[0], a1[1] - a0[1], a1[2] - a0[2]) == (5, 1, 0)
    assert Y.is_cuda and tuple(Y.shape) == (n, m) and Y.dtype == torch.float64
    err = np.linalg.norm(Y.cpu().numpy() - ref, axis=0) / np.linalg.norm(X, axis=0)
    print("max column error / |X|:", err.max())
    assert np.all(err <= 1e-10)


@pytest.mark.gpu
def test_eigenvalue_gradient(hip):
    """loss = the sum of the eigenvalues inside: d loss / d A_ij = (V V^T)_ij on the stored entries, V numpy's 25 inside eigenvectors,
    within 1e-6 absolute.  With tol = 1e-9 the invariant subspace is off by at most |r| / gap, V V^T by twice that:
    2 * 1e-9 * max |lambda inside| / (the smallest gap between an inside and an outside eigenvalue) <= 1e-7, asserted from numpy."""
    import torch
    from gcge_amd import eigsh
    A, S, lam, V = lap12()
    inside = slice(BELOW, BELOW + INSIDE)
    gap = min(lam[BELOW] - lam[BELOW - 1], lam[BELOW + INSIDE] - lam[BELOW + INSIDE - 1])
    assert gap >= 0.039 and 2 * 1e-9 * np.abs(lam[inside]).max() / gap <= 1e-7
    rp, ci, va = csr_arrays(A)
    crow, col = torch.from_numpy(rp.astype(np.int64)).cuda(), torch.from_numpy(ci.astype(np.int64)).cuda()
    val = torch.from_numpy(va.copy()).cuda().requires_grad_()
    r = eigsh((crow, col, val), interval=(LO, HI), tol=1e-9, backend=hip, **band_kw(lam))
    assert r.eigenvalues.requires_grad and r.converged == INSIDE and not r.eigenvectors.requires_grad
    r.eigenvalues.sum().backward()
    rows = np.repeat(np.arange(A.nrows), np.diff(rp))
    want = np.einsum("ec,ec->e", V[rows, inside], V[ci, inside])
    got = val.grad.cpu().numpy()
    print("max gradient error:", np.abs(got - want).max())
    assert np.abs(got - want).max() <= 1e-6
