"""Gradients through EIGENVECTORS (gcge_amd.grad.eigenvector_grads and eigsh(..., eigenvector_grad=True): the k x k algebra inside
the computed space, the deflated and shifted solves of LinearSolver.solve_deflated outside it, one sampled rank-2k product per
matrix) against dense torch float64 on the CPU.

Reference.  The matrix is assembled from the values leaf by indexing and SYMMETRISED, 1/2 (A + A^T), before torch.linalg.eigh, so
that the gradient of a stored entry is the one along symmetric directions, entry (i, j) and (j, i) each with its own value: the
convention of gcge_amd/grad.py.  The generalised problem goes through the Cholesky reduction M = L L^T, C = L^-1 A L^-T, X = L^-T Y.
The loss is invariant under the sign of every vector and touches both outputs:
    loss = sum_c x_c^T diag(D_c) x_c + COEF . lambda ,      D = default_rng(11).standard_normal((n, K)),
so G = d loss / d X has the columns g_c = 2 D_c o x_c.

Bound, to first order, standard problem.  The gradient is sum_c sym(z'_c x_c^T) with z'_c = -R_c g_c + COEF_c x_c, R_c the reduced
resolvent (A - lambda_c)^+ on the complement of x_c, |R_c| = 1 / gap_c with gap_c the distance from lambda_c to the nearest OTHER
eigenvalue of the dense matrix (the (K+1)-th included: the test asserts gap_c > 1e-3 |lambda_c| on its own input).  The code
evaluates the same expression at the computed pairs: a vector with the absolute residual r_c (residual_norms) has
sin theta_c <= r_c / gap_c, so |x~_c - x_c| <= s_c := 2 r_c / gap_c.  What that moves, per column:
    g_c = 2 D_c o x_c            by 2 |D|_inf s_c                          -> 2 |D|_inf s_c / gap_c
    R_c, whose part inside the computed space is built from ALL the computed vectors (F) and whose part outside it is the
    solve deflated by all of them: relatively by 2 S, S = sum_d s_d       -> 2 |g_c| S / gap_c
    the factor x_c^T             by s_c                                    -> |g_c| s_c / gap_c
    the solve, stopped at the relative projected residual tol: an error of tol |g_c| / (lambda_{K+1} - lambda_c)   -> tol |g_c| / gap_c
(eigenvalue errors are of second order, r_c^2 / gap_c).  |z x^T| bounds every entry of z x^T and of its symmetric part.  The bound
takes twice the sum, 1e-13 |g_c| / gap_c per column for the rounding of the dense reference itself, and the eigenvalue part's bound
of tests/test_grad.py for the term COEF . lambda:
    2 sum_c [ (2 |D|_inf s_c + 2 |g_c| S + |g_c| s_c + tol |g_c|) / gap_c ] + 1e-13 sum_c |g_c| / gap_c
        + 4 sum_c |COEF_c| r_c / gap_c + 1e-13 sum_c |COEF_c|.

Generalised problem, mu the smallest eigenvalue of M, as tests/test_grad.py: in the variables y = L^T x the residual is at most
r_c / sqrt(mu), so s_c = 2 r_c / (sqrt(mu) gap_c) is the error of y_c; |x_c| <= mu^-1/2, |x~_c - x_c| <= s_c mu^-1/2, and
R_c = L^-T (C - lambda_c)^+ L^-1 has |R_c| <= 1 / (mu gap_c).  The four terms become
    2 |D|_inf s_c / (mu^2 gap_c),   2 |g_c| S / (mu^1.5 gap_c),   |g_c| s_c / (mu^1.5 gap_c),   tol |g_c| / (mu^1.5 gap_c)
with |g_c| of the reference, the rounding term 1e-13 |g_c| / (mu^1.5 gap_c).  For M the gradient is sym(z"_c x_c^T) with
z"_c = -lambda_c z_c - (1/2 H_cc + COEF_c lambda_c) x_c, H_cc = x_c^T g_c: |lambda_c| times the terms above, the eigenvalue part with
|COEF_c lambda_c|, and for the H term, with |d H_cc| <= (|g_c| s_c + 2 |D|_inf s_c mu^-1/2) mu^-1/2 and |d (x x^T)| <= 2 s_c / mu:
1/2 |d H_cc| / mu + 1/2 |H_cc| 2 s_c / mu <= 1.5 |g_c| s_c mu^-1.5 + |D|_inf s_c mu^-2, taken twice.

The test also asserts that the reference's VECTOR part — the reference minus the eigenvalue term sampled on the pattern — is more
than 1e3 times the bound in max-norm: the check resolves the new term, and the eigenvalue gradient alone cannot pass it.

Handle loop against autograd: both within their bound of the same truth, so within the sum of both bounds of each other.
Degenerate pair: two decoupled copies of the shifted 4^3 Laplacian, k = 2: the lowest eigenvalue is double, with the eigenspace
span{(u, 0), (0, u)}.  For a loss that weights the pair equally, sum over the pair of x^T diag(D) x = u^T D_1 u + u^T D_2 u, the
reference is the sum of two dense references on one copy (a simple eigenvalue there), and the bound is the one above with the gap
to the next eigenvalue of a copy."""
import numpy as np
import pytest

from gcge_amd.lib import mat_device_stats
from test_grad import COEF, EIG_TOL, K, cuda, gaps, report, shifted

ADJ_TOL = 1e-10


def dense_reference(n, rows, ci, va, D, coef, M=None):
    """dense torch float64 on the CPU: dict(lam_all, X (n, k), gA, gM or None, mu) for loss = sum_c x_c^T diag(D_c) x_c + coef . lambda
    over the k = len(coef) smallest pairs"""
    import torch
    k = len(coef)
    val = torch.from_numpy(va.copy()).requires_grad_()
    Ad = torch.zeros((n, n), dtype=torch.float64).index_put((torch.from_numpy(rows), torch.from_numpy(ci.astype(np.int64))), val)
    Ad = 0.5 * (Ad + Ad.T)
    mu, valm = 1.0, None
    if M is None:
        lam, X = torch.linalg.eigh(Ad)
    else:
        rpb, cib, vb, rowsb = M
        valm = torch.from_numpy(vb.copy()).requires_grad_()
        Md = torch.zeros((n, n), dtype=torch.float64).index_put((torch.from_numpy(rowsb), torch.from_numpy(cib.astype(np.int64))), valm)
        Md = 0.5 * (Md + Md.T)
        L = torch.linalg.cholesky(Md)
        Y = torch.linalg.solve_triangular(L, Ad, upper=False)                                # L^-1 A
        Cd = torch.linalg.solve_triangular(L, Y.T, upper=False)                              # L^-1 A L^-T
        lam, Y = torch.linalg.eigh(0.5 * (Cd + Cd.T))
        X = torch.linalg.solve_triangular(L.T, Y, upper=True)                                # L^-T Y
        mu = float(torch.linalg.eigvalsh(Md.detach())[0])
    Xk = X[:, :k]
    ((Xk * torch.from_numpy(D) * Xk).sum() + (torch.tensor(coef, dtype=torch.float64) * lam[:k]).sum()).backward()
    return dict(lam_all=lam.detach().numpy(), X=Xk.detach().numpy(), gA=val.grad.numpy(), gM=valm.grad.numpy() if valm is not None else None, mu=mu)


def loss_of(r, D, coef):
    return (r.eigenvectors * cuda(D) * r.eigenvectors).sum() + (cuda(np.array(coef)) * r.eigenvalues).sum()


def bound_of(ref, rn, gap, D, coef, for_M=False, g=None):
    """the bound of the module docstring (A, or M with for_M) for residuals rn and gaps gap; g: |g_c| (default: of the reference)"""
    mu, k = ref["mu"], len(coef)
    lam = ref["lam_all"][:k]
    d_inf = np.abs(D).max()
    g = np.linalg.norm(2.0 * D * ref["X"], axis=0) if g is None else g
    s = 2.0 * rn / (np.sqrt(mu) * gap)
    S = s.sum()
    per = (2.0 * d_inf * s / mu ** 2 + (2.0 * g * S + g * s + ADJ_TOL * g) / mu ** 1.5) / gap
    scale = np.abs(lam) if for_M else np.ones(k)
    c = np.abs(coef) * scale
    b = 2.0 * np.sum(scale * per) + 1e-13 * np.sum(scale * g / gap) / mu ** 1.5
    b += 4.0 * np.sum(c * rn / gap) / mu ** 1.5 + 1e-13 * np.sum(c) / mu
    if for_M:
        b += 2.0 * np.sum(1.5 * g * s / mu ** 1.5 + d_inf * s / mu ** 2) + 1e-13 * np.sum(g) / mu ** 1.5
    return b


def vector_part(ref, rows, ci, coef, for_M=False):
    """the reference minus the eigenvalue term X diag(coef) X^T (M: -X diag(coef lambda) X^T) sampled on the pattern"""
    X, k = ref["X"], len(coef)
    w = np.array(coef) * (-ref["lam_all"][:k] if for_M else 1.0)
    return (ref["gM"] if for_M else ref["gA"]) - np.einsum("ec,ec,c->e", X[rows], X[ci], w)


_cache = {}


def standard():
    if "std" not in _cache:
        rp, ci, va, rows, _ = shifted("lap3d", 8)
        n = rp.size - 1
        D = np.random.default_rng(11).standard_normal((n, K))
        ref = dense_reference(n, rows, ci, va, D, COEF)
        _cache["std"] = dict(n=n, rp=rp, ci=ci, va=va, rows=rows, D=D, ref=ref, gap=gaps(ref["lam_all"]), crow=cuda(rp), col=cuda(ci))
    return _cache["std"]


def autograd_standard(hip, amg_levels):
    """eigsh(..., eigenvector_grad=True) on the standard problem and its backward: once per amg_levels"""
    key = ("auto", amg_levels)
    if key not in _cache:
        from gcge_amd import eigsh
        s = standard()
        val = cuda(s["va"]).requires_grad_()
        s0 = mat_device_stats()
        r = eigsh((s["crow"], s["col"], val), K, tol=EIG_TOL, amg_levels=amg_levels, backend=hip, eigenvector_grad=dict(tol=ADJ_TOL))
        created = mat_device_stats()[0] - s0[0]
        loss = loss_of(r, s["D"], COEF)
        loss.backward()
        _cache[key] = dict(val=val, r=r, loss=loss, created=created)
    return _cache[key]


@pytest.mark.gpu
@pytest.mark.parametrize("amg_levels", [0, 2])
def test_eigenvector_gradients_standard(hip, amg_levels):
    s, a = standard(), autograd_standard(hip, amg_levels)
    r, ref = a["r"], s["ref"]
    assert s["n"] == 512 and r.eigenvalues.requires_grad and r.eigenvectors.requires_grad and not r.residual_norms.requires_grad
    assert amg_levels > 0 or a["created"] == 1                        # (with a hierarchy the W solves' levels are created too)
    rn = r.residual_norms.cpu().numpy()
    bound = bound_of(ref, rn, s["gap"], s["D"], COEF)
    vec = np.abs(vector_part(ref, s["rows"], s["ci"], COEF)).max()
    print("residuals", rn, "gaps", s["gap"], "vector part %.3e of %.3e" % (vec, np.abs(ref["gA"]).max()))
    assert vec > 1e3 * bound                                          # (the check resolves the eigenvector term)
    assert report("amg_levels=%d: d loss / d A" % amg_levels, a["val"].grad.cpu().numpy(), ref["gA"], bound) <= 1.0
    with pytest.raises(RuntimeError):                                 # a second backward through the same graph
        a["loss"].backward()


@pytest.mark.gpu
def test_eigenvector_gradients_generalised(hip):
    from gcge_amd import eigsh
    rp, ci, va, rows, M = shifted("fe3d", 6)
    rpb, cib, vb, rowsb = M
    n = rp.size - 1
    assert n == 216
    D = np.random.default_rng(11).standard_normal((n, K))
    ref = dense_reference(n, rows, ci, va, D, COEF, M)
    gap = gaps(ref["lam_all"])
    valA, valM = cuda(va).requires_grad_(), cuda(vb).requires_grad_()
    r = eigsh((cuda(rp), cuda(ci), valA), K, M=(cuda(rpb), cuda(cib), valM), tol=EIG_TOL, backend=hip, eigenvector_grad=dict(tol=ADJ_TOL))
    assert r.eigenvectors.requires_grad
    loss_of(r, D, COEF).backward()
    rn = r.residual_norms.cpu().numpy()
    bA, bM = bound_of(ref, rn, gap, D, COEF), bound_of(ref, rn, gap, D, COEF, for_M=True)
    vA, vM = np.abs(vector_part(ref, rows, ci, COEF)).max(), np.abs(vector_part(ref, rowsb, cib, COEF, for_M=True)).max()
    print("residuals", rn, "gaps", gap, "mu", ref["mu"], "vector parts %.3e (A) %.3e (M)" % (vA, vM))
    assert vA > 1e3 * bA and vM > 1e3 * bM
    eA = report("d loss / d A", valA.grad.cpu().numpy(), ref["gA"], bA)
    eM = report("d loss / d M", valM.grad.cpu().numpy(), ref["gM"], bM)
    assert eA <= 1.0 and eM <= 1.0


@pytest.mark.gpu
def test_handle_loop_agrees_with_autograd(hip):
    """eigenvector_grads with live handles and a Hierarchy against the autograd form, and against the dense reference"""
    from gcge_amd import eigenvector_grads, eigsh
    s, a = standard(), autograd_standard(hip, 0)
    m = hip.matrix_from_device(s["crow"], s["col"], cuda(s["va"]))
    h = hip.multigrid(m, levels=2, block_size=K)
    try:
        r = eigsh(m, K, tol=EIG_TOL, amg=h, backend=hip)
        assert not r.eigenvalues.requires_grad and not r.eigenvectors.requires_grad
        s0 = mat_device_stats()
        gA, gM = eigenvector_grads((s["crow"], s["col"]), r, 2.0 * cuda(s["D"]) * r.eigenvectors, cuda(np.array(COEF)), A=m, amg=h,
                                   tol=ADJ_TOL, backend=hip)
        assert gM is None and mat_device_stats()[0] == s0[0]
    finally:
        h.close()
        hip.free_matrix(m)
    b_handle = bound_of(s["ref"], r.residual_norms.cpu().numpy(), s["gap"], s["D"], COEF)
    b_auto = bound_of(s["ref"], a["r"].residual_norms.cpu().numpy(), s["gap"], s["D"], COEF)
    assert report("handle loop against the dense reference", gA.cpu().numpy(), s["ref"]["gA"], b_handle) <= 1.0
    assert report("handle loop against autograd", gA.cpu().numpy(), a["val"].grad.cpu().numpy(), b_handle + b_auto) <= 1.0


@pytest.mark.gpu
def test_without_eigenvector_grad_nothing_changes(hip):
    """eigenvector_grad=False: eigenvectors are not attached and the eigenvalue gradient is eigenvalue_grads', bit for bit; and
    eigenvector_grads with G = 0 (or None) is eigenvalue_grads bit for bit"""
    import torch
    from gcge_amd import eigenvalue_grads, eigenvector_grads, eigsh
    s = standard()
    val, coef = cuda(s["va"]).requires_grad_(), cuda(np.array(COEF))
    s0 = mat_device_stats()
    r = eigsh((s["crow"], s["col"], val), K, tol=EIG_TOL, backend=hip)
    assert mat_device_stats()[0] - s0[0] == 1
    assert r.eigenvalues.requires_grad and not r.eigenvectors.requires_grad and not r.residual_norms.requires_grad
    (coef * r.eigenvalues).sum().backward()
    assert mat_device_stats()[0] - s0[0] == 1
    direct, _ = eigenvalue_grads((s["crow"], s["col"]), r, coef, backend=hip)
    assert torch.equal(val.grad, direct)
    m = hip.matrix_from_device(s["crow"], s["col"], val.detach())
    try:
        for G in (torch.zeros_like(r.eigenvectors), None):
            gA, gM = eigenvector_grads((s["crow"], s["col"]), r, G, coef, A=m, backend=hip)
            assert gM is None and torch.equal(gA, direct)
    finally:
        hip.free_matrix(m)


@pytest.mark.gpu
def test_a_degenerate_pair_with_equal_weights(hip):
    import torch
    from gcge_amd import eigsh
    rp, ci, va, rows, _ = shifted("lap3d", 4)
    n1, nnz = rp.size - 1, ci.size
    assert n1 == 64
    rp2, ci2, va2 = np.concatenate([rp, rp[1:] + nnz]), np.concatenate([ci, ci + n1]), np.concatenate([va, va])
    D = np.random.default_rng(11).standard_normal((2 * n1, 1))
    # the reference: one copy, its lowest pair (simple there), once per half of D
    refs = [dense_reference(n1, rows, ci, va, D[h * n1:(h + 1) * n1], [0.0]) for h in (0, 1)]
    g_ref = np.concatenate([refs[0]["gA"], refs[1]["gA"]])
    lam1 = refs[0]["lam_all"]
    gap = np.full(2, lam1[1] - lam1[0])
    assert gap[0] > 1e-3 * abs(lam1[0])
    val = cuda(va2).requires_grad_()
    r = eigsh((cuda(rp2), cuda(ci2), val), 2, tol=EIG_TOL, backend=hip, eigenvector_grad=dict(tol=ADJ_TOL))
    lam = r.eigenvalues.detach().cpu().numpy()
    assert abs(lam[1] - lam[0]) <= 1e-8 * abs(lam[0]) and abs(lam[0] - lam1[0]) <= 1e-8 * abs(lam1[0])      # a cluster by the rule
    (r.eigenvectors * cuda(D) * r.eigenvectors).sum().backward()
    got = val.grad.cpu().numpy()
    assert np.all(np.isfinite(got))
    # the bound's quantities for the pair: |g_c| <= 2 |D|_inf for ANY unit vector of the eigenspace, both with the copy's gap
    pair = dict(mu=1.0, lam_all=np.array([lam1[0], lam1[0]]))
    bound = bound_of(pair, r.residual_norms.cpu().numpy(), gap, D, [0.0, 0.0], g=np.full(2, 2.0 * np.abs(D).max()))
    assert np.abs(g_ref).max() > 1e3 * bound
    assert report("degenerate pair: d loss / d A", got, g_ref, bound) <= 1.0


@pytest.mark.gpu
def test_solve_deflated_against_the_dense_projected_solve_by_hooks_and_by_slots(hip, monkeypatch):
    """LinearSolver.solve_deflated on the HIP table with X, lambda of the dense reference: the solution within kappa_proj (tol + n eps)
    |y| of the dense one, kappa_proj = (lambda_max - lambda_c) / (lambda_{K+1} - lambda_c) (a residual of tol |Q^T b| on the complement,
    where the operator's eigenvalues are lambda_i - lambda_c, i > K; n eps for the reference), the reported residual the true
    projected one, y orthogonal to X; and the same through the slots (GCGE_NO_PCG_SWEEPS: no pcg_shift), so within twice that of
    each other"""
    s = standard()
    n, X, lam_all = s["n"], s["ref"]["X"], s["ref"]["lam_all"]
    lam = lam_all[:K]
    A = np.zeros((n, n))
    A[s["rows"], s["ci"]] = s["va"]
    b = np.random.default_rng(13).standard_normal((n, K))
    Q = np.eye(n) - X @ X.T
    yd = np.column_stack([Q @ np.linalg.lstsq(Q @ (A - lam[c] * np.eye(n)) @ Q, Q @ b[:, c], rcond=1e-12)[0] for c in range(K)])
    bound = (lam_all[-1] - lam) / (lam_all[K] - lam) * (ADJ_TOL + n * np.finfo(np.float64).eps) * np.linalg.norm(yd, axis=0)
    m = hip.matrix_from_device(s["crow"], s["col"], cuda(s["va"]))
    h = hip.multigrid(m, levels=2, block_size=4)                     # (6 columns over a block of 4: two chunks)
    try:
        with hip.linear_solver(m, amg=h, max_cols=K) as solver:
            out = []
            for slots in (False, True):
                if slots:
                    monkeypatch.setenv("GCGE_NO_PCG_SWEEPS", "1")
                r = solver.solve_deflated(cuda(b), cuda(X), lam, tol=ADJ_TOL)
                monkeypatch.delenv("GCGE_NO_PCG_SWEEPS", raising=False)
                y, rel = r.x.cpu().numpy(), r.residual_norms.cpu().numpy()
                true = np.linalg.norm(Q @ (b - (A @ y - y * lam)), axis=0) / np.linalg.norm(Q @ b, axis=0)
                err = np.linalg.norm(y - yd, axis=0)
                print("slots" if slots else "hooks", "error / bound", err / bound, "rel_res", rel, "recomputed", true, "iterations", solver.column_iterations)
                assert bool(r.converged.all()) and np.all(rel <= ADJ_TOL) and np.all(np.abs(true - rel) <= 1e-3 * rel + 1e-14)
                assert np.all(err <= bound)
                assert np.all(np.linalg.norm(X.T @ y, axis=0) <= 1e-10 * np.linalg.norm(y, axis=0))
                out.append(y)
            assert np.all(np.linalg.norm(out[0] - out[1], axis=0) <= 2.0 * bound)
    finally:
        h.close()
        hip.free_matrix(m)


@pytest.mark.gpu
def test_value_errors_and_no_convergence_from_backward(hip):
    from gcge_amd import NoConvergence, eigsh
    s = standard()
    m = hip.matrix_from_device(s["crow"], s["col"], cuda(s["va"]))
    try:
        with pytest.raises(ValueError, match="eigenvector_grads"):     # a handle
            eigsh(m, K, tol=EIG_TOL, backend=hip, eigenvector_grad=True)
    finally:
        hip.free_matrix(m)
    with pytest.raises(ValueError, match="eigenvector_grads"):         # no tensor that requires grad
        eigsh((s["crow"], s["col"], cuda(s["va"])), K, tol=EIG_TOL, backend=hip, eigenvector_grad=True)
    val = cuda(s["va"]).requires_grad_()
    s0 = mat_device_stats()
    r = eigsh((s["crow"], s["col"], val), K, tol=EIG_TOL, backend=hip, eigenvector_grad=dict(tol=ADJ_TOL, maxiter=1))
    with pytest.raises(NoConvergence) as e:
        loss_of(r, s["D"], COEF).backward()
    assert e.value.result.x.shape == (s["n"], K) and not bool(e.value.result.converged.all())
    assert val.grad is None and mat_device_stats()[0] - s0[0] == 1
