"""Gradients through gcge_amd.eigsh and gcge_amd.solve (gcge_amd/grad.py over HipBackend.sample_outer) against dense torch float64 on
the CPU, where the matrix is assembled from the same values leaf by indexing.

Bounds.

Eigenvalues, standard problem.  d lambda_c / d A_ij = x_ic x_jc for the unit eigenvector x_c.  The returned vector has the absolute
residual r_c = |A x_c - lambda_c x_c| (residual_norms), so its angle to the true eigenvector satisfies sin theta <= r_c / gap_c with
gap_c the distance from lambda_c to the nearest OTHER eigenvalue (of the dense matrix); the error of x x^T is <= 2 sin theta in norm,
hence in every entry; the bound takes twice that, and 1e-13 per unit of |c_c| for the rounding of the dense reference itself:
    |grad - reference| <= 4 sum_c |c_c| r_c / gap_c + 1e-13 sum_c |c_c|        for loss = sum_c c_c lambda_c.
The test asserts min gap_c > 1e-3 |lambda_c| as a condition on its own input (a cluster has no single derivatives).

Generalised problem A x = lambda M x.  The same form in the variables in which the problem is a standard one: with M = L L^T and
y = L^T x the unit eigenvector of L^-1 A L^-T, its residual is L^-1 (A x - lambda M x), at most r_c / sqrt(mu) for mu the smallest
eigenvalue of M, so sin theta <= r_c / (sqrt(mu) gap_c); x x^T = L^-T (y y^T) L^-1 multiplies the error of y y^T by at most
|L^-1|^2 = 1 / mu.  The returned x is M-orthonormal only to the solver's orthogonalisation accuracy; that error is of the order of
the rounding unit and is carried by the second term, scaled like x x^T itself (|x|^2 <= 1 / mu):
    A:  |grad - reference| <= 4 sum_c |c_c| r_c / (gap_c mu^1.5) + 1e-13 sum_c |c_c| / mu
    M:  d lambda_c / d M_ij = -lambda_c x_ic x_jc: the same with |c_c lambda_c| in place of |c_c|.
For the standard problem mu = 1 and this is the bound above.  (With mu left out the form cannot hold for this pair, mu = 6.4e-4:
two dense float64 evaluations of the A gradient already differ by 1.5e-11, above that form's second term of 1.3e-12, and the
solver's result, 5.8e-7 from the reference at residuals of 2e-8 to 3e-8, is 10 times that form and 1.7e-4 of the bound used;
the test prints both.)

Handle loop: eigenvalue_grads on a handle that took the values in place against the autograd result on the same values: both lie
within the bound of the same truth, each with its own residuals, so they differ by at most the bound formed with r_c(handle) +
r_c(autograd).

Solve.  A X = B to the relative residual tol per column: the error of a column is at most kappa tol times its norm (kappa the dense
condition number, computed in the test), for the solution X and the adjoint Z = A^-1 (dL/dX) alike; the dense reference's own error,
kappa n eps, is added.  grad_b = Z: every entry of column c within kappa (tol + n eps) |Z_c|.  grad_A_ij = -Z_i . X_j: allowed
4 kappa (tol + n eps) |Z_i| |X_j|, the row norms of the reference (first order: |dZ_i| |X_j| + |Z_i| |dX_j|, twice that)."""
import numpy as np
import pytest

from gcge_amd.lib import csr_arrays, make_problem, mat_device_stats

K = 6
COEF = [3.0, -2.0, 1.0, 2.0, -1.0, 4.0]
EIG_TOL = 1e-10
SOLVE_TOL = 1e-12
EPS = 2.0 ** -53


def shifted(kind, size):
    """(crow, col, val of A with 6 U(0,1) from default_rng(7) added to the diagonal, rows, val of M or None) as numpy arrays"""
    A, B = make_problem(kind, size)
    rp, ci, va = (np.array(a) for a in csr_arrays(A))
    rows = np.repeat(np.arange(A.nrows), np.diff(rp))
    d = 6.0 * np.random.default_rng(7).random(A.nrows)
    va[rows == ci] += d
    assert np.count_nonzero(rows == ci) == A.nrows
    if B is None:
        return rp, ci, va, rows, None
    rpb, cib, vb = (np.array(a) for a in csr_arrays(B))
    return rp, ci, va, rows, (rpb, cib, vb, np.repeat(np.arange(B.nrows), np.diff(rpb)))


def dense_reference(n, rows, ci, va, M=None):
    """dense torch float64 on the CPU: (all eigenvalues, d loss / d val_A, d loss / d val_M or None, mu) for loss = COEF . the K smallest"""
    import torch
    val = torch.from_numpy(va.copy()).requires_grad_()
    Ad = torch.zeros((n, n), dtype=torch.float64).index_put((torch.from_numpy(rows), torch.from_numpy(ci.astype(np.int64))), val)
    mu, valm = 1.0, None
    if M is None:
        lam = torch.linalg.eigvalsh(Ad)
    else:
        rpb, cib, vb, rowsb = M
        valm = torch.from_numpy(vb.copy()).requires_grad_()
        Md = torch.zeros((n, n), dtype=torch.float64).index_put((torch.from_numpy(rowsb), torch.from_numpy(cib.astype(np.int64))), valm)
        L = torch.linalg.cholesky(Md)
        Y = torch.linalg.solve_triangular(L, Ad, upper=False)                                # L^-1 A
        lam = torch.linalg.eigvalsh(torch.linalg.solve_triangular(L, Y.T, upper=False))      # L^-1 (L^-1 A)^T = L^-1 A L^-T
        mu = float(torch.linalg.eigvalsh(Md.detach())[0])
    (torch.tensor(COEF, dtype=torch.float64) * lam[:K]).sum().backward()
    return lam.detach().numpy(), val.grad.numpy(), (valm.grad.numpy() if valm is not None else None), mu


def gaps(lam_all):
    lam = lam_all[:K]
    other = np.abs(lam[:, None] - lam_all[None, :])
    other[np.arange(K), np.arange(K)] = np.inf
    g = other.min(axis=1)
    assert np.all(g > 1e-3 * np.abs(lam)), (g, lam)
    return g


def eig_bound(rn, gap, mu=1.0, scale=None):
    c = np.abs(COEF) * (np.ones(K) if scale is None else np.abs(scale))
    return 4.0 * np.sum(c * rn / gap) / mu ** 1.5 + 1e-13 * np.sum(c) / mu


def cuda(a, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def report(what, got, ref, bound):
    err = np.max(np.abs(got - ref) / bound)
    print("%s: largest error %.3e, %.3g of its bound (bound %s)" % (what, np.max(np.abs(got - ref)), err,
                                                                   "%.3e" % bound if np.ndim(bound) == 0 else "per entry"))
    return err


_cache = {}


def standard(hip):
    """the standard problem, its dense reference and the autograd result through the triple: once per module"""
    if "std" not in _cache:
        import torch
        from gcge_amd import eigsh
        rp, ci, va, rows, _ = shifted("lap3d", 8)
        n = rp.size - 1
        lam_all, g_ref, _, _ = dense_reference(n, rows, ci, va)
        crow, col, val = cuda(rp), cuda(ci), cuda(va).requires_grad_()
        s0 = mat_device_stats()
        r = eigsh((crow, col, val), K, tol=EIG_TOL, backend=hip)
        s1 = mat_device_stats()
        (cuda(np.array(COEF)) * r.eigenvalues).sum().backward()
        _cache["std"] = dict(n=n, rp=rp, ci=ci, va=va, rows=rows, lam_all=lam_all, g_ref=g_ref, crow=crow, col=col, val=val, r=r,
                             created=s1[0] - s0[0], created_by_backward=mat_device_stats()[0] - s1[0])
    return _cache["std"]


@pytest.mark.gpu
def test_eigenvalue_gradients_standard(hip):
    s = standard(hip)
    r = s["r"]
    assert s["n"] == 512 and r.eigenvalues.requires_grad and not r.eigenvectors.requires_grad and not r.residual_norms.requires_grad
    assert s["created"] == 1 and s["created_by_backward"] == 0
    lam, rn = r.eigenvalues.detach().cpu().numpy(), r.residual_norms.cpu().numpy()
    gap = gaps(s["lam_all"])
    assert np.all(np.abs(lam - s["lam_all"][:K]) <= 1e-8 * np.abs(lam))
    bound = eig_bound(rn, gap)
    print("residuals", rn, "gaps", gap)
    assert report("d loss / d A", s["val"].grad.cpu().numpy(), s["g_ref"], bound) <= 1.0
    assert np.abs(s["g_ref"]).max() > 1e4 * bound                  # (the check resolves the gradient)


@pytest.mark.gpu
def test_eigenvalue_gradients_generalised(hip):
    import torch
    from gcge_amd import eigsh
    rp, ci, va, rows, M = shifted("fe3d", 6)
    rpb, cib, vb, rowsb = M
    n = rp.size - 1
    assert n == 216
    lam_all, gA_ref, gM_ref, mu = dense_reference(n, rows, ci, va, M)
    gap = gaps(lam_all)
    valA, valM = cuda(va).requires_grad_(), cuda(vb).requires_grad_()
    r = eigsh((cuda(rp), cuda(ci), valA), K, M=(cuda(rpb), cuda(cib), valM), tol=EIG_TOL, backend=hip)
    (cuda(np.array(COEF)) * r.eigenvalues).sum().backward()
    lam, rn = r.eigenvalues.detach().cpu().numpy(), r.residual_norms.cpu().numpy()
    print("residuals", rn, "gaps", gap, "mu", mu)
    assert np.all(np.abs(lam - lam_all[:K]) <= 1e-8 * np.abs(lam))
    eA = report("d loss / d A", valA.grad.cpu().numpy(), gA_ref, eig_bound(rn, gap, mu))
    eM = report("d loss / d M", valM.grad.cpu().numpy(), gM_ref, eig_bound(rn, gap, mu, scale=lam_all[:K]))
    report("d loss / d A against the bound without mu", valA.grad.cpu().numpy(), gA_ref, eig_bound(rn, gap))
    assert eA <= 1.0 and eM <= 1.0
    # only M's values require grad: A takes none, M's is the same
    valM2 = cuda(vb).requires_grad_()
    r2 = eigsh((cuda(rp), cuda(ci), cuda(va)), K, M=(cuda(rpb), cuda(cib), valM2), tol=EIG_TOL, backend=hip)
    (cuda(np.array(COEF)) * r2.eigenvalues).sum().backward()
    assert torch.equal(valM2.grad, valM.grad)


@pytest.mark.gpu
def test_sparse_csr_tensor_gives_the_same_bits(hip):
    import torch
    from gcge_amd import eigsh
    s = standard(hip)
    val = cuda(s["va"]).requires_grad_()
    S = torch.sparse_csr_tensor(s["crow"].to(torch.int64), s["col"].to(torch.int64), val, size=(s["n"], s["n"]))
    r = eigsh(S, K, tol=EIG_TOL, backend=hip)
    assert r.eigenvalues.requires_grad
    (cuda(np.array(COEF)) * r.eigenvalues).sum().backward()
    assert torch.equal(val.grad, s["val"].grad)


@pytest.mark.gpu
def test_handle_loop(hip):
    """a handle created with other values takes the standard problem's in place; eigenvalue_grads on its result"""
    from gcge_amd import eigsh, eigenvalue_grads
    s = standard(hip)
    other = s["va"].copy()
    other[s["rows"] == s["ci"]] += 0.5
    m = hip.matrix_from_device(s["crow"], s["col"], cuda(other), updatable=True)
    try:
        assert hip.matrix_update_values(m, s["val"].detach())
        s0 = mat_device_stats()
        r = eigsh(m, K, tol=EIG_TOL, backend=hip)
        assert not r.eigenvalues.requires_grad
        gA, gM = eigenvalue_grads((s["crow"], s["col"]), r, cuda(np.array(COEF)), backend=hip)
        assert gM is None and mat_device_stats()[0] == s0[0]
    finally:
        hip.free_matrix(m)
    gap = gaps(s["lam_all"])
    rn = r.residual_norms.cpu().numpy()
    assert report("handle loop against the dense reference", gA.cpu().numpy(), s["g_ref"], eig_bound(rn, gap)) <= 1.0
    both = eig_bound(rn + s["r"].residual_norms.cpu().numpy(), gap)
    assert report("handle loop against autograd", gA.cpu().numpy(), s["val"].grad.cpu().numpy(), both) <= 1.0


def solve_reference(s, b, W):
    if "solve_ref" not in _cache:
        import torch
        n = s["n"]
        val, bt = torch.from_numpy(s["va"].copy()).requires_grad_(), torch.from_numpy(b.copy()).requires_grad_()
        Ad = torch.zeros((n, n), dtype=torch.float64).index_put((torch.from_numpy(s["rows"]), torch.from_numpy(s["ci"].astype(np.int64))), val)
        x = torch.linalg.solve(Ad, bt)
        (torch.from_numpy(W) * x).sum().backward()
        _cache["solve_ref"] = (x.detach().numpy(), bt.grad.numpy(), val.grad.numpy(), float(torch.linalg.cond(Ad.detach())))
    return _cache["solve_ref"]


def solve_data(s):
    rng = np.random.default_rng(11)
    return rng.standard_normal((s["n"], 3)), rng.standard_normal((s["n"], 3))


@pytest.mark.gpu
@pytest.mark.parametrize("amg_levels", [0, 2])
def test_solve_gradients(hip, amg_levels):
    from gcge_amd import solve
    s = standard(hip)
    b, W = solve_data(s)
    x_ref, gb_ref, gA_ref, kappa = solve_reference(s, b, W)
    rel = kappa * (SOLVE_TOL + s["n"] * EPS)
    val, bt = cuda(s["va"]).requires_grad_(), cuda(b).requires_grad_()
    s0 = mat_device_stats()
    r = solve((s["crow"], s["col"], val), bt, tol=SOLVE_TOL, amg_levels=amg_levels, backend=hip)
    s1 = mat_device_stats()
    assert r.x.requires_grad and bool(r.converged.all()) and not r.residual_norms.requires_grad
    loss = (cuda(W) * r.x).sum()
    loss.backward()
    assert mat_device_stats() == s1                                  # backward creates no matrix (nor a hierarchy's levels)
    print("kappa %.3f, matrices created by the call %d" % (kappa, s1[0] - s0[0]))
    assert np.all(np.abs(r.x.detach().cpu().numpy() - x_ref) <= rel * np.linalg.norm(x_ref, axis=0))
    assert report("d loss / d b", bt.grad.cpu().numpy(), gb_ref, rel * np.linalg.norm(gb_ref, axis=0)[None, :]) <= 1.0
    bound = 4.0 * rel * np.linalg.norm(gb_ref, axis=1)[s["rows"]] * np.linalg.norm(x_ref, axis=1)[s["ci"]]
    assert report("d loss / d A", val.grad.cpu().numpy(), gA_ref, bound) <= 1.0
    with pytest.raises(RuntimeError):                                # a second backward through the same graph
        loss.backward()
    # the same call without a tensor that requires grad creates as many matrices
    s2 = mat_device_stats()
    r0 = solve((s["crow"], s["col"], val.detach()), bt.detach(), tol=SOLVE_TOL, amg_levels=amg_levels, backend=hip)
    assert mat_device_stats()[0] - s2[0] == s1[0] - s0[0] and not r0.x.requires_grad


@pytest.mark.gpu
def test_solve_on_a_handle_gives_grad_b(hip):
    """gcge_amd.solve and LinearSolver.solve on a handle: the gradient with respect to b alone; a second backward raises; a graph that
    is dropped without a backward frees what the call created"""
    from gcge_amd import solve
    s = standard(hip)
    b, W = solve_data(s)
    x_ref, gb_ref, _, kappa = solve_reference(s, b, W)
    bound = kappa * (SOLVE_TOL + s["n"] * EPS) * np.linalg.norm(gb_ref, axis=0)[None, :]
    m = hip.matrix_from_device(s["crow"], s["col"], s["val"].detach())
    try:
        bt = cuda(b).requires_grad_()
        r = solve(m, bt, tol=SOLVE_TOL, backend=hip)
        assert r.x.requires_grad
        loss = (cuda(W) * r.x).sum()
        loss.backward()
        assert report("solve(handle): d loss / d b", bt.grad.cpu().numpy(), gb_ref, bound) <= 1.0
        with pytest.raises(RuntimeError):
            loss.backward()
        dropped = solve(m, cuda(b).requires_grad_(), tol=SOLVE_TOL, backend=hip)
        del dropped                                                   # (no backward: the graph goes, and the solver with it)
        with hip.linear_solver(m, max_cols=3) as solver:
            b2 = cuda(b).requires_grad_()
            r2 = solver.solve(b2, tol=SOLVE_TOL)
            (cuda(W) * r2.x).sum().backward()
            assert report("LinearSolver.solve: d loss / d b", b2.grad.cpu().numpy(), gb_ref, bound) <= 1.0
            b1 = cuda(b[:, 0]).requires_grad_()                       # an (n,) right-hand side
            r1 = solver.solve(b1, tol=SOLVE_TOL)
            assert r1.x.shape == (s["n"],)
            (cuda(W[:, 0]) * r1.x).sum().backward()
            assert np.all(np.abs(b1.grad.cpu().numpy() - gb_ref[:, 0]) <= bound[0, 0])
    finally:
        hip.free_matrix(m)


@pytest.mark.gpu
def test_nothing_changes_without_a_tensor_that_requires_grad(hip):
    import torch
    from gcge_amd import eigsh, solve
    s = standard(hip)
    b, _ = solve_data(s)
    val = cuda(s["va"])
    s0 = mat_device_stats()
    r = eigsh((s["crow"], s["col"], val), K, tol=EIG_TOL, backend=hip)
    assert mat_device_stats()[0] - s0[0] == s["created"] == 1
    assert not r.eigenvalues.requires_grad and r.eigenvalues.grad_fn is None
    assert torch.equal(r.eigenvalues, s["r"].eigenvalues.detach()) and torch.equal(r.eigenvectors, s["r"].eigenvectors)
    x = solve((s["crow"], s["col"], val), cuda(b), tol=SOLVE_TOL, backend=hip).x
    assert not x.requires_grad
    with torch.no_grad():
        leaf, bl = cuda(s["va"]).requires_grad_(), cuda(b).requires_grad_()
        s1 = mat_device_stats()
        r = eigsh((s["crow"], s["col"], leaf), K, tol=EIG_TOL, backend=hip)
        assert mat_device_stats()[0] - s1[0] == 1
        assert not r.eigenvalues.requires_grad and torch.equal(r.eigenvalues, s["r"].eigenvalues.detach())
        x2 = solve((s["crow"], s["col"], leaf), bl, tol=SOLVE_TOL, backend=hip).x
        assert not x2.requires_grad and torch.equal(x2, x)
