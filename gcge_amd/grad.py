"""gcge_amd.grad: gradients of eigenvalues, of eigenvectors and of a linear solve with respect to the matrix VALUES on the stored
entries.

All are the value of a rank-k product on the CSR pattern, which HipBackend.sample_outer computes in one kernel call
(csrc/hip/sample_outer.hip) without forming anything of size nnz x k:

    eigenvalues of A x = lambda M x, x M-orthonormal:   d lambda_c / d A_ij = x_ic x_jc,   d lambda_c / d M_ij = -lambda_c x_ic x_jc
    A X = B, loss L(X), Z = A^-1 (dL/dX):               dL/dB = Z,                         dL/dA_ij = -Z_i . X_j
    eigenvectors, loss L(lambda, X), G = dL/dX:         dL/dA = 1/2 (Z' X^T + X Z'^T),     Z' = X F - Y + X diag(dL/dlambda)
        (F the k x k part inside the computed space, Y the deflated, shifted solves outside it: eigenvector_grads)

An entry (i, j) is differentiated as a variable of its own: a symmetric matrix that stores a_ij and a_ji gets the gradient of each
(add the two for the derivative along a symmetric direction).  The eigenvector gradients are the symmetrised ones — a symmetric
matrix has eigenvectors only along symmetric directions —: again each of the two stored entries gets its own value, and their sum
is the derivative along E_ij + E_ji.

eigenvalue_grads, eigenvector_grads and solve_grads are what a loop that keeps a matrix handle calls itself:

    hip.matrix_update_values(m, vals.detach())
    r = eigsh(m, k, backend=hip)
    gA, _ = eigenvalue_grads((crow, col), r, g, backend=hip)
    vals.backward(gA)

(with a loss of the eigenvectors: gA, _ = eigenvector_grads((crow, col), r, G, g, A=m, amg=h, backend=hip).)

eigsh, LinearSolver.solve and gcge_amd.solve attach the same gradients to the graph when they are given tensors that require grad
(the autograd Functions below); eigenvectors are attached only by eigsh(..., eigenvector_grad=True), since their backward solves k
linear systems.  Not differentiable: residual norms, a second backward, and a loss that depends on the choice of basis inside a
cluster of equal eigenvalues."""
import weakref


def _structure(s):
    """(crow, col) of a sparse_csr tensor, a (crow, col) pair or a (crow, col, val, ...) tuple"""
    import torch
    if isinstance(s, torch.Tensor):
        if s.layout != torch.sparse_csr:
            raise TypeError("a sparse_csr tensor, (crow, col) or (crow, col, val) is required")
        return s.crow_indices(), s.col_indices()
    if isinstance(s, (tuple, list)) and len(s) >= 2:
        return s[0], s[1]
    raise TypeError("a sparse_csr tensor, (crow, col) or (crow, col, val) is required")


def eigenvalue_grads(structure_A, result, grad_eigenvalues, structure_M=None, backend=None):
    """(d loss / d A values, d loss / d M values or None) for loss = f(eigenvalues) with grad_eigenvalues = d loss / d eigenvalues.

    structure_A, structure_M:  the CSR pattern the gradient is wanted on — a sparse_csr tensor, (crow, col) or (crow, col, val) on the
        device; the result is in that entry order, one value per stored entry (a handle's internal order never shows).
    result:  an EigshResult, or (eigenvalues (k,), eigenvectors (n, k)); grad_eigenvalues: (k,).
    Two kernel calls: weights g_c for A and -g_c lambda_c for M.

    The eigenvectors are taken as M-orthonormal, x_c^T M x_c = 1, which the solver guarantees to the accuracy of its
    orthogonalisation.  For a cluster of equal eigenvalues the single derivatives are not defined (any rotation of the cluster's
    vectors is as good a basis); only a loss that weights the cluster's members equally — the sum over the cluster — has a
    well-defined gradient, and that one is what comes out."""
    from .eigsh import _backend_for
    lam, V = (result.eigenvalues, result.eigenvectors) if hasattr(result, "eigenvectors") else result
    lam, V, g = lam.detach(), V.detach(), grad_eigenvalues.detach().reshape(-1)
    if V.dim() != 2 or lam.numel() != V.shape[1] or g.numel() != V.shape[1]:
        raise ValueError("eigenvalue_grads: k eigenvalues, an (n, k) block of eigenvectors and k gradients are required")
    backend = _backend_for(backend, V)
    g = g.to(device=V.device, dtype=V.dtype)
    crow, col = _structure(structure_A)
    gA = backend.sample_outer(crow, col, V, V, weights=g)
    gM = None
    if structure_M is not None:
        crow, col = _structure(structure_M)
        gM = backend.sample_outer(crow, col, V, V, weights=-g * lam.reshape(-1).to(dtype=V.dtype))
    return gA, gM


def eigenvector_grads(structure_A, result, grad_eigenvectors, grad_eigenvalues=None, structure_M=None, *, A, M=None, amg=None, tol=1e-10,
                      maxiter=200, cluster_tol=1e-8, backend=None):
    """(d loss / d A values, d loss / d M values or None) for loss = f(eigenvalues, eigenvectors) of A x = lambda M x, with
    grad_eigenvectors = G = d loss / d X (n, k) and grad_eigenvalues = d loss / d lambda (k,; None: zeros).

    structure_A, structure_M, result:  as for eigenvalue_grads (structure_A None: only M's gradient is wanted).
    A, M:  the LIVE matrix handles the eigenpairs belong to (M None: the identity); amg: a Hierarchy built on A, the preconditioner
        of the solves (None: none).  tol, maxiter: of those solves (relative projected residual).

    With H = X^T G:
      inside the computed space   F_dc = H_dc / (lambda_c - lambda_d), F_cc = 0; a pair with |lambda_c - lambda_d| <= cluster_tol
          max(|lambda_c|, |lambda_d|) gets F_dc = F_cd = 0;
      outside it   (A - lambda_c M) y_c = g_c - M X (X^T g_c) with X^T M y_c = 0: one LinearSolver.solve_deflated over the k columns;
      Z = X F - Y;   grad A = 1/2 (Z' X^T + X Z'^T) with Z' = Z + X diag(grad_eigenvalues);   grad M = 1/2 (Z" X^T + X Z"^T) with
          Z" = -Z diag(lambda) - X diag(1/2 diag(H) + grad_eigenvalues lambda)
    on the stored entries: one sample_outer call of width 2 k per matrix.  These are the symmetrised gradients (see the module).
    With G = 0 (or None) no system is solved and the result is eigenvalue_grads', bit for bit.

    Conditioning.  The systems are positive definite on the complement of X as long as lambda_c < lambda_{k+1}, the first eigenvalue
    that was NOT returned, and conditioned like 1 / (lambda_{k+1} - lambda_c): choose k at a gap of the spectrum.  The error of the
    result carries the eigenpairs' residuals over the gaps between the computed eigenvalues as well (F).
    Clusters.  Inside a cluster of equal eigenvalues any rotation of the vectors is as good a basis, so a loss that depends on that
    choice has no gradient; the cluster rule drops exactly the terms such a loss would bring, and a loss that is invariant under the
    rotation (one that weights the cluster's members equally) gets its gradient, because its H is symmetric on the cluster and
    those terms cancel.  Raises NoConvergence (of solve_deflated) when a system did not converge."""
    import torch
    from .eigsh import _backend_for
    lam, X = (result.eigenvalues, result.eigenvectors) if hasattr(result, "eigenvectors") else result
    lam, X = lam.detach().reshape(-1), X.detach()
    if X.dim() != 2 or lam.numel() != X.shape[1]:
        raise ValueError("eigenvector_grads: k eigenvalues and an (n, k) block of eigenvectors are required")
    k = int(X.shape[1])
    gl = torch.zeros_like(lam) if grad_eigenvalues is None else grad_eigenvalues.detach().reshape(-1).to(device=X.device, dtype=X.dtype)
    G = None if grad_eigenvectors is None else grad_eigenvectors.detach().to(device=X.device, dtype=X.dtype)
    if gl.numel() != k or (G is not None and tuple(G.shape) != tuple(X.shape)):
        raise ValueError("eigenvector_grads: grad_eigenvectors has the shape of the eigenvectors, grad_eigenvalues k entries")
    if structure_M is not None and M is None:
        raise ValueError("eigenvector_grads: structure_M without the handle M")
    backend = _backend_for(backend, X)
    if G is None or not bool(G.any()):
        if structure_A is not None:
            return eigenvalue_grads(structure_A, (lam, X), gl, structure_M, backend=backend)
        return None, (backend.sample_outer(*_structure(structure_M), X, X, weights=-gl * lam) if structure_M is not None else None)
    lam = lam.to(dtype=X.dtype)
    H = X.T @ G
    diff = lam[None, :] - lam[:, None]                                  # [d, c] = lambda_c - lambda_d
    apart = diff.abs() > cluster_tol * torch.maximum(lam.abs()[None, :], lam.abs()[:, None])
    apart.fill_diagonal_(False)
    F = torch.where(apart, H / torch.where(apart, diff, torch.ones_like(diff)), torch.zeros_like(H))
    with backend.linear_solver(A, amg=amg, max_cols=k) as solver:
        Y = solver.solve_deflated(G, X, lam, M=M, tol=tol, maxiter=maxiter).x
    Z = X @ F - Y

    def on_pattern(structure, Zs):
        crow, col = _structure(structure)
        return backend.sample_outer(crow, col, torch.cat([Zs, X], dim=1), torch.cat([X, Zs], dim=1), alpha=0.5)

    gA = on_pattern(structure_A, Z + X * gl[None, :]) if structure_A is not None else None
    gM = on_pattern(structure_M, -Z * lam[None, :] - X * (0.5 * torch.diagonal(H) + gl * lam)[None, :]) if structure_M is not None else None
    return gA, gM


def solve_grads(structure_A, x, grad_b, backend=None):
    """d loss / d A values on the stored entries of structure_A for A x = b: -grad_b_i . x_j, where grad_b = A^-1 (d loss / d x) is the
    gradient with respect to b (what the backward solve returns).  x, grad_b: (n, m) or (n,).  One kernel call with alpha = -1."""
    from .eigsh import _backend_for
    x, z = x.detach(), grad_b.detach()
    if x.dim() == 1:
        x = x.reshape(-1, 1)
    if z.dim() == 1:
        z = z.reshape(-1, 1)
    if x.dim() != 2 or tuple(x.shape) != tuple(z.shape):
        raise ValueError("solve_grads: x and grad_b are blocks of one shape")
    backend = _backend_for(backend, x)
    crow, col = _structure(structure_A)
    return backend.sample_outer(crow, col, z, x, alpha=-1.0)


def _functions():
    import torch
    from torch.autograd.function import once_differentiable

    class EigshFunction(torch.autograd.Function):
        """eigenvalues attached to the values of A and M: forward(val_A, val_M, run, backend, structure_A, structure_M) runs the
        solve on detached values, backward is eigenvalue_grads"""

        @staticmethod
        def forward(ctx, val_A, val_M, run, backend, structure_A, structure_M):
            r = run()
            ctx.backend, ctx.structure_A, ctx.structure_M = backend, structure_A, structure_M
            ctx.save_for_backward(r.eigenvalues, r.eigenvectors)
            ctx.mark_non_differentiable(r.eigenvectors, r.residual_norms)
            return r.eigenvalues, r.eigenvectors, r.residual_norms

        @staticmethod
        @once_differentiable
        def backward(ctx, g_lam, g_vec, g_res):
            lam, V = ctx.saved_tensors
            need_A = ctx.structure_A is not None and ctx.needs_input_grad[0]
            need_M = ctx.structure_M is not None and ctx.needs_input_grad[1]
            gA = gM = None
            if need_A:
                gA, gM = eigenvalue_grads(ctx.structure_A, (lam, V), g_lam, ctx.structure_M if need_M else None, backend=ctx.backend)
            elif need_M:
                gM = ctx.backend.sample_outer(ctx.structure_M[0], ctx.structure_M[1], V, V, weights=-g_lam.reshape(-1) * lam)
            return gA, gM, None, None, None, None

    class EigshVectorFunction(torch.autograd.Function):
        """eigenvalues AND eigenvectors attached to the values of A and M (eigsh(..., eigenvector_grad=True)): forward(val_A, val_M,
        run, backend, structure_A, structure_M, kept, options); `kept` holds the handles A and M of the solve and what owns them,
        `options` amg_levels and the keywords of eigenvector_grads, which is the backward; it releases what `kept` owns"""

        @staticmethod
        def forward(ctx, val_A, val_M, run, backend, structure_A, structure_M, kept, options):
            r = run()
            ctx.backend, ctx.structure_A, ctx.structure_M, ctx.kept, ctx.options = backend, structure_A, structure_M, kept, options
            ctx.save_for_backward(r.eigenvalues, r.eigenvectors)
            ctx.mark_non_differentiable(r.residual_norms)
            return r.eigenvalues, r.eigenvectors, r.residual_norms

        @staticmethod
        @once_differentiable
        def backward(ctx, g_lam, g_vec, g_res):
            lam, V = ctx.saved_tensors
            need_A = ctx.structure_A is not None and ctx.needs_input_grad[0]
            need_M = ctx.structure_M is not None and ctx.needs_input_grad[1]
            options = dict(ctx.options)
            levels, built = options.pop("amg_levels"), None
            try:
                if levels >= 2:
                    built = ctx.backend.multigrid(ctx.kept["A"], levels=levels, block_size=min(int(V.shape[1]), 64), refreshable=False)
                gA, gM = eigenvector_grads(ctx.structure_A if need_A else None, (lam, V), g_vec, g_lam, ctx.structure_M if need_M else None,
                                           A=ctx.kept["A"], M=ctx.kept["M"], amg=built, backend=ctx.backend, **options)
            finally:
                if built is not None:
                    built.close()
                ctx.kept["owned"].release()
            return gA, gM, None, None, None, None, None, None

    class SolveFunction(torch.autograd.Function):
        """x attached to b and to the values of A: forward(b, val_A, run, solver, structure_A, tol, maxiter, owned); backward solves
        A Z = grad_x with the same solver (NoConvergence when it does not converge) and releases what `owned` holds"""

        @staticmethod
        def forward(ctx, b, val_A, run, solver, structure_A, tol, maxiter, owned):
            r = run()
            ctx.solver, ctx.structure_A, ctx.tol, ctx.maxiter, ctx.owned = solver, structure_A, tol, maxiter, owned
            ctx.save_for_backward(r.x)
            return r.x

        @staticmethod
        @once_differentiable
        def backward(ctx, g_x):
            x, = ctx.saved_tensors
            try:
                z = ctx.solver._solve(g_x, None, ctx.tol, ctx.maxiter).x
                gA = None
                if ctx.structure_A is not None and ctx.needs_input_grad[1]:
                    gA = solve_grads(ctx.structure_A, x, z, backend=ctx.solver.backend)
            finally:
                if ctx.owned is not None:
                    ctx.owned.release()
            return (z if ctx.needs_input_grad[0] else None), gA, None, None, None, None, None, None

    return EigshFunction, SolveFunction, EigshVectorFunction


_cache = []


def _function(which):
    """the EigshFunction (0), the SolveFunction (1) or the EigshVectorFunction (2); torch is imported when a gradient is first asked for, as everywhere in this package"""
    if not _cache:
        _cache.extend(_functions())
    return _cache[which]


class _Owned:
    """What gcge_amd.solve or eigsh(..., eigenvector_grad=True) created for one differentiable call — the solver, the hierarchy it
    built, the matrix (or a list of matrices) — kept until backward has run or the graph that holds it is freed, whichever comes
    first"""

    def __init__(self, backend, solver, built, made):
        self._release = weakref.finalize(self, _Owned._free, backend, solver, built, made)
        self._release.atexit = False          # (a graph that outlives the interpreter: the process frees the device)

    @staticmethod
    def _free(backend, solver, built, made):
        if solver is not None:
            solver.close()
        if built is not None:
            built.close()
        for m in made if isinstance(made, (list, tuple)) else (made,):
            if m is not None:
                backend.free_matrix(m)

    def release(self):
        self._release()


def _solve_attached(solver, b, x0, tol, maxiter, structure_A=None, val_A=None, owned=None):
    """LinearSolver.solve with x attached to the graph of b (and of val_A, the values of the pattern structure_A the solver's
    matrix was created from)"""
    import torch
    box = {}

    def run():
        box["result"] = solver._solve(b.detach() if isinstance(b, torch.Tensor) else b, x0, tol, maxiter)
        return box["result"]

    # (a foreign array takes no gradient: apply gets nothing in its place)
    x = _function(1).apply(b if isinstance(b, torch.Tensor) else None, val_A, run, solver, structure_A, tol, maxiter, owned)
    return box["result"]._replace(x=x)
