"""gcge_amd.solve: A X = B for a symmetric positive definite A and a few right-hand sides, from torch, with nothing of size O(n) on
the host.

Plumbing only: the matrix goes in through HipBackend.matrix_from_device, the right-hand sides through HipBackend.mv_from_torch, the
solve is GCGE_PCGSolve (csrc/host/block_fpcg.c: flexible block CG preconditioned by a BlockAMG V-cycle, or the fused block CG
alone), the solution comes out through HipBackend.mv_to_torch.  HipBackend.linear_solver keeps the solver across solves."""
import collections
import ctypes as C

from .eigsh import NoConvergence, _backends, _device_of, _differentiable, _is_handle  # noqa: F401

SolveResult = collections.namedtuple("SolveResult", ["x", "converged", "iterations", "residual_norms", "seconds"])


def solve(A, b, x0=None, tol=1e-8, maxiter=200, amg=None, amg_levels=0, backend=None):
    """X with |b_j - A x_j| <= tol |b_j| in every column, by preconditioned block CG on the GPU.

    A:     a torch sparse_csr CUDA tensor, a (crow, col, val) triple of device arrays, or a matrix handle of the back-end.  A handle
           stays the caller's; what is created here is freed here.
    b:     an (n, m) or (n,) CUDA tensor, or an object with __cuda_array_interface__;  x0: likewise, or None for a zero start.
    amg_levels:  0: the fused block CG without a preconditioner; L >= 2: one V-cycle of a BlockAMG hierarchy of at most L levels per
           iteration, built and freed inside this call, its work blocks min(m, 64) columns wide.
    amg:   a Hierarchy (HipBackend.multigrid) built on the handle A: the preconditioner, as it is.  ValueError: amg_levels given
           as well, A is not the handle the hierarchy was built on, a hierarchy of another back-end.
    backend:  a HipBackend (default: one per device, kept for the process).

    Returns SolveResult(x, converged, iterations, residual_norms, seconds) as LinearSolver.solve does (x of b's shape, converged a
    bool tensor per column, residual_norms the true relative residuals); raises NoConvergence, carrying the result, when a column
    did not converge.  A sequence of solves on one handle keeps a solver instead: HipBackend.linear_solver(A, amg=h).

    Gradients: when b requires grad, or A is given as a sparse_csr tensor or a (crow, col, val) triple whose values require grad, and
    grad mode is on, x comes back attached to the graph.  Backward solves A Z = d loss / d x with the same solver, hierarchy, tol
    and maxiter (NoConvergence when that solve does not converge) and gives Z for b and -Z_i . x_j on the stored entries for the
    values (gcge_amd.grad.solve_grads); with a handle for A the gradient with respect to b alone.  The matrix is created from the
    detached values; what this call created is then freed when backward has run or the graph is freed, not on return.  Double
    backward raises."""
    from .lib import HipBackend

    amg_levels = int(amg_levels)
    if amg_levels == 1 or amg_levels < 0:
        raise ValueError("solve: amg_levels is 0 (no hierarchy) or at least 2")
    if amg is not None:
        as_int = lambda a: (a.value if isinstance(a, C.c_void_p) else a) if _is_handle(a) else None
        if amg_levels > 0:
            raise ValueError("solve: amg (a hierarchy that exists) and amg_levels (one built inside the call) exclude each other")
        if as_int(A) is None or as_int(A) != amg.A.value:
            raise ValueError("solve: amg was not built on this matrix handle")
        if backend is not None and backend is not amg.backend:
            raise ValueError("solve: amg belongs to another back-end")
        backend = amg.backend
    if backend is None:
        dev = _device_of(A, b, x0)
        backend = _backends.get(dev)
        if backend is None:
            backend = _backends[dev] = HipBackend(device=dev)
    shape = tuple(b.shape) if hasattr(b, "shape") else tuple(getattr(b, "__cuda_array_interface__", {}).get("shape", ()))
    if len(shape) not in (1, 2):
        raise (ValueError if shape else TypeError)("solve: b is an (n, m) or (n,) device block")
    m = shape[1] if len(shape) == 2 else 1
    if m < 1:
        raise ValueError("solve: at least one right-hand side is required")

    import torch
    dA = _differentiable(A)
    attached = dA is not None or (isinstance(b, torch.Tensor) and b.requires_grad and torch.is_grad_enabled())
    if dA is not None:                                                  # the matrix is created from the detached values
        A = A.detach() if isinstance(A, torch.Tensor) else (A[0], A[1], A[2].detach()) + tuple(A[3:])
    made, built, solver = None, None, None
    try:
        if _is_handle(A):
            mA = A if isinstance(A, C.c_void_p) else C.c_void_p(A)
        else:
            mA = made = backend.matrix_from_device(*A) if isinstance(A, (tuple, list)) else backend.matrix_from_device(A)
        if amg_levels > 0:
            built = backend.multigrid(mA, levels=amg_levels, block_size=min(m, 64), refreshable=False)
        solver = backend.linear_solver(mA, amg=amg if amg is not None else built, max_cols=m)
        if not attached:
            return solver.solve(b, x0=x0, tol=tol, maxiter=maxiter)
        # x attached to the graph: what was created here now lives until backward has run or the graph is freed
        from .grad import _Owned, _solve_attached
        owned, kept = _Owned(backend, solver, built, made), solver
        made, built, solver = None, None, None
        try:
            return _solve_attached(kept, b, x0, tol, maxiter, structure_A=dA[:2] if dA is not None else None,
                                   val_A=dA[2] if dA is not None else None, owned=owned)
        except BaseException:
            owned.release()
            raise
    finally:
        if solver is not None:
            solver.close()
        if built is not None:
            built.close()
        if made is not None:
            backend.free_matrix(made)
