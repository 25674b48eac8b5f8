"""gcge_amd.eigsh: the smallest eigenpairs of A x = lambda M x from torch, with nothing of size O(n) on the host.

Plumbing only: the matrices go in through HipBackend.matrix_from_device, start vectors through HipBackend.mv_from_torch, the solve is
the harness (GCGE_RunGCG, or GCGE_RunGCGGiven with start vectors), the eigenvectors come out through HipBackend.mv_to_torch and the
residual norms through GCGE_ResidualNorms (the back-end's residual_sq, the routine the solver's convergence check uses)."""
import collections
import ctypes as C

EigshResult = collections.namedtuple("EigshResult", ["eigenvalues", "eigenvectors", "converged", "iterations", "seconds", "residual_norms"])


class NoConvergence(RuntimeError):
    """Fewer than k pairs converged; .result is the EigshResult of what the solve reached (all k columns, .converged of them done)."""

    def __init__(self, message, result):
        super().__init__(message)
        self.result = result


_backends = {}


def _is_handle(a):
    return isinstance(a, (C.c_void_p, int))


def _device_of(*things):
    import torch
    for a in things:
        for t in (a if isinstance(a, (tuple, list)) else (a,)):
            if isinstance(t, torch.Tensor) and t.is_cuda:
                return t.device.index
    return torch.cuda.current_device()


def _check_method(k, M, nev_max, block_size, amg_levels, amg, method, degree, lower_bound, interval, eigenvector_grad=False):
    """the ValueErrors of eigsh that depend on method, degree, interval and k alone: raised before anything touches the device"""
    import math
    if method not in ("gcg", "chebyshev"):
        raise ValueError("eigsh: method is \"gcg\" or \"chebyshev\"")
    chebyshev = method == "chebyshev"
    if interval is not None and not chebyshev:
        raise ValueError("eigsh: interval requires method=\"chebyshev\" (the band-pass filter is the only solver for interior pairs)")
    if chebyshev and (M is not None or amg is not None or amg_levels or block_size is not None):
        raise ValueError("eigsh: method=\"chebyshev\" is for the standard problem and solves no linear system: M, amg, amg_levels and "
                         "block_size do not go with it")
    if interval is None:
        if k is None:
            raise ValueError("eigsh: k is required (k=None goes with interval=(a, b) only)")
        if lower_bound is not None:
            raise ValueError("eigsh: lower_bound goes with interval only (the low-pass filter takes its lower end from the Ritz values)")
        if chebyshev and degree is not None and int(degree) < 1:
            raise ValueError("eigsh: degree >= 1 is required")
        return
    if k is not None:
        raise ValueError("eigsh: interval requires k=None (every pair inside the interval is returned; nev_max is the block's width)")
    if nev_max is None:
        raise ValueError("eigsh: interval requires nev_max, the width of the filtered block (more than the eigenvalues inside)")
    if int(nev_max) < 1:
        raise ValueError("eigsh: nev_max >= 1 is required")
    try:
        a, b = (float(v) for v in interval)
    except (TypeError, ValueError):
        raise ValueError("eigsh: interval is a pair (a, b) of numbers") from None
    if not (math.isfinite(a) and math.isfinite(b) and a < b):
        raise ValueError("eigsh: interval=(a, b) requires a < b, both finite")
    if degree is not None and int(degree) < 2:
        raise ValueError("eigsh: interval requires degree >= 2 (or None: the driver's choice)")
    if eigenvector_grad:
        raise ValueError("eigsh: eigenvector_grad does not go with interval: the pairs below the interval are not in the computed space, "
                         "so the deflated systems (A - lambda_c) y = g would be indefinite")


def eigsh(A, k=None, M=None, X0=None, tol=1e-8, maxiter=None, nev_max=None, block_size=None, amg_levels=0, backend=None, gcge_args=(), amg=None,
          eigenvector_grad=False, method="gcg", degree=None, upper_bound=None, lower_bound=None, interval=None):
    """The k smallest eigenvalues and their eigenvectors of the symmetric problem A x = lambda M x (M=None: the identity; M positive
    definite) by GCG on the GPU.  The smallest eigenvalues are the only mode.

    A, M:  a torch sparse_csr CUDA tensor, a (crow, col, val) triple of device arrays, or a matrix handle of the back-end.  Handles
           stay the caller's; what is created here is freed here.  A sequence of nearby operators on one sparsity structure keeps
           ONE handle and gives it new values between the solves (HipBackend.matrix_update_values), so no step re-creates the matrix:
               m = hip.matrix_from_device(A0, updatable=True); h = hip.multigrid(m, levels=6, block_size=b)
               r = eigsh(m, k, amg=h, backend=hip)
               for V in potentials:
                   hip.matrix_update_values(m, values_of(V)) or recreate(...)    # declined: nothing was written; free m and h, create both again
                   h.refresh()                                                   # the coarse levels follow, in place (False: built again)
                   r = eigsh(m, k, X0=r.eigenvectors, amg=h, backend=hip)
           (updatable=True matters for real-space Hamiltonians — a Laplacian star, a local potential on the diagonal, atom blocks:
           their handles keep the provenance of their stored values only on request; the star's coefficients must not change —
           and for matrices in a numbering that shows no grid, which the back-end re-orders inside the handle: such a handle is
           declined only when it was created without updatable=True; the values stay in the caller's entry order.
           Without a hierarchy the loop is the same minus the lines that name h.)
    X0:    (n, j) device tensor of start vectors, j <= nev_max (a warm start: the previous eigenvectors of a nearby operator).
    tol:   relative residual tolerance, ||A x - lambda M x|| <= tol |lambda|;  maxiter: outer iterations at most (default 500).
    nev_max (default 2 k), block_size:  columns of the eigenvector block and of the W block, as for the harness.
    amg_levels:  0: the W systems by the fused block CG; L >= 2: by BlockAMG over a hierarchy of at most L levels, built and freed
           inside this call.
    amg:   a Hierarchy (HipBackend.multigrid) built on the handles A (and M): the W systems by BlockAMG over it, as it is — nothing is
           built here; Hierarchy.refresh() keeps it in step with new values.  block_size=None then means the hierarchy's block size.
           ValueError: amg_levels given as well, A (or M) is not the handle the hierarchy was built on, a larger block_size than the
           hierarchy's, a hierarchy of another back-end.
    backend:  a HipBackend (default: one per device, kept for the process).
    gcge_args:  harness options ("-gcge_compW_cg_max_iter", 40, ...), appended as they are; they win over the arguments above.
    method:  "gcg" (the default), or "chebyshev": Chebyshev-filtered subspace iteration (GCGE_RunChFSI) in place of the harness, for
           the standard problem only.  It solves no linear system, so it needs no hierarchy, no preconditioner and no definite A: per
           outer iteration the unconverged columns are filtered by a polynomial of A of the given `degree` (default 20) that damps the
           spectrum between the block's largest Ritz value and `upper_bound` (None: a bound on the largest eigenvalue from ten Lanczos
           steps; a value from the caller must be such a bound), orthonormalised, and a Rayleigh-Ritz step follows; `iterations`
           counts these outer iterations, nev_max is the width of the filtered block.  Everything else — A, X0, the result, the
           residual norms, NoConvergence, gradients — is as for "gcg".  ValueError: M, amg, amg_levels or block_size given with it, or
           an unknown method.  A loop over a handle in the manner of real-space electronic-structure codes does ONE filter pass per
           step of the outer (self-consistency) loop and takes whatever that reaches: maxiter=1 and the .result of NoConvergence,
               try: r = eigsh(m, k, X0=r.eigenvectors, method="chebyshev", maxiter=1, backend=hip)
               except NoConvergence as e: r = e.result
           Measured (profiles/chfsi/README.md: Lap3D 128^3, k = 50) it is 3.6 times SLOWER than GCG with a kept hierarchy, cold and
           warm: use it for matrices GCG cannot take — an indefinite A, or no hierarchy that can be built or kept — not instead of it.
           degree=None means 20 here.
    interval:  (a, b), a < b, both finite, with method="chebyshev", k=None and nev_max given: EVERY eigenpair with a <= lambda <= b
           (GCGE_RunChFSIBand) — the states round a gap, the modes of a frequency band, an indefinite A — in place of the k smallest.
           Per outer iteration all nev_max columns are filtered by the Jackson-damped Chebyshev expansion of the interval's indicator
           (about 1 inside, about 0 outside, 1/2 at the ends), orthonormalised, and a Rayleigh-Ritz step follows; Ritz values inside
           the interval that are mixtures of outside eigenvectors are told from genuine pairs by x^T p(A) x.  nev_max is the width
           of the filtered block and must EXCEED the number of eigenvalues inside (twice it is a good choice;
           gcge_amd.eigenvalue_count estimates that number, suggests an nev_max and shows the gaps before anything is solved); `degree` (>= 2) is the
           expansion's, None: the driver's 6 (lmax - lmin) / (b - a) within [20, 1000]; `lower_bound`, `upper_bound`: bounds of the
           whole spectrum, each taken as it is, what is left out comes from one Lanczos run (given bounds that hug the spectrum need
           fewer iterations than Lanczos's safeguarded ones).  Put a and b in GAPS of the spectrum: an eigenvalue at an end may be
           counted either way, and one close to an end converges slowly.  Do NOT use this for the smallest pairs of a definite
           matrix: GCG with a kept hierarchy finds those several times faster.
           The result holds the j genuine pairs inside, ascending: eigenvalues (j,), eigenvectors (n, j), residual_norms (j,),
           converged = j; `iterations` outer iterations (iterations + 1 filters were applied).  X0, tol, maxiter, gcge_args, backend
           and the forms of A are as for the other methods; a warm start from the eigenvectors of a nearby operator is the loop
               r = eigsh(m, interval=(a, b), nev_max=N, X0=r.eigenvectors, method="chebyshev", backend=hip)
           NoConvergence, with what the run reached in .result: the run ended (maxiter) before every genuine pair passed tol, or
           every column of the block held a wanted pair — more pairs may lie inside than the block can hold: raise nev_max.
           ValueError: another method, k given, no nev_max, a >= b or an end that is not finite, degree < 2, M, amg, amg_levels or
           block_size, eigenvector_grad.  The eigenvalues take gradients as below (the sum over the returned pairs, however many);
           eigenvector_grad is refused: its deflated systems (A - lambda_c) y = g would be INDEFINITE, because the pairs below the
           interval are not in the computed space — call gcge_amd.eigenvector_grads on a space that holds them.

    Gradients: when A (or M) is given as a sparse_csr tensor or a (crow, col, val) triple whose values require grad, and grad mode is
    on, `eigenvalues` comes back attached to the graph and backward gives d loss / d values on the stored entries
    (gcge_amd.grad.eigenvalue_grads: d lambda_c / d A_ij = x_ic x_jc, d lambda_c / d M_ij = -lambda_c x_ic x_jc, one kernel call per
    matrix); the matrix is created from the detached values.  `eigenvectors` and `residual_norms` are marked non-differentiable.
    Double backward raises.  With handles, or without a tensor that requires grad, nothing is attached and nothing else changes.
    eigenvector_grad=True (or a dict of the keywords tol, maxiter, cluster_tol of gcge_amd.grad.eigenvector_grads, whose defaults
    True takes): `eigenvectors` comes back attached as well, for a loss such as one of the density sum_c f_c x_c^2.  Backward then
    runs eigenvector_grads with both incoming gradients: the k x k algebra inside the computed space and k deflated, shifted
    systems (A - lambda_c M) y_c = g_c - M X (X^T g_c) outside it (LinearSolver.solve_deflated; with amg_levels >= 2 preconditioned
    by a hierarchy on A that backward builds and frees, block min(k, 64); otherwise unpreconditioned), then one rank-2k product per
    matrix; NoConvergence of those solves propagates from backward.  The gradients are the symmetrised ones (each of the stored
    entries (i, j) and (j, i) gets its own value; their sum is the derivative along E_ij + E_ji).  The systems are conditioned like
    1 / (lambda_{k+1} - lambda_c) with lambda_{k+1} the first eigenvalue NOT returned: choose k at a gap.  Eigenvalues closer than
    cluster_tol (relative, default 1e-8) are a cluster: the terms between its members are dropped, so a loss that depends on the
    choice of basis inside a cluster has no gradient, while one that weights the members equally gets its own.  The matrices
    this call created then live until backward has run or the graph is freed.  ValueError: eigenvector_grad with a handle for A
    or M, or without a tensor that requires grad — a loop over handles calls gcge_amd.eigenvector_grads itself.

    Returns EigshResult(eigenvalues (k,), eigenvectors (n, k), converged, iterations, seconds, residual_norms (k,)), tensors float64
    on the device (with interval: the j pairs inside in place of k).  Raises NoConvergence, carrying the partial result, when fewer
    than k pairs converged (with interval: see there)."""
    _check_method(k, M, nev_max, block_size, amg_levels, amg, method, degree, lower_bound, interval, eigenvector_grad)
    import torch
    dA, dM = _differentiable(A), _differentiable(M)
    kw = dict(X0=X0, tol=tol, maxiter=maxiter, nev_max=nev_max, block_size=block_size, amg_levels=amg_levels, gcge_args=gcge_args, amg=amg,
              method=method, degree=degree, upper_bound=upper_bound, lower_bound=lower_bound, interval=interval)
    if eigenvector_grad and (_is_handle(A) or _is_handle(M) or (dA is None and dM is None)):
        raise ValueError("eigsh: eigenvector_grad needs A (or M) given as tensors whose values require grad, with grad mode on, and no "
                         "matrix handle; a loop that keeps handles calls gcge_amd.eigenvector_grads itself")
    if dA is None and dM is None:
        return _eigsh(A, k, M, backend=backend, **kw)
    from .grad import _function
    backend = _backend_for(backend, A, M, X0)
    detached = lambda a, d: a if d is None else (a.detach() if isinstance(a, torch.Tensor) else (a[0], a[1], a[2].detach()) + tuple(a[3:]))
    box = {}
    if eigenvector_grad:
        from .grad import _Owned
        options = dict(eigenvector_grad) if isinstance(eigenvector_grad, dict) else {}
        if set(options) - {"tol", "maxiter", "cluster_tol"}:
            raise ValueError("eigsh: eigenvector_grad takes the keywords tol, maxiter, cluster_tol")
        options["amg_levels"] = int(amg_levels)
        kept = {}

        def run_kept():
            box["result"] = _eigsh(detached(A, dA), k, detached(M, dM) if M is not None else None, backend=backend, _keep=kept, **kw)
            kept["owned"] = _Owned(backend, None, None, kept.pop("made"))
            return box["result"]

        lam, V, rn = _function(2).apply(dA[2] if dA is not None else None, dM[2] if dM is not None else None, run_kept, backend,
                                          dA[:2] if dA is not None else None, dM[:2] if dM is not None else None, kept, options)
        return box["result"]._replace(eigenvalues=lam, eigenvectors=V, residual_norms=rn)

    def run():
        box["result"] = _eigsh(detached(A, dA), k, detached(M, dM) if M is not None else None, backend=backend, **kw)
        return box["result"]

    lam, V, rn = _function(0).apply(dA[2] if dA is not None else None, dM[2] if dM is not None else None, run, backend,
                                      dA[:2] if dA is not None else None, dM[:2] if dM is not None else None)
    return box["result"]._replace(eigenvalues=lam, eigenvectors=V, residual_norms=rn)


def _differentiable(a):
    """(crow, col, val) when `a` is a matrix given as tensors whose values require grad while grad mode is on, else None"""
    import torch
    if a is None or _is_handle(a) or not torch.is_grad_enabled():
        return None
    if isinstance(a, torch.Tensor):
        return (a.crow_indices(), a.col_indices(), a.values()) if a.layout == torch.sparse_csr and a.requires_grad else None
    if isinstance(a, (tuple, list)) and len(a) >= 3 and isinstance(a[2], torch.Tensor) and a[2].requires_grad:
        return (a[0], a[1], a[2])
    return None


def _backend_for(backend, *things):
    """`backend`, or the HipBackend kept for the device of the first CUDA tensor among `things` (torch's current device without one)"""
    from .lib import HipBackend
    if backend is None:
        dev = _device_of(*things)
        backend = _backends.get(dev)
        if backend is None:
            backend = _backends[dev] = HipBackend(device=dev)
    return backend


def _eigsh(A, k, M=None, X0=None, tol=1e-8, maxiter=None, nev_max=None, block_size=None, amg_levels=0, backend=None, gcge_args=(), amg=None,
           _keep=None, method="gcg", degree=None, upper_bound=None, lower_bound=None, interval=None):
    """eigsh on detached inputs: see there.  _keep: a dict that, when all k pairs converged, takes the handles "A" and "M" of the solve
    and the list "made" of those created here, which are then NOT freed (the caller owns them)"""
    import numpy as np
    import torch
    from .lib import host_lib, run_chfsi, run_chfsi_band, run_gcg

    _check_method(k, M, nev_max, block_size, amg_levels, amg, method, degree, lower_bound, interval)
    chebyshev, band = method == "chebyshev", interval is not None
    if band:
        k = 0                          # (the count comes out of the run)
        nev_max = int(nev_max)
    else:
        k = int(k)
        nev_max = 2 * k if nev_max is None else int(nev_max)
        if k < 1 or nev_max < k:
            raise ValueError("eigsh: 1 <= k <= nev_max is required")
    amg_levels = int(amg_levels)
    if amg_levels == 1 or amg_levels < 0:
        raise ValueError("eigsh: amg_levels is 0 (no hierarchy) or at least 2")
    if amg is not None:
        as_int = lambda a: (a.value if isinstance(a, C.c_void_p) else a) if _is_handle(a) else None
        if amg_levels > 0:
            raise ValueError("eigsh: amg (a hierarchy that exists) and amg_levels (one built inside the call) exclude each other")
        if as_int(A) is None or as_int(A) != amg.A.value or as_int(M) != (amg.M.value if amg.M is not None else None):
            raise ValueError("eigsh: amg was not built on these matrix handles")
        if block_size is not None and int(block_size) > amg.block_size:
            raise ValueError("eigsh: block_size %d exceeds the hierarchy's %d" % (int(block_size), amg.block_size))
        if backend is not None and backend is not amg.backend:
            raise ValueError("eigsh: amg belongs to another back-end")
        backend = amg.backend
        if block_size is None:
            block_size = amg.block_size
    backend = _backend_for(backend, A, M, X0)
    gcge_args = [str(a) for a in gcge_args]
    own = ([] if band else [("-nevConv", k)]) + [("-nevMax", nev_max), ("-gcge_rel_tol", repr(float(tol)))]
    if maxiter is not None:
        own.append(("-gcge_max_niter", int(maxiter)))
    if block_size is not None:
        own.append(("-blockSize", int(block_size)))
    if amg_levels > 0:
        own.append(("-gcge_amg_levels", amg_levels))
    if chebyshev:
        if band:
            own += [("-chfsi_band_lo", repr(float(interval[0]))), ("-chfsi_band_hi", repr(float(interval[1])))]
        if degree is not None or not band:                 # (the band's None is the driver's own choice)
            own.append(("-chfsi_degree", 20 if degree is None else int(degree)))
        if lower_bound is not None:
            own.append(("-chfsi_lower_bound", repr(float(lower_bound))))
        if upper_bound is not None:
            own.append(("-chfsi_upper_bound", repr(float(upper_bound))))
    args = []
    for name, value in own:             # (the harness takes the first occurrence of an option)
        if name not in gcge_args:
            args += [name, value]
    args += gcge_args
    for i, a in enumerate(gcge_args[:-1]):
        if a == "-nevMax":
            nev_max = int(gcge_args[i + 1])

    made = []

    def handle(a):
        if _is_handle(a):
            return a if isinstance(a, C.c_void_p) else C.c_void_p(a)
        m = backend.matrix_from_device(*a) if isinstance(a, (tuple, list)) else backend.matrix_from_device(a)
        made.append(m)
        return m

    evec = result = None
    try:
        mA = handle(A)
        mB = handle(M) if M is not None else None
        flag = 1 if amg_levels > 0 or amg is not None else 0
        if amg is not None:
            amg.install()
        shape = None
        if X0 is not None:
            shape = tuple(X0.shape) if hasattr(X0, "shape") else tuple(X0.__cuda_array_interface__["shape"])
            if len(shape) != 2 or shape[1] > nev_max:
                raise ValueError("eigsh: X0 is an (n, j) block with j <= nev_max")
        band_rc = 0
        if chebyshev:
            evec = backend.ops.mv_create(nev_max, mA)
            if X0 is not None:
                backend.mv_from_torch(mA, X0, mv=evec, c0=0)
            ev, res, rc = (run_chfsi_band if band else run_chfsi)(backend.ops_handle, mA, args, evec, given=int(shape[1]) if X0 is not None else 0)
            if band and rc in (0, -6):                     # (-6: every column holds a wanted pair; the columns are what the run reached)
                band_rc, k = rc, int(res.nevConv)
            elif rc != 0:
                raise RuntimeError("%s rc=%d" % ("GCGE_RunChFSIBand" if band else "GCGE_RunChFSI", rc))
        elif X0 is not None:
            evec = backend.ops.mv_create(nev_max, mA)
            backend.mv_from_torch(mA, X0, mv=evec, c0=0)
            ev, res = run_gcg(backend.ops_handle, mA, mB, args, flag=flag, given=(evec, int(shape[1])))
        else:
            ev, res, evec = run_gcg(backend.ops_handle, mA, mB, args, flag=flag, keep_evec=True)
        h = host_lib()
        lam = np.ascontiguousarray(ev[:k], dtype=np.float64)
        rn = np.zeros(k)
        rc = h.GCGE_ResidualNorms(mA, mB, evec, 0, k, lam.ctypes.data_as(C.POINTER(C.c_double)), rn.ctypes.data_as(C.POINTER(C.c_double)),
                                  backend.ops_handle) if k > 0 else 0
        if rc != 0:
            raise RuntimeError("GCGE_ResidualNorms rc=%d" % rc)
        V = backend.mv_to_torch(evec, 0, k)
        result = EigshResult(torch.from_numpy(lam).to(V.device), V, int(res.nevConv), int(res.numIter), float(res.seconds),
                             torch.from_numpy(rn).to(V.device))
    finally:
        if evec is not None and evec.value:
            backend.ops.mv_destroy(evec, nev_max)
        if _keep is not None and result is not None and not band and result.converged >= k:
            _keep.update(A=mA, M=mB, made=list(made))
        else:
            for m in made:
                backend.free_matrix(m)
    if band:
        if band_rc == -6:
            raise NoConvergence("eigsh: all %d columns hold eigenpairs inside [%r, %r] after %d iterations: more may lie inside than the block "
                                "can hold; raise nev_max" % (result.converged, float(interval[0]), float(interval[1]), result.iterations), result)
        if not res.converged:
            raise NoConvergence("eigsh: the %d pairs found inside [%r, %r] did not all converge in %d iterations"
                                % (result.converged, float(interval[0]), float(interval[1]), result.iterations), result)
        return result
    if result.converged < k:
        raise NoConvergence("eigsh: %d of %d pairs converged in %d iterations" % (result.converged, k, result.iterations), result)
    return result
