"""gcge_amd.eigenvalue_count, count_from_moments, spectral_density: counting before solving, by the kernel polynomial method.

eigsh(A, interval=(a, b), nev_max=N, method="chebyshev") wants to know in advance how many eigenvalues lie inside (N must exceed it),
where the gaps of the spectrum are (a and b belong in gaps) and a degree.  All three come out of the Chebyshev moments
mu_j = v^T T_j((A - c) / e) v of a few random probe vectors: the trace of the band-pass polynomial estimates the count, the Jackson-damped
series the density of states.

Plumbing only: the moments are GCGE_ChebMoments (HipBackend.chebyshev_moments: ceil(degree / 2) steps of the recurrence on a block of
`probes` columns, each step ONE call of the back-end's cheb_step_dots), the count is GCGE_ChebCountFromMoments; the probes are drawn on
the device and the moments stay there, so nothing of size O(n) is on the host."""
import collections
import ctypes as C
import math

CountResult = collections.namedtuple("CountResult", ["count", "stderr", "per_probe", "moments", "degree", "lower_bound", "upper_bound",
                                                     "suggested_nev_max"])

LANCZOS_STEPS = 10          # as the drivers' -chfsi_lanczos_steps
DEGREE_FACTOR = 6.0         # GCGE_CHFSI_BAND_DEGREE_FACTOR (include/gcge_solver.h): the band driver's rule


def _interval(interval, who):
    try:
        a, b = (float(v) for v in interval)
    except (TypeError, ValueError):
        raise ValueError("%s: interval is a pair (a, b) of numbers" % who) from None
    if not (math.isfinite(a) and math.isfinite(b) and a < b):
        raise ValueError("%s: interval=(a, b) requires a < b, both finite" % who)
    return a, b


def _bounds(lower_bound, upper_bound, a, b, who):
    """the checks that need no device: each given bound finite, and when both are given lower < upper and [a, b] meeting them"""
    lo = None if lower_bound is None else float(lower_bound)
    up = None if upper_bound is None else float(upper_bound)
    if (lo is not None and not math.isfinite(lo)) or (up is not None and not math.isfinite(up)):
        raise ValueError("%s: lower_bound and upper_bound are finite numbers (or None: Lanczos bounds)" % who)
    if lo is not None and up is not None and not lo < up:
        raise ValueError("%s: lower_bound < upper_bound is required" % who)
    if (up is not None and not a <= up) or (lo is not None and not b >= lo):
        raise ValueError("%s: the interval misses the bounds of the spectrum" % who)
    return lo, up


def suggested_nev_max(count, stderr):
    """A block width for eigsh(interval=): ceil(1.5 (count + 3 stderr)) + 4.  A HEURISTIC, not a bound: three standard errors cover the
    probes' scatter, the factor 1.5 and the 4 leave the filtered block the slack the band driver converges with; an end inside a
    cluster of eigenvalues biases the count itself (the polynomial is 1/2 at an end), which no margin on the scatter repairs."""
    return int(math.ceil(1.5 * (max(float(count), 0.0) + 3.0 * float(stderr)))) + 4


def _result(mom_host, moments, lower_bound, upper_bound, interval):
    import torch
    from .lib import count_from_moments as count_c
    count, err, per = count_c(mom_host, lower_bound, upper_bound, interval)
    per_t = torch.from_numpy(per)
    if isinstance(moments, torch.Tensor):
        per_t = per_t.to(moments.device)
    return CountResult(count, err, per_t, moments, int(mom_host.shape[0]) - 1, float(lower_bound), float(upper_bound), suggested_nev_max(count, err))


def count_from_moments(moments, lower_bound, upper_bound, interval):
    """The count of another interval from moments that exist (CountResult.moments, or HipBackend.chebyshev_moments over the same
    bounds): a CountResult as eigenvalue_count returns it, without touching the matrix.  moments: a (degree + 1, m) tensor or array,
    degree >= 2.  The polynomial's degree is that of the moments, so a narrow interval wants moments of a degree that resolves it
    (about 6 (upper_bound - lower_bound) / (b - a)).  ValueError: a >= b, lower_bound >= upper_bound, an interval that misses the
    bounds, fewer than three rows of moments."""
    a, b = _interval(interval, "count_from_moments")
    lo, up = _bounds(lower_bound, upper_bound, a, b, "count_from_moments")
    if lo is None or up is None:
        raise ValueError("count_from_moments: the bounds the moments were taken over are required")
    import numpy as np
    import torch
    host = moments.detach().cpu().numpy() if isinstance(moments, torch.Tensor) else np.asarray(moments, dtype=np.float64)
    if host.ndim != 2 or host.shape[0] < 3 or host.shape[1] < 1:
        raise ValueError("count_from_moments: moments is a (degree + 1, m) block with degree >= 2 and m >= 1")
    return _result(np.ascontiguousarray(host, dtype=np.float64), moments, lo, up, (a, b))


def spectral_density(moments, lower_bound, upper_bound, points):
    """The density of states of A at `points` from its Chebyshev moments over [lower_bound, upper_bound], averaged over the probes: the
    Jackson-damped series of the kernel polynomial method,
        rho(lambda) = (g_0 mu_0 + 2 sum_{j >= 1} g_j mu_j T_j(t)) / (pi e sqrt(1 - t^2)),   t = (lambda - c) / e,
    with mu_j the mean of moments[j] over the probes and g_j the Jackson factors of GCGE_ChebBandCoefficients.  It is nonnegative,
    resolves about pi e / degree, and integrates over the bounds to the mean of mu_0, which is n for +-1 probes (and for any probes
    with v^T v = n).  Gaps of the spectrum show as intervals where it vanishes: the places for the ends of eigsh's interval.
    moments: a (degree + 1, m) tensor or array; points: a tensor or array of any shape; returns a float64 tensor of that shape on the
    device of `moments` (0 at points outside the open interval of the bounds).  ValueError: lower_bound >= upper_bound."""
    import torch
    lo, up = float(lower_bound), float(upper_bound)
    if not (math.isfinite(lo) and math.isfinite(up) and lo < up):
        raise ValueError("spectral_density: lower_bound < upper_bound, both finite, is required")
    mom = torch.as_tensor(moments, dtype=torch.float64)
    if mom.dim() != 2 or mom.shape[0] < 1 or mom.shape[1] < 1:
        raise ValueError("spectral_density: moments is a (degree + 1, m) block")
    lam = torch.as_tensor(points, dtype=torch.float64, device=mom.device)
    c, e = 0.5 * (up + lo), 0.5 * (up - lo)
    p = mom.shape[0] - 1
    j = torch.arange(p + 1, dtype=torch.float64, device=mom.device)
    al = math.pi / (p + 2)
    g = ((p + 2 - j) * torch.cos(j * al) + torch.sin(j * al) * (math.cos(al) / math.sin(al))) / (p + 2)
    w = g * mom.mean(dim=1)
    w[1:] *= 2.0
    t = (lam.reshape(-1) - c) / e
    inside = (t > -1.0) & (t < 1.0)
    tc = torch.where(inside, t, torch.zeros_like(t))
    series = torch.cos(torch.outer(torch.acos(tc), j)) @ w
    rho = torch.where(inside, series / (math.pi * e * torch.sqrt(1.0 - tc * tc)), torch.zeros_like(t))
    return rho.reshape(lam.shape)


def eigenvalue_count(A, interval, probes=32, degree=None, lower_bound=None, upper_bound=None, seed=0, V=None, backend=None):
    """An estimate of the number of eigenvalues of the symmetric matrix A inside interval = (a, b), before any eigenpair is computed:
    the stochastic trace of the band-pass polynomial p of eigsh(interval=), count = mean over the probes of v^T p(A) v, whose
    expectation is sum_i p(lambda_i) — the number of eigenvalues inside when a and b lie in gaps wider than the polynomial's
    resolution (p is 1/2 at an end, so an end inside a cluster counts about half of it).

    A:       a torch sparse_csr CUDA tensor, a (crow, col, val) triple of device arrays, or a matrix handle of the back-end, as for
             eigsh; a handle stays the caller's, what is created here is freed here.
    probes:  the number of probe vectors: +-1 columns drawn on the device by a torch.Generator seeded with `seed` (the same count for the
             same seed).  V: the caller's (n, m) device tensor of probes in their place (`probes` and `seed` are then ignored); the
             estimate assumes v^T v = n and independent entries of mean 0.
    degree:  of the polynomial (>= 2); None: the band driver's rule, ceil(6 (upper - lower) / (b - a)) within [20, 1000].  The cost is
             ceil(degree / 2) products of A with a block of m columns.
    lower_bound, upper_bound:  bounds of the whole spectrum, each taken as it is; what is left out comes from one run of
             GCGE_LanczosBounds (ten steps from one random column, safeguarded at both ends).
    backend: a HipBackend (default: one per device, kept for the process).

    Returns CountResult(count, stderr, per_probe, moments, degree, lower_bound, upper_bound, suggested_nev_max): stderr is the sample
    standard deviation of the per-probe estimates / sqrt(m) (0 for one probe), per_probe (m,) and moments (degree + 1, m) float64
    device tensors — count_from_moments recounts another interval and spectral_density draws the density of states from the same
    moments, without touching the matrix — and suggested_nev_max = ceil(1.5 (count + 3 stderr)) + 4, a heuristic block width for
    eigsh(interval=(a, b), nev_max=...) (see suggested_nev_max).
    ValueError, raised before anything touches the device: an interval that is no pair a < b of finite numbers, probes < 1,
    degree < 2, bounds that are not finite, not ordered or missed by the interval."""
    a, b = _interval(interval, "eigenvalue_count")
    lo, up = _bounds(lower_bound, upper_bound, a, b, "eigenvalue_count")
    if degree is not None and int(degree) < 2:
        raise ValueError("eigenvalue_count: degree >= 2 is required (or None: the band driver's rule)")
    if V is None and int(probes) < 1:
        raise ValueError("eigenvalue_count: probes >= 1 is required")
    if V is not None and (not hasattr(V, "shape") or len(V.shape) != 2 or int(V.shape[1]) < 1):
        raise ValueError("eigenvalue_count: V is an (n, m) block of probes with m >= 1")
    import torch
    from .eigsh import _backend_for, _is_handle
    from .lib import host_lib
    backend = _backend_for(backend, A, V)
    made = None
    try:
        if _is_handle(A):
            mA = A if isinstance(A, C.c_void_p) else C.c_void_p(A)
        else:
            mA = made = backend.matrix_from_device(*A) if isinstance(A, (tuple, list)) else backend.matrix_from_device(A)
        n = int(backend.g.gcge_hip_mat_nrows(mA))
        if lo is None or up is None:
            C.CDLL(None).srand(0)                          # (the drivers' seed: the same bounds on every call)
            l0, u0 = C.c_double(), C.c_double()
            rc = host_lib().GCGE_LanczosBounds(mA, LANCZOS_STEPS, C.cast(C.byref(l0), C.c_void_p), C.cast(C.byref(u0), C.c_void_p), backend.ops_handle)
            if rc != 0:
                raise RuntimeError("GCGE_LanczosBounds rc=%d" % rc)
            lo, up = l0.value if lo is None else lo, u0.value if up is None else up
            if not lo < up or not a <= up or not b >= lo:
                raise ValueError("eigenvalue_count: the interval misses the bounds of the spectrum [%r, %r]" % (lo, up))
        if degree is None:
            degree = min(max(int(math.ceil(DEGREE_FACTOR * (up - lo) / (b - a))), 20), 1000)
        if V is None:
            gen = torch.Generator(device=backend.torch_device())
            gen.manual_seed(int(seed))
            V = torch.randint(0, 2, (n, int(probes)), generator=gen, device=backend.torch_device()).to(torch.float64) * 2.0 - 1.0
        elif int(V.shape[0]) != n:
            raise ValueError("eigenvalue_count: V has %d rows, the matrix %d" % (int(V.shape[0]), n))
        moments = backend.chebyshev_moments(mA, V, int(degree), lo, up)
    finally:
        if made is not None:
            backend.free_matrix(made)
    return _result(moments.cpu().numpy(), moments, lo, up, (a, b))
