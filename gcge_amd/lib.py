"""ctypes bindings of libgcge_host.so / libgcge_hip.so (C ABI: include/*.h).

There is NO CPU fallback here: HipBackend() raises if the HIP library or a GPU is
missing.  The CPU oracle lives under oracle/ and is imported by tests only.
"""
import ctypes as C
import os
import subprocess

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_LIBDIR = os.path.join(_HERE, "lib")


class CSR(C.Structure):
    """GCGE_CSR (include/gcge_problems.h)."""
    _fields_ = [("nrows", C.c_int), ("ncols", C.c_int), ("row_begin", C.c_int),
                ("nnz", C.c_int64), ("rowptr", C.POINTER(C.c_int)),
                ("colidx", C.POINTER(C.c_int)), ("val", C.POINTER(C.c_double))]


class MG(C.Structure):
    """GCGE_MG (include/gcge_multigrid.h)."""
    _fields_ = [("num_levels", C.c_int), ("box_levels", C.c_int), ("A", C.POINTER(CSR)), ("B", C.POINTER(CSR)),
                ("P", C.POINTER(CSR)), ("PT", C.POINTER(CSR)), ("dims", C.POINTER(C.c_int * 3))]


class Timing(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("initX", "checkconv", "compP", "compRR", "rr_matW",
                                          "dsyevx", "compRV", "compW", "linsol", "compX", "total")]


class RunResult(C.Structure):
    _fields_ = [("nevConv", C.c_int), ("numIter", C.c_int), ("nevMax", C.c_int),
                ("block_size", C.c_int), ("nevInit", C.c_int), ("seconds", C.c_double),
                ("timing", Timing)]


class PASResult(C.Structure):
    """GCGE_PAS_RESULT (include/gcge_solver.h): PAS's converged pairs, iterations, levels and seconds, then the warm-started GCG."""
    _fields_ = [("nevConv", C.c_int), ("numIter", C.c_int), ("num_levels", C.c_int), ("seconds", C.c_double),
                ("gcg", RunResult)]


def build_libs(hip=True, verbose=False):
    """make -C gcge_amd/csrc [host|all]  (hipcc cross-compiles gfx950 without a GPU)."""
    target = "all" if hip else "host"
    r = subprocess.run(["make", "-C", os.path.join(_HERE, "csrc"), target],
                       capture_output=not verbose, text=True)
    if r.returncode != 0:
        raise RuntimeError("building gcge libraries failed:\n" + (r.stdout or "") + (r.stderr or ""))


_host = None
_hip = None


def host_lib():
    global _host
    if _host is None:
        path = os.path.join(_LIBDIR, "libgcge_host.so")
        if not os.path.exists(path):
            build_libs(hip=False)
        lib = C.CDLL(path, mode=C.RTLD_GLOBAL)
        abi.declare(lib, abi.HOST, "libgcge_host.so")
        _host = lib
    return _host


def hip_lib():
    """Load the HIP back-end; fails loudly when it is missing (no fallback)."""
    global _hip
    if _hip is None:
        host_lib()
        path = os.path.join(_LIBDIR, "libgcge_hip.so")
        if not os.path.exists(path):
            raise RuntimeError("libgcge_hip.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
        lib = C.CDLL(path, mode=C.RTLD_GLOBAL)
        abi.declare(lib, abi.HIP, "libgcge_hip.so")
        _hip = lib
    return _hip


def csr_arrays(A):
    """(rowptr, colidx, val) numpy copies of a host CSR struct."""
    import numpy as np
    n, nnz = A.nrows, int(A.nnz)
    return (np.ctypeslib.as_array(A.rowptr, (n + 1,)).copy(),
            np.ctypeslib.as_array(A.colidx, (max(nnz, 1),))[:nnz].copy(),
            np.ctypeslib.as_array(A.val, (max(nnz, 1),))[:nnz].copy())


def csr_to_scipy(A):
    """A host CSR struct as a scipy matrix (copies)."""
    import scipy.sparse as sp
    rp, ci, va = csr_arrays(A)
    return sp.csr_matrix((va, ci, rp), shape=(A.nrows, A.ncols))


def _take_csr(out):
    arrs = csr_arrays(out)
    host_lib().gcge_csr_free(C.byref(out))
    return arrs


def multigrid_mode(mode=None):
    """Where the HIP back-end builds its multigrid hierarchy: 0 on the device (default), 1 on the host; returns the mode in force."""
    h = hip_lib()
    if mode is not None:
        h.gcge_hip_multigrid_mode(int(mode))
    return h.gcge_hip_multigrid_get_mode()


def multigrid_stats():
    """The last MultiGridCreate of the HIP back-end: (dict of seconds per phase, bytes copied device to host)."""
    s, b = (C.c_double * 6)(), C.c_long()
    hip_lib().gcge_hip_multigrid_stats(s, C.byref(b))
    return dict(zip(("detect", "aggregate", "galerkin", "transfers", "coarse_upload", "other"), list(s))), b.value


def multigrid_masked_cells(on=None):
    """Whether MultiGridCreate of the HIP back-end coarsens a matrix on a masked grid (a handle with a geometry, mat_geometry) by the
    2 x 2 x 2 cells of its box (1, the default) or as a matrix without a grid (0); returns the setting in force."""
    h = hip_lib()
    if on is not None:
        h.gcge_hip_multigrid_masked_cells(int(on))
    return h.gcge_hip_multigrid_get_masked_cells()


def multigrid_device_levels(on=None):
    """Whether the device build of a grid or MIS-2 hierarchy hands its coarse levels to gcge_hip_mat_create_device straight from the
    Galerkin output (1, the default) or downloads them for the host constructors (0); returns the setting in force."""
    h = hip_lib()
    if on is not None:
        h.gcge_hip_multigrid_device_levels(int(on))
    return h.gcge_hip_multigrid_get_device_levels()


def mat_device_stats():
    """gcge_hip_mat_device_stats: (matrices analysed on the device, fall-backs to the host path, fall-backs caused by a hash
    collision, bytes copied device to host) since the library was loaded."""
    out = (C.c_long * 4)()
    hip_lib().gcge_hip_mat_device_stats(out)
    return tuple(out)


def mat_update_stats():
    """gcge_hip_mat_update_stats: (updates that kept the form, of those value-table rewrites, conversions to "+values", declines,
    bad-argument returns, bytes copied device to host) of gcge_hip_mat_update_values_device since the library was loaded."""
    out = (C.c_long * 6)()
    hip_lib().gcge_hip_mat_update_stats(out)
    return tuple(out)


def mat_update_form_stats():
    """gcge_hip_mat_update_form_stats: (star handles updated, dense handles updated, declines by a pinned entry, declines by a NaN
    diagonal) of gcge_hip_mat_update_values_device since the library was loaded."""
    out = (C.c_long * 4)()
    hip_lib().gcge_hip_mat_update_form_stats(out)
    return tuple(out)


def mat_device_hash_bits(bits):
    """Tests: the device pattern search keeps only the low `bits` bits of its row hash (64: all of it, the default)."""
    hip_lib().gcge_hip_mat_device_hash_bits(int(bits))


def mat_pattern_table(mat):
    """Tests: (pid, table) of a HIP matrix handle's pattern form as numpy arrays — pid uint16 per row, the table as raw bytes (16
    per entry: value, column offset) — or (None, None) when the matrix has no pattern form."""
    import numpy as np
    h = hip_lib()
    nt = h.gcge_hip_mat_pattern_table(mat, None, None)
    if nt == 0:
        return None, None
    pid, tab = np.zeros(h.gcge_hip_mat_nrows(mat), dtype=np.uint16), np.zeros(nt * 16, dtype=np.uint8)
    h.gcge_hip_mat_pattern_table(mat, pid.ctypes.data_as(C.c_void_p), tab.ctypes.data_as(C.c_void_p))
    return pid, tab


def mat_geometry(mat):
    """The geometry a HIP matrix handle carries: (kind, dims, box_of_row) with kind 0 none (dims, box None), 1 named by the caller
    (HipBackend.matrix_grid), 2 recovered at upload; box_of_row[r] = x + nx (y + ny z) as a numpy int32 array."""
    import numpy as np
    h = hip_lib()
    dims = (C.c_int * 3)()
    kind = h.gcge_hip_mat_geometry(mat, dims, None)
    if kind == 0:
        return 0, None, None
    box = np.zeros(h.gcge_hip_mat_nrows(mat), dtype=np.int32)
    h.gcge_hip_mat_geometry(mat, dims, box.ctypes.data_as(C.POINTER(C.c_int)))
    return kind, tuple(dims), box


def mg_aggregate_masked(dims, box_of_row, device=False):
    """The 2 x 2 x 2 cells of a masked grid (gcge_mg_aggregate_masked, include/gcge_multigrid.h): (nc, agg, cdims, cbox) from the
    host routine, or with device=True (nc, agg, cdims, cbox, ptr, mem) from the kernels of the HIP back-end (ptr / mem: the members
    of every cell in ascending row order).  nc < 0: the geometry was refused (the arrays are then None)."""
    import numpy as np
    box = np.ascontiguousarray(box_of_row, dtype=np.int32)
    n = len(box)
    ip = C.POINTER(C.c_int)
    agg, cbox, cd = np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1), dtype=np.int32), (C.c_int * 3)()
    d = (C.c_int * 3)(*[int(v) for v in dims])
    if not device:
        f = host_lib().gcge_mg_aggregate_masked
        nc = f(C.byref(d), box.ctypes.data_as(ip), n, agg.ctypes.data_as(ip), C.byref(cd), cbox.ctypes.data_as(ip))
        return (nc, agg[:n], tuple(cd), cbox[:nc].copy()) if nc >= 0 else (nc, None, None, None)
    ptr, mem = np.zeros(n + 1, dtype=np.int32), np.zeros(max(n, 1), dtype=np.int32)
    f = hip_lib().gcge_hip_mg_aggregate_masked
    nc = f(C.byref(d), box.ctypes.data_as(ip), n, agg.ctypes.data_as(ip), ptr.ctypes.data_as(ip), mem.ctypes.data_as(ip),
           cbox.ctypes.data_as(ip), C.byref(cd))
    return (nc, agg[:n], tuple(cd), cbox[:nc].copy(), ptr[:nc + 1].copy(), mem[:n]) if nc >= 0 else (nc, None, None, None, None, None)


def multigrid_graph_method(method=None):
    """How a matrix without a grid is aggregated (gcge_mg_set_graph_method, include/gcge_multigrid.h), process-wide, by the host
    builders and by MultiGridCreate of every back-end: 0 the greedy routine (default), 1 MIS-2; returns the method in force."""
    h = host_lib()
    if method is not None:
        h.gcge_mg_set_graph_method(C.c_int(int(method)))
    return h.gcge_mg_get_graph_method()


def mg_aggregate_graph(arrays_or_mat, theta=0.25, device=False):
    """MIS-2 aggregation (gcge_mg_aggregate_mis2, include/gcge_multigrid.h) of a symmetric matrix: (nc, agg) from the host routine
    for (rowptr, colidx, val) arrays, or with device=True (nc, agg, ptr, mem) from the kernels of the HIP back-end for such arrays
    or a HIP matrix handle (its device CSR; ptr / mem: the members of every aggregate in ascending row order).  nc < 0: the routine
    failed (the arrays are then None)."""
    import numpy as np
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    if isinstance(arrays_or_mat, (tuple, list)):
        rp, ci, va = (np.ascontiguousarray(arrays_or_mat[0], dtype=np.int32), np.ascontiguousarray(arrays_or_mat[1], dtype=np.int32),
                      np.ascontiguousarray(arrays_or_mat[2], dtype=np.float64))
        n, mat = len(rp) - 1, None
    else:
        if not device:
            raise ValueError("the host routine takes (rowptr, colidx, val) arrays")
        h = hip_lib()
        n, mat = h.gcge_hip_mat_nrows(arrays_or_mat), arrays_or_mat
    agg = np.zeros(max(n, 1), dtype=np.int32)
    if not device:
        A = CSR(n, n, 0, len(ci), rp.ctypes.data_as(ip), ci.ctypes.data_as(ip), va.ctypes.data_as(dp))
        f = host_lib().gcge_mg_aggregate_mis2
        nc = f(C.byref(A), float(theta), agg.ctypes.data_as(ip))
        return (nc, agg[:n]) if nc >= 0 else (nc, None)
    ptr, mem = np.zeros(n + 1, dtype=np.int32), np.zeros(max(n, 1), dtype=np.int32)
    h = hip_lib()
    if mat is None:
        f = h.gcge_hip_mg_aggregate_graph_csr
        nc = f(n, rp.ctypes.data_as(ip), ci.ctypes.data_as(ip), va.ctypes.data_as(dp), float(theta), agg.ctypes.data_as(ip),
               ptr.ctypes.data_as(ip), mem.ctypes.data_as(ip))
    else:
        f = h.gcge_hip_mg_aggregate_graph
        nc = f(mat, float(theta), agg.ctypes.data_as(ip), ptr.ctypes.data_as(ip), mem.ctypes.data_as(ip))
    return (nc, agg[:n], ptr[:nc + 1].copy(), mem[:n]) if nc >= 0 else (nc, None, None, None)


def mg_galerkin_device(mat, agg, nc, scale):
    """scale P^T A P on the device for a HIP matrix handle and an aggregate map (numpy int32): (rowptr, colidx, val)."""
    import numpy as np
    agg = np.ascontiguousarray(agg, dtype=np.int32)
    out = CSR()
    rc = hip_lib().gcge_hip_mg_galerkin(mat, agg.ctypes.data_as(C.POINTER(C.c_int)), int(nc), float(scale), C.byref(out))
    if rc != 0:
        raise RuntimeError("gcge_hip_mg_galerkin failed: %d" % rc)
    return _take_csr(out)


def mg_galerkin_values_device(mat, agg, nc, scale, rowptr_c, colidx_c, out):
    """The values of scale P^T A P on the device for a HIP matrix handle, an aggregate map and a coarse structure that exists
    (gcge_hip_mg_galerkin_values_device through gcge_hip_mg_galerkin_values): `out` (numpy float64, one value per coarse entry) goes
    up as it is and comes back as the device function left it.  Returns 0 (written) or 1 (an entry's coarse column is not in its
    coarse row: out is unchanged)."""
    import numpy as np
    ip = C.POINTER(C.c_int)
    agg = np.ascontiguousarray(agg, dtype=np.int32)
    rp, ci = np.ascontiguousarray(rowptr_c, dtype=np.int32), np.ascontiguousarray(colidx_c, dtype=np.int32)
    if out.dtype != np.float64 or not out.flags.c_contiguous or len(out) != len(ci) or len(rp) != int(nc) + 1:
        raise ValueError("mg_galerkin_values_device: nc + 1 row pointers and a contiguous float64 value per coarse entry are required")
    rc = hip_lib().gcge_hip_mg_galerkin_values(mat, agg.ctypes.data_as(ip), int(nc), float(scale), rp.ctypes.data_as(ip), ci.ctypes.data_as(ip),
                                               out.ctypes.data_as(C.POINTER(C.c_double)))
    if rc < 0:
        raise RuntimeError("gcge_hip_mg_galerkin_values failed: %d" % rc)
    return rc


def multigrid_refresh_stats():
    """gcge_hip_multigrid_refresh_stats: (refreshes completed in place, calls that ended in a decline, levels written, bytes copied
    device to host) since the library was loaded."""
    out = (C.c_long * 4)()
    hip_lib().gcge_hip_multigrid_refresh_stats(out)
    return tuple(out)


def mat_to_csr(mat, transpose=False):
    """A HIP matrix handle's device CSR (P^T of a rectangular handle with transpose=True) as numpy (rowptr, colidx, val)."""
    out = CSR()
    rc = (hip_lib().gcge_hip_mat_to_csr_t if transpose else hip_lib().gcge_hip_mat_to_csr)(mat, C.byref(out))
    if rc != 0:
        raise RuntimeError("gcge_hip_mat_to_csr failed: %d" % rc)
    return _take_csr(out)


def load_petsc_binary(path, row_begin=0, row_end=-1):
    """PETSc binary Mat file (what the reference's SLEPc driver reads: test/test_app_slepc.c:416-445) -> host CSR;
    rows [row_begin, row_end) with global columns (row_end < 0: to the end)."""
    h = host_lib()
    A = CSR()
    rc = h.gcge_load_petsc_binary(os.fsencode(path), row_begin, row_end, C.byref(A))
    if rc != 0:
        raise RuntimeError("gcge_load_petsc_binary(%r) failed: %d" % (path, rc))
    return A


def load_matrix_market(path):
    """Matrix Market coordinate file (the form SuiteSparse ships the reference's SiO2 / Ga41As41H72 ... in) -> host CSR, full
    matrix (symmetric files are expanded), ascending columns."""
    h = host_lib()
    A = CSR()
    rc = h.gcge_load_matrix_market(os.fsencode(path), C.byref(A))
    if rc != 0:
        raise RuntimeError("gcge_load_matrix_market(%r) failed: %d" % (path, rc))
    return A


def make_problem(kind, size, row_begin=0, row_end=-1, **kw):
    """Returns (A, B) CSR structs (B is None for standard problems)."""
    h = host_lib()
    A, B = CSR(), CSR()
    if kind == "lap3d":
        rc = h.gcge_problem_lap3d(C.c_int(size), C.c_int64(row_begin), C.c_int64(row_end), C.byref(A)); B = None
    elif kind == "fe1d":
        rc = h.gcge_problem_fe1d(C.c_int(size), C.byref(A), C.byref(B))
    elif kind == "fe3d":
        rc = h.gcge_problem_fe3d(C.c_int(size), C.c_int64(row_begin), C.c_int64(row_end), C.byref(A), C.byref(B))
    elif kind == "sio2":
        rc = h.gcge_problem_sio2_like(C.c_int(size), C.c_int(kw.get("K", 8)), C.c_double(kw.get("R0", 1.5)),
                                      C.c_double(kw.get("R1", 3.0)), C.c_uint64(kw.get("seed", 12345)),
                                      C.c_int64(row_begin), C.c_int64(row_end), C.byref(A)); B = None
    elif kind == "sio2ball":
        rc = h.gcge_problem_sio2_ball(C.c_int(size), C.c_int(kw.get("K", 8)), C.c_double(kw.get("R0", 1.5)),
                                      C.c_double(kw.get("R1", 3.0)), C.c_uint64(kw.get("seed", 12345)),
                                      C.c_int64(row_begin), C.c_int64(row_end), C.byref(A), None); B = None
    else:
        raise ValueError(kind)
    if rc != 0:
        raise RuntimeError("problem generator failed rc=%d" % rc)
    return A, B


def ball_geometry(size, row_begin=0, row_end=-1):
    """box index x + G (y + G z) of every row of the ball matrix make_problem("sio2ball", size) (numpy int32 array)."""
    import numpy as np
    h = host_lib()
    A = CSR()
    bp = C.POINTER(C.c_int)()
    rc = h.gcge_problem_sio2_ball(C.c_int(size), C.c_int(0), C.c_double(1.0), C.c_double(0.0), C.c_uint64(1),
                                  C.c_int64(row_begin), C.c_int64(row_end), C.byref(A), C.byref(bp))
    if rc != 0:
        raise RuntimeError("gcge_problem_sio2_ball failed rc=%d" % rc)
    out = np.ctypeslib.as_array(bp, shape=(A.nrows,)).astype(np.int32).copy()
    h.gcge_free_ints(bp)
    h.gcge_csr_free(C.byref(A))
    return out


def make_argv(args):
    arr = (C.c_char_p * (len(args) + 1))()
    for i, a in enumerate(args):
        arr[i] = str(a).encode()
    return len(args), arr


def _solver_args(args, quiet):
    """(argc, argv, zeroed eigenvalue array of nevMax entries) of a GCGE_Run* call: -gcge_print_usage 0 appended when quiet,
    nevMax from -nevMax, else twice -nevConv (30 when absent)."""
    import numpy as np
    args = ["gcge"] + [str(a) for a in args]
    if quiet and "-gcge_print_usage" not in args:
        args += ["-gcge_print_usage", "0"]
    nev, nev_max = 30, None
    for i, a in enumerate(args):
        if a == "-nevConv":
            nev = int(args[i + 1])
        if a == "-nevMax":
            nev_max = int(args[i + 1])
    return make_argv(args) + (np.zeros(nev_max or 2 * nev),)


def run_gcg(ops, matA, matB, args, flag=0, quiet=True, keep_evec=False, given=None):
    """GCGE_RunGCG through the operator table `ops` (a void* OPS handle).
    keep_evec: also return the eigenvector multivector handle (nevMax columns; the caller destroys it).
    given = (multivector handle with nevMax columns, nevGiven): warm start from its first nevGiven columns
    (GCGE_RunGCGGiven); the eigenvectors come back in the same block, which stays the caller's."""
    h = host_lib()
    argc, argv, ev = _solver_args(args, quiet)
    res = RunResult()
    evec = C.c_void_p()
    if given is not None:
        rc = h.GCGE_RunGCGGiven(matA, matB, flag, argc, C.cast(argv, C.c_void_p), ops,
                                ev.ctypes.data_as(C.c_void_p), given[0], int(given[1]), C.cast(C.byref(res), C.c_void_p))
        if rc != 0:
            raise RuntimeError("GCGE_RunGCGGiven rc=%d" % rc)
        return ev, res
    rc = h.GCGE_RunGCG(matA, matB, flag, argc, argv, ops,
                       ev.ctypes.data_as(C.POINTER(C.c_double)), C.byref(evec) if keep_evec else None, C.byref(res))
    if rc != 0:
        raise RuntimeError("GCGE_RunGCG rc=%d" % rc)
    if keep_evec:
        return ev, res, evec
    return ev, res


class ChFSIResult(C.Structure):
    """GCGE_CHFSI_RESULT (include/gcge_solver.h)."""
    _fields_ = [("nevConv", C.c_int), ("numIter", C.c_int), ("degree", C.c_int), ("seconds", C.c_double), ("lower", C.c_double),
                ("upper", C.c_double)]


def run_chfsi(ops, matA, args, evec, given=0, quiet=True):
    """GCGE_RunChFSI (Chebyshev-filtered subspace iteration, standard problem) through the operator table `ops`: `evec` is the
    caller's block of nevMax columns whose first `given` columns are start vectors; the eigenvectors come back in it.  Returns
    (eval of nevMax entries, ChFSIResult, return code) — the code is 0 for a completed run, converged or not."""
    h = host_lib()
    argc, argv, ev = _solver_args(args, quiet)
    res = ChFSIResult()
    rc = h.GCGE_RunChFSI(matA, argc, C.cast(argv, C.c_void_p), ops, ev.ctypes.data_as(C.c_void_p), evec, int(given),
                         C.cast(C.byref(res), C.c_void_p))
    return ev, res, rc


class ChFSIBandResult(C.Structure):
    """GCGE_CHFSI_BAND_RESULT (include/gcge_solver.h)."""
    _fields_ = [("nevConv", C.c_int), ("numIter", C.c_int), ("degree", C.c_int), ("spurious", C.c_int), ("converged", C.c_int),
                ("seconds", C.c_double), ("lmin", C.c_double), ("lmax", C.c_double), ("edge", C.c_double)]


def run_chfsi_band(ops, matA, args, evec, given=0, quiet=True):
    """GCGE_RunChFSIBand (every eigenpair inside [-chfsi_band_lo, -chfsi_band_hi]) through the operator table `ops`: `evec` is the
    caller's block of -nevMax columns whose first `given` columns are start vectors; the pairs inside the interval come back in its
    first res.nevConv columns, ascending.  Returns (eval of nevMax entries, ChFSIBandResult, return code) — the code is 0 for a
    completed run (res.converged says whether the test passed), -6 for a block that is too small."""
    h = host_lib()
    argc, argv, ev = _solver_args(args, quiet)
    res = ChFSIBandResult()
    rc = h.GCGE_RunChFSIBand(matA, argc, C.cast(argv, C.c_void_p), ops, ev.ctypes.data_as(C.c_void_p), evec, int(given),
                             C.cast(C.byref(res), C.c_void_p))
    return ev, res, rc


def band_coefficients(degree, a, b, lmin, lmax):
    """GCGE_ChebBandCoefficients: the degree + 1 coefficients of the band filter as a numpy array; ValueError when it refuses."""
    import numpy as np
    mu = np.zeros(max(int(degree), 0) + 1)
    if host_lib().GCGE_ChebBandCoefficients(int(degree), float(a), float(b), float(lmin), float(lmax), mu.ctypes.data_as(C.c_void_p)) != 0:
        raise ValueError("band_coefficients: lmin < lmax, a < b, [a, b] meeting [lmin, lmax] and degree >= 2 are required")
    return mu


def cheb_stats():
    """gcge_hip_cheb_stats: (Chebyshev steps taken fused, steps taken as product + sweep, calls declined) since the library was loaded."""
    out = (C.c_long * 3)()
    hip_lib().gcge_hip_cheb_stats(out)
    return tuple(out)


def cheb_accum_stats():
    """gcge_hip_cheb_accum_stats: (two-term sums of a band filter taken in one sweep, one-term sums, calls declined) since the library
    was loaded."""
    out = (C.c_long * 3)()
    hip_lib().gcge_hip_cheb_accum_stats(out)
    return tuple(out)


def cheb_step_dots_stats():
    """gcge_hip_cheb_step_dots_stats: (steps with sums taken fused, taken as product + sweep, calls declined) since the library was
    loaded."""
    out = (C.c_long * 3)()
    hip_lib().gcge_hip_cheb_step_dots_stats(out)
    return tuple(out)


def count_from_moments(moments, lower_bound, upper_bound, interval):
    """GCGE_ChebCountFromMoments on a (degree + 1, m) numpy array of Chebyshev moments taken over [lower_bound, upper_bound]:
    (count, stderr, per_probe) for interval = (a, b); ValueError when the library refuses (degree < 2, a >= b, lower_bound >=
    upper_bound, an interval that misses the bounds)."""
    import numpy as np
    mom = np.ascontiguousarray(moments, dtype=np.float64)
    if mom.ndim != 2 or mom.shape[0] < 3 or mom.shape[1] < 1:
        raise ValueError("count_from_moments: a (degree + 1, m) array with degree >= 2 and m >= 1 is required")
    a, b = (float(v) for v in interval)
    count, err, per = C.c_double(), C.c_double(), np.zeros(mom.shape[1])
    rc = host_lib().GCGE_ChebCountFromMoments(mom.ctypes.data_as(C.c_void_p), mom.shape[1], mom.shape[0] - 1, a, b, float(lower_bound),
                                              float(upper_bound), C.cast(C.byref(count), C.c_void_p), C.cast(C.byref(err), C.c_void_p),
                                              per.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise ValueError("count_from_moments: a < b, lower_bound < upper_bound and an interval that meets the bounds are required")
    return count.value, err.value, per


def run_pas(ops, matA, matB, args, flag=0, quiet=True, keep_evec=False):
    """GCGE_RunPAS through the operator table `ops`: PAS (the multigrid eigensolver over the back-end's hierarchy), then GCG
    warm-started from PAS's converged vectors unless args hold -gcge_pas_only 1.  Returns (eval, pas_result, gcg_result)
    (and the eigenvector block handle, nevMax columns, with keep_evec: the caller destroys it).  Raises on an error code
    (-7: no MultiGridCreate or fewer than 2 levels, -8: a re-ordered level, -9: B is None and the back-end has no identity)."""
    h = host_lib()
    argc, argv, ev = _solver_args(args, quiet)
    res = PASResult()
    evec = C.c_void_p()
    rc = h.GCGE_RunPAS(matA, matB, flag, argc, argv, ops, ev.ctypes.data_as(C.POINTER(C.c_double)),
                       C.cast(C.byref(evec), C.c_void_p) if keep_evec else None, C.byref(res))
    if rc != 0:
        raise RuntimeError("GCGE_RunPAS rc=%d" % rc)
    if keep_evec:
        return ev, res, res.gcg, evec
    return ev, res, res.gcg


class HipBackend:
    """Placeholder filled in by gcge_amd/hip_backend.py once the HIP library is loaded."""
    def __init__(self, *a, **k):
        from .hip_backend import HipBackendImpl
        self.__class__ = HipBackendImpl
        HipBackendImpl.__init__(self, *a, **k)
