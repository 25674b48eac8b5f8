"""Python handle on the HIP back-end (libgcge_hip.so).  Plumbing only."""
import contextlib
import ctypes as C

import numpy as np

from .lib import host_lib, hip_lib
from .ops_struct import OpsTable


class HipBackendImpl:
    def __init__(self, device=0, quiet=True):
        self.h = host_lib()
        self.g = hip_lib()
        self.device = device
        if self.g.gcge_hip_init(device) != 0:
            raise RuntimeError("HIP back-end: no GPU visible (there is no CPU fallback)")
        self.ops_handle = C.c_void_p()
        self.h.OPS_Create(C.byref(self.ops_handle))
        self.g.OPS_HIP_Set(self.ops_handle)
        self.h.OPS_Setup(self.ops_handle)
        self.h.GCGE_SetQuiet(self.ops_handle, 1 if quiet else 0)
        self.ops = OpsTable(self.ops_handle)

    def torch_device(self):
        """The torch device this back-end runs on (torch's current one when it was opened with device < 0)."""
        import torch
        return torch.device("cuda", self.device if self.device >= 0 else torch.cuda.current_device())

    @contextlib.contextmanager
    def _keeping_value_maps(self, updatable):
        """gcge_hip_mat_keep_value_maps(1) around one creation (the switch is process-wide and off by default); afterwards the setting
        that was in force before is back"""
        if not updatable:
            yield
            return
        was = self.g.gcge_hip_mat_keep_value_maps(1)
        try:
            yield
        finally:
            self.g.gcge_hip_mat_keep_value_maps(was)

    def matrix(self, csr, updatable=False):
        """updatable=True: a handle that takes the star or the dense form also keeps where its stored values came from (about 4 bytes
        per block and remainder slot on the device, gcge_hip_mat_value_maps), so that matrix_update_values can give it new values in
        place; without it such a handle declines every update.  The forms and the products are the same either way.  A handle that
        re-orders its rows keeps, under the same switch, which of the caller's entries sits at each of its own positions (4 bytes
        per entry, gcge_hip_mat_entry_map), and declines every update without it."""
        with self._keeping_value_maps(updatable):
            m = self.g.gcge_hip_mat_create_csr(C.byref(csr))
        if not m:
            raise RuntimeError("gcge_hip_mat_create_csr failed")
        return C.c_void_p(m)

    def matrix_from_device(self, crow, col=None, val=None, nrows=None, updatable=False):
        """A whole square matrix from CSR arrays that live on the GPU (gcge_hip_mat_create_device): a torch sparse_csr tensor alone,
        three torch device tensors, or three objects with __cuda_array_interface__ (row pointers, ascending columns, values).
        Indices are converted to int32 and values to float64 on the device where needed; the producer's stream is synchronised
        before the call (torch's current stream for tensors, the whole device for other objects); the handle owns copies and
        nothing of the caller's is kept.  updatable: as for HipBackend.matrix.  ValueError: the arrays are not a matrix (the library
        says why on stderr)."""
        import torch
        if col is None and val is None:
            if not (isinstance(crow, torch.Tensor) and crow.layout == torch.sparse_csr):
                raise TypeError("matrix_from_device: one argument must be a torch sparse_csr tensor")
            if crow.dim() != 2 or crow.shape[0] != crow.shape[1]:
                raise ValueError("matrix_from_device: a square matrix is required")
            nrows = crow.shape[0]
            crow, col, val = crow.crow_indices(), crow.col_indices(), crow.values()
        elif col is None or val is None:
            raise TypeError("matrix_from_device: row pointers, columns and values are required")
        foreign = not all(isinstance(t, torch.Tensor) for t in (crow, col, val))
        dev = self.torch_device()

        def on_device(t, dtype):
            if not isinstance(t, torch.Tensor):
                if not hasattr(t, "__cuda_array_interface__"):
                    raise TypeError("matrix_from_device: torch device tensors or objects with __cuda_array_interface__ are required")
                t = torch.as_tensor(t, device=dev)
            if not t.is_cuda:
                raise TypeError("matrix_from_device: the arrays must live on the GPU (HipBackend.matrix takes host arrays)")
            return t.reshape(-1).to(dtype=dtype).contiguous()

        rp, ci, va = on_device(crow, torch.int32), on_device(col, torch.int32), on_device(val, torch.float64)
        if nrows is None:
            nrows = rp.numel() - 1
        if rp.numel() != nrows + 1 or ci.numel() != va.numel():
            raise ValueError("matrix_from_device: nrows + 1 row pointers and as many columns as values are required")
        if foreign:
            torch.cuda.synchronize(rp.device)
        else:
            torch.cuda.current_stream(rp.device).synchronize()
        with self._keeping_value_maps(updatable):
            m = self.g.gcge_hip_mat_create_device(int(nrows), int(va.numel()), rp.data_ptr(), ci.data_ptr(), va.data_ptr())
        if not m:
            raise ValueError("gcge_hip_mat_create_device refused the arrays")
        return C.c_void_p(m)

    def matrix_update_values(self, m, values, agree=None):
        """New values for a live matrix handle, in place (gcge_hip_mat_update_values_device): `values` holds one value per stored
        entry of the CSR arrays the handle was created from, in their order — a torch CUDA tensor, the .values() of a sparse_csr
        tensor, or an object with __cuda_array_interface__.  Converted to float64 on the device only if it is something else; the
        producer's stream is synchronised before the call (torch's current stream for tensors, the whole device for other objects).
        True: every product through the handle is now that of the new values (its K1 form may have become a "+values" form).
        A handle with a star or a dense form (real-space Hamiltonians: a Laplacian star, a diagonal, atom blocks) takes new values
        when it was created with updatable=True: the diagonal and every entry the star does not carry may change, the star's
        coefficients stay (an entry that equalled its coefficient at creation must keep it).
        A handle that re-ordered its rows (a matrix that shows no grid in the numbering it arrives in) takes new values when it was
        created with updatable=True as well: it then keeps which of the caller's entries sits where (4 bytes per entry on the
        device), `values` stays in the CALLER's entry order, and the call gathers it through a transient block of 8 bytes per entry.
        A row slab (gcge_amd.dist.hip_slab_matrix, NativeComm.slab_matrix, lap3d_slab; updatable=True there for star and dense
        slabs) takes new values the same way: one value per entry of the slab's own CSR arrays, in their order.  The library call
        is rank-local and collective-free, so its answer is this rank's alone; agree=comm (a gcge_amd.dist.Comm or NativeComm:
        anything with allreduce_sum_host) makes the returned bool the AND over the ranks by one all-reduce every rank reaches.  If
        it is False, EVERY rank frees its slab and creates it again (a rank that accepted holds the new values, one that declined
        the old ones; creation is collective).
        False: the library declined and wrote nothing (a star / dense handle or a re-ordered handle created without updatable=True,
        other star coefficients or a NaN diagonal, tile forms, a 16-slot table whose classes do not stay uniform, an
        explicitly stored zero) — or, with agree=, some rank's did: free the handle and create the matrix again.
        TypeError: a host tensor; ValueError: another count of values than the handle has entries (checked here)."""
        import torch
        foreign = not isinstance(values, torch.Tensor)
        if foreign:
            if not hasattr(values, "__cuda_array_interface__"):
                raise TypeError("matrix_update_values: a torch device tensor or an object with __cuda_array_interface__ is required")
            values = torch.as_tensor(values, device=self.torch_device())
        if not values.is_cuda:
            raise TypeError("matrix_update_values: the values must live on the GPU")
        nnz = int(self.g.gcge_hip_mat_nnz(m))
        if values.numel() != nnz:
            raise ValueError("matrix_update_values: %d values for a handle of %d entries" % (values.numel(), nnz))
        va = values.reshape(-1)
        if va.dtype != torch.float64:
            va = va.to(dtype=torch.float64)
        va = va.contiguous()
        if nnz == 0:
            va = torch.zeros(1, dtype=torch.float64, device=va.device)     # (the library wants an array)
        if foreign:
            torch.cuda.synchronize(va.device)
        else:
            torch.cuda.current_stream(va.device).synchronize()
        rc = self.g.gcge_hip_mat_update_values_device(m, nnz, va.data_ptr())
        if agree is not None:
            votes = np.array([1.0 if rc != 0 else 0.0])          # (before any exception: every rank reaches the all-reduce)
            agree.allreduce_sum_host(votes)
        if rc < 0:
            raise ValueError("gcge_hip_mat_update_values_device refused its arguments")
        return rc == 0 and (agree is None or float(votes[0]) == 0.0)

    def multigrid(self, A, M=None, levels=6, block_size=8, cycles=1, smooth0=5, smooth=4, rate=1e-2, refreshable=True):
        """A BlockAMG hierarchy over the matrix handle A (and M), kept by the caller across solves (GCGE_AMGCreate): at most `levels`
        levels, work blocks of `block_size` columns per level, `cycles` V-cycles of smooth0 (level 0) / smooth (coarse levels) CG
        iterations, level 0 smoothed to `rate`.  eigsh(A, k, M, amg=h) solves its W systems with it.  refreshable=True creates the
        coarse levels with their value maps kept (as updatable=True does for a matrix), so that Hierarchy.refresh() can give a coarse
        level with a star or dense form new values in place; the hierarchy and its products are the same either way.  The handles stay
        the caller's and must outlive the hierarchy."""
        return Hierarchy(self, A, M, int(levels), int(block_size), int(cycles), int(smooth0), int(smooth), float(rate), bool(refreshable))

    def linear_solver(self, A, amg=None, max_cols=8):
        """A LinearSolver for A X = B on the matrix handle A with up to `max_cols` right-hand sides per solve (GCGE_PCGCreate): flexible
        block CG preconditioned by one V-cycle of the Hierarchy `amg` (HipBackend.multigrid, built on A), or with amg=None the fused
        block CG alone.  The handle and the hierarchy stay the caller's and must outlive the solver; new values in the handle
        (matrix_update_values, then amg.refresh()) need no new solver.  ValueError: amg was built on another handle or belongs to
        another back-end."""
        return LinearSolver(self, A, amg, int(max_cols))

    def mv_to_torch(self, mv, c0, c1):
        """Columns [c0, c1) of a block of vectors as a new (n, c1 - c0) float64 tensor on the GPU, rows in the caller's order
        (gcge_hip_mv_to_device): nothing passes through the host."""
        import torch
        n = self.g.gcge_hip_mv_nrows(mv)
        out = torch.empty((n, c1 - c0), dtype=torch.float64, device=self.torch_device())
        if out.numel():
            self.g.gcge_hip_mv_to_device(mv, c0, c1, out.data_ptr(), c1 - c0)
        return out

    def mv_from_torch(self, mat, t, mv=None, c0=0):
        """Columns of a block of vectors from an (n, m) tensor that lives on the GPU (gcge_hip_mv_from_device): a 2-D CUDA tensor or
        an object with __cuda_array_interface__, rows in the caller's order.  With mv=None a new block of m columns is created for
        `mat` and returned; otherwise columns [c0, c0 + m) of `mv` are written and `mv` is returned.  The tensor is converted to
        float64 on the device only if it is something else and is NOT made contiguous: its two strides go to the library as they are
        (rows contiguous: the block-stream kernel; columns contiguous: the LDS transpose) unless two of its
        entries alias (an expanded tensor), which costs one contiguous copy.  The producer's stream is synchronised before the call
        (torch's current stream for tensors, the whole device for other objects).  TypeError: a host tensor; ValueError: another
        row count, a column range outside the block, a tensor that overlaps the block."""
        import torch
        foreign = not isinstance(t, torch.Tensor)
        if foreign:
            if not hasattr(t, "__cuda_array_interface__"):
                raise TypeError("mv_from_torch: a torch device tensor or an object with __cuda_array_interface__ is required")
            t = torch.as_tensor(t, device=self.torch_device())
        if not t.is_cuda:
            raise TypeError("mv_from_torch: the tensor must live on the GPU (HipBackend.mv_from_numpy takes host arrays)")
        if t.dim() != 2:
            raise ValueError("mv_from_torch: an (n, m) tensor is required")
        n, m = int(t.shape[0]), int(t.shape[1])
        c0 = int(c0)
        if mv is None:
            if c0 != 0:
                raise ValueError("mv_from_torch: a new block is written from column 0")
            if n != self.g.gcge_hip_mat_nrows(mat):
                raise ValueError("mv_from_torch: the tensor has %d rows, the matrix %d" % (n, self.g.gcge_hip_mat_nrows(mat)))
        else:
            if n != self.g.gcge_hip_mv_nrows(mv):
                raise ValueError("mv_from_torch: the tensor has %d rows, the block %d" % (n, self.g.gcge_hip_mv_nrows(mv)))
            if c0 < 0 or c0 + m > self.g.gcge_hip_mv_ncols(mv):
                raise ValueError("mv_from_torch: columns [%d, %d) are outside the block's %d" % (c0, c0 + m, self.g.gcge_hip_mv_ncols(mv)))
        if t.dtype != torch.float64:
            t = t.to(dtype=torch.float64)
        if n and m:
            rs, cs = (int(v) for v in t.stride())
            if not (rs >= 1 and cs >= 1 and ((cs == 1 and rs >= m) or (rs == 1 and cs >= n) or rs >= m * cs or cs >= n * rs)):
                t = t.contiguous()
                rs, cs = m, 1
            if mv is not None:
                ld = C.c_long()
                b0 = self.g.gcge_hip_mv_device_ptr(mv, C.byref(ld)) or 0
                b1 = b0 + 8 * ld.value * n
                s0 = t.data_ptr()
                s1 = s0 + 8 * ((n - 1) * rs + (m - 1) * cs + 1)
                if s0 < b1 and b0 < s1:
                    raise ValueError("mv_from_torch: the tensor overlaps the block it is written to")
        created = mv is None
        if created:
            mv = self.ops.mv_create(m, mat)
        if n and m:
            if foreign:
                torch.cuda.synchronize(t.device)
            else:
                torch.cuda.current_stream(t.device).synchronize()
            self.g.gcge_hip_mv_from_device(mv, c0, c0 + m, t.data_ptr(), rs, cs)
        return mv

    def chebyshev_filter(self, A, X, degree, lower, upper, lowest):
        """p(A) X for the matrix handle A and an (n, m) device tensor X, as a new (n, m) float64 tensor (GCGE_ChebFilter): p is the
        Chebyshev polynomial of the given degree scaled to 1 at `lowest` and bounded by 1 on [lower, upper] — the components of X along
        eigenvectors with eigenvalues in [lower, upper] are damped relative to those below `lower`.  X goes in through mv_from_torch
        and out through mv_to_torch; the two work blocks are created and freed here.  Every step is the back-end's cheb_step (fused
        into one sweep on matrices whose product it can rebuild there, product + one sweep otherwise; lib.cheb_stats counts them).
        ValueError: degree < 1, lower >= upper, lowest >= lower."""
        if int(degree) < 1 or not float(lower) < float(upper) or not float(lowest) < float(lower):
            raise ValueError("chebyshev_filter: degree >= 1 and lowest < lower < upper are required")
        mx = self.mv_from_torch(A, X)
        m = self.g.gcge_hip_mv_ncols(mx)
        w1 = w2 = None
        try:
            if m == 0:
                return self.mv_to_torch(mx, 0, 0)
            w1, w2 = self.ops.mv_create(m, A), self.ops.mv_create(m, A)
            rc = self.h.GCGE_ChebFilter(A, mx, 0, m, int(degree), float(lower), float(upper), float(lowest), w1, w2, self.ops_handle)
            if rc != 0:
                raise RuntimeError("GCGE_ChebFilter rc=%d" % rc)
            return self.mv_to_torch(mx, 0, m)
        finally:
            for w in (w1, w2, mx):
                if w is not None:
                    self.ops.mv_destroy(w, m)

    def chebyshev_band_filter(self, A, X, degree, a, b, lmin, lmax):
        """p(A) X for the matrix handle A and an (n, m) device tensor X, as a new (n, m) float64 tensor (GCGE_ChebBandFilter): p is the
        Jackson-damped Chebyshev expansion of the given degree of the indicator of [a, b] over the bounds [lmin, lmax] of A's spectrum
        — about 1 inside the interval, about 0 outside, 1/2 at its ends (lib.band_coefficients gives its coefficients).  X goes in
        through mv_from_torch and out through mv_to_torch; the two work blocks and the accumulator are created and freed here.
        Every step is the back-end's cheb_step, every sum of a pair of iterates its cheb_accum (one sweep; lib.cheb_stats and
        lib.cheb_accum_stats count them).  ValueError: degree < 2, a >= b, lmin >= lmax, an interval that misses the bounds."""
        degree, a, b, lmin, lmax = int(degree), float(a), float(b), float(lmin), float(lmax)
        if degree < 2 or not a < b or not lmin < lmax or not a <= lmax or not b >= lmin:
            raise ValueError("chebyshev_band_filter: degree >= 2, a < b, lmin < lmax and an interval [a, b] that meets [lmin, lmax] are required")
        mx = self.mv_from_torch(A, X)
        m = self.g.gcge_hip_mv_ncols(mx)
        w1 = w2 = acc = None
        try:
            if m == 0:
                return self.mv_to_torch(mx, 0, 0)
            w1, w2, acc = self.ops.mv_create(m, A), self.ops.mv_create(m, A), self.ops.mv_create(m, A)
            rc = self.h.GCGE_ChebBandFilter(A, mx, 0, m, degree, a, b, lmin, lmax, w1, w2, acc, self.ops_handle)
            if rc != 0:
                raise RuntimeError("GCGE_ChebBandFilter rc=%d" % rc)
            return self.mv_to_torch(mx, 0, m)
        finally:
            for w in (w1, w2, acc, mx):
                if w is not None:
                    self.ops.mv_destroy(w, m)

    def chebyshev_moments(self, A, V, degree, lmin, lmax):
        """The Chebyshev moments mu[j, col] = v_col^T T_j((A - c) / e) v_col, j = 0 .. degree, of the columns of an (n, m) device tensor V
        for the matrix handle A, c and e the centre and half width of the bounds [lmin, lmax] of A's spectrum, as a (degree + 1, m)
        float64 device tensor (GCGE_ChebMoments: ceil(degree / 2) steps of the recurrence, each ONE call of the back-end's
        cheb_step_dots, which returns the step's two inner products with it; lib.cheb_step_dots_stats counts them).  V goes in
        through mv_from_torch and is not changed; the three work blocks are created and freed here.  ValueError: degree < 1,
        lmin >= lmax, a V without columns."""
        import torch
        degree, lmin, lmax = int(degree), float(lmin), float(lmax)
        if degree < 1 or not lmin < lmax:
            raise ValueError("chebyshev_moments: degree >= 1 and lmin < lmax are required")
        if not hasattr(V, "shape") or len(V.shape) != 2 or int(V.shape[1]) < 1:
            raise ValueError("chebyshev_moments: V is an (n, m) block with m >= 1")
        mv = self.mv_from_torch(A, V)
        m = self.g.gcge_hip_mv_ncols(mv)
        work = []
        try:
            work = [self.ops.mv_create(m, A) for _ in range(3)]
            mom = np.zeros((degree + 1, m))
            rc = self.h.GCGE_ChebMoments(A, mv, 0, m, degree, lmin, lmax, work[0], work[1], work[2], mom.ctypes.data_as(C.c_void_p), self.ops_handle)
            if rc != 0:
                raise RuntimeError("GCGE_ChebMoments rc=%d" % rc)
            return torch.from_numpy(mom).to(self.torch_device())
        finally:
            for w in work + [mv]:
                self.ops.mv_destroy(w, m)

    def sample_outer(self, crow, col, U, V, weights=None, alpha=1.0):
        """The rank-k product U diag(weights) V^T on the stored entries of a CSR pattern (gcge_hip_csr_sample_outer): an (nnz,)
        float64 device tensor with out[e] = alpha sum_c weights[c] U[i, c] V[col[e], c] for every entry e of row i, in the entry order
        of `crow`, `col` — never in a handle's.  crow (n + 1), col (nnz): device index tensors, converted to int32 on the device if
        they are something else; U (n, k), V (rows for every column index, k): 2-D CUDA tensors, converted to float64 if they are
        something else, taken as they are when their rows are contiguous (any row stride >= k) and copied once otherwise; U and V
        may be the same tensor; weights: k values (None: all ones).  The producer's stream (torch's current one) is synchronised
        before the call, the kernel runs on the library's stream and has finished on return.  TypeError: a host tensor;
        ValueError: shapes that do not belong together."""
        import torch
        for name, t in (("crow", crow), ("col", col), ("U", U), ("V", V)) + ((("weights", weights),) if weights is not None else ()):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise TypeError("sample_outer: %s must be a torch tensor that lives on the GPU" % name)
        if U.dim() != 2 or V.dim() != 2 or U.shape[1] != V.shape[1] or U.shape[1] < 1:
            raise ValueError("sample_outer: U and V are (n, k) and (ncols, k) blocks of the same k >= 1 columns")
        n, k = int(U.shape[0]), int(U.shape[1])
        rp = crow.reshape(-1).to(dtype=torch.int32).contiguous()
        ci = col.reshape(-1).to(dtype=torch.int32).contiguous()
        if rp.numel() != n + 1:
            raise ValueError("sample_outer: %d row pointers for a U of %d rows" % (rp.numel(), n))
        if weights is not None and weights.numel() != k:
            raise ValueError("sample_outer: %d weights for %d columns" % (weights.numel(), k))

        def rows_contiguous(t):
            t = t.to(dtype=torch.float64)
            return t if t.stride(1) == 1 and (t.stride(0) >= k or t.shape[0] <= 1) else t.contiguous()

        Ud, Vd = rows_contiguous(U), rows_contiguous(V)
        w = weights.reshape(-1).to(dtype=torch.float64).contiguous() if weights is not None else None
        nnz = int(ci.numel())
        out = torch.empty(nnz, dtype=torch.float64, device=Ud.device)
        if n == 0 or nnz == 0:
            return out
        torch.cuda.current_stream(Ud.device).synchronize()
        rc = self.g.gcge_hip_csr_sample_outer(n, rp.data_ptr(), ci.data_ptr(), Ud.data_ptr(), max(int(Ud.stride(0)), k), Vd.data_ptr(),
                                              max(int(Vd.stride(0)), k), k, w.data_ptr() if w is not None else None, float(alpha),
                                              out.data_ptr(), self.g.gcge_hip_stream())
        self.sync()
        if rc != 0:
            raise RuntimeError("gcge_hip_csr_sample_outer rc=%d" % rc)
        return out

    def matrix_grid(self, csr, dims, box_of_row, updatable=False):
        """A matrix on a masked grid: box_of_row[r] = x + nx (y + ny z) (int32 array, ascending); see gcge_hip_mat_create_grid.
        updatable: as for HipBackend.matrix."""
        g = self.g
        box = np.ascontiguousarray(box_of_row, dtype=np.int32)
        with self._keeping_value_maps(updatable):
            m = g.gcge_hip_mat_create_grid(csr.nrows, csr.rowptr, csr.colidx, csr.val, int(dims[0]), int(dims[1]), int(dims[2]),
                                           box.ctypes.data_as(C.POINTER(C.c_int)))
        if not m:
            raise RuntimeError("gcge_hip_mat_create_grid failed")
        return C.c_void_p(m)

    def free_matrix(self, m):
        self.g.gcge_hip_mat_destroy(m)

    def matrix_rect(self, csr):
        """A rectangular matrix (a prolongation of a multigrid hierarchy): MatDotMultiVec applies it, MatTransDotMultiVec its
        transpose (gcge_hip_mat_create_rect_csr, csrc/hip/multigrid.hip)."""
        m = self.g.gcge_hip_mat_create_rect_csr(C.byref(csr))
        if not m:
            raise RuntimeError("gcge_hip_mat_create_rect_csr failed")
        return C.c_void_p(m)

    def free_matrix_rect(self, m):
        self.g.gcge_hip_mat_destroy(m)

    def mv_from_numpy(self, mat, arr):
        """arr: (n, ncols) array -> device multivector with the same columns."""
        a = np.asfortranarray(arr, dtype=np.float64)
        mv = self.ops.mv_create(a.shape[1], mat)
        self.g.gcge_hip_mv_from_host(mv, 0, a.shape[1], a.ctypes.data_as(C.POINTER(C.c_double)), a.shape[0])
        return mv

    def mv_to_numpy(self, mv, n, c0, c1):
        out = np.zeros((n, c1 - c0), order="F")
        self.g.gcge_hip_mv_to_host(mv, c0, c1, out.ctypes.data_as(C.POINTER(C.c_double)), n)
        return out

    def set_random_mode(self, mode, seed=12345):
        self.g.gcge_hip_set_random_mode(mode, seed)

    def sync(self):
        self.g.gcge_hip_sync()


class _AMGHead(C.Structure):
    """The leading fields of GCGE_AMG (include/gcge_solver.h)."""
    _fields_ = [("A_array", C.POINTER(C.c_void_p)), ("B_array", C.POINTER(C.c_void_p)), ("P_array", C.POINTER(C.c_void_p)),
                ("num_levels", C.c_int), ("block_size", C.c_int), ("own_smoother", C.c_int)]


class Hierarchy:
    """What HipBackend.multigrid returns: a live GCGE_AMG (hierarchy, work blocks, parameter arrays) over the handles A and M.
    .num_levels, .block_size, .A, .M; refresh() after the handles took new values in place; close() (or a with block) frees it."""

    def __init__(self, backend, A, M, levels, block_size, cycles, smooth0, smooth, rate, refreshable):
        if levels < 2 or block_size < 1:
            raise ValueError("multigrid: at least 2 levels and a block of at least 1 column are required")
        as_handle = lambda a: a if isinstance(a, C.c_void_p) or a is None else C.c_void_p(a)
        self.backend, self.A, self.M = backend, as_handle(A), as_handle(M)
        self._args = (levels, block_size, cycles, smooth0, smooth, rate)
        self._refreshable = refreshable
        self._graph_method = backend.h.gcge_mg_get_graph_method()
        self._amg = None
        self._create()

    def _create(self):
        b = self.backend
        before = b.h.gcge_mg_get_graph_method()
        b.h.gcge_mg_set_graph_method(self._graph_method)
        try:
            with b._keeping_value_maps(self._refreshable):
                amg = b.h.GCGE_AMGCreate(self.A, self.M, *self._args, b.ops_handle)
        finally:
            b.h.gcge_mg_set_graph_method(before)
        if not amg:
            raise RuntimeError("GCGE_AMGCreate failed")
        self._amg = C.c_void_p(amg)
        head = C.cast(self._amg, C.POINTER(_AMGHead)).contents
        self.num_levels, self.block_size = int(head.num_levels), int(head.block_size)

    def _head(self):
        if self._amg is None:
            raise ValueError("the hierarchy is closed")
        return C.cast(self._amg, C.POINTER(_AMGHead)).contents

    def level_handles(self):
        """(A handles of all levels, M handles of all levels ([] without M), P handles): the back-end's, valid until the next
        refresh() that returns False or close()."""
        h = self._head()
        L = h.num_levels
        Ah = [C.c_void_p(h.A_array[l]) for l in range(L)]
        Bh = [C.c_void_p(h.B_array[l]) for l in range(L)] if self.M is not None and h.B_array else []
        return Ah, Bh, [C.c_void_p(h.P_array[l]) for l in range(L - 1)]

    def refresh(self):
        """After A (and M) took new values in place (HipBackend.matrix_update_values): the coarse levels recomputed where they are
        (GCGE_AMGRefresh).  True: refreshed in place.  False: a level declined or the back-end wrote nothing — the hierarchy was
        destroyed and built again from the same handles and arguments.  Either way it now belongs to the present values.  A level 0
        that re-ordered its rows is refreshed like any other (it took its values in place only if created with updatable=True).
        A hierarchy of row slabs is refreshed the same way, every rank its own levels; GCGE_AMGRefresh agrees on the outcome over
        the communicator, so every rank gets the same answer here and the rebuild (collective) happens on all ranks or on none."""
        self._head()
        if self.backend.h.GCGE_AMGRefresh(self._amg, self.backend.ops_handle) == 0:
            return True
        self.close()
        self._create()
        return False

    def install(self):
        """BlockAMG over this hierarchy into the back-end's table (GCGE_AMGInstall): the solver of a harness run with flag 1."""
        self._head()
        self.backend.h.GCGE_AMGInstall(self._amg, self.backend.ops_handle)

    def close(self):
        if self._amg is not None:
            self.backend.h.GCGE_AMGDestroy(C.byref(self._amg), self.backend.ops_handle)
            self._amg = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


class LinearSolver:
    """What HipBackend.linear_solver returns: a live GCGE_PCG (include/gcge_solver.h) with its work blocks and a right-hand-side and a
    solution block of max_cols columns.  solve(b, ...) as often as wanted; close() (or a with block) frees it.  .column_iterations: the
    iteration count of every column of the last solve (numpy int32)."""

    def __init__(self, backend, A, amg, max_cols):
        as_handle = lambda a: a if isinstance(a, C.c_void_p) else C.c_void_p(a)
        if max_cols < 1:
            raise ValueError("linear_solver: at least one column is required")
        if amg is not None:
            if amg.backend is not backend:
                raise ValueError("linear_solver: amg belongs to another back-end")
            if as_handle(A).value != amg.A.value:
                raise ValueError("linear_solver: amg was not built on this matrix handle")
        self.backend, self.A, self.amg, self.max_cols = backend, as_handle(A), amg, max_cols
        self.n = int(backend.g.gcge_hip_mat_nrows(self.A))
        self._s = self._b = self._x = self._X = self.column_iterations = None
        self._X_cols = 0
        self._b = backend.ops.mv_create(max_cols, self.A)
        self._x = backend.ops.mv_create(max_cols, self.A)
        try:
            self._create()
        except Exception:
            self.close()
            raise

    def _create(self):
        b = self.backend
        if self._s is not None:
            b.h.GCGE_PCGDestroy(C.byref(self._s), b.ops_handle)
            self._s = None
        if self.amg is not None:
            self.amg._head()                                           # ValueError: the hierarchy is closed
        self._amg_ptr = self.amg._amg.value if self.amg is not None else None
        s = b.h.GCGE_PCGCreate(self.A, self.amg._amg if self.amg is not None else None, self.max_cols, b.ops_handle)
        if not s:
            raise RuntimeError("GCGE_PCGCreate failed")
        self._s = C.c_void_p(s)

    def _block(self, t, what):
        """(2-D device tensor, was 1-D) of a right-hand side or a start block"""
        import torch
        if not isinstance(t, torch.Tensor):
            if not hasattr(t, "__cuda_array_interface__"):
                raise TypeError("solve: %s must be a torch device tensor or an object with __cuda_array_interface__" % what)
            t = torch.as_tensor(t, device=self.backend.torch_device())
            torch.cuda.synchronize(t.device)                           # (a producer torch knows nothing of)
        if not t.is_cuda:
            raise TypeError("solve: %s must live on the GPU" % what)
        flat = t.dim() == 1
        if flat:
            t = t.reshape(-1, 1)
        if t.dim() != 2 or t.shape[1] < 1:
            raise ValueError("solve: %s is an (n, m) or (n,) block" % what)
        if t.shape[0] != self.n:
            raise ValueError("solve: %s has %d rows, the matrix %d" % (what, t.shape[0], self.n))
        if t.shape[1] > self.max_cols:
            raise ValueError("solve: %d columns, the solver was created for %d" % (t.shape[1], self.max_cols))
        return t, flat

    def solve(self, b, x0=None, tol=1e-8, maxiter=200):
        """A X = b to the relative residual |b_j - A x_j| <= tol |b_j| in every column, within `maxiter` outer iterations (V-cycles per
        column; without a hierarchy: iterations of the block CG).  b: an (n, m) or (n,) CUDA tensor or an object with
        __cuda_array_interface__, m <= max_cols, rows in the caller's order, any strides (mv_from_torch); x0: likewise, or None for a
        zero start.  Returns SolveResult(x, converged, iterations, residual_norms, seconds): x a float64 device tensor of b's shape,
        converged a bool tensor per column, iterations the largest count of any column, residual_norms the TRUE relative residuals
        |b_j - A x_j| / |b_j| the library formed after its last step.  Raises gcge_amd.NoConvergence, carrying that result, when a
        column did not converge.  TypeError: a host tensor; ValueError: another row count, more than max_cols columns, x0 of
        another shape than b.
        When b is a tensor that requires grad and grad mode is on, x comes back attached to the graph: backward solves
        A Z = d loss / d x with this solver, the same tol and maxiter (NoConvergence when that solve does not converge), and Z is
        the gradient with respect to b.  The solver must then be open when backward runs.  Double backward raises."""
        import torch
        if isinstance(b, torch.Tensor) and b.requires_grad and torch.is_grad_enabled():
            from .grad import _solve_attached
            return _solve_attached(self, b, x0, tol, maxiter)
        return self._solve(b, x0, tol, maxiter)

    def solve_deflated(self, b, X, shifts, M=None, tol=1e-8, maxiter=200):
        """The deflated, per-column-shifted systems  Q^T (A - shifts[j] M) y_j = Q^T b_j,  y_j in range(Q),  Q = I - X X^T M
        (GCGE_PCGSolveDeflated): the adjoint systems of eigenvector gradients, with X the (n, k) block of computed, M-orthonormal
        eigenvectors and shifts their eigenvalues.  b as for solve; X: an (n, k) CUDA tensor (k = 0: no deflation), copied into a
        block the solver keeps; shifts: m values (a tensor, an array or a sequence); M: a matrix handle of the back-end or None for
        the identity.  The preconditioner is the solver's V-cycle on A, unchanged (without a hierarchy: none).  The operator is
        positive definite on range(Q) while every shift is below the first eigenvalue that is not in X, and conditioned like the
        inverse of that gap.  Returns SolveResult as solve does, residual_norms the TRUE projected residuals
        |Q^T (b_j - (A - shifts[j] M) y_j)| / |Q^T b_j| (a b_j inside span(M X): y_j = 0, residual 0); raises NoConvergence carrying
        the result.  Nothing is attached to a graph.  TypeError / ValueError as solve, and ValueError for X of another row count or
        another number of shifts than columns."""
        import numpy as np
        import torch
        if self._s is None:
            raise ValueError("the solver is closed")
        bt, flat = self._block(b.detach() if isinstance(b, torch.Tensor) else b, "b")
        m = int(bt.shape[1])
        if not isinstance(X, torch.Tensor) or not X.is_cuda:
            raise TypeError("solve_deflated: X must be a torch tensor that lives on the GPU")
        if X.dim() != 2 or X.shape[0] != self.n:
            raise ValueError("solve_deflated: X is an (n, k) block with the matrix's %d rows" % self.n)
        sh = np.ascontiguousarray(shifts.detach().cpu().numpy() if isinstance(shifts, torch.Tensor) else shifts, dtype=np.float64).reshape(-1)
        if sh.size != m:
            raise ValueError("solve_deflated: %d shifts for %d columns" % (sh.size, m))
        k = int(X.shape[1])
        if k > self._X_cols:
            if self._X is not None:
                self.backend.ops.mv_destroy(self._X, self._X_cols)
            self._X, self._X_cols = self.backend.ops.mv_create(k, self.A), k
        if k > 0:
            self.backend.mv_from_torch(self.A, X.detach(), mv=self._X, c0=0)
        as_handle = lambda a: a if isinstance(a, C.c_void_p) or a is None else C.c_void_p(a)
        return self._solve(bt.reshape(-1) if flat else bt, None, tol, maxiter, deflation=(as_handle(M), k, sh))

    def _solve(self, b, x0, tol, maxiter, deflation=None):
        """solve on a detached b: see there; deflation = (M handle or None, k, shifts): GCGE_PCGSolveDeflated with the block _X"""
        import time
        import numpy as np
        import torch
        from .eigsh import NoConvergence
        from .solve import SolveResult
        if self._s is None:
            raise ValueError("the solver is closed")
        if self.amg is not None and self.amg._amg is None:
            raise ValueError("the hierarchy is closed")
        bk = self.backend
        bt, flat = self._block(b, "b")
        m = int(bt.shape[1])
        if x0 is not None:
            xt, _ = self._block(x0, "x0")
            if tuple(xt.shape) != tuple(bt.shape):
                raise ValueError("solve: x0 has another shape than b")
        if self.amg is not None and self.amg._amg.value != self._amg_ptr:   # refresh() built the hierarchy again
            self._create()
        bk.mv_from_torch(self.A, bt, mv=self._b, c0=0)
        if x0 is not None:
            bk.mv_from_torch(self.A, xt, mv=self._x, c0=0)
        rel, it = np.zeros(m), np.zeros(m, dtype=np.int32)
        bk.sync()
        t0 = time.perf_counter()
        tail = (self._b, 0, self._x, 0, m, float(tol), int(maxiter), 1 if x0 is None else 0, rel.ctypes.data_as(C.c_void_p),
                it.ctypes.data_as(C.c_void_p), bk.ops_handle)
        if deflation is None:
            name, rc = "GCGE_PCGSolve", bk.h.GCGE_PCGSolve(self._s, *tail)
        else:
            M, k, sh = deflation
            name, rc = "GCGE_PCGSolveDeflated", bk.h.GCGE_PCGSolveDeflated(self._s, M, self._X, 0, k, sh.ctypes.data_as(C.c_void_p), *tail)
        bk.sync()
        seconds = time.perf_counter() - t0
        self.column_iterations = it.copy()                             # per column: V-cycles (amg=None: the one call's count)
        if rc < 0:
            raise RuntimeError("%s rc=%d%s" % (name, rc, " (a communicator is set: single rank only)" if rc == -2 else ""))
        x = bk.mv_to_torch(self._x, 0, m)
        if flat:
            x = x.reshape(-1)
        result = SolveResult(x, torch.from_numpy(rel <= tol).to(x.device), int(it.max()), torch.from_numpy(rel).to(x.device), seconds)
        if rc < m:
            raise NoConvergence("solve: %d of %d columns converged in %d iterations" % (rc, m, result.iterations), result)
        return result

    def close(self):
        b = self.backend
        if self._s is not None:
            b.h.GCGE_PCGDestroy(C.byref(self._s), b.ops_handle)
            self._s = None
        for name, cols in (("_b", self.max_cols), ("_x", self.max_cols), ("_X", self._X_cols)):
            mv = getattr(self, name)
            if mv is not None and mv.value:
                b.ops.mv_destroy(mv, cols)
            setattr(self, name, None)
        self._X_cols = 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
