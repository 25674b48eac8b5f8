"""Row slabs of the matrices of tests/test_mat_update_forms.py with LOCAL columns, for tests/test_mat_update_slab.py and its GPU worker
(tests/slab_update_worker.py): the rows [a, b) of the global matrix, columns renamed the way gcge_dist_localize does it (own columns
c - a, halo columns n_loc + their rank among the ascending global halo rows; the ENTRY ORDER stays the caller's), the entry masks of
test_mat_update_forms.case cut to the slab, and the two value sets of its real_values."""
import ctypes as C

import numpy as np

ip_, dp_ = C.POINTER(C.c_int), C.POINTER(C.c_double)
G = 24


class Slab:
    pass


def slab_of(c, a, b):
    """c: a test_mat_update_forms.Case (global matrix, sorted CSR); rows [a, b)"""
    S = c.S
    s = Slab()
    q0, q1 = int(S.indptr[a]), int(S.indptr[b])
    s.a, s.b, s.n_loc, s.n_global, s.sel = a, b, b - a, S.shape[0], slice(q0, q1)
    s.rp = np.ascontiguousarray(S.indptr[a:b + 1] - q0, dtype=np.int32)
    gcol = S.indices[q0:q1].astype(np.int64)
    own = (gcol >= a) & (gcol < b)
    s.ghosts = np.ascontiguousarray(np.unique(gcol[~own]), dtype=np.int32)
    s.ci = np.ascontiguousarray(np.where(own, gcol - a, s.n_loc + np.searchsorted(s.ghosts, gcol)), dtype=np.int32)
    s.gcol = gcol
    s.ncols = s.n_loc + int(s.ghosts.size)
    s.pinned, s.diag, s.free = c.pinned[q0:q1], c.diag[q0:q1], c.free[q0:q1]
    s.box_local = None
    if c.box is not None:
        s.box_local = np.ascontiguousarray(np.concatenate([c.box[a:b], c.box[s.ghosts]]), dtype=np.int32)
    s.dims = c.dims
    return s


def values(c, s, step):
    from test_mat_update_forms import real_values
    return np.ascontiguousarray(real_values(c, step)[s.sel], dtype=np.float64)


def scipy_rows(s, v):
    """the slab's rows with GLOBAL columns and the values v"""
    import scipy.sparse as sp
    return sp.csr_matrix((v, s.gcol, s.rp.astype(np.int64)), shape=(s.n_loc, s.n_global))


def plane_partitions():
    """three plane-aligned slabs of the 24^3 grid, then the same with one odd cut"""
    plane = G * G
    return [[0, 8 * plane, 16 * plane, 24 * plane], [0, 7 * plane, 16 * plane, 24 * plane]]
