"""The entry map of a re-ordered matrix handle (gcge_hip_reorder_entry_map: the routine gcge_hip_mat_create re-orders with,
csrc/hip/mat_upload.hip "row orders", on the caller's arrays; host only): P A P^T as CSR with ascending columns, and emap[q] = the index
in the caller's arrays of the entry at position q of the re-ordered ones — what gcge_hip_mat_update_values_device gathers through
(tests/test_mat_update_reordered.py runs that on the GPU).  Against scipy's S[p][:, p] on four structures, each under a random perm."""
import ctypes as C

import numpy as np
import pytest

from gcge_amd.lib import csr_to_scipy, hip_lib, make_problem

IP = C.POINTER(C.c_int)


def permuted(kind, size, pseed, **kw):
    """(the pattern of tests/test_reorder.py::permuted: a generator's matrix in a random numbering)"""
    import scipy.sparse as sp
    A, B = make_problem(kind, size, **kw)
    S = csr_to_scipy(A).tocsr()
    p = np.random.default_rng(pseed).permutation(S.shape[0])
    Sp = sp.csr_matrix(S[p][:, p])
    Sp.sort_indices()
    return Sp


def empty_and_single():
    """9 rows: row 2 empty, row 5 one entry (off the diagonal), row 7 the diagonal alone, the others 2 .. 4 entries"""
    import scipy.sparse as sp
    rows = [0, 0, 1, 1, 1, 3, 3, 3, 3, 4, 4, 5, 6, 6, 6, 7, 8, 8]
    cols = [0, 3, 1, 4, 8, 0, 3, 6, 8, 1, 4, 2, 3, 6, 7, 7, 1, 8]
    S = sp.csr_matrix((np.arange(1.0, len(rows) + 1.0), (rows, cols)), shape=(9, 9))
    S.sort_indices()
    assert S.nnz == len(rows) and np.diff(S.indptr)[2] == 0 and np.diff(S.indptr)[5] == 1
    return S


def inputs():
    from test_mat_update import random300
    return {"lap3d6_permuted": lambda: permuted("lap3d", 6, 3), "fe3d5_permuted": lambda: permuted("fe3d", 5, 4), "random300": random300,
            "empty_and_single": empty_and_single}


def entry_map(S, p):
    g = hip_lib()
    n = S.shape[0]
    rp, ci = np.ascontiguousarray(S.indptr, dtype=np.int32), np.ascontiguousarray(S.indices, dtype=np.int32)
    p = np.ascontiguousarray(p, dtype=np.int32)
    rp_new, ci_new, emap = np.full(n + 1, -7, dtype=np.int32), np.full(max(S.nnz, 1), -7, dtype=np.int32), np.full(max(S.nnz, 1), -7, dtype=np.int32)
    rc = g.gcge_hip_reorder_entry_map(n, rp.ctypes.data_as(IP), ci.ctypes.data_as(IP), p.ctypes.data_as(IP), rp_new.ctypes.data_as(IP),
                                      ci_new.ctypes.data_as(IP), emap.ctypes.data_as(IP))
    return rc, rp_new, ci_new[:S.nnz], emap[:S.nnz]


@pytest.mark.parametrize("name", ["lap3d6_permuted", "fe3d5_permuted", "random300", "empty_and_single"])
def test_entry_map_reproduces_the_permuted_matrix(name):
    import scipy.sparse as sp
    S = inputs()[name]().tocsr()
    S.sort_indices()
    n = S.shape[0]
    rng = np.random.default_rng(100 + n)
    p = rng.permutation(n)
    assert not np.array_equal(p, np.arange(n))
    want = sp.csr_matrix(S[p][:, p])
    want.sort_indices()
    rc, rp_new, ci_new, emap = entry_map(S, p)
    assert rc == 0
    assert np.array_equal(rp_new, want.indptr) and np.array_equal(ci_new, want.indices)
    assert np.array_equal(np.sort(emap), np.arange(S.nnz))               # a permutation of the entries
    assert np.array_equal(S.data[emap].view(np.uint64), want.data.view(np.uint64))      # the creation values ...
    val = rng.standard_normal(S.nnz)                                     # ... and any others on the same structure
    T = S.copy()
    T.data = val
    Tp = sp.csr_matrix(T[p][:, p])
    Tp.sort_indices()
    assert np.array_equal(Tp.indices, want.indices) and np.array_equal(val[emap], Tp.data)
    # the sources of a re-ordered row are one row of the caller's arrays
    for i in (0, n // 2, n - 1):
        src = np.sort(emap[rp_new[i]:rp_new[i + 1]])
        assert np.array_equal(src, np.arange(S.indptr[p[i]], S.indptr[p[i] + 1]))


def test_identity_order_maps_every_entry_to_itself():
    S = inputs()["random300"]()
    rc, rp_new, ci_new, emap = entry_map(S, np.arange(S.shape[0]))
    assert rc == 0 and np.array_equal(rp_new, S.indptr) and np.array_equal(ci_new, S.indices) and np.array_equal(emap, np.arange(S.nnz))


def test_no_rows_and_no_permutation():
    g = hip_lib()
    rp_new = np.full(1, -7, dtype=np.int32)
    zero = np.zeros(1, dtype=np.int32)
    assert g.gcge_hip_reorder_entry_map(0, zero.ctypes.data_as(IP), None, None, rp_new.ctypes.data_as(IP), None, None) == 0      # n = 0 returns cleanly
    assert rp_new[0] == 0
    S = empty_and_single()
    for bad in ([0, 1, 2, 3, 4, 5, 6, 7, 7], [0, 1, 2, 3, 4, 5, 6, 7, 9], [-1, 1, 2, 3, 4, 5, 6, 7, 8]):
        rc, rp_new, ci_new, emap = entry_map(S, np.array(bad))
        assert rc == -1 and np.all(ci_new == -7) and np.all(emap == -7)  # refused before anything is written
