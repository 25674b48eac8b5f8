"""Matrices from device-resident CSR arrays (gcge_hip_mat_create_device, csrc/hip/mat_device.hip; HipBackend.matrix_from_device),
blocks out to device memory (gcge_hip_mv_to_device; HipBackend.mv_to_torch) and the hierarchy's coarse levels through the device
constructor (gcge_hip_multigrid_device_levels).

Every case creates the same arrays twice: H = hip.matrix(csr) on the host path, D = hip.matrix_from_device(...) from torch tensors made
by torch.from_numpy(...).cuda().  For a matrix the device search accepts, D's pattern table, pid, spans (through chain / form), row
order, CSR and products must equal H's bit for bit: part (b) of the search is the same host code for both (pattern_table.h), part (a)
— ids by first occurrence — is what the kernels have to reproduce.  Products use integer data of magnitude <= 3 on at most 16 entries
per row, so every sum is exact in any order and scipy on the same arrays is the reference where the matrix is integer-valued too.
No matrix here stores a zero on its diagonal (the one case in which the two searches differ by design: include/gcge_hip.h)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from gcge_amd.lib import (csr_arrays, csr_to_scipy, make_problem, mat_device_hash_bits, mat_device_stats, mat_pattern_table,
                          mat_to_csr, multigrid_device_levels, multigrid_graph_method, multigrid_stats, run_gcg)
from helpers import bits, csr_from_scipy, draw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (1, 7, 16, 64)


# ---- CPU: the public face -----------------------------------------------------------------------------------------------------------
def test_prototypes_are_public_and_lib_imports_without_torch():
    text = open(os.path.join(ROOT, "include", "gcge_hip.h")).read()
    assert re.search(r"GCGE_HIP_MAT \*gcge_hip_mat_create_device \(int nrows, long nnz, const int \*d_rowptr, const int \*d_colidx, const double \*d_val\);", text)
    assert re.search(r"void gcge_hip_mat_device_stats \(long out\[4\]\);", text)
    assert re.search(r"void gcge_hip_mv_to_device \(void \*\*mv, int c0, int c1, double \*d_out, long ldo\);", text)
    assert re.search(r"void gcge_hip_multigrid_device_levels \(int on\);", text)
    code = "import sys; import gcge_amd.lib, gcge_amd.hip_backend; assert 'torch' not in sys.modules; print('ok')"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr


# ---- the matrices -------------------------------------------------------------------------------------------------------------------
def lap(n):
    return csr_to_scipy(make_problem("lap3d", n)[0])


def tridiag(n):
    import scipy.sparse as sp
    i = np.arange(n)
    rows, cols = np.concatenate([i, i[1:], i[:-1]]), np.concatenate([i, i[:-1], i[1:]])
    return sp.csr_matrix((np.where(rows == cols, 2.0, -1.0), (rows, cols)), shape=(n, n))


def lap6_emptied():
    S = lap(6).tolil()
    n = S.shape[0]
    for r in (0, 17, 100, n - 1):
        S.rows[r], S.data[r] = [], []
    for r in (5, 60, 150):
        S.rows[r], S.data[r] = [r], [6.0]
    S = S.tocsr()
    S.eliminate_zeros()
    return S


def lap6_last_bit():
    S = lap(6)
    r = 1 + 6 * (2 + 6 * 3)                                        # an interior row
    k = S.indptr[r] + int(np.flatnonzero(S.indices[S.indptr[r]:S.indptr[r + 1]] == r)[0])
    S.data[k] = np.nextafter(S.data[k], 7.0)
    return S


def lap6_signed_zero():
    S = lap(6)
    ra, rb = 2 + 6 * (2 + 6 * 2), 3 + 6 * (3 + 6 * 3)              # two interior rows: their last entries (offset + 36) become -0.0 / +0.0
    S.data[S.indptr[ra + 1] - 1] = -0.0
    S.data[S.indptr[rb + 1] - 1] = 0.0
    assert S.indices[S.indptr[ra + 1] - 1] == ra + 36 and np.signbit(S.data[S.indptr[ra + 1] - 1]) and S.nnz == lap(6).nnz
    return S


def fe(n, which):
    A, B = make_problem("fe3d", n)
    return csr_to_scipy(A if which == "A" else B)


def stencil15(N):
    """star + the 8 cube diagonals on an N^3 grid, integer values: rows of up to 15 entries (table width 16)"""
    import scipy.sparse as sp
    x, y, z = np.meshgrid(np.arange(N), np.arange(N), np.arange(N), indexing="ij")
    x, y, z = x.ravel(), y.ravel(), z.ravel()
    r = x + N * (y + N * z)
    rows, cols, vals = [r], [r], [np.full(r.size, 14.0)]
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                k = abs(dx) + abs(dy) + abs(dz)
                if k not in (1, 3):
                    continue
                ok = (x + dx >= 0) & (x + dx < N) & (y + dy >= 0) & (y + dy < N) & (z + dz >= 0) & (z + dz < N)
                rows.append(r[ok]); cols.append((r + dx + N * (dy + N * dz))[ok]); vals.append(np.full(ok.sum(), -2.0 if k == 1 else -1.0))
    return sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(N ** 3, N ** 3))


def tridiag_plus(n):
    """8 entries per interior row (table width 8): offsets -4 .. 4 without 0 ... plus the diagonal makes 9, so -4 .. 3"""
    import scipy.sparse as sp
    return sp.diags([np.full(n - abs(o), 3.0 if o == 0 else -1.0) for o in range(-4, 4)], list(range(-4, 4)), format="csr")


# name: (builder, integer-valued)
ACCEPTED = {
    "stencil15_8": (lambda: stencil15(8), True), "band8_70": (lambda: tridiag_plus(70), True),
    "lap3d5": (lambda: lap(5), True), "lap3d6": (lambda: lap(6), True), "lap3d7": (lambda: lap(7), True), "lap3d9": (lambda: lap(9), True),
    "lap3d8": (lambda: lap(8), True), "lap3d16": (lambda: lap(16), True),
    "tridiag1": (lambda: tridiag(1), True), "tridiag2": (lambda: tridiag(2), True), "tridiag65": (lambda: tridiag(65), True),
    "tridiag4097": (lambda: tridiag(4097), True),
    "lap3d6_emptied": (lap6_emptied, True), "lap3d6_last_bit": (lap6_last_bit, False), "lap3d6_signed_zero": (lap6_signed_zero, True),
}


class G:
    """ctypes faces of the handle queries"""

    def __init__(self, hip):
        self.g = hip.g

    def facts(self, m):
        g = self.g
        return (g.gcge_hip_mat_patterns(m), g.gcge_hip_mat_pattern_chain(m), g.gcge_hip_mat_spmm_form(m).decode(), g.gcge_hip_mat_row_order(m).decode())


@pytest.fixture(scope="module")
def q(hip):
    return G(hip)


@pytest.fixture(autouse=True)
def defaults(request):
    """hash bits 64, tile mode 0, reorder mode 0, device levels 1 before and after every GPU test"""
    if "hip" not in request.fixturenames:
        yield
        return
    hip = request.getfixturevalue("hip")
    g = G(hip).g

    def reset():
        mat_device_hash_bits(64)
        g.gcge_hip_spmm_tile_mode(0)
        g.gcge_hip_spmm_reorder_mode(0)
        multigrid_device_levels(1)
        multigrid_graph_method(0)
    reset()
    yield
    reset()


def to_device(S_or_arrays):
    import torch
    rp, ci, va = S_or_arrays
    return tuple(torch.from_numpy(np.ascontiguousarray(a) if a.size else np.zeros(0, dtype=a.dtype)).cuda() for a in (rp, ci, va))


def both(hip, S):
    """(H, D, arrays): the host-path and the device-path handle of the same arrays"""
    A, keep = csr_from_scipy(S)
    H = hip.matrix(A)
    s0 = mat_device_stats()
    D = hip.matrix_from_device(*to_device(keep))
    return H, D, keep, s0, mat_device_stats()


def products(hip, m, n, widths=WIDTHS, seed=11):
    out = []
    X = draw(seed, (n, max(widths)), False)
    for w in widths:
        xh, yh = hip.mv_from_numpy(m, X[:, :w]), hip.mv_from_numpy(m, np.zeros((n, w)))
        hip.ops.spmm(m, xh, yh, (0, 0), (w, w))
        out.append(hip.mv_to_numpy(yh, n, 0, w))
        hip.ops.mv_destroy(xh, w)
        hip.ops.mv_destroy(yh, w)
    return X, out


def same_handles(hip, q, H, D, S, exact, table=True):
    n = S.shape[0]
    assert q.facts(D) == q.facts(H), (q.facts(D), q.facts(H))
    for a, b in zip(mat_to_csr(D), mat_to_csr(H)):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
    if table:
        (pd, td), (ph, th) = mat_pattern_table(D), mat_pattern_table(H)
        assert ph is not None and pd is not None
        assert np.array_equal(pd, ph), np.flatnonzero(pd != ph)[:8]
        assert td.size == th.size and np.array_equal(td, th), np.flatnonzero(td != th)[:8] // 16
    X, yd = products(hip, D, n)
    _, yh = products(hip, H, n)
    for w, a, b in zip(WIDTHS, yd, yh):
        assert np.array_equal(bits(a), bits(b)), ("D against H", w)
        if exact:
            assert np.array_equal(a, S @ X[:, :w]), ("D against scipy", w)


def check_accepted(hip, q, S, exact):
    H, D, keep, s0, s1 = both(hip, S)
    try:
        assert q.g.gcge_hip_mat_patterns(H) > 0, "the case is vacuous: the host path finds no pattern form"
        assert s1[0] == s0[0] + 1 and s1[1] == s0[1], (s0, s1)
        same_handles(hip, q, H, D, S, exact)
    finally:
        hip.free_matrix(H)
        hip.free_matrix(D)


# ---- accepted matrices --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ACCEPTED))
def test_device_search_equals_the_host_search(hip, q, name):
    make, exact = ACCEPTED[name]
    S = make()
    if name == "lap3d8":
        H, D, keep, _, _ = both(hip, S)
        try:                                                       # S = 64, L = 8: chain2 and the ring table
            assert q.g.gcge_hip_mat_pattern_chain(H) == 2 and q.g.gcge_hip_mat_pattern_chain(D) == 2
        finally:
            hip.free_matrix(H)
            hip.free_matrix(D)
    check_accepted(hip, q, S, exact)


@pytest.mark.gpu
def test_fe3d_pair_shares_its_order(hip, q):
    """the FE pair, B after A: the second matrix of a size adopts the identity order the first registered (the generator's rows hold
    at most 7 entries: the table of width 16 is reached by the 15-point stencil among the accepted matrices)"""
    SA, SB = fe(12, "A"), fe(12, "B")
    assert SA.shape[0] == 1728
    HA, DA, _, a0, a1 = both(hip, SA)
    HB, DB, _, b0, b1 = both(hip, SB)
    try:
        assert q.g.gcge_hip_mat_patterns(HA) > 0 and q.g.gcge_hip_mat_patterns(HB) > 0
        assert (a1[0], a1[1]) == (a0[0] + 1, a0[1]) and (b1[0], b1[1]) == (b0[0] + 1, b0[1])
        same_handles(hip, q, HA, DA, SA, False)
        same_handles(hip, q, HB, DB, SB, False)
    finally:
        for m in (HA, DA, HB, DB):
            hip.free_matrix(m)


@pytest.mark.gpu
def test_other_ways_in(hip, q):
    """a torch sparse_csr tensor alone (int64 indices: converted on the device), and objects that only have __cuda_array_interface__"""
    import torch
    S = lap(6)
    A, keep = csr_from_scipy(S)
    H = hip.matrix(A)
    rp, ci, va = to_device(keep)
    T = torch.sparse_csr_tensor(rp.to(torch.int64), ci.to(torch.int64), va, size=S.shape)

    class Foreign:
        def __init__(self, t):
            self.t = t
            self.__cuda_array_interface__ = t.__cuda_array_interface__
    made = [hip.matrix_from_device(T), hip.matrix_from_device(Foreign(rp), Foreign(ci), Foreign(va))]
    try:
        for D in made:
            same_handles(hip, q, H, D, S, True)
        with pytest.raises(TypeError):
            hip.matrix_from_device(torch.from_numpy(keep[0]), ci, va)          # a host tensor
    finally:
        for m in made + [H]:
            hip.free_matrix(m)


# ---- designed give-ups ---------------------------------------------------------------------------------------------------------------
def check_give_up(hip, q, S, collision=False, table=False):
    H, D, keep, s0, s1 = both(hip, S)
    try:
        assert s1[1] == s0[1] + 1 and s1[0] == s0[0], (s0, s1)
        assert (s1[2] == s0[2] + 1) if collision else (s1[2] == s0[2]), (s0, s1)
        assert s1[3] - s0[3] >= (S.shape[0] + 1) * 4 + S.nnz * 12
        same_handles(hip, q, H, D, S, False, table=table)
    finally:
        hip.free_matrix(H)
        hip.free_matrix(D)


@pytest.mark.gpu
def test_give_up_on_too_many_classes(hip, q):
    import scipy.sparse as sp
    n, rng = 2000, np.random.default_rng(5)
    S = sp.diags([rng.random(n - 1) + 1.0, rng.random(n) + 4.0, rng.random(n - 1) + 1.0], [-1, 0, 1], format="csr")
    assert np.unique(S.diagonal()).size == n > 585
    check_give_up(hip, q, S)


@pytest.mark.gpu
def test_give_up_on_long_rows(hip, q):
    S = csr_to_scipy(make_problem("sio2", 24)[0])
    assert np.diff(S.indptr).max() > 16
    check_give_up(hip, q, S)


@pytest.mark.gpu
@pytest.mark.parametrize("hash_bits", [4, 0])
def test_give_up_on_a_hash_collision(hip, q, hash_bits):
    """a hash of 4 bits (16 values for the 27 classes of lap3d 8) or of none: the verify pass finds rows that differ from the first
    row of their class, and the matrix takes the host path — same pid and table as H through the fall-back"""
    mat_device_hash_bits(hash_bits)
    check_give_up(hip, q, lap(8), collision=True, table=True)


@pytest.mark.gpu
def test_give_up_in_tile_mode_2(hip, q):
    q.g.gcge_hip_spmm_tile_mode(2)
    check_give_up(hip, q, lap(6), table=True)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def _edit(which):
    S = lap(5)
    rp, ci, va = S.indptr.astype(np.int32).copy(), S.indices.astype(np.int32).copy(), S.data.copy()
    n = S.shape[0]
    if which == "rowptr0":
        rp[0] = 1
    elif which == "decreasing":
        rp[40] = rp[39] - 1
    elif which == "last":
        rp[n] -= 1
    elif which == "col_n":
        ci[ci.size // 2] = n
    elif which == "col_minus_1":
        ci[3] = -1
    return rp, ci, va


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["rowptr0", "decreasing", "last", "col_n", "col_minus_1"])
def test_malformed_arrays_are_refused(hip, q, which):
    rp, ci, va = _edit(which)
    s0 = mat_device_stats()
    with pytest.raises(ValueError):
        hip.matrix_from_device(*to_device((rp, ci, va)), nrows=rp.size - 1)
    s1 = mat_device_stats()
    assert s1[:3] == s0[:3]
    check_accepted(hip, q, lap(5), True)                            # the process is as usable as before


# ---- round trip ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gcg_on_a_device_matrix_and_eigenvectors_out(hip, q):
    S = lap(12)
    H, D, keep, _, _ = both(hip, S)
    n = S.shape[0]
    got = {}
    try:
        for name, m in (("D", D), ("H", H)):
            hip.set_random_mode(0)
            C.CDLL(None).srand(0)
            ev, res, evec = run_gcg(hip.ops_handle, m, None, ["-nevConv", 8], keep_evec=True)
            assert res.nevConv >= 8
            t = hip.mv_to_torch(evec, 0, 8)
            assert t.is_cuda and tuple(t.shape) == (n, 8) and str(t.dtype) == "torch.float64"
            V = hip.mv_to_numpy(evec, n, 0, 8)
            assert np.array_equal(bits(np.ascontiguousarray(t.cpu().numpy())), bits(np.ascontiguousarray(V)))
            got[name] = (ev.copy(), res.numIter, V)
            hip.ops.mv_destroy(evec, 16)
        assert np.array_equal(bits(got["D"][0]), bits(got["H"][0])) and got["D"][1] == got["H"][1]
        assert np.array_equal(bits(np.ascontiguousarray(got["D"][2])), bits(np.ascontiguousarray(got["H"][2])))
    finally:
        hip.free_matrix(H)
        hip.free_matrix(D)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,size", [("lap3d", 8), ("geometric", 3000)])
def test_block_out_of_a_reordered_handle(hip, q, kind, size):
    """A block that lives in the back-end's own row order comes out in the caller's: mv_to_torch against mv_to_numpy, bit for bit, and
    against the array that went in.  The permuted lap3d 8 has 512 rows, fewer than the 585 patterns a table of width 7 holds, so the
    upload gives every row a pattern of its own and never searches for an order: that handle stays "as given" under reorder mode 1
    (on the parent commit as well), and the comparison runs on it as it is.  The geometric graph of tests/test_mg_graph.py is the
    matrix that mode 1 does re-order (reverse Cuthill-McKee): there the row order must not be "as given"."""
    from test_mg_graph import geometric_graph, permuted
    S = permuted("lap3d", size) if kind == "lap3d" else geometric_graph(size)
    A, keep = csr_from_scipy(S)
    q.g.gcge_hip_spmm_reorder_mode(1)
    H = hip.matrix(A)
    try:
        order = q.g.gcge_hip_mat_row_order(H).decode()
        print(kind, size, "row order:", order)
        if S.shape[0] > 585:
            assert order != "as given"
        X = draw(3, (S.shape[0], 9), True)
        xh = hip.mv_from_numpy(H, X)
        t = hip.mv_to_torch(xh, 2, 9).cpu().numpy()
        V = hip.mv_to_numpy(xh, S.shape[0], 2, 9)
        assert np.array_equal(bits(np.ascontiguousarray(t)), bits(np.ascontiguousarray(V))) and np.array_equal(t, X[:, 2:9])
        hip.ops.mv_destroy(xh, 9)
    finally:
        q.g.gcge_hip_spmm_reorder_mode(0)
        hip.free_matrix(H)


# ---- the hierarchy -------------------------------------------------------------------------------------------------------------------
def hierarchy(hip, q, mA, levels):
    from test_mg_graph import slot_multigrid
    Ah, _, Ph, done = slot_multigrid(hip, mA, None, levels)
    nbytes = multigrid_stats()[1]
    out = {"A": [mat_to_csr(a) for a in Ah], "P": [mat_to_csr(p) for p in Ph], "PT": [mat_to_csr(p, transpose=True) for p in Ph],
           "facts": [q.facts(a) for a in Ah], "bytes": nbytes}
    done()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["grid", "mis2"])
def test_hierarchy_is_the_same_with_and_without_device_levels(hip, q, case):
    from test_mg_graph import permuted
    S, nlev = (lap(32), 4) if case == "grid" else (permuted("lap3d", 16), 3)
    A, keep = csr_from_scipy(S)
    mA = hip.matrix(A)
    got, solve = {}, {}
    try:
        for on in (1, 0):
            multigrid_device_levels(on)
            multigrid_graph_method(1 if case == "mis2" else 0)
            got[on] = hierarchy(hip, q, mA, 4)
            multigrid_graph_method(0)
            hip.set_random_mode(0)
            C.CDLL(None).srand(0)
            ev, res = run_gcg(hip.ops_handle, mA, None, ["-nevConv", 6, "-gcge_amg_levels", 4] + (["-gcge_amg_graph", 1] if case == "mis2" else []))
            assert res.nevConv >= 6
            solve[on] = (ev.copy(), res.numIter)
    finally:
        hip.free_matrix(mA)
    d, h = got[1], got[0]
    assert len(h["A"]) == nlev == len(d["A"])
    for key in ("A", "P", "PT"):
        for x, y in zip(d[key], h[key]):
            for a, b in zip(x, y):
                assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), key
    assert d["facts"] == h["facts"], (d["facts"], h["facts"])
    assert np.array_equal(bits(solve[1][0]), bits(solve[0][0])) and solve[1][1] == solve[0][1], (solve[1][1], solve[0][1])
    pattern_levels = [lev for lev in range(1, nlev) if h["facts"][lev][0] > 0]
    if case == "grid":
        assert pattern_levels == list(range(1, nlev)), h["facts"]     # every coarse level of lap3d 32 has a pattern form: the bound bites
    saved = sum((h["A"][lev][0].size) * 4 + h["A"][lev][1].size * 12 for lev in pattern_levels)
    print("bytes device to host: device levels %d, host levels %d, CSR of the pattern levels %d" % (d["bytes"], h["bytes"], saved))
    assert d["bytes"] <= h["bytes"] - saved + 2 * 65536 * len(pattern_levels), (d["bytes"], h["bytes"], saved)
