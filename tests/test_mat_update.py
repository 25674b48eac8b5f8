"""New values for a live matrix handle from a device array (gcge_hip_mat_update_values_device, csrc/hip/mat_values.hip;
HipBackend.matrix_update_values): the structure stays, the values are re-derived on the device, the handle keeps its K1 form or becomes
the "+values" form of the table it has.

Data is exact: integer-valued matrix entries and integer X in [-4, 4], so S_new @ X in numpy is the product in any summation order and no
tolerance appears in the product tests.  Three kinds of new values on every structure:
  U  every value doubled                              (the classes of a value table stay uniform)
  V  diag[r] += (7 r) % 5                             (an SCF step: another diagonal in every row)
  W  a_ij = -(1 + (i + j) % 3), a_ii = 20 + i % 4     (symmetric where the structure is, everything varies)
What a handle must become is read off the handle the way include/gcge_hip.h states it — from pid (are all rows of a class equal, as
bits, under the new values, none of them 0?) and the table width — and pinned by name for the cases the contract lists.

The by-offsets handle of the host path: a table of width 7 holds 585 classes, so a 7-point stencil of 8^3 = 512 rows ALWAYS gets a value
table, whatever its coefficients (every row a class of its own).  The smallest grids on which hip.matrix leaves the "+values" forms are
9^3 (729 rows, plain) and 16^3 (S = 256, the smallest S % 32 == 0 above 585 rows: chain2); those two stand for that row of the contract,
with a diagonal 100 + r that makes every row its own class."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from gcge_amd.lib import csr_to_scipy, make_problem, mat_device_stats, mat_pattern_table, mat_to_csr, mat_update_stats
from helpers import bits, csr_from_scipy, perturbed_stencil

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (1, 7, 16, 64)                     # (tests/test_mat_device.py)
D2H_PER_UPDATE = 65536 + 64
KINDS = ("U", "V", "W")


# ---- CPU --------------------------------------------------------------------------------------------------------------------------------
def test_prototypes_are_public():
    from gcge_amd import abi
    text = open(os.path.join(ROOT, "include", "gcge_hip.h")).read()
    assert re.search(r"int  gcge_hip_mat_update_values_device \(GCGE_HIP_MAT \*A, long nnz, const double \*d_val\);", text)
    assert re.search(r"void gcge_hip_mat_update_stats \(long out\[6\]\);", text)
    assert abi.HIP["gcge_hip_mat_update_values_device"] == (C.c_int, [C.c_void_p, C.c_long, C.c_void_p])
    assert abi.HIP["gcge_hip_mat_update_stats"] == (None, [C.c_void_p])
    from gcge_amd.lib import hip_lib
    assert hasattr(hip_lib(), "gcge_hip_mat_update_values_device") and hasattr(hip_lib(), "gcge_hip_mat_update_stats")      # dlopen only


def test_slot_rule_host_check(tmp_path):
    """tools/pattern_values_check.cpp under AddressSanitizer + UBSan, as a program of its own: the slot rule the kernels share
    (gcge_pat_value_slot, csrc/hip/pattern_table.h) on the 8^3 and 5^3 7-point and the 8^3 15-point stencils, U, V and W values, value
    and offsets-only tables; a stored zero is flagged"""
    exe = str(tmp_path / "pattern_values_check")
    r = subprocess.run(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + os.path.join(ROOT, "gcge_amd", "csrc", "hip"), os.path.join(ROOT, "tools", "pattern_values_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    assert r.stdout.count("U V W reproduced") == 5


# ---- the matrices -----------------------------------------------------------------------------------------------------------------------
def lap(n):
    return csr_to_scipy(make_problem("lap3d", n)[0])


def lap_distinct_diagonal(n):
    S = lap(n)
    S.setdiag(100.0 + np.arange(S.shape[0]))
    return S.tocsr()


def random300():
    """300 rows, symmetric random structure, 9 .. 13 entries per row (table width 16 holds 256 classes: no pattern form), integer values"""
    import scipy.sparse as sp
    rng = np.random.default_rng(300)
    n = 300
    i = np.repeat(np.arange(n), 5)
    j = rng.integers(0, n, i.size)
    keep = i != j
    P = sp.coo_matrix((np.ones(keep.sum()), (i[keep], j[keep])), shape=(n, n)).tocsr()
    P = ((P + P.T) > 0).astype(np.float64).tocoo()
    S = sp.coo_matrix((-(1.0 + (P.row + P.col) % 3), (P.row, P.col)), shape=(n, n)).tocsr() + sp.diags(40.0 + np.arange(n) % 7)
    S = S.tocsr()
    S.sort_indices()
    return S


def structures():
    from test_mat_device import stencil15, tridiag, tridiag_plus
    return {
        "lap3d6": (lambda: lap(6), "device"), "lap3d8": (lambda: lap(8), "device"), "band8_70": (lambda: tridiag_plus(70), "device"),
        "stencil15_8": (lambda: stencil15(8), "device"),
        "tridiag1": (lambda: tridiag(1), "device"), "tridiag2": (lambda: tridiag(2), "device"), "tridiag65": (lambda: tridiag(65), "device"),
        "tridiag4097": (lambda: tridiag(4097), "device"),
        "offsets9": (lambda: lap_distinct_diagonal(9), "host"), "offsets16": (lambda: lap_distinct_diagonal(16), "host"),
        "random300": (random300, "host"),
    }


STRUCTURES = ("lap3d6", "lap3d8", "band8_70", "stencil15_8", "tridiag1", "tridiag2", "tridiag65", "tridiag4097", "offsets9", "offsets16", "random300")
# (structure, kind) -> (return code, form before, form after, chain): the rows of the contract in include/gcge_hip.h, by name
PINNED = {
    ("lap3d6", "U"): (0, "spmm_pattern", "spmm_pattern", 0), ("lap3d6", "V"): (0, "spmm_pattern", "spmm_pattern+values", 0),
    ("lap3d6", "W"): (0, "spmm_pattern", "spmm_pattern+values", 0),
    ("lap3d8", "U"): (0, "spmm_pattern_chain2", "spmm_pattern_chain2", 2), ("lap3d8", "V"): (0, "spmm_pattern_chain2", "spmm_pattern_chain2+values", 2),
    ("lap3d8", "W"): (0, "spmm_pattern_chain2", "spmm_pattern_chain2+values", 2),
    ("stencil15_8", "U"): (0, "spmm_pattern", "spmm_pattern", 0), ("stencil15_8", "V"): (1, "spmm_pattern", "spmm_pattern", 0),
    ("stencil15_8", "W"): (1, "spmm_pattern", "spmm_pattern", 0),
    ("offsets9", "U"): (0, "spmm_pattern+values", "spmm_pattern+values", 0), ("offsets9", "V"): (0, "spmm_pattern+values", "spmm_pattern+values", 0),
    ("offsets9", "W"): (0, "spmm_pattern+values", "spmm_pattern+values", 0),
    ("offsets16", "U"): (0, "spmm_pattern_chain2+values", "spmm_pattern_chain2+values", 2),
    ("offsets16", "V"): (0, "spmm_pattern_chain2+values", "spmm_pattern_chain2+values", 2),
    ("offsets16", "W"): (0, "spmm_pattern_chain2+values", "spmm_pattern_chain2+values", 2),
    ("random300", "U"): (0, "spmm_pad8", "spmm_pad8", 0), ("random300", "V"): (0, "spmm_pad8", "spmm_pad8", 0), ("random300", "W"): (0, "spmm_pad8", "spmm_pad8", 0),
}


def new_values(S, kind):
    """the matrix of S's structure with the values of `kind` (S sorted CSR); O: S itself"""
    S = S.tocsr().copy()
    S.sort_indices()
    rows, cols = np.repeat(np.arange(S.shape[0]), np.diff(S.indptr)), S.indices
    if kind == "U":
        S.data = S.data * 2.0
    elif kind == "V":
        S.data = S.data + np.where(rows == cols, (7 * rows) % 5, 0).astype(np.float64)
    elif kind == "W":
        S.data = np.where(rows == cols, 20.0 + rows % 4, -(1.0 + (rows + cols) % 3)).astype(np.float64)
    else:
        assert kind == "O"
    return S


def to_device(arrays):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


def create(hip, S, how):
    A, keep = csr_from_scipy(S)
    return hip.matrix(A) if how == "host" else hip.matrix_from_device(*to_device(keep))


def facts(hip, m):
    g = hip.g
    return g.gcge_hip_mat_spmm_form(m).decode(), g.gcge_hip_mat_pattern_chain(m)


_X = {}


def x_block(n):
    if n not in _X:
        _X[n] = np.random.default_rng(4 + n).integers(-4, 5, (n, max(WIDTHS))).astype(np.float64)
    return _X[n]


def products(hip, m, n, widths=WIDTHS):
    X, out = x_block(n), []
    for w in widths:
        xh, yh = hip.mv_from_numpy(m, X[:, :w]), hip.mv_from_numpy(m, np.full((n, w), 5.0))
        hip.ops.spmm(m, xh, yh, (0, 0), (w, w))
        out.append(hip.mv_to_numpy(yh, n, 0, w))
        hip.ops.mv_destroy(xh, w)
        hip.ops.mv_destroy(yh, w)
    return out


def check_products(hip, m, S, what):
    n, X = S.shape[0], x_block(S.shape[0])
    for w, y in zip(WIDTHS, products(hip, m, n)):
        assert np.array_equal(y, S @ X[:, :w]), (what, "width", w, np.argwhere(y != S @ X[:, :w])[:4].tolist())
    rp, ci, va = mat_to_csr(m)
    assert np.array_equal(rp, S.indptr) and np.array_equal(ci, S.indices) and np.array_equal(bits(va), bits(S.data)), (what, "gcge_hip_mat_to_csr")


def expected(hip, m, S, Snew):
    """(return code, form after) by the contract, from the handle's pid and table width"""
    form, _ = facts(hip, m)
    pid, tab = mat_pattern_table(m)
    if pid is None or form.endswith("+values"):
        return 0, form
    npat = hip.g.gcge_hip_mat_patterns(m)
    lt = tab.size // 16 // npat
    uniform = True
    for p in np.unique(pid):
        r = np.flatnonzero(pid == p)
        L = int(S.indptr[r[0] + 1] - S.indptr[r[0]])
        v = bits(Snew.data)[S.indptr[r][:, None] + np.arange(L)[None, :]]
        uniform = uniform and bool(np.all(v == v[0])) and bool(np.all(Snew.data[S.indptr[r[0]]:S.indptr[r[0]] + L] != 0.0))
    if uniform:
        return 0, form
    return (0, "spmm_pattern_chain2+values" if form == "spmm_pattern_chain2" else "spmm_pattern+values") if lt <= 8 else (1, form)


def update(hip, m, Snew):
    """HipBackend.matrix_update_values around the counters: (accepted, stats before, stats after)"""
    import torch
    u0, d0 = mat_update_stats(), mat_device_stats()
    ok = hip.matrix_update_values(m, torch.from_numpy(np.ascontiguousarray(Snew.data)).cuda())
    u1, d1 = mat_update_stats(), mat_device_stats()
    assert d1 == d0, ("gcge_hip_mat_device_stats moved", d0, d1)
    assert 0 <= u1[5] - u0[5] <= D2H_PER_UPDATE, (u0, u1)
    assert u1[4] == u0[4]
    return ok, u0, u1


def check_counters(rc, kept_form, was_value_table, u0, u1):
    d = tuple(b - a for a, b in zip(u0, u1))[:5]
    if rc == 1:
        assert d == (0, 0, 0, 1, 0), d
    elif kept_form:
        assert d == (1, 1 if was_value_table else 0, 0, 0, 0), d
    else:
        assert d == (0, 0, 1, 0, 0), d


# ---- GPU: products through updated handles ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", STRUCTURES)
def test_products_through_an_updated_handle(hip, name, kind):
    make, how = structures()[name]
    S = make().tocsr()
    S.sort_indices()
    Snew = new_values(S, kind)
    m = create(hip, S, how)
    fresh = None
    try:
        form0, chain0 = facts(hip, m)
        value_table = hip.g.gcge_hip_mat_patterns(m) > 0 and not form0.endswith("+values")
        rc_want, form_want = expected(hip, m, S, Snew)
        if (name, kind) in PINNED:
            assert (rc_want, form0, form_want, chain0) == PINNED[(name, kind)], ((rc_want, form0, form_want, chain0), PINNED[(name, kind)])
        if kind == "U":
            assert (rc_want, form_want) == (0, form0)
        check_products(hip, m, S, "before")
        table0 = mat_pattern_table(m)
        ok, u0, u1 = update(hip, m, Snew)
        print(name, kind, "form", form0, "->", facts(hip, m)[0], "accepted", ok, "bytes device to host", u1[5] - u0[5])
        assert ok == (rc_want == 0), (ok, rc_want)
        assert facts(hip, m) == (form_want, chain0), (facts(hip, m), form_want, chain0)
        check_counters(rc_want, form_want == form0, value_table, u0, u1)
        if rc_want == 1:                                           # declined: nothing was written
            check_products(hip, m, S, "after a decline")
            t1 = mat_pattern_table(m)
            assert np.array_equal(t1[0], table0[0]) and np.array_equal(t1[1], table0[1])
            return
        check_products(hip, m, Snew, "after")
        if table0[0] is not None:                                  # pid and the table's offsets are untouched
            t1 = mat_pattern_table(m)
            assert np.array_equal(t1[0], table0[0])
            assert np.array_equal(t1[1].reshape(-1, 16)[:, 8:], table0[1].reshape(-1, 16)[:, 8:])
        fresh = create(hip, Snew, how)
        if kind == "U" or name.startswith("offsets") and kind != "W":
            assert facts(hip, fresh) == facts(hip, m), (facts(hip, fresh), facts(hip, m))
        if facts(hip, fresh) == facts(hip, m):
            for w, a, b in zip(WIDTHS, products(hip, m, S.shape[0]), products(hip, fresh, S.shape[0])):
                assert np.array_equal(bits(a), bits(b)), ("updated against fresh", w)
            if kind == "U" and value_table:                        # a rewritten table is the fresh handle's table
                (pa, ta), (pb, tb) = mat_pattern_table(m), mat_pattern_table(fresh)
                assert np.array_equal(pa, pb) and np.array_equal(ta, tb)
    finally:
        hip.free_matrix(m)
        if fresh is not None:
            hip.free_matrix(fresh)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["lap3d6", "lap3d8", "band8_70", "tridiag65", "offsets9", "random300"])
def test_a_sequence_of_updates_on_one_handle(hip, name):
    """U, then V, then W, then the original values: products after every step; a value table is converted exactly once"""
    make, how = structures()[name]
    S = make().tocsr()
    S.sort_indices()
    m = create(hip, S, how)
    try:
        form0, chain0 = facts(hip, m)
        value_table = hip.g.gcge_hip_mat_patterns(m) > 0 and not form0.endswith("+values")
        start = mat_update_stats()
        for kind in ("U", "V", "W", "O"):
            Snew = new_values(S, kind)
            ok, _, _ = update(hip, m, Snew)
            assert ok, kind
            check_products(hip, m, Snew, kind)
            assert facts(hip, m)[1] == chain0
        end = mat_update_stats()
        assert end[2] - start[2] == (1 if value_table else 0), (start, end)
        assert end[0] - start[0] == (3 if value_table else 4) and end[3] == start[3], (start, end)
        if value_table:
            assert facts(hip, m)[0] == ("spmm_pattern_chain2+values" if form0 == "spmm_pattern_chain2" else "spmm_pattern+values")     # no way back
        else:
            assert facts(hip, m)[0] == form0
    finally:
        hip.free_matrix(m)


# ---- GPU: the fused passes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("nrhs", [4, 16])
@pytest.mark.parametrize("kind", ["V", "U"])
def test_fused_cg_through_an_updated_handle(hip, kind, nrhs):
    """One fused block-CG solve (gcge_hip_bpcg_setup, ops->MultiLinearSolver) on the 8^3 handle after V (converted between two solves) and
    after U (chain2 and the ring sweep kept) against the same solve on a fresh handle of the same values: the same iteration count;
    solutions equal as bits where the two handles have one form.  Otherwise the two solves apply the same operator through different
    kernels, each stops at ||b - A x|| <= rate ||b|| (x0 = 0), and the solutions are compared within that stopping tolerance times ||b||
    per column — solver parameters and rule are those of tests/test_hip_parity.py::test_fused_cg_device_scalars_equal_host_scalars
    (25 iterations, rate 1e-3, tol 1e-10 "abs")."""
    from helpers import uniform
    g = hip.g
    S = lap(8)
    S.sort_indices()
    Snew = new_values(S, kind)
    n = S.shape[0]
    max_iter, rate, tol = 25, 1e-3, 1e-10
    Bm = uniform(71, (n, nrhs)) - 0.5
    m, fresh = create(hip, S, "device"), create(hip, Snew, "device")
    out = {}
    try:
        # a solve through the handle BEFORE the update: whatever the solver keeps across calls has seen the old form
        g.gcge_hip_bpcg_setup(hip.ops_handle, max_iter, rate, tol, b"abs")
        b, x = hip.mv_from_numpy(m, Bm), hip.mv_from_numpy(m, np.zeros((n, nrhs)))
        hip.ops.multi_linear_solver(m, b, x, (0, 0), (nrhs, nrhs))
        hip.ops.mv_destroy(b, nrhs); hip.ops.mv_destroy(x, nrhs)
        ok, _, _ = update(hip, m, Snew)
        assert ok
        want_form = "spmm_pattern_chain2" if kind == "U" else "spmm_pattern_chain2+values"
        assert facts(hip, m) == (want_form, 2), facts(hip, m)
        for tag, h in (("updated", m), ("fresh", fresh)):
            g.gcge_hip_bpcg_setup(hip.ops_handle, max_iter, rate, tol, b"abs")
            b, x = hip.mv_from_numpy(h, Bm), hip.mv_from_numpy(h, np.zeros((n, nrhs)))
            hip.ops.multi_linear_solver(h, b, x, (0, 0), (nrhs, nrhs))
            it = C.c_int(); g.gcge_hip_bpcg_stats(None, None, C.byref(it))
            out[tag] = (hip.mv_to_numpy(x, n, 0, nrhs), it.value)
            hip.ops.mv_destroy(b, nrhs); hip.ops.mv_destroy(x, nrhs)
        same_form = facts(hip, fresh) == facts(hip, m)
    finally:
        g.gcge_hip_bpcg_setup(hip.ops_handle, 30, 1e-2, 1e-14, b"abs")
        hip.free_matrix(m)
        hip.free_matrix(fresh)
    (xu, itu), (xf, itf) = out["updated"], out["fresh"]
    dx = np.linalg.norm(xu - xf, axis=0) / np.linalg.norm(Bm, axis=0)
    res = np.linalg.norm(Bm - Snew @ xu, axis=0) / np.linalg.norm(Bm, axis=0)
    print(kind, nrhs, "iterations", itu, itf, "same form", same_form, "max |dx| / |b| %.3e" % dx.max(), "residual / |b| %.3e" % res.max())
    assert itu == itf and 0 < itu <= max_iter, (itu, itf)
    assert np.all(res <= rate * (1.0 + 1e-6)) or itu == max_iter, res
    if kind == "U":
        assert same_form
    if same_form:
        assert np.array_equal(bits(np.ascontiguousarray(xu)), bits(np.ascontiguousarray(xf)))
    else:
        assert np.all(dx <= rate), dx


# ---- GPU: declines leave the handle as it was ---------------------------------------------------------------------------------------------
def raw_update(hip, m, nnz, values):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(values, dtype=np.float64)).cuda() if values is not None else None
    torch.cuda.synchronize()
    return hip.g.gcge_hip_mat_update_values_device(m, int(nnz), t.data_ptr() if t is not None else None)


def lap6_stored_zero(zero):
    S = lap(6)
    S.sort_indices()
    r = 2 + 6 * (2 + 6 * 2)                                         # an interior row: its last entry (offset + 36) is stored as a zero
    S.data[S.indptr[r + 1] - 1] = zero
    assert S.indices[S.indptr[r + 1] - 1] == r + 36 and S.nnz == lap(6).nnz
    return S


def check_decline(hip, m, S, values):
    n = S.shape[0]
    before, csr0, tab0, f0 = products(hip, m, n), mat_to_csr(m), mat_pattern_table(m), facts(hip, m)
    u0, d0 = mat_update_stats(), mat_device_stats()
    rc = raw_update(hip, m, S.nnz, values)
    u1 = mat_update_stats()
    assert rc == 1, rc
    assert tuple(b - a for a, b in zip(u0, u1))[:5] == (0, 0, 0, 1, 0) and u1[5] - u0[5] <= D2H_PER_UPDATE, (u0, u1)
    assert mat_device_stats() == d0 and facts(hip, m) == f0
    for w, a, b in zip(WIDTHS, before, products(hip, m, n)):
        assert np.array_equal(bits(a), bits(b)), w
    for a, b in zip(csr0, mat_to_csr(m)):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    if tab0[0] is not None:
        t1 = mat_pattern_table(m)
        assert np.array_equal(tab0[0], t1[0]) and np.array_equal(tab0[1], t1[1])
    return u1[5] - u0[5]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["sio2_24", "stencil15_V", "stored_zero", "stored_minus_zero"])
def test_declines_leave_the_handle_as_it_was(hip, case):
    from test_mat_device import stencil15
    if case == "sio2_24":
        S = csr_to_scipy(make_problem("sio2", 24)[0])
        how, values = "host", None
    elif case == "stencil15_V":
        S = stencil15(8)
        how, values = "device", "V"
    else:
        S = lap6_stored_zero(0.0 if case == "stored_zero" else -0.0)
        how, values = "device", "U"
    S = S.tocsr()
    S.sort_indices()
    m = create(hip, S, how)
    try:
        form = facts(hip, m)[0]
        if case == "sio2_24":
            assert "spmm_star" in form or "spmm_dense" in form, form
        else:
            assert form == "spmm_pattern", form
        moved = check_decline(hip, m, S, S.data * 2.0 if values is None else new_values(S, values).data)
        print(case, form, "bytes device to host", moved)
        if case == "sio2_24":
            assert moved == 0                                      # decided from the handle alone
    finally:
        hip.free_matrix(m)


@pytest.mark.gpu
def test_a_rectangular_handle_is_declined(hip):
    import scipy.sparse as sp
    from test_mat_device import tridiag
    nf, nc = 20, 10
    P = sp.csr_matrix((1.0 + np.arange(nf) % 3, (np.arange(nf), np.arange(nf) // 2)), shape=(nf, nc))
    A, keep = csr_from_scipy(P)
    Af, keepf = csr_from_scipy(tridiag(nf))
    m, sq = hip.matrix_rect(A), hip.matrix(Af)
    try:
        X = np.random.default_rng(2).integers(-4, 5, (nc, 7)).astype(np.float64)

        def product():
            xh, yh = hip.mv_from_numpy(m, X), hip.mv_from_numpy(sq, np.zeros((nf, 7)))
            hip.ops.spmm(m, xh, yh, (0, 0), (7, 7))
            y = hip.mv_to_numpy(yh, nf, 0, 7)
            hip.ops.mv_destroy(xh, 7); hip.ops.mv_destroy(yh, 7)
            return y
        y0, c0, t0, u0 = product(), mat_to_csr(m), mat_to_csr(m, transpose=True), mat_update_stats()
        assert np.array_equal(y0, P @ X)
        assert raw_update(hip, m, P.nnz, P.data * 2.0) == 1
        u1 = mat_update_stats()
        assert tuple(b - a for a, b in zip(u0, u1)) == (0, 0, 0, 1, 0, 0), (u0, u1)
        assert np.array_equal(bits(product()), bits(y0))
        for a, b in zip(c0 + t0, mat_to_csr(m) + mat_to_csr(m, transpose=True)):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    finally:
        hip.free_matrix_rect(m)
        hip.free_matrix(sq)


@pytest.mark.gpu
def test_a_reordered_handle_is_declined(hip):
    """the geometric graph of tests/test_mg_graph.py is what reorder mode 1 re-orders (tests/test_mat_device.py says why lap3d 8 is not)"""
    from test_mg_graph import geometric_graph
    S = geometric_graph(3000).tocsr()
    S.sort_indices()
    A, keep = csr_from_scipy(S)
    hip.g.gcge_hip_spmm_reorder_mode(1)
    m = None
    try:
        m = hip.matrix(A)
        assert hip.g.gcge_hip_mat_row_order(m).decode() != "as given"
        n = S.shape[0]
        before, u0 = products(hip, m, n, (7, 16)), mat_update_stats()
        assert raw_update(hip, m, hip.g.gcge_hip_mat_nnz(m), S.data * 2.0) == 1
        u1 = mat_update_stats()
        assert tuple(b - a for a, b in zip(u0, u1)) == (0, 0, 0, 1, 0, 0), (u0, u1)
        for a, b in zip(before, products(hip, m, n, (7, 16))):
            assert np.array_equal(bits(a), bits(b))
    finally:
        hip.g.gcge_hip_spmm_reorder_mode(0)
        if m is not None:
            hip.free_matrix(m)


@pytest.mark.gpu
def test_bad_arguments(hip):
    S = lap(6)
    S.sort_indices()
    m = create(hip, S, "device")
    try:
        for nnz, values, handle in ((S.nnz - 1, S.data, m), (S.nnz + 1, S.data, m), (S.nnz, None, m), (S.nnz, S.data, None)):
            u0 = mat_update_stats()
            assert raw_update(hip, handle, nnz, values) < 0
            u1 = mat_update_stats()
            assert tuple(b - a for a, b in zip(u0, u1)) == (0, 0, 0, 0, 1, 0), (u0, u1)
        check_products(hip, m, S, "after the refused calls")
    finally:
        hip.free_matrix(m)


# ---- GPU: the Python entry ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_python_entry(hip):
    import torch
    S = lap(6)
    S.sort_indices()
    m = create(hip, S, "device")
    try:
        with pytest.raises(TypeError):
            hip.matrix_update_values(m, torch.from_numpy(S.data.copy()))                      # a host tensor
        with pytest.raises(TypeError):
            hip.matrix_update_values(m, S.data.copy())                                        # a numpy array
        u0 = mat_update_stats()
        with pytest.raises(ValueError):
            hip.matrix_update_values(m, torch.from_numpy(S.data[:-1].copy()).cuda())          # a wrong count: the library is not called
        assert mat_update_stats() == u0
        U, V = new_values(S, "U"), new_values(S, "V")
        assert hip.matrix_update_values(m, torch.from_numpy(U.data.astype(np.float32)).cuda())      # float32: converted on the device
        check_products(hip, m, U, "float32 values")
        rp, ci = (torch.from_numpy(a.astype(np.int64)).cuda() for a in (S.indptr, S.indices))
        T = torch.sparse_csr_tensor(rp, ci, torch.from_numpy(V.data).cuda(), size=S.shape)
        assert hip.matrix_update_values(m, T.values())                                        # the .values() of a sparse_csr tensor
        check_products(hip, m, V, "values of a sparse_csr tensor")

        class Foreign:
            def __init__(self, t):
                self.t = t
                self.__cuda_array_interface__ = t.__cuda_array_interface__
        assert hip.matrix_update_values(m, Foreign(torch.from_numpy(S.data.copy()).cuda()))
        check_products(hip, m, S, "an object with __cuda_array_interface__")
    finally:
        hip.free_matrix(m)


# ---- GPU: eigsh over a sequence of nearby operators -----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("size", [12, 8])
def test_eigsh_over_a_sequence_of_potentials(hip, size):
    """lap3d + 0.1 t v on the diagonal, t = 0, 1, 2, one handle from matrix_from_device: step 0 rewrites the table with the values it
    has, step 1 is a conversion between two solves, step 2 a re-scatter; every step starts from the previous eigenvectors.  Bounds and
    reasoning: tests/test_eigsh.py::check_result."""
    import torch
    from gcge_amd import eigsh
    from test_eigsh import K, check_result
    S = lap(size)
    S.sort_indices()
    n = S.shape[0]
    v = np.random.default_rng(17).random(n)
    rows, cols = np.repeat(np.arange(n), np.diff(S.indptr)), S.indices
    dev = to_device((S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data))
    m = hip.matrix_from_device(*dev)
    try:
        created = mat_device_stats()
        form0, chain0 = facts(hip, m)
        assert form0 == ("spmm_pattern_chain2" if size == 8 else "spmm_pattern")
        r = None
        for t in range(3):
            St = S.copy()
            St.data = S.data + np.where(rows == cols, 0.1 * t * v[rows], 0.0)
            u0 = mat_update_stats()
            assert hip.matrix_update_values(m, torch.from_numpy(St.data).cuda())
            d = tuple(b - a for a, b in zip(u0, mat_update_stats()))
            assert d[:5] == ((1, 1, 0, 0, 0), (0, 0, 1, 0, 0), (1, 0, 0, 0, 0))[t] and d[5] <= D2H_PER_UPDATE, (t, d)
            assert facts(hip, m) == (form0 if t == 0 else ("spmm_pattern_chain2+values" if size == 8 else "spmm_pattern+values"), chain0)
            r = eigsh(m, K, X0=None if r is None else r.eigenvectors, backend=hip)
            print("step", t, "iterations", r.iterations)
            check_result(r, St, None, np.linalg.eigvalsh(St.toarray())[:K])
            assert mat_device_stats()[0:2] == created[0:2]
    finally:
        hip.free_matrix(m)


@pytest.mark.gpu
def test_eigsh_generalised_pair_after_an_update(hip):
    """fe3d 8: A takes the coefficients of helpers.perturbed_stencil, B stays; against scipy.linalg.eigh.  The loop is the documented one:
    a declined update (a table of 16 slots) frees the handle and creates the matrix again."""
    import scipy.linalg
    import torch
    from gcge_amd import eigsh
    from test_eigsh import K, check_result
    A, B = make_problem("fe3d", 8)
    SA, SB = csr_to_scipy(A), csr_to_scipy(B)
    SA.sort_indices(); SB.sort_indices()
    Ap, keep = perturbed_stencil("fe3d", 8, 33)
    SP = csr_to_scipy(Ap)
    SP.sort_indices()
    assert np.array_equal(SP.indptr, SA.indptr) and np.array_equal(SP.indices, SA.indices)
    mA = hip.matrix_from_device(*to_device((SA.indptr.astype(np.int32), SA.indices.astype(np.int32), SA.data)))
    mB = hip.matrix_from_device(*to_device((SB.indptr.astype(np.int32), SB.indices.astype(np.int32), SB.data)))
    try:
        r = eigsh(mA, K, M=mB, backend=hip)
        check_result(r, SA, SB, scipy.linalg.eigh(SA.toarray(), SB.toarray(), eigvals_only=True)[:K])
        before = facts(hip, mA)
        ok = hip.matrix_update_values(mA, torch.from_numpy(SP.data).cuda())
        print("fe3d 8 A:", before, "->", facts(hip, mA), "accepted", ok)
        if not ok:
            hip.free_matrix(mA)
            mA = hip.matrix_from_device(*to_device((SP.indptr.astype(np.int32), SP.indices.astype(np.int32), SP.data)))
        else:
            assert np.array_equal(bits(mat_to_csr(mA)[2]), bits(SP.data))
        r = eigsh(mA, K, M=mB, X0=r.eigenvectors, backend=hip)
        check_result(r, SP, SB, scipy.linalg.eigh(SP.toarray(), SB.toarray(), eigvals_only=True)[:K])
    finally:
        hip.free_matrix(mA)
        hip.free_matrix(mB)
