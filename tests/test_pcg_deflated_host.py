"""GCGE_PCGSolveDeflated (csrc/host/block_fpcg.c) over the CPU oracle's table, where the back-end record is empty and the shift, p.w
and the projections all go through the slots: the deflated, per-column-shifted systems

    Q^T (A - lambda_c B) y_c = Q^T b_c ,   y_c in range(Q) ,   Q = I - X X^T B

on Lap3D 12^3 with X the 4 lowest dense eigenvectors (the single lowest and the triple above it: k ends at a gap) and the shifts
their eigenvalues, against the dense solution of the projected system.

Bound.  On range(Q), in the variables B^1/2 y, the operator has the eigenvalues lambda_i - lambda_c, i > k, so a residual of
tol |Q^T b_c| leaves an error of at most kappa_proj tol |y_c| with kappa_proj = (lambda_max - lambda_c) / (lambda_5 - lambda_c) for the
standard problem, computed here from the dense spectrum; the dense reference's own error, kappa_proj n eps, is added:
    |y_c - reference| <= kappa_proj (tol + n eps) |y_c|.
With a B the change of variables costs |B^1/2| |B^-1/2| on each side: the same with kappa_proj cond(B), lambda the generalised
eigenvalues."""
import ctypes as C

import numpy as np
import pytest

from gcge_amd.lib import csr_to_scipy, host_lib, make_problem
from helpers import bits, csr_from_scipy, uniform

EPS = np.finfo(np.float64).eps
N, K, TOL = 12, 4, 1e-10


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class Case:
    """Lap3D 12^3 on the oracle with a 3-level hierarchy of block 4, one solver with it and one without, an optional B, and the
    dense eigenpairs"""

    def __init__(self, oracle, with_B):
        import scipy.linalg as sla
        import scipy.sparse as sp
        self.o, self.h, self.n = oracle, host_lib(), N ** 3
        self.A, _ = make_problem("lap3d", N)
        self.S = csr_to_scipy(self.A)
        self.mA = oracle.matrix(self.A)
        self.Ad = self.S.toarray()
        self.Bd, self.mB = None, None
        if with_B:                                                      # SPD: the identity plus a scaled Laplacian
            SB = (sp.identity(self.n) + 0.05 * self.S).tocsr()
            self.B, self._keep = csr_from_scipy(SB)
            self.mB, self.Bd = oracle.matrix(self.B), SB.toarray()
        self.lam, V = sla.eigh(self.Ad, self.Bd)
        self.X = np.asfortranarray(V[:, :K])                             # B-orthonormal
        self.MX = self.X if self.Bd is None else self.Bd @ self.X
        assert self.lam[K] - self.lam[K - 1] > 1e-2                      # k ends at a gap
        self.amg = C.c_void_p(self.h.GCGE_AMGCreate(self.mA, None, 3, 4, 1, 5, 4, 1e-2, oracle.ops_handle))
        assert self.amg.value
        self.solver = {True: C.c_void_p(self.h.GCGE_PCGCreate(self.mA, self.amg, 4, oracle.ops_handle)),
                       False: C.c_void_p(self.h.GCGE_PCGCreate(self.mA, None, 4, oracle.ops_handle))}
        assert self.solver[True].value and self.solver[False].value

    def close(self):
        for s in self.solver.values():
            self.h.GCGE_PCGDestroy(C.byref(s), self.o.ops_handle)
        self.h.GCGE_AMGDestroy(C.byref(self.amg), self.o.ops_handle)

    def deflated(self, b, shift, amg=True, y0=None, X=None, k=K, tol=TOL, max_iter=500, alias=None):
        """(y, rel_res, col_iters, return code) of one GCGE_PCGSolveDeflated; alias "b" / "y": X is that block"""
        o, m = self.o, b.shape[1]
        mb = o.mv_from_numpy(self.mA, b)
        my = o.mv_from_numpy(self.mA, np.zeros_like(b) if y0 is None else y0)
        X = self.X if X is None else X
        mX = o.mv_from_numpy(self.mA, X)
        shift = np.ascontiguousarray(shift, dtype=np.float64)
        rel, it = np.full(m, -1.0), np.full(m, -1, dtype=np.int32)
        try:
            rc = self.h.GCGE_PCGSolveDeflated(self.solver[amg], self.mB, {"b": mb, "y": my}.get(alias, mX), 0, k, ptr(shift), mb, 0, my, 0,
                                              m, tol, max_iter, 1 if y0 is None else 0, ptr(rel), ptr(it), o.ops_handle)
            y = o.mv_to_numpy(my, self.n, 0, m)
        finally:
            for mv, cols in ((mb, m), (my, m), (mX, X.shape[1])):
                o.ops.mv_destroy(mv, cols)
        return y, rel, it, rc

    def plain(self, b, amg=True):
        """x of GCGE_PCGSolve on the same solver"""
        o, m = self.o, b.shape[1]
        mb, mx = o.mv_from_numpy(self.mA, b), o.mv_from_numpy(self.mA, np.zeros_like(b))
        rel, it = np.zeros(m), np.zeros(m, dtype=np.int32)
        try:
            rc = self.h.GCGE_PCGSolve(self.solver[amg], mb, 0, mx, 0, m, 1e-8, 200, 1, ptr(rel), ptr(it), o.ops_handle)
            assert rc == m
            return o.mv_to_numpy(mx, self.n, 0, m), rel, it
        finally:
            o.ops.mv_destroy(mb, m)
            o.ops.mv_destroy(mx, m)

    def Qt(self, v):
        return v - self.MX @ (self.X.T @ v)

    def Q(self, v):
        return v - self.X @ (self.MX.T @ v)

    def op(self, y, shift):
        return self.Ad @ y - (y if self.Bd is None else self.Bd @ y) * shift[None, :]

    def dense(self, b, shift):
        """the solution of the projected systems, column by column: Q lstsq(Q^T (A - shift B) Q, Q^T b)"""
        I = np.eye(self.n)
        Qm = I - self.X @ self.MX.T
        out = np.zeros_like(b)
        for j in range(b.shape[1]):
            Op = Qm.T @ (self.Ad - shift[j] * (I if self.Bd is None else self.Bd)) @ Qm
            out[:, j] = Qm @ np.linalg.lstsq(Op, Qm.T @ b[:, j], rcond=1e-12)[0]
        return out

    def bound(self, y, shift):
        kappa = (self.lam[-1] - shift) / (self.lam[K] - shift)
        if self.Bd is not None:
            kappa = kappa * np.linalg.cond(self.Bd)
        return kappa * (TOL + self.n * EPS) * np.linalg.norm(y, axis=0)

    def true_rel(self, b, y, shift):
        return np.linalg.norm(self.Qt(b - self.op(y, shift)), axis=0) / np.linalg.norm(self.Qt(b), axis=0)


@pytest.fixture(scope="module")
def std(oracle):
    c = Case(oracle, False)
    yield c
    c.close()


@pytest.fixture(scope="module")
def std_data(std):
    """(b, shifts, the dense solution, the solver's result with the hierarchy) shared by the tests on the standard problem"""
    b = np.asfortranarray(np.random.default_rng(5).standard_normal((std.n, K)))
    shift = std.lam[:K].copy()
    return b, shift, std.dense(b, shift), std.deflated(b, shift)


def check(c, b, shift, yd, result, what):
    y, rel, it, rc = result
    err, bound = np.linalg.norm(y - yd, axis=0), c.bound(yd, shift)
    true = c.true_rel(b, y, shift)
    orth = np.linalg.norm(c.MX.T @ y, axis=0) / np.linalg.norm(y, axis=0)
    print(what, "error / bound:", err / bound, "rel_res:", rel, "recomputed:", true, "|X^T M y| / |y|:", orth, "iterations:", it)
    assert rc == b.shape[1]
    assert np.all(err <= bound)                                         # (a)
    assert np.all(rel <= TOL) and np.all(true <= TOL)                   # (b): the TRUE projected residual
    assert np.all(orth <= 1e-10)
    assert np.all(it >= 1)


def test_solution_against_the_dense_projected_solve(std, std_data):
    b, shift, yd, result = std_data
    assert np.linalg.norm(std.Q(yd) - yd) <= 1e-9 * np.linalg.norm(yd)   # (the reference lies in range(Q))
    check(std, b, shift, yd, result, "V-cycle:")


def test_without_a_hierarchy_the_same_answer_in_more_iterations(std, std_data):
    b, shift, yd, (y, rel, it, rc) = std_data
    plain = std.deflated(b, shift, amg=False)
    check(std, b, shift, yd, plain, "identity:")
    print("iterations with the V-cycle:", it, "with the identity:", plain[2])
    assert np.all(np.linalg.norm(plain[0] - y, axis=0) <= std.bound(yd, shift))
    assert np.all(it < plain[2])


def test_generalised(oracle):
    c = Case(oracle, True)
    try:
        b = np.asfortranarray(np.random.default_rng(6).standard_normal((c.n, K)))
        shift = c.lam[:K].copy()
        check(c, b, shift, c.dense(b, shift), c.deflated(b, shift), "generalised:")
    finally:
        c.close()


def test_a_right_hand_side_inside_the_span_of_MX_gives_zero(std, std_data):
    b, shift, yd, (y, rel, it, rc) = std_data
    b2 = b.copy(order="F")
    b2[:, 2] = std.MX @ np.array([1.0, -2.0, 0.5, 3.0])
    y0 = np.asfortranarray(uniform(61, b.shape) - 0.5)                   # a start that is NOT zero: the column is still zeroed
    for start in (None, y0):
        y2, rel2, it2, rc2 = std.deflated(b2, shift, y0=start)
        assert rc2 == K and rel2[2] == 0.0 and it2[2] == 0 and np.all(y2[:, 2] == 0.0)
        keep = [0, 1, 3]
        assert np.all(np.linalg.norm(y2[:, keep] - yd[:, keep], axis=0) <= std.bound(yd, shift)[keep])


class Comm(C.Structure):
    """GCGE_COMM (include/gcge_ops.h)"""
    _fields_ = [("rank", C.c_int), ("size", C.c_int), ("allreduce_sum", C.c_void_p), ("ctx", C.c_void_p)]


def test_bad_arguments_and_a_communicator_write_nothing(std, std_data):
    b, shift, _, _ = std_data
    y0 = np.asfortranarray(uniform(67, b.shape))

    def nothing_written(result, code):
        y, rel, it, rc = result
        assert rc == code
        assert np.array_equal(bits(np.ascontiguousarray(y)), bits(np.ascontiguousarray(y0)))
        assert np.all(rel == -1.0) and np.all(it == -1)

    nothing_written(std.deflated(b, shift, y0=y0, k=-1), -1)
    nothing_written(std.deflated(b, shift, y0=y0, alias="b"), -1)
    nothing_written(std.deflated(b, shift, y0=y0, alias="y"), -1)
    wide = np.asfortranarray(np.hstack([b, b[:, :1]]))                   # 5 columns on a solver of 4
    y, rel, it, rc = std.deflated(wide, np.append(shift, shift[0]))
    assert rc == -1 and np.all(y == 0.0) and np.all(rel == -1.0) and np.all(it == -1)
    reduce = C.CFUNCTYPE(None, C.POINTER(C.c_double), C.c_int, C.c_void_p)(lambda buf, n, ctx: None)
    comm = Comm(0, 2, C.cast(reduce, C.c_void_p), None)
    std.h.GCGE_SetComm(C.byref(comm))
    try:
        for amg in (True, False):
            nothing_written(std.deflated(b, shift, y0=y0, amg=amg), -2)
    finally:
        std.h.GCGE_SetComm(None)


def test_the_plain_solve_on_the_same_solver_keeps_its_bits_and_the_table_is_left_as_found(std, std_data):
    b, shift, _, _ = std_data
    ops = std.o.ops.struct
    for amg in (True, False):
        before = std.plain(b, amg)
        was = (ops.MultiLinearSolver, ops.multi_linear_solver_workspace)
        assert std.deflated(b, shift, amg=amg)[3] == K
        assert (ops.MultiLinearSolver, ops.multi_linear_solver_workspace) == was
        after = std.plain(b, amg)
        for u, v in zip(before[:2], after[:2]):
            assert np.array_equal(bits(np.ascontiguousarray(u)), bits(np.ascontiguousarray(v)))
        assert np.array_equal(before[2], after[2])
