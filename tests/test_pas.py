"""PAS: the composite (augmented) operator table, the PAS eigensolver with GCG warm-started from it, and the fused bordered
product of the HIP back-end (include/gcge_pas.h, csrc/host/pas.c, csrc/hip/pas_border.hip).

CPU cases run over the oracle table (its slots are the reference's app_ccs restated); GPU cases are marked `gpu`.
Correctness is pinned against numpy on the assembled augmented matrices, closed forms and the oracle's plain GCG."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import pyoracle as po
from gcge_amd.lib import CSR, MG, host_lib, make_problem, run_gcg, run_pas
from gcge_amd.ops_struct import OPS, OpsTable
from helpers import OracleBackend, csr_from_scipy, lap3d_exact, uniform

_IDFN = C.CFUNCTYPE(C.c_void_p, C.c_void_p)
_FREEFN = C.CFUNCTYPE(None, C.c_void_p)
_kept = {}


def _oracle_identity(like):
    """The identity of the size of an oracle matrix (ORACLE_CCS), for PAS's coarse masses of a standard problem."""
    n = C.cast(like, C.POINTER(po.OCcs)).contents.nrows
    rp = np.arange(n + 1, dtype=np.int32)
    ci = np.arange(n, dtype=np.int32)
    va = np.ones(n)
    m = po.OCcs()
    m.data = va.ctypes.data_as(C.POINTER(C.c_double))
    m.i_row = ci.ctypes.data_as(C.POINTER(C.c_int))
    m.j_col = rp.ctypes.data_as(C.POINTER(C.c_int))
    m.nrows = m.ncols = n
    _kept[C.addressof(m)] = (m, rp, ci, va)
    return C.addressof(m)


def _oracle_free(p):
    _kept.pop(p, None)


_CALLBACKS = (_IDFN(_oracle_identity), _FREEFN(_oracle_free))


def oracle_backend():
    """The oracle table with an identity upload registered for PAS (the oracle registers no back-end record)."""
    h = host_lib()
    h.GCGE_PAS_SetMatIdentity(*_CALLBACKS)
    return OracleBackend()


class PASMAT(C.Structure):
    _fields_ = [("QQ", C.c_void_p), ("alpha", C.c_double), ("QX", C.c_void_p), ("XX", C.POINTER(C.c_double)),
                ("size", C.c_int), ("mat_H", C.c_void_p)]


class Dense(C.Structure):
    _fields_ = [("data", C.POINTER(C.c_double)), ("nrows", C.c_int), ("ncols", C.c_int), ("ldd", C.c_int)]


class PASVEC(C.Structure):
    _fields_ = [("q", C.c_void_p), ("x", Dense), ("owned", C.c_int)]


def hierarchy(backend, mA, mB, levels):
    """ops->MultiGridCreate of the backend: (A handles, B handles, P handles, destroy())."""
    st = C.cast(backend.ops_handle, C.POINTER(OPS)).contents
    A_arr, B_arr, P_arr, nl = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int(levels)
    create = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.c_void_p,
                         C.c_void_p)(st.MultiGridCreate)
    destroy = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_void_p)(st.MultiGridDestroy)
    create(C.byref(A_arr), C.byref(B_arr), C.byref(P_arr), C.byref(nl), mA, mB, backend.ops_handle)
    L = nl.value
    Ah = [C.c_void_p(v) for v in C.cast(A_arr, C.POINTER(C.c_void_p * L)).contents]
    Bh = [C.c_void_p(v) for v in C.cast(B_arr, C.POINTER(C.c_void_p * L)).contents]
    Ph = [C.c_void_p(v) for v in C.cast(P_arr, C.POINTER(C.c_void_p * max(1, L - 1))).contents][:L - 1]
    return Ah, Bh, Ph, lambda: destroy(C.byref(A_arr), C.byref(B_arr), C.byref(P_arr), C.byref(nl), backend.ops_handle)


def mg_scale():
    h = host_lib()
    s, r, t = C.c_double(), C.c_int(), C.c_double()
    h.gcge_mg_get_defaults(C.byref(s), C.byref(r), C.byref(t))
    return s.value


class Setup:
    """A 3-level hierarchy of `kind` through `backend`, the coarse A_H / B_H as dense arrays, and a composite table."""

    def __init__(self, backend, kind, size):
        h = host_lib()
        self.b = backend
        A, B = make_problem(kind, size)
        self.A = A
        self.mA = backend.matrix(A)
        if B is None:
            Ic, self._ikeep = csr_from_scipy(sp.identity(A.nrows, format="csr"))
            self.mI = backend.matrix(Ic)
            self.mB0 = None
        else:
            self.mI = backend.matrix(B)
            self.mB0 = self.mI
        # small problems: let the hierarchy go down to a few rows (restored right after the build)
        sc, mr, th = C.c_double(), C.c_int(), C.c_double()
        h.gcge_mg_get_defaults(C.byref(sc), C.byref(mr), C.byref(th))
        h.gcge_mg_set_defaults(sc, C.c_int(4), th)
        try:
            self.Ah, self.Bh, self.Ph, self.done = hierarchy(backend, self.mA, self.mI, 3)
            self.nH = self.apply_dense_rows()
        finally:
            h.gcge_mg_set_defaults(sc, mr, th)
        assert len(self.Ah) == 3
        self.H = 2
        self.AH = self.dense(self.Ah[2])
        self.BH = self.dense(self.Bh[2])
        self.alpha = mg_scale() ** -self.H
        self.pas = C.c_void_p()
        h.OPS_Create(C.byref(self.pas))
        h.OPS_PAS_Set(self.pas, backend.ops_handle)
        h.OPS_Setup(self.pas)
        h.GCGE_SetQuiet(self.pas, 1)
        self.t = OpsTable(self.pas)
        self._keep = []

    def apply_dense_rows(self):
        """rows of level H, from the host builder the back-ends' MultiGridCreate runs (gcge_mg_build, same defaults)"""
        h = host_lib()
        mg = MG()
        assert h.gcge_mg_build(C.byref(self.A), None, 3, 0, 0.0, C.byref(mg)) == 0
        assert mg.num_levels == 3
        n = mg.A[2].nrows
        h.gcge_mg_free(C.byref(mg))
        return n

    def dense(self, m):
        n = self.nH
        x = self.b.mv_from_numpy(self.Ah[2], np.eye(n))
        y = self.b.ops.mv_create(n, self.Ah[2])
        self.b.ops.spmm(m, x, y, (0, 0), (n, n))
        return self.b.mv_to_numpy(y, n, 0, n)

    def pasmat(self, QX_block, XX, s, b_matrix=False):
        XXa = np.asfortranarray(XX, dtype=np.float64) if XX is not None else None
        m = PASMAT(self.Bh[2].value if b_matrix else self.Ah[2].value, 1.0 if b_matrix else self.alpha,
                   None if b_matrix else QX_block, None if b_matrix else XXa.ctypes.data_as(C.POINTER(C.c_double)), s,
                   self.Ah[2].value)
        self._keep.append((m, XXa))
        return C.cast(C.pointer(m), C.c_void_p)

    def pasvec(self, q, x):
        """A composite block around a coarse block holding q (nH x k) and a host tail x (s x k)."""
        xa = np.asfortranarray(x, dtype=np.float64)
        qb = self.b.mv_from_numpy(self.Ah[2], q)
        v = PASVEC(qb, Dense(xa.ctypes.data_as(C.POINTER(C.c_double)), xa.shape[0], xa.shape[1], xa.shape[0]), 0)
        self._keep.append((v, xa))
        return C.cast(C.pointer(v), C.c_void_p), xa

    def read(self, pv, k):
        v = C.cast(pv, C.POINTER(PASVEC)).contents
        q = self.b.mv_to_numpy(C.c_void_p(v.q), self.nH, 0, k)
        x = np.ctypeslib.as_array(v.x.data, shape=(k, v.x.ldd)).T[:v.x.nrows].copy()
        return np.vstack([q, x])


def augmented(S, QX, XX):
    M = np.block([[S.alpha * S.AH, QX], [QX.T, XX]])
    Bm = np.block([[S.BH, np.zeros((S.nH, QX.shape[1]))], [np.zeros((QX.shape[1], S.nH)), np.eye(QX.shape[1])]])
    return M, Bm


def cols(xr, yr):
    """(x columns, y columns) -> the (start, end) pairs of the slot calls"""
    return (xr[0], yr[0]), (xr[1], yr[1])


def rel(a, b):
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


def composite_algebra(backend, kind, size, s=5, k=7):
    S = Setup(backend, kind, size)
    n = S.nH
    QX = uniform(11, (n, s)) - 0.5
    XX = uniform(12, (s, s)) - 0.5
    XX = XX + XX.T
    QXb = backend.mv_from_numpy(S.Ah[2], QX)
    mA = S.pasmat(QXb, XX, s)
    mB = S.pasmat(None, None, s, b_matrix=True)
    M, Bm = augmented(S, QX, XX)
    Z = uniform(13, (n + s, k)) - 0.5
    Y0 = uniform(14, (n + s, k)) - 0.5
    X, _ = S.pasvec(Z[:n], Z[n:])
    Y, _ = S.pasvec(Y0[:n], Y0[n:])
    t = S.t
    out = {}
    # products on odd column ranges
    t.spmm(mA, X, Y, *cols((1, 6), (2, 7)))
    R = S.read(Y, k)
    out["A"] = rel(R[:, 2:7], M @ Z[:, 1:6])
    t.spmm(mB, X, Y, *cols((3, 6), (0, 3)))
    R = S.read(Y, k)
    out["B"] = rel(R[:, 0:3], Bm @ Z[:, 3:6])
    # inner products 'N', 'S', 'D'
    W = S.read(Y, k)
    out["N"] = rel(t.inner_prod("N", X, Y, *cols((1, 4), (2, 7))), Z[:, 1:4].T @ W[:, 2:7])
    out["S"] = rel(t.inner_prod("S", X, X, *cols((1, 6), (1, 6))), Z[:, 1:6].T @ Z[:, 1:6])
    out["D"] = rel(t.inner_prod("D", X, Y, *cols((1, 6), (2, 7))), np.einsum("ij,ij->j", Z[:, 1:6], W[:, 2:7]))
    # Q^T A P through the composite product
    ws, _ = S.pasvec(np.zeros((n, k)), np.zeros((s, k)))
    out["QtAP"] = rel(t.qtap("S", "N", X, mA, X, *cols((0, 3), (1, 6)), ws), Z[:, 0:3].T @ M @ Z[:, 1:6])
    # LinearComb and Axpby
    coef = uniform(15, (3, 4))
    beta = np.array([0.5, -1.0, 2.0, 0.25])
    W = S.read(Y, k)
    t.lincomb(X, Y, *cols((1, 4), (3, 7)), coef, 3, beta, 1)
    out["LinearComb"] = rel(S.read(Y, k)[:, 3:7], Z[:, 1:4] @ coef + W[:, 3:7] * beta)
    W = S.read(Y, k)
    t.axpby(0.75, X, -1.5, Y, *cols((0, 5), (1, 6)))
    out["Axpby"] = rel(S.read(Y, k)[:, 1:6], 0.75 * Z[:, 0:5] - 1.5 * W[:, 1:6])
    S.done()
    return out


@pytest.mark.parametrize("kind,size", [("lap3d", 8), ("fe3d", 6)])
def test_composite_algebra_matches_numpy(kind, size):
    errs = composite_algebra(oracle_backend(), kind, size)
    assert all(v < 1e-13 for v in errs.values()), errs


def galerkin_gap(backend, kind, size):
    """x = 0: the composite Rayleigh quotient of a coarse q against the fine-level one of P_H q."""
    S = Setup(backend, kind, size)
    s = 3
    n = S.nH
    q = uniform(21, (n, 2)) - 0.5
    QXb = backend.mv_from_numpy(S.Ah[2], np.zeros((n, s)))
    mA = S.pasmat(QXb, np.zeros((s, s)), s)
    mB = S.pasmat(None, None, s, b_matrix=True)
    X, _ = S.pasvec(q, np.zeros((s, 2)))
    ws, _ = S.pasvec(np.zeros((n, 2)), np.zeros((s, 2)))
    num = S.t.qtap("S", "D", X, mA, X, *cols((0, 2), (0, 2)), ws)
    den = S.t.qtap("S", "D", X, mB, X, *cols((0, 2), (0, 2)), ws)
    # P_0 P_1 q on level 0
    qb = backend.mv_from_numpy(S.Ah[2], q)
    mid = backend.ops.mv_create(2, S.Ah[1])
    fine = backend.ops.mv_create(2, S.Ah[0])
    backend.ops.spmm(S.Ph[1], qb, mid, (0, 0), (2, 2))
    backend.ops.spmm(S.Ph[0], mid, fine, (0, 0), (2, 2))
    v = backend.mv_to_numpy(fine, S.A.nrows, 0, 2)
    Af = backend.ops.mv_create(2, S.mA)
    backend.ops.spmm(S.mA, fine, Af, (0, 0), (2, 2))
    Av = backend.mv_to_numpy(Af, S.A.nrows, 0, 2)
    if S.mB0 is not None:
        Bf = backend.ops.mv_create(2, S.mA)
        backend.ops.spmm(S.mB0, fine, Bf, (0, 0), (2, 2))
        Bv = backend.mv_to_numpy(Bf, S.A.nrows, 0, 2)
    else:
        Bv = v
    rq_fine = np.einsum("ij,ij->j", v, Av) / np.einsum("ij,ij->j", v, Bv)
    S.done()
    return float(np.max(np.abs(num / den - rq_fine) / np.abs(rq_fine)))


@pytest.mark.parametrize("kind,size", [("lap3d", 8), ("fe3d", 6)])
def test_galerkin_exactness(kind, size):
    assert galerkin_gap(oracle_backend(), kind, size) < 1e-13


def pas_on(backend, kind, size, args, **kw):
    A, B = make_problem(kind, size, **kw)
    mA = backend.matrix(A)
    mB = backend.matrix(B) if B is not None else None
    return run_pas(backend.ops_handle, mA, mB, args), (mA, mB)


def test_pas_alone_closed_form():
    o = oracle_backend()
    (ev, pr, gr), _ = pas_on(o, "lap3d", 20, ["-nevConv", 20, "-gcge_pas_only", 1, "-gcge_pas_rel_tol", 1e-8])
    assert pr.nevConv >= 20 and pr.num_levels == 3
    assert gr.numIter == 0
    assert np.max(np.abs(ev[:20] - lap3d_exact(20, 20))) < 1e-10


@pytest.mark.parametrize("kind,size,nev", [("lap3d", 20, 20), ("fe3d", 12, 10)])
def test_pas_then_gcg_matches_plain_gcg(kind, size, nev):
    o = oracle_backend()
    (ev, pr, gr), (mA, mB) = pas_on(o, kind, size, ["-nevConv", nev])
    ev0, r0 = run_gcg(o.ops_handle, mA, mB, ["-nevConv", nev])
    assert gr.nevConv >= nev and r0.nevConv >= nev
    assert np.max(np.abs(ev[:nev] - ev0[:nev])) < 1e-10
    assert 2 * gr.numIter <= r0.numIter, (gr.numIter, r0.numIter)
    # the file-level state of the GCG driver belongs to the last solve: a GCG after PAS reports its own run
    ev1, r1 = run_gcg(o.ops_handle, mA, mB, ["-nevConv", nev])
    assert r1.numIter == r0.numIter and np.array_equal(ev1, ev0)


def test_pas_error_codes():
    o = oracle_backend()
    A, _ = make_problem("lap3d", 8)
    mA = o.matrix(A)
    with pytest.raises(RuntimeError, match="rc=-7"):
        run_pas(o.ops_handle, mA, None, ["-nevConv", 4, "-gcge_pas_levels", 1])
    st = C.cast(o.ops_handle, C.POINTER(OPS)).contents
    st.MultiGridCreate = None
    with pytest.raises(RuntimeError, match="rc=-7"):
        run_pas(o.ops_handle, mA, None, ["-nevConv", 4])


# ---------------------------------------------------------------------------------------------------------------- GPU
def border_call(g, QX, s, q, q0, y, y0, m, beta, t, gout):
    fn = g.gcge_hip_pas_border
    tt = np.asfortranarray(t)
    rc = fn(QX, s, q, q0, y, y0, m, beta, tt.ctypes.data_as(C.POINTER(C.c_double)), tt.shape[0],
            gout.ctypes.data_as(C.POINTER(C.c_double)), gout.shape[0])
    assert rc == 0


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1000, 65537])
def test_border_kernel_against_numpy(n):
    from gcge_amd import HipBackend
    hip = HipBackend()
    Ac, keep = csr_from_scipy(sp.identity(n, format="csr"))
    mat = hip.matrix(Ac)
    for s in (1, 7, 64, 128, 200, 256):
        QXh = uniform(31 + s, (n, s + 3)) - 0.5
        QX = hip.mv_from_numpy(mat, QXh)
        for m in (1, 5, 64, 128):
            q0, y0 = 3, 1
            qh = uniform(41 + m, (n, q0 + m + 2)) - 0.5
            yh = uniform(51 + m, (n, y0 + m)) - 0.5
            t = uniform(61 + s + m, (s, m)) - 0.5
            q = hip.mv_from_numpy(mat, qh)
            outs = []
            for _ in range(2):
                y = hip.mv_from_numpy(mat, yh)
                g = np.zeros((s, m), order="F")
                border_call(hip.g, QX, s, q, q0, y, y0, m, 0.5, t, g)
                outs.append((hip.mv_to_numpy(y, n, 0, y0 + m), g.copy()))
            Yref = 0.5 * yh[:, y0:y0 + m] + QXh[:, :s] @ t
            Gref = QXh[:, :s].T @ qh[:, q0:q0 + m]
            Y, G = outs[0]
            assert rel(Y[:, y0:], Yref) < 1e-13, (s, m)
            assert np.array_equal(Y[:, :y0], yh[:, :y0])
            assert rel(G, Gref) < 1e-13, (s, m)
            assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]), (s, m)
    hip.free_matrix(mat)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,size", [("lap3d", 8), ("fe3d", 6)])
def test_composite_product_hip_fused_equals_oracle_slots(kind, size):
    from gcge_amd import HipBackend
    res = {}
    for name, b in (("hip", HipBackend()), ("oracle", oracle_backend())):
        S = Setup(b, kind, size)
        n, s, k = S.nH, 5, 7
        QX = uniform(11, (n, s)) - 0.5
        XX = uniform(12, (s, s)) - 0.5
        XX = XX + XX.T
        mA = S.pasmat(b.mv_from_numpy(S.Ah[2], QX), XX, s)
        Z = uniform(13, (n + s, k)) - 0.5
        X, _ = S.pasvec(Z[:n], Z[n:])
        Y, _ = S.pasvec(np.zeros((n, k)), np.zeros((s, k)))
        S.t.spmm(mA, X, Y, *cols((1, 6), (2, 7)))
        res[name] = S.read(Y, k)[:, 2:7]
        M, _ = augmented(S, QX, XX)
        assert rel(res[name], M @ Z[:, 1:6]) < 1e-13, name
        S.done()
    assert rel(res["hip"], res["oracle"]) < 1e-13


@pytest.mark.gpu
@pytest.mark.parametrize("kind,size,nev", [("lap3d", 24, 20), ("fe3d", 16, 10), ("sio2", 20, 10)])
def test_pas_then_gcg_hip_matches_oracle_gcg(kind, size, nev):
    from gcge_amd import HipBackend
    hip = HipBackend()
    (ev, pr, gr), _ = pas_on(hip, kind, size, ["-nevConv", nev])
    o = OracleBackend()
    A, B = make_problem(kind, size)
    ev0, r0 = run_gcg(o.ops_handle, o.matrix(A), o.matrix(B) if B is not None else None, ["-nevConv", nev])
    assert gr.nevConv >= nev and r0.nevConv >= nev
    assert np.max(np.abs(ev[:nev] - ev0[:nev]) / np.abs(ev0[:nev])) < 1e-10
