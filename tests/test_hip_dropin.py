"""GPU: the literal drop-in.  The REFERENCE's compiled solver stack — its GCG
(src/ops_eig_sol_gcg.c:1253), its ModifiedGramSchmidt (src/ops_orth.c:203-393), its BlockPCG
(src/ops_lin_sol.c:140-437), its OPS_Setup defaults (src/ops.c:60-149) — from oracle/_ref/libgcge_ref.so
drives the slots OPS_HIP_Set filled, exactly as test/test_app_ccs.c drives OPS_CCS_Set.  Checked against the
reference-only runs in tests/golden/.  Plus the slots no other GPU test calls directly (a5, a11) and the file
ingestion path end to end (f3)."""
import ctypes as C
import os

import numpy as np
import pytest

import pyoracle as po
from helpers import csr_to_scipy, load_golden, uniform
from gcge_amd.lib import CSR, host_lib, make_problem, run_gcg

pytestmark = pytest.mark.gpu
GCG = load_golden("gcg.json")
SHAPES = load_golden("gcg_shapes.json")


def _fresh_hip_table(hip):
    """A table only OPS_HIP_Set has touched: every default is then back-filled by the REFERENCE's OPS_Setup."""
    ops = C.c_void_p()
    hip.h.OPS_Create(C.byref(ops))
    hip.g.OPS_HIP_Set(ops)
    return ops


def _ref_stack_on_hip(hip, c, flag):
    ref = po.ref_lib()
    ops = _fresh_hip_table(hip)
    if flag == 1:      # test_app_ccs.c:109-120: the back-end's own solver behind ops->MultiLinearSolver
        hip.g.gcge_hip_bpcg_setup(ops, 30, 1e-2, 1e-14, b"abs")
    hip.set_random_mode(0)
    A, B = make_problem(c["kind"], c["size"], **c.get("kw", {}))
    mA = hip.matrix(A)
    mB = hip.matrix(B) if B is not None else None
    ref.ref_gcg_solve_foreign.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.c_double, C.c_double, C.c_int, C.c_int, C.POINTER(C.c_double),
                                          C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double)]
    nm = c["nev_max"] or 2 * c["nev"]
    ev = np.zeros(nm)
    conv, it, sec = C.c_int(), C.c_int(), C.c_double()
    rc = ref.ref_gcg_solve_foreign(ops, mA, mB, c["nev"], c["nev_max"], c["block"], c.get("nev_init", 0),
                                   1e-1, 1e-8, 500, flag, ev.ctypes.data_as(C.POINTER(C.c_double)),
                                   C.byref(conv), C.byref(it), C.byref(sec))
    assert rc == 0
    hip.free_matrix(mA)
    if mB is not None:
        hip.free_matrix(mB)
    return ev, conv.value, it.value, sec.value


@pytest.mark.skipif(po.ref_lib() is None, reason="oracle/_ref not present on this box")
@pytest.mark.parametrize("flag", [0, 1])
@pytest.mark.parametrize("key", ["lap3d_12_nev10", "fe3d_12_nev10", "lap3d_16_nev12_b8"])
def test_reference_stack_drives_hip_slots(hip, key, flag):
    c = GCG[key]
    ev, conv, it, _ = _ref_stack_on_hip(hip, c, flag)
    assert conv == c["nevConv"] and abs(it - c["numIter"]) <= 2, (conv, it, c["numIter"])
    refv = np.array(c["eval"])
    assert np.max(np.abs(ev[:len(refv)] - refv) / np.abs(refv)) < 1e-10


@pytest.mark.skipif(po.ref_lib() is None, reason="oracle/_ref not present on this box")
@pytest.mark.parametrize("flag", [0, 1])
@pytest.mark.parametrize("key", ["lap3d_12_nev10", "fe3d_12_nev10"])
def test_reference_harness_function_over_the_hip_table(hip, key, flag):
    """north_star, literally: "TestEigenSolverGCG() is a drop-in".  The reference's OWN harness function
    (test/test_eig_sol_gcg.c:28-169, compiled from /root/reference into oracle/_ref/libgcge_ref.so, linked -Bsymbolic so that
    every call inside it stays inside the reference) runs over a table only OPS_HIP_Set has touched, with the back-end's matrix
    handles and the command line test/main.c would pass; what it prints through ops->Printf — "numIter = .., nevConv = .."
    and one line per eigenvalue (:139-165) — is parsed and compared with the reference-only run in tests/golden/gcg.json."""
    import re
    c = GCG[key]
    ref = po.ref_lib()
    ops = _fresh_hip_table(hip)
    if flag == 1:
        hip.g.gcge_hip_bpcg_setup(ops, 30, 1e-2, 1e-14, b"abs")
    hip.set_random_mode(0)
    A, B = make_problem(c["kind"], c["size"], **c.get("kw", {}))
    mA = hip.matrix(A)
    mB = hip.matrix(B) if B is not None else None
    words = ["test_app_hip", "-nevConv", str(c["nev"]), "-gcge_print_usage", "0"]
    argv = (C.c_char_p * len(words))(*[w.encode() for w in words])
    log = C.c_char_p()
    ref.ref_test_eigen_solver_gcg.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p)]
    rc = ref.ref_test_eigen_solver_gcg(ops, mA, mB, flag, len(words), argv, C.byref(log))
    text = log.value.decode()
    hip.free_matrix(mA)
    if mB is not None:
        hip.free_matrix(mB)
    assert rc == 0 and "GCG Eigen Solver" in text, text[-600:]
    m = re.search(r"numIter = (\d+), nevConv = (\d+)", text)
    assert m, text[-600:]
    it, conv = int(m.group(1)), int(m.group(2))
    vals = [float(v) for v in re.findall(r"^\d+: ([-+0-9.eE]+)$", text.split("eigenvalues")[-1], flags=re.M)]
    assert len(vals) == conv and conv == c["nevConv"] and abs(it - c["numIter"]) <= 2, (conv, it, c["nevConv"], c["numIter"])
    refv = np.array(c["eval"][:conv])
    assert np.max(np.abs(np.array(vals) - refv) / np.abs(refv)) < 1e-10


def test_c_main_calls_the_compiled_TestAppHIP(tmp_path):
    """the back-end exports `TestAppHIP(int argc, char **argv)` — the counterpart of TestAppCCS
    (test/test_app_ccs.c:86-140) — and a plain-C main (tools/test_app_hip_main.c = test/main.c with that one call) runs it:
    the reference's stock 1-D pair (n = 807: 38 iterations, lambda_1 = 9.8696 — the values SURVEY 8c lists), the same through the
    back-end's fused CG, and a matrix read from a Matrix Market file (the SuiteSparse form of the reference's SiO2 & co.)."""
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "gcge_amd", "lib")
    exe = str(tmp_path / "test_app_hip")
    subprocess.run(["gcc", "-O2", "-I" + os.path.join(root, "include"), os.path.join(root, "tools", "test_app_hip_main.c"), "-o", exe,
                    "-L" + lib, "-lgcge_hip", "-lgcge_host", "-Wl,-rpath," + lib, "-lm"], check=True)

    def run(*args):
        p = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        assert p.returncode == 0, p.stdout[-2000:]
        m = re.search(r"numIter = (\d+), nevConv = (\d+)", p.stdout)
        assert m, p.stdout[-2000:]
        vals = [float(v) for v in re.findall(r"^\d+: ([-+0-9.eE]+)$", p.stdout.split("eigenvalues")[-1], flags=re.M)]
        return int(m.group(1)), int(m.group(2)), np.array(vals)

    c = GCG.get("fe1d_807_nev30")
    it, conv, ev = run()                                            # no arguments: the stock pair, harness defaults (nevConv 30)
    assert conv >= 30 and abs(ev[0] - 9.86959196776013) < 1e-9 * 9.87, (it, conv, ev[:3])
    if c is not None:
        assert abs(it - c["numIter"]) <= 2 and np.max(np.abs(ev[:len(c["eval"])] - np.array(c["eval"])) / np.array(c["eval"])) < 1e-10
    else:
        assert abs(it - 38) <= 2, it                                # 38 iterations
    it1, conv1, ev1 = run("-hip_flag", 1)
    assert conv1 >= 30 and np.max(np.abs(ev1[:30] - ev[:30]) / ev[:30]) < 1e-9
    # a Matrix Market file -> TestAppHIP -> the same Ritz values as the generator's matrix
    h = host_lib()
    A, _ = make_problem("lap3d", 12)
    mtx = str(tmp_path / "lap12.mtx")
    assert h.gcge_save_matrix_market(mtx.encode(), C.byref(A), 1) == 0
    g = GCG["lap3d_12_nev10"]
    it2, conv2, ev2 = run("-hip_mtx_A", mtx, "-nevConv", g["nev"])
    refv = np.array(g["eval"])
    assert conv2 == g["nevConv"] and abs(it2 - g["numIter"]) <= 2 and np.max(np.abs(ev2[:len(refv)] - refv) / refv) < 1e-10


def _check_shape_run(c, ev, conv, it):
    """With block = 64 / 128 a whole block of pairs locks per iteration, so a run that reaches nev one iteration
    earlier or later than the reference's ends with a different converged count (the reference itself: 60 of the
    wanted 50 at the C2 shape): the wanted count, the iteration count (+-2) and every commonly converged value are
    pinned."""
    assert conv >= c["nev"] and abs(it - c["numIter"]) <= 2, (conv, c["nevConv"], it, c["numIter"])
    k = min(conv, c["nevConv"])
    refv = np.array(c["eval"][:k])
    assert np.max(np.abs(ev[:k] - refv) / np.abs(refv)) < 1e-10


@pytest.mark.skipif(po.ref_lib() is None, reason="oracle/_ref not present on this box")
def test_reference_stack_drives_hip_slots_c2_shape(hip):
    """BASELINE config 2's solver shape (nev 50, block 64, nevMax 128) on a 24^3 grid, fused CG behind flag 1."""
    c = SHAPES["c2shape_lap3d_24"]
    ev, conv, it, _ = _ref_stack_on_hip(hip, c, 1)
    _check_shape_run(c, ev, conv, it)


@pytest.mark.parametrize("key,variant", [("c2shape_lap3d_24", "mgs"), ("c2shape_lap3d_24", "chol+fused"),
                                         ("c3shape_fe3d_20", "mgs"), ("c3shape_fe3d_20", "chol+fused"),
                                         ("c4shape_lap3d_28", "chol+fused"),
                                         ("c5shape_sio2_24", "mgs"), ("c5shape_sio2_24", "chol+fused"),
                                         ("c1_lap3d_50", "mgs"), ("c1_lap3d_50", "chol+fused")])
def test_gcg_on_hip_at_baseline_solver_shapes(hip, key, variant):
    """Our driver over the HIP slots at the block / nevMax of BASELINE configs 2-5 (reduced grids; config 5: the
    SiO2-like matrix, dense-block + remainder SpMM) and BASELINE config 1 at FULL size (Lap3D 50^3, nev 20, harness
    defaults: the values SURVEY 8c lists), against the reference's own runs at those shapes: default column-wise MGS +
    host-scalar BlockPCG, and what bench.py runs (block Cholesky-QR + fused device CG)."""
    c = SHAPES[key]
    args = ["-nevConv", c["nev"]]
    if c["nev_max"]:
        args += ["-nevMax", c["nev_max"], "-blockSize", c["block"]]
    flag = 0
    if variant == "chol+fused":
        hip.g.gcge_hip_bpcg_setup(hip.ops_handle, 30, 1e-2, 1e-14, b"abs")
        args += ["-gcge_initX_orth_method", "chol", "-gcge_compW_orth_method", "chol"]
        flag = 1
    hip.set_random_mode(0)
    A, B = make_problem(c["kind"], c["size"], **c.get("kw", {}))
    mA = hip.matrix(A)
    mB = hip.matrix(B) if B is not None else None
    ev, res = run_gcg(hip.ops_handle, mA, mB, args, flag=flag)
    hip.free_matrix(mA)
    if mB is not None:
        hip.free_matrix(mB)
    _check_shape_run(c, ev, res.nevConv, res.numIter)


# ---- slots without a direct test so far ---------------------------------------------------------------------------

def test_mat_trans_dot_multivec_slot(hip):
    """a5: MatTransDotMultiVec (app/app_ccs.c:140-150) — symmetric matrices, so A^T X = A X."""
    A, B = make_problem("fe3d", 9)
    S = csr_to_scipy(B)
    n = B.nrows
    mat = hip.matrix(B)
    X = uniform(5, (n, 12)) - 0.5
    x = hip.mv_from_numpy(mat, X)
    y = hip.mv_from_numpy(mat, uniform(6, (n, 9)))
    fn = hip.ops.fn("MatTransDotMultiVec")
    fn(mat, x, y, (C.c_int * 2)(3, 1), (C.c_int * 2)(10, 8), hip.ops.handle)
    got = hip.mv_to_numpy(y, n, 0, 9)
    np.testing.assert_allclose(got[:, 1:8], S.T @ X[:, 3:10], rtol=0, atol=1e-13 * np.abs(S).max() * 15)
    assert np.array_equal(got[:, 0], uniform(6, (n, 9))[:, 0]) and np.array_equal(got[:, 8], uniform(6, (n, 9))[:, 8])
    hip.ops.mv_destroy(x, 12); hip.ops.mv_destroy(y, 9)
    hip.free_matrix(mat)


def test_multivec_create_by_multivec_and_view(hip, capfd):
    """a11: MultiVecCreateByMultiVec (zero-filled block of the donor's row count, app/app_lapack.c:245-259) and
    MultiVecView (rows x columns through ops->Printf in %6.4e, app/app_lapack.c:270-298)."""
    A, _ = make_problem("lap3d", 5)
    n = A.nrows
    mat = hip.matrix(A)
    X = uniform(9, (n, 6)) - 0.5
    x = hip.mv_from_numpy(mat, X)
    y = C.c_void_p()
    hip.ops.fn("MultiVecCreateByMultiVec")(C.byref(y), 4, x, hip.ops.handle)
    assert hip.g.gcge_hip_mv_nrows(y) == n and hip.g.gcge_hip_mv_ncols(y) == 4
    assert np.array_equal(hip.mv_to_numpy(y, n, 0, 4), np.zeros((n, 4)))
    hip.ops.axpby(2.0, x, 0.0, y, (1, 0), (5, 4))                # the new block works with the donor's columns
    np.testing.assert_array_equal(hip.mv_to_numpy(y, n, 0, 4), 2.0 * X[:, 1:5])
    view = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_int, C.c_void_p)(hip.ops.struct.MultiVecView)
    hip.h.GCGE_SetQuiet(hip.ops_handle, 0)
    try:
        capfd.readouterr()
        view(x, 2, 5, hip.ops.handle)
        C.CDLL(None).fflush(None)
        out = capfd.readouterr().out
    finally:
        hip.h.GCGE_SetQuiet(hip.ops_handle, 1)
    rows = [ln.split() for ln in out.strip().splitlines()]
    assert len(rows) == n and all(len(r) == 3 for r in rows)
    np.testing.assert_allclose(np.array(rows, dtype=float), X[:, 2:5], rtol=1e-4, atol=1e-12)   # 5 significant digits
    hip.ops.mv_destroy(y, 4)
    assert not y.value                                            # MultiVecDestroy clears the handle
    hip.ops.mv_destroy(x, 6)
    hip.free_matrix(mat)


# ---- f3: file -> PETSc binary loader -> CSR upload -> solve ---------------------------------------------------------

@pytest.mark.parametrize("key", ["lap3d_12_nev10", "fe3d_12_nev10"])
def test_petsc_binary_file_to_hip_solve(hip, tmp_path, key):
    """The reference's file path (test/test_app_slepc.c:416-445: MatLoad of a PETSc binary file, then the solver):
    matrices written in the published big-endian format by numpy, read back by gcge_load_petsc_binary, uploaded
    through gcge_hip_mat_create_csr, solved on the GPU; Ritz values against the reference's run on the same pair."""
    c = GCG[key]
    h = host_lib()
    A0, B0 = make_problem(c["kind"], c["size"])
    loaded = []
    for tag, M in (("A", A0), ("B", B0)):
        if M is None:
            loaded.append(None)
            continue
        S = csr_to_scipy(M)
        S.sort_indices()
        path = str(tmp_path / (tag + ".petsc"))
        with open(path, "wb") as f:
            np.array([1211216, S.shape[0], S.shape[1], S.nnz], dtype=">i4").tofile(f)
            np.diff(S.indptr).astype(">i4").tofile(f)
            S.indices.astype(">i4").tofile(f)
            S.data.astype(">f8").tofile(f)
        L = CSR()
        assert h.gcge_load_petsc_binary(os.fsencode(path), 0, -1, C.byref(L)) == 0
        loaded.append(L)
    mA = hip.matrix(loaded[0])
    mB = hip.matrix(loaded[1]) if loaded[1] is not None else None
    hip.set_random_mode(0)
    ev, res = run_gcg(hip.ops_handle, mA, mB, ["-nevConv", c["nev"]])
    assert res.nevConv == c["nevConv"] and abs(res.numIter - c["numIter"]) <= 2
    refv = np.array(c["eval"])
    assert np.max(np.abs(ev[:len(refv)] - refv) / np.abs(refv)) < 1e-10
    hip.free_matrix(mA)
    if mB is not None:
        hip.free_matrix(mB)
    for L in loaded:
        if L is not None:
            h.gcge_csr_free(C.byref(L))


def test_masked_grid_from_a_matrix_market_file_takes_the_sweep(hip, oracle, tmp_path):
    """VERDICT r3 item 3, end to end: the operator on the ball (rows = grid points inside a sphere in scan order, the layout of the
    PARSEC matrices of test/submit.sh:9-15) written as a Matrix-Market file (symmetric, lower triangle: how SuiteSparse ships
    them), read back, uploaded by gcge_hip_mat_create — which recovers the grid from the rows, so the file's matrix takes the
    plane sweep — and solved; against the CPU oracle's solve of the same file."""
    from gcge_amd import load_matrix_market
    h, g = host_lib(), hip.g
    A, _ = make_problem("sio2ball", 22, K=8, R0=1.5, R1=3.0, seed=12345)
    path = str(tmp_path / "ball22.mtx")
    assert h.gcge_save_matrix_market(path.encode(), C.byref(A), 1) == 0
    L = load_matrix_market(path)
    assert (L.nrows, L.nnz) == (A.nrows, A.nnz)
    g.gcge_hip_spmm_dense_mode(1)
    try:
        mA = hip.matrix(L)
        form = g.gcge_hip_mat_spmm_form(mA).decode()
        assert form.startswith("spmm_star+spmm_dense"), form
        args = ["-nevConv", 8, "-nevMax", 24, "-blockSize", 8]
        g.gcge_hip_bpcg_setup(hip.ops_handle, 30, 1e-2, 1e-14, b"abs")
        hip.set_random_mode(0)
        ev, res = run_gcg(hip.ops_handle, mA, None, args + ["-gcge_initX_orth_method", "chol", "-gcge_compW_orth_method", "chol"], flag=1)
        evo, reso = run_gcg(oracle.ops_handle, oracle.matrix(L), None, args)
        hip.free_matrix(mA)
    finally:
        g.gcge_hip_spmm_dense_mode(0)
    k = min(res.nevConv, reso.nevConv)
    assert res.nevConv >= 8 and reso.nevConv >= 8 and abs(res.numIter - reso.numIter) <= max(2, reso.numIter // 4), (res.nevConv, res.numIter, reso.nevConv, reso.numIter)
    assert np.max(np.abs(ev[:k] - evo[:k]) / np.abs(evo[:k])) < 1e-10
    h.gcge_csr_free(C.byref(L))


def test_ccs_triples_to_hip_solve(hip):
    """MATLAB-style CCS triples (app/app_matlab.c:80-98: jc/ir/pr, 0-based) -> gcge_csr_from_ccs -> HIP solve."""
    c = GCG["lap3d_12_nev10"]
    h = host_lib()
    A0, _ = make_problem(c["kind"], c["size"])
    S = csr_to_scipy(A0).tocsc()
    S.sort_indices()
    jc = np.ascontiguousarray(S.indptr, dtype=np.int32); ir = np.ascontiguousarray(S.indices, dtype=np.int32)
    pr = np.ascontiguousarray(S.data, dtype=np.float64)
    L = CSR()
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    assert h.gcge_csr_from_ccs(S.shape[0], S.shape[1], jc.ctypes.data_as(ip), ir.ctypes.data_as(ip), pr.ctypes.data_as(dp), 0, C.byref(L)) == 0
    mA = hip.matrix(L)
    hip.set_random_mode(0)
    ev, res = run_gcg(hip.ops_handle, mA, None, ["-nevConv", c["nev"]])
    assert res.nevConv == c["nevConv"] and abs(res.numIter - c["numIter"]) <= 2
    refv = np.array(c["eval"])
    assert np.max(np.abs(ev[:len(refv)] - refv) / np.abs(refv)) < 1e-10
    hip.free_matrix(mA)
    h.gcge_csr_free(C.byref(L))
