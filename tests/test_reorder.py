"""Row orders the HIP back-end chooses for itself (round 5, csrc/hip/reorder.hip + mat_upload.hip "row orders"): a matrix that shows
no grid in the order it arrives in — the reference's run list holds SuiteSparse files and tetrahedral FE matrices in whatever
numbering their producers chose (test/submit.sh:9-10, test/get_mat_phg.c:148) — is re-ordered INSIDE the opaque handle: grid
coordinates recovered from the graph of a star stencil (the plane sweep applies again) or reverse Cuthill-McKee.  Nothing of that may
show at the boundary: products, inner products, whole eigensolves and the reference-order random start block are checked against
scipy / the CPU oracle on the SAME permuted arrays."""
import ctypes as C

import numpy as np
import pytest

from gcge_amd.lib import hip_lib, make_problem, run_gcg
from helpers import csr_from_scipy, csr_to_scipy, uniform

IP = C.POINTER(C.c_int)


def permuted(kind, size, pseed, **kw):
    import scipy.sparse as sp
    A, B = make_problem(kind, size, **kw)
    S = csr_to_scipy(A).tocsr()
    p = np.random.default_rng(pseed).permutation(S.shape[0])
    Sp = sp.csr_matrix(S[p][:, p])
    Sp.sort_indices()
    Bp = None
    if B is not None:
        Bp = sp.csr_matrix(csr_to_scipy(B).tocsr()[p][:, p])
        Bp.sort_indices()
    return Sp, Bp, p


# ---------------------------------------------------------------------------------------------- host algorithms (no GPU: dlopen only)
@pytest.mark.parametrize("kind,size,kw,min_fill", [("lap3d", 14, {}, 1.0), ("fe3d", 10, {}, 1.0), ("sio2", 24, dict(K=12, R0=2.0, R1=5.0, seed=12345), 0.9),
                                                   ("sio2", 40, dict(K=26, R0=2.0, R1=5.0, seed=12345), 0.9),
                                                   ("sio2ball", 28, dict(K=8, R0=1.5, R1=3.0, seed=12345), 0.9)])
def test_grid_coordinates_come_back_from_the_star_couplings(kind, size, kw, min_fill):
    """gcge_hip_reorder_star_grid on a randomly permuted matrix: the flood fill places >= 90 % of the rows (everything outside the
    dense atom blocks), the placement is one-to-one, and the recovered coordinates are the true ones up to a symmetry of the cube
    (pairs of rows: the same |dx|, |dy|, |dz| up to a permutation of the axes) — on the box for >= 99.9 % of sampled pairs (a few
    rows deep inside large atoms have no exact stencil entry to the outside and take free positions)."""
    g = hip_lib()
    Sp, _, p = permuted(kind, size, 7, **kw)
    n = Sp.shape[0]
    A, keep = csr_from_scipy(Sp)
    dims = (C.c_int * 3)()
    box = np.zeros(n, dtype=np.int32)
    placed = g.gcge_hip_reorder_star_grid(n, A.rowptr, A.colidx, A.val, dims, box.ctypes.data_as(IP))
    assert placed >= min_fill * n, (placed, n)
    assert len(np.unique(box)) == n and box.min() >= 0 and box.max() < dims[0] * dims[1] * dims[2]
    if kind == "sio2ball":
        assert max(dims) <= size and dims[0] * dims[1] * dims[2] >= n
        return
    assert sorted(dims) == [size] * 3
    G = size
    tx, ty, tz = p % G, (p // G) % G, p // (G * G)
    bx, by, bz = box % dims[0], (box // dims[0]) % dims[1], box // (dims[0] * dims[1])
    rng = np.random.default_rng(3)
    i, j = rng.integers(0, n, 20000), rng.integers(0, n, 20000)
    dt = np.sort(np.abs(np.stack([tx[i] - tx[j], ty[i] - ty[j], tz[i] - tz[j]])), axis=0)
    dr = np.sort(np.abs(np.stack([bx[i] - bx[j], by[i] - by[j], bz[i] - bz[j]])), axis=0)
    assert np.mean(np.all(dt == dr, axis=0)) >= (1.0 if min_fill == 1.0 else 0.999)


def test_star_recovery_refuses_what_is_no_star_grid_and_rcm_bands_it():
    import scipy.sparse as sp
    g = hip_lib()
    rng = np.random.default_rng(11)
    n = 3000
    pts = rng.random((n, 3))
    # a random geometric graph (what an unstructured mesh looks like to the solver): symmetric, values all different
    from scipy.spatial import cKDTree
    pairs = cKDTree(pts).query_pairs(0.11, output_type="ndarray")
    w = rng.random(len(pairs)) + 0.5
    S = sp.coo_matrix((np.concatenate([-w, -w]), (np.concatenate([pairs[:, 0], pairs[:, 1]]), np.concatenate([pairs[:, 1], pairs[:, 0]]))), shape=(n, n)).tocsr()
    S = (S + sp.diags(np.asarray(np.abs(S).sum(axis=1)).ravel() + 0.1)).tocsr()
    S.sort_indices()
    A, keep = csr_from_scipy(S)
    dims = (C.c_int * 3)()
    box = np.zeros(n, dtype=np.int32)
    assert g.gcge_hip_reorder_star_grid(n, A.rowptr, A.colidx, A.val, dims, box.ctypes.data_as(IP)) == 0
    perm = np.zeros(n, dtype=np.int32)
    assert g.gcge_hip_reorder_rcm(n, A.rowptr, A.colidx, perm.ctypes.data_as(IP)) == 0
    assert np.array_equal(np.sort(perm), np.arange(n))
    ip = np.zeros(n, dtype=np.int32)
    ip[perm] = np.arange(n, dtype=np.int32)
    b0 = g.gcge_hip_mean_bandwidth(n, A.rowptr, A.colidx, None)
    b1 = g.gcge_hip_mean_bandwidth(n, A.rowptr, A.colidx, ip.ctypes.data_as(IP))
    assert b1 < 0.35 * b0, (b0, b1)


# ---------------------------------------------------------------------------------------------- GPU: nothing shows at the boundary
@pytest.fixture()
def reorder_on(hip):
    hip.g.gcge_hip_spmm_reorder_mode(1)
    yield hip
    hip.g.gcge_hip_spmm_reorder_mode(0)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,size,kw,want_form,want_order", [
    ("lap3d", 17, {}, "spmm_pattern", "grid 17 x 17 x 17 recovered"),
    ("sio2", 23, dict(K=11, R0=2.0, R1=5.0, seed=12345), "spmm_star", "grid 23 x 23 x 23 recovered"),
    ("sio2ball", 27, dict(K=8, R0=1.5, R1=3.0, seed=12345), "spmm_star", "recovered"),
])
def test_permuted_grid_matrices_take_the_grid_kernels_again(reorder_on, kind, size, kw, want_form, want_order):
    """(Sizes no other test uses: a matrix of the same size that is still alive in the process pins its row order for later ones.)
    A randomly permuted Laplacian / SiO2-like matrix / ball matrix: the upload recovers the grid, the K1 form is the one of the
    natural order, products (odd offsets, 1 ... 66 columns), inner products and a round trip through the host agree with scipy on the
    PERMUTED arrays; with the re-ordering switched off the same handle calls give the same numbers through the generic kernels."""
    hip = reorder_on
    g = hip.g
    g.gcge_hip_spmm_dense_mode(1)
    try:
        Sp, _, p = permuted(kind, size, 5, **kw)
        n = Sp.shape[0]
        A, keep = csr_from_scipy(Sp)
        results = {}
        for mode in (1, -1):
            g.gcge_hip_spmm_reorder_mode(mode)
            mat = hip.matrix(A)
            form, order = g.gcge_hip_mat_spmm_form(mat).decode(), g.gcge_hip_mat_row_order(mat).decode()
            if mode == 1:
                assert form.startswith(want_form) and want_order in order, (form, order)
            else:
                assert order == "as given" and not form.startswith("spmm_star") and not form.startswith("spmm_pattern"), (form, order)
            X = uniform(41, (n, 70)) - 0.5
            x = hip.mv_from_numpy(mat, X)
            assert np.array_equal(hip.mv_to_numpy(x, n, 0, 70), X)                     # round trip: the caller's row order
            y = hip.ops.mv_create(70, mat)
            out = []
            for m, a, b in ((64, 0, 0), (17, 1, 2), (2, 5, 0), (66, 2, 3), (1, 7, 7)):
                hip.ops.spmm(mat, x, y, (a, b), (a + m, b + m))
                got = hip.mv_to_numpy(y, n, b, b + m)
                want = Sp @ X[:, a:a + m]
                assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want)), (mode, m)
                out.append(got)
            ip_ = hip.ops.inner_prod("N", x, x, (0, 3), (5, 9))
            assert np.max(np.abs(ip_ - X[:, 0:5].T @ X[:, 3:9])) < 1e-11
            hip.set_random_mode(0)                                                    # the reference's rand() stream, in the CALLER's row order
            C.CDLL(None).srand(3)
            hip.ops.set_random(y, 0, 2)
            results[mode] = hip.mv_to_numpy(y, n, 0, 2)
            hip.ops.mv_destroy(x, 70)
            hip.ops.mv_destroy(y, 70)
            hip.free_matrix(mat)
        assert np.array_equal(results[1], results[-1])
        C.CDLL(None).srand(3)
        ref = np.array([C.CDLL(None).rand() for _ in range(2 * n)], dtype=np.float64).reshape(2, n).T / (2147483647.0 + 1.0)
        assert np.array_equal(results[1], ref)
    finally:
        g.gcge_hip_spmm_dense_mode(0)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,size,nev,kw,amg", [("lap3d", 18, 10, {}, 3), ("sio2", 21, 10, dict(K=8, R0=1.5, R1=3.0, seed=12345), 0), ("fe3d", 19, 10, {}, 0)])
def test_gcg_on_permuted_matrices_matches_the_oracle(reorder_on, oracle, kind, size, nev, kw, amg):
    """Whole eigensolves on randomly permuted matrices (standard and generalised: B adopts A's row order) with the fused CG — and with
    BlockAMG on the recovered grid — against the CPU oracle on the same permuted arrays: Ritz values <= 1e-10; the eigenvectors
    come back in the caller's row order (residuals recomputed with scipy)."""
    hip = reorder_on
    g = hip.g
    Sp, Bp, p = permuted(kind, size, 9, **kw)
    n = Sp.shape[0]
    A, keepA = csr_from_scipy(Sp)
    B, keepB = csr_from_scipy(Bp) if Bp is not None else (None, None)
    o_ev, o_res = run_gcg(oracle.ops_handle, oracle.matrix(A), oracle.matrix(B) if B is not None else None, ["-nevConv", nev])
    mA = hip.matrix(A)
    mB = hip.matrix(B) if B is not None else None
    assert "recovered" in g.gcge_hip_mat_row_order(mA).decode()
    if mB is not None:
        assert "recovered" in g.gcge_hip_mat_row_order(mB).decode()
    g.gcge_hip_bpcg_setup(hip.ops_handle, 30, 1e-2, 1e-14, b"abs")
    hip.set_random_mode(0)
    C.CDLL(None).srand(0)
    args = ["-nevConv", nev, "-gcge_initX_orth_method", "chol", "-gcge_compW_orth_method", "chol"] + (["-gcge_amg_levels", amg] if amg else [])
    ev, res, evec = run_gcg(hip.ops_handle, mA, mB, args, flag=1, keep_evec=True)
    k = min(res.nevConv, o_res.nevConv)
    assert res.nevConv >= nev and np.max(np.abs(ev[:k] - o_ev[:k]) / np.abs(o_ev[:k])) < 1e-10
    V = hip.mv_to_numpy(evec, n, 0, nev)
    BV = Bp @ V if Bp is not None else V
    R = Sp @ V - BV * ev[:nev]
    scale = np.sqrt(np.sum(V * BV, axis=0))
    assert np.max(np.linalg.norm(R, axis=0) / (np.abs(ev[:nev]) * scale)) < 1e-7
    hip.ops.mv_destroy(evec, 2 * nev)
    hip.free_matrix(mA)
    if mB is not None:
        hip.free_matrix(mB)


@pytest.mark.gpu
def test_matrix_without_any_grid_gets_cuthill_mckee(reorder_on):
    """An unstructured matrix (random geometric graph in random numbering): reverse Cuthill-McKee inside the handle, same products as
    scipy on the caller's arrays, and a solve whose eigenvalues match scipy's."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as sla
    from scipy.spatial import cKDTree
    hip = reorder_on
    g = hip.g
    rng = np.random.default_rng(2)
    n = 6000
    pts = rng.random((n, 3))
    pairs = cKDTree(pts).query_pairs(0.085, output_type="ndarray")
    w = rng.random(len(pairs)) + 0.5
    S = sp.coo_matrix((np.concatenate([-w, -w]), (np.concatenate([pairs[:, 0], pairs[:, 1]]), np.concatenate([pairs[:, 1], pairs[:, 0]]))), shape=(n, n)).tocsr()
    S = (S + sp.diags(np.asarray(np.abs(S).sum(axis=1)).ravel() + 0.05)).tocsr()
    S.sort_indices()
    A, keep = csr_from_scipy(S)
    mat = hip.matrix(A)
    assert "Cuthill" in g.gcge_hip_mat_row_order(mat).decode()
    X = uniform(51, (n, 40)) - 0.5
    x = hip.mv_from_numpy(mat, X)
    y = hip.ops.mv_create(40, mat)
    for m, a, b in ((40, 0, 0), (16, 3, 1), (5, 2, 2)):
        hip.ops.spmm(mat, x, y, (a, b), (a + m, b + m))
        want = S @ X[:, a:a + m]
        assert np.max(np.abs(hip.mv_to_numpy(y, n, b, b + m) - want)) <= 1e-12 * np.max(np.abs(want))
    hip.ops.mv_destroy(x, 40)
    hip.ops.mv_destroy(y, 40)
    hip.set_random_mode(0)
    ev, res = run_gcg(hip.ops_handle, mat, None, ["-nevConv", 8, "-gcge_initX_orth_method", "chol", "-gcge_compW_orth_method", "chol"])
    exact = np.sort(sla.eigsh(S.tocsc(), k=res.nevConv, sigma=0.0, which="LM", return_eigenvectors=False))
    assert res.nevConv >= 8 and np.max(np.abs(ev[:res.nevConv] - exact) / exact) < 1e-9
    hip.free_matrix(mat)
