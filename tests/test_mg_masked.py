"""Multigrid on masked grids (the grid points inside a sphere, rows in scan order: the PARSEC matrices behind BASELINE config 5):
the 2 x 2 x 2 cells of the bounding box at every level — the host routines (csrc/host/multigrid.c: gcge_mg_aggregate_masked,
gcge_mg_build_masked) against a few lines of numpy and scipy, the device kernels (csrc/hip/mg_device.hip) against the host routines
byte for byte, the geometry a handle carries (gcge_hip_mat_geometry), MultiGridCreate of the HIP back-end in both modes, solves
that use the hierarchy, the products of every level, and the switch back to the graph branch."""
import ctypes as C

import numpy as np
import pytest

from gcge_amd.lib import CSR, MG, ball_geometry, host_lib, make_problem
from helpers import csr_from_scipy, csr_to_scipy, load_golden, mg_hierarchy, uniform

BALL16 = dict(K=6, R0=1.5, R1=2.0, seed=12345)          # the golden case sio2ball_16_nev10
BALL28 = dict(K=8, R0=1.5, R1=3.0, seed=12345)


# ---------------------------------------------------------------------------------------------- inputs and the numpy reference
def ball(G, **kw):
    A, _ = make_problem("sio2ball", G, **kw)
    return A, None, (G, G, G), ball_geometry(G)


def cut(S, dims, keep):
    """principal submatrix of a matrix on the box `dims` on the box points `keep` (boolean, box order): CSR struct, keepalive, box"""
    idx = np.flatnonzero(keep)
    A, hold = csr_from_scipy(S[idx][:, idx].tocsr())
    return A, hold, idx.astype(np.int32)


def ellipsoid():
    """13 x 10 x 7 Laplacian cut to an ellipsoid: odd and unequal edges, empty cells, thin last layers"""
    nx, ny, nz = 13, 10, 7
    A = CSR()
    assert host_lib().gcge_problem_lap3d_box(C.c_int(nx), C.c_int(ny), C.c_int(nz), C.c_int64(0), C.c_int64(-1), C.byref(A)) == 0
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    keep = (((x - 6.0) / 6.6) ** 2 + ((y - 4.5) / 5.1) ** 2 + ((z - 3.0) / 3.6) ** 2 <= 1.0).ravel()
    Ac, hold, box = cut(csr_to_scipy(A), (nx, ny, nz), keep)
    return Ac, hold, (nx, ny, nz), box


def fe3d_ball(N=12):
    """the P1 pair (A, B) of an N^3 grid cut to the inscribed ball: B is coarsened as well"""
    A, B = make_problem("fe3d", N)
    z, y, x = np.meshgrid(np.arange(N), np.arange(N), np.arange(N), indexing="ij")
    c = 0.5 * (N - 1)
    keep = ((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2 <= (0.5 * N) ** 2).ravel()
    Ac, holdA, box = cut(csr_to_scipy(A), (N, N, N), keep)
    Bc, holdB, _ = cut(csr_to_scipy(B), (N, N, N), keep)
    return Ac, Bc, (holdA, holdB), (N, N, N), box


def np_cells(dims, box):
    """the cells in numpy: (nc, agg, cdims, cbox)"""
    nx, ny, nz = dims
    cx, cy, cz = (nx + 1) // 2, (ny + 1) // 2, (nz + 1) // 2
    b = np.asarray(box, dtype=np.int64)
    x, y, z = b % nx, (b // nx) % ny, b // (nx * ny)
    cell = cx * ((y // 2) + cy * (z // 2)) + x // 2
    cbox, agg = np.unique(cell, return_inverse=True)
    return len(cbox), agg.astype(np.int32), (cx, cy, cz), cbox.astype(np.int32)


def np_levels(dims, box, max_levels, min_rows=64):
    """[(dims, box)] of every level under gcge_mg_build's stopping rules"""
    out = [(tuple(dims), np.asarray(box, dtype=np.int32))]
    while len(out) < max_levels and len(out[-1][1]) > min_rows:
        nc, _, cd, cb = np_cells(*out[-1])
        if nc * 3 > len(out[-1][1]) * 2:
            break
        out.append((cd, cb))
    return out


def np_members(agg, nc):
    mem = np.argsort(agg, kind="stable").astype(np.int32)
    ptr = np.concatenate(([0], np.cumsum(np.bincount(agg, minlength=nc)))).astype(np.int32)
    return ptr, mem


def host_hierarchy(A, B, dims, box, max_levels):
    """gcge_mg_build_masked as scipy matrices and numpy box arrays"""
    h = host_lib()
    ip = C.POINTER(C.c_int)
    mg = MG()
    box = np.ascontiguousarray(box, dtype=np.int32)
    rc = h.gcge_mg_build_masked(C.byref(A), C.byref(B) if B is not None else None, C.byref((C.c_int * 3)(*dims)), box.ctypes.data_as(ip),
                                max_levels, 0, 0.0, C.byref(mg))
    if rc != 0:
        return rc

    L = mg.num_levels
    out = {"A": [csr_to_scipy(mg.A[l]) for l in range(L)], "B": [csr_to_scipy(mg.B[l]) for l in range(L)] if B is not None else [],
           "P": [csr_to_scipy(mg.P[l]) for l in range(L - 1)], "PT": [csr_to_scipy(mg.PT[l]) for l in range(L - 1)],
           "dims": [tuple(mg.dims[l]) for l in range(L)],
           "box": [np.ctypeslib.as_array(C.cast(h.gcge_mg_level_box(C.byref(mg), l), ip), (mg.A[l].nrows,)).copy() for l in range(L)]}
    assert not h.gcge_mg_level_box(C.byref(mg), L)
    h.gcge_mg_free(C.byref(mg))
    return out


def _aggregate(dims, box, device=False):
    from gcge_amd.lib import mg_aggregate_masked
    return mg_aggregate_masked(dims, box, device=device)


# ---------------------------------------------------------------------------------------------- CPU: the host reference
@pytest.mark.parametrize("case,sizes", [("ball14", (1472, 251, 51)), ("ball15", (1791, 296, 57)), ("ball16", (2176, 360, 64)), ("ellipsoid", None)])
def test_masked_cells_are_the_numpy_cells(case, sizes):
    A, hold, dims, box = ball(int(case[4:])) if case.startswith("ball") else ellipsoid()
    nc, agg, cdims, cbox = _aggregate(dims, box)
    rnc, ragg, rcd, rcbox = np_cells(dims, box)
    assert nc == rnc and cdims == rcd
    assert np.array_equal(agg, ragg) and np.array_equal(cbox, rcbox)
    assert np.all(np.diff(cbox) > 0) and cbox[-1] < cdims[0] * cdims[1] * cdims[2]
    per_cell = np.bincount(agg, minlength=nc)
    assert per_cell.min() >= 1 and per_cell.max() == 8 and len(np.unique(per_cell)) >= 4       # ragged cells
    assert nc < cdims[0] * cdims[1] * cdims[2]                                                  # and empty ones
    lev = host_hierarchy(A, None, dims, box, 8)
    ref = np_levels(dims, box, 8)
    assert [a.shape[0] for a in lev["A"]] == [len(b) for _, b in ref]
    if sizes is not None:
        assert tuple(a.shape[0] for a in lev["A"]) == sizes
    for l, (d, b) in enumerate(ref):
        assert lev["dims"][l] == d and np.array_equal(lev["box"][l], b)


def test_full_box_mask_gives_the_grid_aggregates():
    dims = (7, 6, 5)
    n = dims[0] * dims[1] * dims[2]
    h = host_lib()
    ragg, rcd = np.zeros(n, dtype=np.int32), (C.c_int * 3)()
    rnc = h.gcge_mg_aggregate_grid((C.c_int * 3)(*dims), ragg.ctypes.data_as(C.POINTER(C.c_int)), rcd)
    nc, agg, cdims, cbox = _aggregate(dims, np.arange(n, dtype=np.int32))
    assert nc == rnc and cdims == tuple(rcd)
    assert np.array_equal(agg, ragg) and np.array_equal(cbox, np.arange(nc))
    # ... and so does the hierarchy built on it: gcge_mg_build's, which detects the same grid from the rows
    A = CSR()
    assert h.gcge_problem_lap3d_box(C.c_int(7), C.c_int(6), C.c_int(5), C.c_int64(0), C.c_int64(-1), C.byref(A)) == 0
    lev, ref = host_hierarchy(A, None, dims, np.arange(n), 3), mg_hierarchy(A, 3)
    assert lev["dims"] == ref["dims"] and len(lev["A"]) == len(ref["A"]) == 2
    for key in ("A", "P", "PT"):
        for x, y in zip(lev[key], ref[key]):
            assert np.array_equal(x.indptr, y.indptr) and np.array_equal(x.indices, y.indices)
            assert np.array_equal(x.data.view(np.int64), y.data.view(np.int64))


def test_masked_hierarchy_is_galerkin_and_its_lines_are_runs():
    A, _, dims, box = ball(16, **BALL16)
    lev = host_hierarchy(A, None, dims, box, 8)
    assert [a.shape[0] for a in lev["A"]] == [2176, 360, 64]
    for l in range(len(lev["P"])):
        P, Af = lev["P"][l], lev["A"][l]
        assert np.array_equal(np.diff(P.indptr), np.ones(P.shape[0], dtype=P.indptr.dtype)) and np.all(P.data == 1.0)
        assert abs(lev["PT"][l] - P.T).nnz == 0
        ref = 0.5 * (P.T @ Af @ P)
        assert abs(lev["A"][l + 1] - ref).max() <= 1e-13 * abs(ref).max()
    for d, b in zip(lev["dims"], lev["box"]):           # every grid line of every level is one contiguous run of rows
        line = b // d[0]
        same = line[1:] == line[:-1]
        assert np.all(np.diff(b)[same] == 1)
        assert len(np.unique(line)) == 1 + np.count_nonzero(~same)


def test_masked_cells_refuse_a_box_array_that_is_not_one():
    dims = (6, 5, 4)
    good = np.array([3, 7, 8, 30, 119], dtype=np.int32)
    assert _aggregate(dims, good)[0] == 3              # (cells 1, 0, 1, 0 and 17)
    assert _aggregate(dims, good[::-1])[0] < 0                                    # descending
    assert _aggregate(dims, np.array([3, 7, 7, 30], dtype=np.int32))[0] < 0       # not strictly ascending
    assert _aggregate(dims, np.array([3, 7, 120], dtype=np.int32))[0] < 0         # past the box
    assert _aggregate(dims, np.array([-1, 7, 30], dtype=np.int32))[0] < 0
    A, _, bdims, box = ball(14)
    bad = box.copy(); bad[5], bad[6] = box[6], box[5]
    assert host_hierarchy(A, None, bdims, bad, 4) < 0


# ---------------------------------------------------------------------------------------------- GPU
def same_csr(a, b):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(a[2].view(np.int64), b[2].view(np.int64))


def sp_arrays(S):
    return S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data


def slot_multigrid(backend, A_handle, B_handle, levels):
    from gcge_amd.ops_struct import OPS
    st = C.cast(backend.ops_handle, C.POINTER(OPS)).contents
    A_arr, B_arr, P_arr, nl = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int(levels)
    create = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_void_p)(st.MultiGridCreate)
    destroy = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_void_p)(st.MultiGridDestroy)
    create(C.byref(A_arr), C.byref(B_arr) if B_handle is not None else None, C.byref(P_arr), C.byref(nl), A_handle, B_handle, backend.ops_handle)
    L = nl.value
    Ah = [C.c_void_p(v) for v in C.cast(A_arr, C.POINTER(C.c_void_p * L)).contents]
    Bh = [C.c_void_p(v) for v in C.cast(B_arr, C.POINTER(C.c_void_p * L)).contents] if B_handle is not None else []
    Ph = [C.c_void_p(v) for v in C.cast(P_arr, C.POINTER(C.c_void_p * max(1, L - 1))).contents][:L - 1]

    def done():
        destroy(C.byref(A_arr), C.byref(B_arr) if B_handle is not None else None, C.byref(P_arr), C.byref(nl), backend.ops_handle)
    return Ah, Bh, Ph, done


def snapshot(hip, mA, mB, levels):
    from gcge_amd.lib import hip_lib, mat_geometry, mat_to_csr, multigrid_stats
    g = hip_lib()
    Ah, Bh, Ph, done = slot_multigrid(hip, mA, mB, levels)
    snap = {"L": len(Ah), "A": [mat_to_csr(a) for a in Ah], "B": [mat_to_csr(b) for b in Bh],
            "P": [mat_to_csr(p) for p in Ph], "PT": [mat_to_csr(p, transpose=True) for p in Ph],
            "geom": [mat_geometry(a) for a in Ah], "form": [g.gcge_hip_mat_spmm_form(a) for a in Ah], "stats": multigrid_stats()}
    done()
    return snap


def same_snapshot(d, h):
    assert d["L"] == h["L"] and d["form"] == h["form"]
    for key in ("A", "B", "P", "PT"):
        assert len(d[key]) == len(h[key])
        for x, y in zip(d[key], h[key]):
            same_csr(x, y)
    for x, y in zip(d["geom"], h["geom"]):
        assert x[0] == y[0] and x[1] == y[1] and (x[2] is None) == (y[2] is None) and (x[2] is None or np.array_equal(x[2], y[2]))


def both_modes(hip, mA, mB, levels):
    from gcge_amd.lib import multigrid_mode
    snaps = {}
    try:
        for mode in (0, 1):
            multigrid_mode(mode)
            snaps[mode] = snapshot(hip, mA, mB, levels)
    finally:
        multigrid_mode(0)
    return snaps[0], snaps[1]


def _case(name):
    """(A, B, keepalive, dims, box, levels, level count expected)"""
    if name == "ball15":
        A, _, dims, box = ball(15, K=0)
        return A, None, None, dims, box, 5, 3
    if name == "ball28":
        A, _, dims, box = ball(28, **BALL28)
        return A, None, None, dims, box, 5, 4
    if name == "ellipsoid":
        A, hold, dims, box = ellipsoid()
        return A, None, hold, dims, box, 5, 3
    A, B, hold, dims, box = fe3d_ball(12)
    return A, B, hold, dims, box, 4, 3


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ball15", "ball28", "ellipsoid", "fe3d_ball"])
def test_device_cells_and_hierarchy_equal_the_host_ones_byte_for_byte(hip, name):
    from gcge_amd.lib import mat_geometry
    A, B, hold, dims, box, levels, want = _case(name)
    # the aggregation alone, level after level: agg / ptr / mem / coarse box
    d, b = dims, box
    for _ in range(want - 1):
        nc, agg, cdims, cbox = _aggregate(d, b)
        dnc, dagg, dcd, dcbox, dptr, dmem = _aggregate(d, b, device=True)
        ptr, mem = np_members(agg, nc)
        assert dnc == nc and dcd == cdims
        assert np.array_equal(dagg, agg) and np.array_equal(dcbox, cbox) and np.array_equal(dptr, ptr) and np.array_equal(dmem, mem)
        d, b = cdims, cbox
    # the hierarchy behind MultiGridCreate, device mode against host mode against gcge_mg_build_masked
    mA = hip.matrix_grid(A, dims, box)
    mB = hip.matrix_grid(B, dims, box) if B is not None else None
    k, gd, gb = mat_geometry(mA)
    assert k == 1 and gd == tuple(dims) and np.array_equal(gb, box)
    dev, hst = both_modes(hip, mA, mB, levels)
    same_snapshot(dev, hst)
    ref = host_hierarchy(A, B, dims, box, levels)
    assert dev["L"] == len(ref["A"]) == want
    for l in range(want):
        same_csr(dev["A"][l], sp_arrays(ref["A"][l]))
        if B is not None:
            same_csr(dev["B"][l], sp_arrays(ref["B"][l]))
        assert dev["geom"][l][0] == 1 and dev["geom"][l][1] == ref["dims"][l] and np.array_equal(dev["geom"][l][2], ref["box"][l])
    for l in range(want - 1):
        same_csr(dev["P"][l], sp_arrays(ref["P"][l]))
        same_csr(dev["PT"][l], sp_arrays(ref["PT"][l]))
    assert dev["stats"][0]["aggregate"] > 0.0 and dev["stats"][0]["detect"] == 0.0
    hip.free_matrix(mA)
    if mB is not None:
        hip.free_matrix(mB)


@pytest.fixture(scope="module")
def ball28(hip):
    """the G = 28 ball with its geometry named, and its hierarchy in device mode (shared, never changed)"""
    from gcge_amd.lib import multigrid_mode
    A, _, dims, box = ball(28, **BALL28)
    mA = hip.matrix_grid(A, dims, box)
    multigrid_mode(0)
    Ah, Bh, Ph, done = slot_multigrid(hip, mA, None, 5)
    yield {"A": A, "dims": dims, "box": box, "mA": mA, "Ah": Ah, "Ph": Ph}
    done()
    hip.free_matrix(mA)


@pytest.mark.gpu
def test_device_build_on_a_masked_grid_downloads_no_fine_level(hip, ball28):
    from gcge_amd.lib import multigrid_masked_cells, multigrid_mode
    A, mA = ball28["A"], ball28["mA"]
    fine = (A.nrows + 1) * 4 + int(A.nnz) * 12
    multigrid_mode(0)
    cells = snapshot(hip, mA, None, 5)
    try:
        assert multigrid_masked_cells(0) == 0
        graph = snapshot(hip, mA, None, 5)
    finally:
        assert multigrid_masked_cells(1) == 1
    assert cells["L"] == 4 and [len(a[0]) - 1 for a in cells["A"]] == [11536, 1664, 275, 54]
    print("device to host: cells %d bytes, graph branch %d bytes, fine CSR %d bytes" % (cells["stats"][1], graph["stats"][1], fine))
    assert cells["stats"][1] < fine
    assert graph["stats"][1] >= fine


@pytest.mark.gpu
def test_recovered_geometry_gives_the_named_hierarchy(hip, ball28):
    from gcge_amd.lib import mat_geometry
    mI = hip.matrix(ball28["A"])                    # no geometry named: recovered from the rows at upload
    kind, dims, box = mat_geometry(mI)
    assert kind == 2
    assert dims == tuple(ball28["dims"])
    if np.array_equal(box, ball28["box"]):
        named, _ = both_modes(hip, ball28["mA"], None, 5)
        rec, rec_host = both_modes(hip, mI, None, 5)
        same_snapshot(rec, rec_host)
        assert rec["L"] == named["L"] == 4
        for key in ("A", "P", "PT"):
            for x, y in zip(rec[key][1:] if key == "A" else rec[key], named[key][1:] if key == "A" else named[key]):
                same_csr(x, y)
        for x, y in zip(rec["geom"][1:], named["geom"][1:]):
            assert x[0] == y[0] == 1 and x[1] == y[1] and np.array_equal(x[2], y[2])
    hip.free_matrix(mI)


@pytest.mark.gpu
def test_gcg_with_block_amg_on_a_masked_grid_matches_the_golden_run(hip):
    """GCG + BlockAMG over the cell hierarchy on the golden case sio2ball_16_nev10: Ritz values within 1e-10 relative of the
    reference's (the project's bar), no more than 3 outer iterations above its plain run (the margin of
    test_gcg_with_block_amg_on_hip_matches_oracle); device-mode and host-mode solves bit-identical."""
    from gcge_amd.lib import multigrid_mode, run_gcg
    c = load_golden("gcg.json")["sio2ball_16_nev10"]
    A, _, dims, box = ball(16, **BALL16)
    assert A.nrows == c["n"] and int(A.nnz) == c["nnz"]
    mA = hip.matrix_grid(A, dims, box)
    out = {}
    try:
        for mode in (0, 1):
            multigrid_mode(mode)
            hip.set_random_mode(0)
            C.CDLL(None).srand(0)
            ev, res = run_gcg(hip.ops_handle, mA, None, ["-nevConv", c["nev"], "-gcge_amg_levels", 4, "-gcge_initX_orth_method", "chol",
                                                         "-gcge_compW_orth_method", "chol"])
            out[mode] = (ev.copy(), res.nevConv, res.numIter)
    finally:
        multigrid_mode(0)
    hip.free_matrix(mA)
    ev, nconv, nit = out[0]
    refv = np.array(c["eval"])
    print("nevConv %d, numIter %d (golden plain run %d), max relative error %.3e" % (nconv, nit, c["numIter"], np.max(np.abs(ev[:len(refv)] - refv) / refv)))
    assert nconv >= c["nev"]
    assert np.max(np.abs(ev[:len(refv)] - refv) / refv) < 1e-10
    assert nit <= c["numIter"] + 3
    assert np.array_equal(out[0][0].view(np.int64), out[1][0].view(np.int64)) and out[0][1:] == out[1][1:]


@pytest.mark.gpu
def test_products_of_every_masked_level_match_scipy(hip, ball28):
    import scipy.sparse as sp
    from gcge_amd.lib import mat_to_csr
    Ah, Ph = ball28["Ah"], ball28["Ph"]
    assert len(Ah) == 4
    for l, a in enumerate(Ah):
        rp, ci, va = mat_to_csr(a)
        n = len(rp) - 1
        S = sp.csr_matrix((va, ci, rp), shape=(n, n))
        for m in (8, 66):
            x = uniform(40 + l + m, (n, m)) - 0.5
            vx = hip.mv_from_numpy(a, x)
            vy = hip.ops.mv_create(m, a)
            hip.ops.spmm(a, vx, vy, (0, 0), (m, m))
            ref = S @ x
            assert np.max(np.abs(hip.mv_to_numpy(vy, n, 0, m) - ref)) <= 1e-12 * np.max(np.abs(ref)), (l, m)
            hip.ops.mv_destroy(vx, m); hip.ops.mv_destroy(vy, m)
    for l, p in enumerate(Ph):
        rp, ci, va = mat_to_csr(p)
        tp, tc, tv = mat_to_csr(p, transpose=True)
        nf, nc = len(rp) - 1, len(tp) - 1
        P, PT = sp.csr_matrix((va, ci, rp), shape=(nf, nc)), sp.csr_matrix((tv, tc, tp), shape=(nc, nf))
        assert abs(PT - P.T).nnz == 0
        for m in (8, 66):
            xc, xf = uniform(70 + l + m, (nc, m)) - 0.5, uniform(90 + l + m, (nf, m)) - 0.5
            vc, vf = hip.mv_from_numpy(Ah[l + 1], xc), hip.ops.mv_create(m, Ah[l])
            hip.ops.spmm(p, vc, vf, (0, 0), (m, m))
            ref = P @ xc
            assert np.max(np.abs(hip.mv_to_numpy(vf, nf, 0, m) - ref)) <= 1e-12 * np.max(np.abs(ref)), (l, m)
            wf, wc = hip.mv_from_numpy(Ah[l], xf), hip.ops.mv_create(m, Ah[l + 1])
            hip.ops.fn("MatTransDotMultiVec")(p, wf, wc, (C.c_int * 2)(0, 0), (C.c_int * 2)(m, m), hip.ops_handle)
            ref = PT @ xf
            assert np.max(np.abs(hip.mv_to_numpy(wc, nc, 0, m) - ref)) <= 1e-12 * np.max(np.abs(ref)), (l, m)
            for v in (vc, vf, wf, wc):
                hip.ops.mv_destroy(v, m)


@pytest.mark.gpu
def test_switch_restores_the_graph_hierarchy(hip, ball28):
    """masked cells off: the geometry on the handle is ignored — gcge_mg_build on the handle's rows (what it reads off their column
    offsets, greedy aggregates otherwise), level for level, in both modes"""
    from gcge_amd.lib import multigrid_masked_cells
    try:
        multigrid_masked_cells(0)
        dev, hst = both_modes(hip, ball28["mA"], None, 4)
    finally:
        multigrid_masked_cells(1)
    same_snapshot(dev, hst)
    ref = mg_hierarchy(ball28["A"], 4)
    assert dev["L"] == len(ref["A"]) >= 3
    for l in range(dev["L"]):
        same_csr(dev["A"][l], sp_arrays(ref["A"][l]))
    for l in range(dev["L"] - 1):
        same_csr(dev["P"][l], sp_arrays(ref["P"][l]))
        same_csr(dev["PT"][l], sp_arrays(ref["PT"][l]))
    assert dev["geom"][0][0] == 1
    assert [len(a[0]) - 1 for a in dev["A"]] != [11536, 1664, 275, 54][:dev["L"]]
