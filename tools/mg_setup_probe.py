"""Multigrid set-up of the HIP back-end in both modes: the phase split of MultiGridCreate, the bytes copied device to host and the
total set-up time, for one problem of the existing generators.

  python tools/mg_setup_probe.py <lap3d|fe3d|sio2> <size> [levels] [hostlevels]
  python tools/mg_setup_probe.py ball <G> <K> [levels] [solve]
  python tools/mg_setup_probe.py perm <size> [levels] [solve]
  python tools/mg_setup_probe.py delaunay <points> [levels] [solve]
  python tools/mg_setup_probe.py refresh <lap3d|sio2> <size> [levels] [K]

ball: the masked grid of BASELINE config 5 (the ball in the G^3 box, K atoms, R0 = 2.0, R1 = 5.0 as in bench.py --config c5), its
geometry named; each mode is run with the cells of the box and with the graph branch (gcge_hip_multigrid_masked_cells).  With `solve`: one GCG solve (nev 10, block 64 columns of W) with BlockAMG over each of the
two hierarchies, 8 / 24 smoothing steps: outer iterations and seconds.

perm: lap3d <size> under a random symmetric permutation; delaunay: the P1 stiffness matrix on the Delaunay tetrahedra of random points in
a cube (hull nodes eliminated), the matrix of tools/generic_probe.py.  Neither shows a grid in the order it arrives in: both graph
methods are run (gcge_mg_set_graph_method: 0 greedy on the host, 1 MIS-2 on the device), with GCGE_MG_TRACE on in the measured call (the
rounds of every level); with `solve` one GCG solve (nev 10) with BlockAMG over each method's hierarchy.

hostlevels (any kind): gcge_hip_multigrid_device_levels(0) — the device build downloads every coarse level for the host constructors
instead of handing it to gcge_hip_mat_create_device.

refresh: a live hierarchy refreshed in place (gcge_hip_multigrid_refresh) against MultiGridCreate on the same handle, in one process:
an updatable handle (sio2: K atoms, R0 = 2.0, R1 = 5.0 as in bench.py --config c5; default K 2000), a new diagonal for level 0 through
gcge_hip_mat_update_values_device before every timed call, every timed call bracketed by a stream synchronise, one warm-up, then the
median of 5 (min and max beside it); the phase split of the fresh build, the bytes each copies device to host, one JSON line at the end.

Mode 0 builds the hierarchy on the device (csrc/hip/mg_device.hip), mode 1 on the host (csrc/host/multigrid.c); both give the same
hierarchy.  Each mode is timed on a fresh MultiGridCreate after one warm-up call; the rows, K1 form and row order of its levels are listed."""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def refresh_leg(argv):
    import json
    import statistics
    import torch
    from gcge_amd import HipBackend
    from gcge_amd.lib import csr_arrays, hip_lib, make_problem, multigrid_refresh_stats, multigrid_stats
    from gcge_amd.ops_struct import OPS
    kind, size = argv[0], int(argv[1])
    levels = int(argv[2]) if len(argv) > 2 else 6
    K = int(argv[3]) if len(argv) > 3 else 2000
    hip = HipBackend()
    g = hip_lib()
    A, _ = make_problem(kind, size, **(dict(K=K, R0=2.0, R1=5.0, seed=12345) if kind == "sio2" else {}))
    t = time.perf_counter()
    m = hip.matrix(A, updatable=True)
    hip.sync()
    print("%s %d: %d rows, %d non-zeros; upload with value maps kept %.2f s, K1 form %s" % (
        kind, size, A.nrows, A.nnz, time.perf_counter() - t, g.gcge_hip_mat_spmm_form(m).decode()))
    rp, ci, va = (torch.from_numpy(a).cuda() for a in csr_arrays(A))
    rows = torch.repeat_interleave(torch.arange(A.nrows, device=rp.device, dtype=torch.int32), (rp[1:] - rp[:-1]).long())
    diag = (rows == ci).nonzero().reshape(-1)
    pot = 0.25 * (1.0 + (rows[diag] % 11).double())
    del rows, rp, ci

    def values(step):                       # the creation values with step * pot on the diagonal
        v = va.clone()
        v[diag] += step * pot
        return v
    st = C.cast(hip.ops_handle, C.POINTER(OPS)).contents
    create = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_void_p)(st.MultiGridCreate)
    destroy = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_void_p)(st.MultiGridDestroy)

    def build(keep_maps):
        A_arr, P_arr, nl = C.c_void_p(), C.c_void_p(), C.c_int(levels)
        with hip._keeping_value_maps(keep_maps):
            create(C.byref(A_arr), None, C.byref(P_arr), C.byref(nl), m, None, hip.ops_handle)
        return A_arr, P_arr, nl

    def free(hier):
        destroy(C.byref(hier[0]), None, C.byref(hier[1]), C.byref(hier[2]), hip.ops_handle)

    def med(ts):
        return {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts), "calls": len(ts)}
    out = {"kind": kind, "size": size, "K": K if kind == "sio2" else None, "levels_asked": levels, "rows": A.nrows, "nnz": int(A.nnz)}
    assert hip.matrix_update_values(m, values(1)), "level 0 declined the new diagonal"
    for keep_maps in (True, False):
        ts = []
        for rep in range(6):
            hip.sync()
            t = time.perf_counter()
            hier = build(keep_maps)
            hip.sync()
            ts.append(time.perf_counter() - t)
            secs, d2h = multigrid_stats()
            free(hier)
        key = "fresh_build_maps_kept" if keep_maps else "fresh_build"
        out[key] = dict(med(ts[1:]), phases_s=secs, d2h_bytes=d2h)
        print("MultiGridCreate, value maps %s: median %.4f s (min %.4f, max %.4f) of 5 after a warm-up  [%s]  device->host %d bytes" % (
            "kept" if keep_maps else "not kept", out[key]["median_s"], out[key]["min_s"], out[key]["max_s"],
            "  ".join("%s %.4f" % kv for kv in secs.items()), d2h))
    hier = build(True)
    L = hier[2].value
    out["levels"] = []
    for lev, a in enumerate(C.cast(hier[0], C.POINTER(C.c_void_p * L)).contents):
        out["levels"].append({"rows": g.gcge_hip_mat_nrows(a), "nnz": g.gcge_hip_mat_nnz(a), "form": g.gcge_hip_mat_spmm_form(a).decode()})
        print("  level %d: %d rows, %d non-zeros, K1 form %s" % (lev, out["levels"][-1]["rows"], out["levels"][-1]["nnz"], out["levels"][-1]["form"]))
    ts, tu, rcs, moved = [], [], [], []
    for rep in range(6):
        v = values(2 + rep % 2)
        hip.sync()
        t = time.perf_counter()
        assert hip.matrix_update_values(m, v)
        hip.sync()
        tu.append(time.perf_counter() - t)
        s0 = multigrid_refresh_stats()
        t = time.perf_counter()
        rc = g.gcge_hip_multigrid_refresh(hier[0], None, hier[1], L)
        hip.sync()
        ts.append(time.perf_counter() - t)
        rcs.append(rc)
        moved.append(multigrid_refresh_stats()[3] - s0[3])
    free(hier)
    out["refresh"] = dict(med(ts[1:]), returned=rcs, d2h_bytes=moved[-1])
    out["level0_update"] = med(tu[1:])
    print("gcge_hip_multigrid_refresh: median %.4f s (min %.4f, max %.4f) of 5 after a warm-up, returned %s, device->host %d bytes; "
          "the update of level 0 before it: median %.4f s" % (out["refresh"]["median_s"], out["refresh"]["min_s"], out["refresh"]["max_s"], rcs,
                                                              moved[-1], out["level0_update"]["median_s"]))
    print(json.dumps(out))
    hip.free_matrix(m)


def main():
    if sys.argv[1] == "refresh":
        return refresh_leg(sys.argv[2:])
    import torch  # noqa: F401  (one libamdhip64, shared with torch)
    from gcge_amd import HipBackend
    from gcge_amd.lib import (CSR, ball_geometry, csr_to_scipy, hip_lib, make_problem, multigrid_graph_method, multigrid_masked_cells,
                              multigrid_mode, multigrid_stats, run_gcg)
    from gcge_amd.ops_struct import OPS
    kind, size = sys.argv[1], int(sys.argv[2])
    ball, graph = kind == "ball", kind in ("perm", "delaunay")
    rest = sys.argv[4:] if ball else sys.argv[3:]
    solve = "solve" in rest
    hostlevels = "hostlevels" in rest
    rest = [v for v in rest if v not in ("solve", "hostlevels")]
    levels = int(rest[0]) if rest else 6
    hip = HipBackend()
    g = hip_lib()
    if hostlevels:
        from gcge_amd.lib import multigrid_device_levels
        multigrid_device_levels(0)
        print("coarse levels through the host constructors (device levels off)")
    g.gcge_hip_mat_spmm_form.restype = C.c_char_p
    g.gcge_hip_mat_spmm_form.argtypes = [C.c_void_p]
    g.gcge_hip_mat_nrows.argtypes = [C.c_void_p]
    g.gcge_hip_mat_row_order.restype = C.c_char_p
    g.gcge_hip_mat_row_order.argtypes = [C.c_void_p]
    if ball:
        A, B = make_problem("sio2ball", size, K=int(sys.argv[3]), R0=2.0, R1=5.0, seed=12345)
        t = time.perf_counter()
        mA = hip.matrix_grid(A, (size, size, size), ball_geometry(size))
        print("upload with the geometry named: %.2f s" % (time.perf_counter() - t))
    elif graph:
        import numpy as np
        S = permuted_lap3d(make_problem, csr_to_scipy, size) if kind == "perm" else delaunay_stiffness(size)
        keep = (np.ascontiguousarray(S.indptr, dtype=np.int32), np.ascontiguousarray(S.indices, dtype=np.int32), np.ascontiguousarray(S.data))
        A, B = CSR(S.shape[0], S.shape[0], 0, int(S.nnz), keep[0].ctypes.data_as(C.POINTER(C.c_int)), keep[1].ctypes.data_as(C.POINTER(C.c_int)),
                   keep[2].ctypes.data_as(C.POINTER(C.c_double))), None
        t = time.perf_counter()
        mA = hip.matrix(A)
        print("upload: %.2f s, K1 form %s, row order %s" % (time.perf_counter() - t, g.gcge_hip_mat_spmm_form(mA).decode(), g.gcge_hip_mat_row_order(mA).decode()))
    else:
        A, B = make_problem(kind, size)
        mA = hip.matrix(A)
    mB = hip.matrix(B) if B is not None else None
    st = C.cast(hip.ops_handle, C.POINTER(OPS)).contents
    create = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_void_p)(st.MultiGridCreate)
    destroy = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_void_p)(st.MultiGridDestroy)
    fine = (A.nrows + 1) * 4 + int(A.nnz) * 12
    print("%s %d: %d rows, %d non-zeros, fine CSR %.1f MB%s" % (kind, size, A.nrows, A.nnz, fine / 1e6, ", with B" if mB else ""))
    for method, cells in [(m, 1) for m in (0, 1)] if graph else [(None, c) for c in ((1, 0) if ball else (1,))]:
        multigrid_masked_cells(cells)
        if graph:
            multigrid_graph_method(method)
            print("graph method %d (%s)" % (method, "greedy aggregation on the host" if method == 0 else "MIS-2 aggregation on the device"))
        if ball:
            print("masked cells %s" % ("on: 2 x 2 x 2 cells of the box" if cells else "off: the graph branch"))
        for mode in (0, 1):
            multigrid_mode(mode)
            for rep in range(2):
                A_arr, B_arr, P_arr, nl = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int(levels)
                bref = C.byref(B_arr) if mB is not None else None
                if graph and rep == 1:
                    os.environ["GCGE_MG_TRACE"] = "1"
                t = time.perf_counter()
                create(C.byref(A_arr), bref, C.byref(P_arr), C.byref(nl), mA, mB, hip.ops_handle)
                total = time.perf_counter() - t
                os.environ.pop("GCGE_MG_TRACE", None)
                secs, d2h = multigrid_stats()
                if rep == 1:
                    for lev, a in enumerate(C.cast(A_arr, C.POINTER(C.c_void_p * nl.value)).contents):
                        print("  level %d: %d rows, K1 form %s, row order %s" % (lev, g.gcge_hip_mat_nrows(a), g.gcge_hip_mat_spmm_form(a).decode(),
                                                                                g.gcge_hip_mat_row_order(a).decode()))
                destroy(C.byref(A_arr), bref, C.byref(P_arr), C.byref(nl), hip.ops_handle)
            print("mode %d (%s): %d levels, %.3f s  [%s]  device->host %.1f MB (%.1f%% of the fine CSR)" % (
                mode, "device" if mode == 0 else "host", nl.value, total, "  ".join("%s %.3f" % kv for kv in secs.items()), d2h / 1e6, 100.0 * d2h / fine))
        multigrid_mode(0)
        if ball and solve:
            hip.set_random_mode(0)
            C.CDLL(None).srand(0)
            t = time.perf_counter()
            ev, res = run_gcg(hip.ops_handle, mA, None, ["-nevConv", 10, "-gcge_amg_levels", levels, "-gcge_amg_smooth0", 8, "-gcge_amg_smooth", 24,
                                                         "-gcge_initX_orth_method", "chol", "-gcge_compW_orth_method", "chol"])
            print("  GCG + BlockAMG (8 / 24 smoothing steps): nevConv %d, %d outer iterations, %.2f s (set-up included), lambda_1 %.12g" % (
                res.nevConv, res.numIter, time.perf_counter() - t, ev[0]))
        if graph and solve:
            hip.set_random_mode(0)
            C.CDLL(None).srand(0)
            t = time.perf_counter()
            ev, res = run_gcg(hip.ops_handle, mA, None, ["-nevConv", 10, "-gcge_amg_levels", levels, "-gcge_amg_graph", method,
                                                         "-gcge_initX_orth_method", "chol", "-gcge_compW_orth_method", "chol"])
            print("  GCG + BlockAMG over the method-%d hierarchy: nevConv %d, %d outer iterations, %.2f s (set-up included), lambda_1 %.12g" % (
                method, res.nevConv, res.numIter, time.perf_counter() - t, ev[0]))
    multigrid_masked_cells(1)
    multigrid_graph_method(0)


def permuted_lap3d(make_problem, csr_to_scipy, size, seed=7):
    import numpy as np
    S = csr_to_scipy(make_problem("lap3d", size)[0])
    p = np.random.default_rng(seed).permutation(S.shape[0])
    S = S[p][:, p].tocsr()
    S.sort_indices()
    return S


def delaunay_stiffness(npts, seed=1):
    """P1 stiffness matrix on the Delaunay tetrahedra of npts random points in the unit cube, the hull nodes eliminated (Dirichlet)"""
    import numpy as np
    import scipy.sparse as sp
    from scipy.spatial import Delaunay
    pts = np.random.default_rng(seed).random((npts, 3))
    tri = Delaunay(pts)
    T = tri.simplices
    M = np.concatenate([np.ones((T.shape[0], 4, 1)), pts[T]], axis=2)
    vol = np.abs(np.linalg.det(M)) / 6.0
    ok = vol > 1e-14
    T, M, vol = T[ok], M[ok], vol[ok]
    Gm = np.linalg.inv(M)[:, 1:, :]                  # gradients of the barycentric coordinates
    Ke = np.einsum("tdi,tdj->tij", Gm, Gm) * vol[:, None, None]
    I, J = np.repeat(T[:, :, None], 4, axis=2).ravel(), np.repeat(T[:, None, :], 4, axis=1).ravel()
    K = sp.coo_matrix((Ke.ravel(), (I, J)), shape=(npts, npts)).tocsr()
    inner = np.setdiff1d(np.arange(npts), np.unique(tri.convex_hull.ravel()))
    K = K[inner][:, inner].tocsr()
    K = ((K + K.T) * 0.5).tocsr()                    # (the assembly sums in an order of its own: symmetric to the last bit)
    K.sort_indices()
    return K


if __name__ == "__main__":
    main()
