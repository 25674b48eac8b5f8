"""Multigrid set-up of the HIP back-end in both modes: the phase split of MultiGridCreate, the bytes copied device to host and the
total set-up time, for one problem of the existing generators.

  python tools/mg_setup_probe.py <lap3d|fe3d|sio2> <size> [levels]
  python tools/mg_setup_probe.py ball <G> <K> [levels] [solve]

ball: the masked grid of BASELINE config 5 (the ball in the G^3 box, K atoms, R0 = 2.0, R1 = 5.0 as in bench.py --config c5), its
geometry named; each mode is run with the cells of the box and with the graph branch (gcge_hip_multigrid_masked_cells).  With `solve`: one GCG solve (nev 10, block 64 columns of W) with BlockAMG over each of the
two hierarchies, 8 / 24 smoothing steps: outer iterations and seconds.

Mode 0 builds the hierarchy on the device (csrc/hip/mg_device.hip), mode 1 on the host (csrc/host/multigrid.c); both give the same
hierarchy.  Each mode is timed on a fresh MultiGridCreate after one warm-up call; the rows, K1 form and row order of its levels are listed."""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch  # noqa: F401  (one libamdhip64, shared with torch)
    from gcge_amd import HipBackend
    from gcge_amd.lib import ball_geometry, hip_lib, make_problem, multigrid_masked_cells, multigrid_mode, multigrid_stats, run_gcg
    from gcge_amd.ops_struct import OPS
    kind, size = sys.argv[1], int(sys.argv[2])
    ball = kind == "ball"
    rest = sys.argv[4:] if ball else sys.argv[3:]
    solve = "solve" in rest
    rest = [v for v in rest if v != "solve"]
    levels = int(rest[0]) if rest else 6
    hip = HipBackend()
    g = hip_lib()
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
    else:
        A, B = make_problem(kind, size)
        mA = hip.matrix(A)
    mB = hip.matrix(B) if B is not None else None
    st = C.cast(hip.ops_handle, C.POINTER(OPS)).contents
    create = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_void_p)(st.MultiGridCreate)
    destroy = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_void_p)(st.MultiGridDestroy)
    fine = (A.nrows + 1) * 4 + int(A.nnz) * 12
    print("%s %d: %d rows, %d non-zeros, fine CSR %.1f MB%s" % (kind, size, A.nrows, A.nnz, fine / 1e6, ", with B" if mB else ""))
    for cells in ((1, 0) if ball else (1,)):
        multigrid_masked_cells(cells)
        if ball:
            print("masked cells %s" % ("on: 2 x 2 x 2 cells of the box" if cells else "off: the graph branch"))
        for mode in (0, 1):
            multigrid_mode(mode)
            for rep in range(2):
                A_arr, B_arr, P_arr, nl = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int(levels)
                bref = C.byref(B_arr) if mB is not None else None
                t = time.perf_counter()
                create(C.byref(A_arr), bref, C.byref(P_arr), C.byref(nl), mA, mB, hip.ops_handle)
                total = time.perf_counter() - t
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
    multigrid_masked_cells(1)


if __name__ == "__main__":
    main()
