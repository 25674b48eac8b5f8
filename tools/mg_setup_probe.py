"""Multigrid set-up of the HIP back-end in both modes: the phase split of MultiGridCreate, the bytes copied device to host and the
total set-up time, for one problem of the existing generators.

  python tools/mg_setup_probe.py <lap3d|fe3d|sio2> <size> [levels]

Mode 0 builds the hierarchy on the device (csrc/hip/mg_device.hip), mode 1 on the host (csrc/host/multigrid.c); both give the same
hierarchy.  Each mode is timed on a fresh MultiGridCreate after one warm-up call."""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch  # noqa: F401  (one libamdhip64, shared with torch)
    from gcge_amd import HipBackend
    from gcge_amd.lib import hip_lib, make_problem, multigrid_mode, multigrid_stats
    from gcge_amd.ops_struct import OPS
    kind, size = sys.argv[1], int(sys.argv[2])
    levels = int(sys.argv[3]) if len(sys.argv) > 3 else 6
    hip = HipBackend()
    A, B = make_problem(kind, size)
    mA = hip.matrix(A)
    mB = hip.matrix(B) if B is not None else None
    st = C.cast(hip.ops_handle, C.POINTER(OPS)).contents
    create = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_void_p)(st.MultiGridCreate)
    destroy = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_void_p)(st.MultiGridDestroy)
    fine = (A.nrows + 1) * 4 + int(A.nnz) * 12
    print("%s %d: %d rows, %d non-zeros, fine CSR %.1f MB%s" % (kind, size, A.nrows, A.nnz, fine / 1e6, ", with B" if mB else ""))
    for mode in (0, 1):
        multigrid_mode(mode)
        for rep in range(2):
            A_arr, B_arr, P_arr, nl = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int(levels)
            bref = C.byref(B_arr) if mB is not None else None
            t = time.perf_counter()
            create(C.byref(A_arr), bref, C.byref(P_arr), C.byref(nl), mA, mB, hip.ops_handle)
            total = time.perf_counter() - t
            secs, d2h = multigrid_stats()
            destroy(C.byref(A_arr), bref, C.byref(P_arr), C.byref(nl), hip.ops_handle)
        print("mode %d (%s): %d levels, %.3f s  [%s]  device->host %.1f MB (%.1f%% of the fine CSR)" % (
            mode, "device" if mode == 0 else "host", nl.value, total, "  ".join("%s %.3f" % kv for kv in secs.items()), d2h / 1e6, 100.0 * d2h / fine))
    multigrid_mode(0)


if __name__ == "__main__":
    main()
