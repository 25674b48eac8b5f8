"""PAS probe.
    python tools/pas_probe.py kernel            the bordered product (pas_border.hip) alone at (n_H, s, m) = (262144, 128, 64) and
                                                (2097152, 128, 64) against LinearComb + Gram on the same data: time and bytes/s
    python tools/pas_probe.py solve [N]         config 2's problem (Lap3D N^3, default 256; nev 50, block 64, nevMax 128) through
                                                PAS + GCG and through GCG + BlockAMG (bench --amg 6's settings): wall time,
                                                iterations, error against the closed form
Bytes: fused 8 n (s + 3 m) (QX and q once, y read and written), slots 8 n (2 s + 3 m) (QX twice)."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gcge_amd import HipBackend, make_problem, run_gcg, run_pas  # noqa: E402


def kernel():
    hip = HipBackend()
    g = hip.g
    g.gcge_hip_pas_border.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double,
                                      C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double), C.c_int]
    ops = hip.ops
    for n, s, m in ((262144, 128, 64), (2097152, 128, 64)):
        rp = np.arange(n + 1, dtype=np.int32)
        ci = np.arange(n, dtype=np.int32)
        va = np.ones(n)
        from gcge_amd.lib import CSR
        I = CSR(n, n, 0, n, rp.ctypes.data_as(C.POINTER(C.c_int)), ci.ctypes.data_as(C.POINTER(C.c_int)),
                va.ctypes.data_as(C.POINTER(C.c_double)))
        mat = hip.matrix(I)
        QX = ops.mv_create(s, mat); q = ops.mv_create(m, mat); y = ops.mv_create(m, mat)
        ops.set_random(QX, 0, s); ops.set_random(q, 0, m); ops.set_random(y, 0, m)
        t = np.asfortranarray(np.random.default_rng(1).random((s, m)))
        gbuf = np.zeros((s, m), order="F")
        tp, gp = t.ctypes.data_as(C.POINTER(C.c_double)), gbuf.ctypes.data_as(C.POINTER(C.c_double))
        ones = np.ones(m)

        def fused():
            g.gcge_hip_pas_border(QX, s, q, 0, y, 0, m, 1.0, tp, s, gp, s)

        def slots():
            ops.lincomb(QX, y, (0, 0), (s, m), t, s, ones, 1)
            gbuf[:] = ops.inner_prod("N", QX, q, (0, 0), (s, m))

        for name, fn, nbytes in (("fused", fused, 8.0 * n * (s + 3 * m)), ("LinearComb+Gram", slots, 8.0 * n * (2 * s + 3 * m))):
            fn(); hip.sync()
            reps = 10
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            hip.sync()
            dt = (time.perf_counter() - t0) / reps
            print("n_H=%8d s=%3d m=%3d  %-16s %.3f ms  %.2f TB/s on %.0f MB" % (n, s, m, name, 1e3 * dt, nbytes / dt * 1e-12,
                                                                              nbytes / 1e6), flush=True)
        for v, c in ((QX, s), (q, m), (y, m)):
            ops.mv_destroy(v, c)
        hip.free_matrix(mat)


def lap3d_exact(N, count):
    c = 2.0 * np.cos(np.arange(1, N + 1) * np.pi / (N + 1))
    return np.sort((6.0 - c[:, None, None] - c[None, :, None] - c[None, None, :]).ravel())[:count]


def solve(N):
    hip = HipBackend()
    A, _ = make_problem("lap3d", N)
    mA = hip.matrix(A)
    ex = lap3d_exact(N, 50)
    base = ["-nevConv", 50, "-blockSize", 64, "-nevMax", 128]
    t0 = time.perf_counter()
    ev, pr, gr = run_pas(hip.ops_handle, mA, None, base)
    t_pas = time.perf_counter() - t0
    print("PAS+GCG : %.2f s (PAS %.2f s, %d iterations, nevConv %d; GCG %.2f s, %d iterations, nevConv %d)  max |err| %.2e"
          % (t_pas, pr.seconds, pr.numIter, pr.nevConv, gr.seconds, gr.numIter, gr.nevConv, np.max(np.abs(ev[:50] - ex))), flush=True)
    t0 = time.perf_counter()
    ev2, r2 = run_gcg(hip.ops_handle, mA, None, base + ["-gcge_amg_levels", 6])
    t_amg = time.perf_counter() - t0
    print("GCG+AMG : %.2f s (%d iterations, nevConv %d)  max |err| %.2e" % (t_amg, r2.numIter, r2.nevConv,
                                                                           np.max(np.abs(ev2[:50] - ex))), flush=True)
    hip.free_matrix(mA)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    if what == "kernel":
        kernel()
    else:
        solve(int(sys.argv[2]) if len(sys.argv) > 2 else 256)
