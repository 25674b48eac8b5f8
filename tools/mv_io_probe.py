"""Blocks of vectors in and out of the back-end: gcge_hip_mv_from_device (rows contiguous, columns contiguous, general strides, and rows
/ columns contiguous into a re-ordered handle), gcge_hip_mv_to_device, a hipMemcpyDtoD of the same bytes in the same process (the
yardstick for a copy) and gcge_hip_mv_from_host of the same block (the path the device call replaces).  Every call synchronises, so
a host clock round it times the work; `warm` calls first, then the median of `reps`.  GB/s counts the block's bytes once read and
once written (2 * 8 n m).
    python tools/mv_io_probe.py n m [n_reordered] [--out FILE]
n_reordered (default 128^3): rows of the re-ordered handle, a randomly numbered 7-point Laplacian on a cube whose scan order the upload
recovers — a cube number; the host work of that upload is why it is smaller than n."""
import ctypes as C, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from gcge_amd import HipBackend, make_problem
from gcge_amd.lib import csr_to_scipy

argv = [a for a in sys.argv[1:]]
out_path = None
if "--out" in argv:
    i = argv.index("--out"); out_path = argv[i + 1]; del argv[i:i + 2]
n = int(argv[0]) if len(argv) > 0 else 1 << 24
m = int(argv[1]) if len(argv) > 1 else 64
n_re = int(argv[2]) if len(argv) > 2 else 128 ** 3
hip = HipBackend(); g = hip.g
g.gcge_hip_spmm_reorder_mode.argtypes = [C.c_int]
g.gcge_hip_mat_row_order.restype, g.gcge_hip_mat_row_order.argtypes = C.c_char_p, [C.c_void_p]
rt = C.CDLL(None)
rt.hipMemcpyDtoD.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
rt.hipDeviceSynchronize.argtypes = []


def diag_handle(rows):
    rp = np.arange(rows + 1, dtype=np.int32); ci = np.arange(rows, dtype=np.int32); va = np.ones(rows)
    return hip.matrix_from_device(torch.from_numpy(rp).cuda(), torch.from_numpy(ci).cuda(), torch.from_numpy(va).cuda())


def timed(fn, warm, reps):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


results = []


def report(name, rows, cols, t):
    gbs = 2 * 8.0 * rows * cols / t[0] / 1e9
    results.append({"case": name, "n": rows, "m": cols, "median_ms": 1e3 * t[0], "min_ms": 1e3 * t[1], "max_ms": 1e3 * t[2], "GBps": gbs})
    print("%-58s n %9d m %4d  median %10.3f ms  (min %10.3f, max %10.3f)  %8.1f GB/s" % (name, rows, cols, 1e3 * t[0], 1e3 * t[1], 1e3 * t[2], gbs), flush=True)


def device_cases(mat, rows, tag, strided):
    x = torch.rand((rows, m), dtype=torch.float64, device="cuda")
    mv = hip.ops.mv_create(m, mat)
    ptr = lambda t: t.data_ptr()
    report("mv_from_device rows contiguous" + tag, rows, m, timed(lambda: g.gcge_hip_mv_from_device(mv, 0, m, ptr(x), m, 1), 3, 9))
    xt = x.t().contiguous()
    report("mv_from_device columns contiguous" + tag, rows, m, timed(lambda: g.gcge_hip_mv_from_device(mv, 0, m, ptr(xt), 1, rows), 3, 9))
    del xt
    out = torch.empty((rows, m), dtype=torch.float64, device="cuda")
    report("mv_to_device" + tag, rows, m, timed(lambda: g.gcge_hip_mv_to_device(mv, 0, m, ptr(out), m), 3, 9))
    if strided:
        report("mv_from_device general strides (2 m, 2)", rows, m // 2, timed(lambda: g.gcge_hip_mv_from_device(mv, 0, m // 2, ptr(x), m, 2), 3, 9))
        report("mv_from_device rows contiguous, odd first columns", rows, m - 2, timed(lambda: g.gcge_hip_mv_from_device(mv, 1, m - 1, ptr(x) + 8, m, 1), 3, 9))
        report("mv_from_device rows contiguous, 8-byte lanes", rows, m - 2, timed(lambda: g.gcge_hip_mv_from_device(mv, 0, m - 2, ptr(x) + 8, m, 1), 3, 9))

        def dtod():
            rc = rt.hipMemcpyDtoD(ptr(out), ptr(x), 8 * rows * m)
            assert rc == 0, rc
            rt.hipDeviceSynchronize()
        report("hipMemcpyDtoD of the same bytes", rows, m, timed(dtod, 3, 9))
    del x, out
    return mv


print("device:", torch.cuda.get_device_name(0), flush=True)
mat = diag_handle(n)
mv = device_cases(mat, n, "", True)
h = np.ones((n, m), order="F")
hp = h.ctypes.data_as(C.POINTER(C.c_double))
report("mv_from_host (the path replaced)", n, m, timed(lambda: g.gcge_hip_mv_from_host(mv, 0, m, hp, n), 1, 3))
del h
hip.ops.mv_destroy(mv, m)
hip.free_matrix(mat)
g.gcge_hip_pool_release()
torch.cuda.empty_cache()

# a re-ordered handle
N = round(n_re ** (1.0 / 3.0))
assert N ** 3 == n_re, "n_reordered is a cube number"
S = csr_to_scipy(make_problem("lap3d", N)[0])
p = np.random.default_rng(7).permutation(n_re)
S = S[p][:, p].tocsr(); S.sort_indices()
rp, ci, va = S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data.astype(np.float64)
from gcge_amd.lib import CSR
A = CSR(n_re, n_re, 0, int(S.nnz), rp.ctypes.data_as(C.POINTER(C.c_int)), ci.ctypes.data_as(C.POINTER(C.c_int)), va.ctypes.data_as(C.POINTER(C.c_double)))
g.gcge_hip_spmm_reorder_mode(1)
t0 = time.perf_counter()
mat = hip.matrix(A)
order = g.gcge_hip_mat_row_order(mat).decode()
print("re-ordered handle: %d rows, row order: %s (upload %.1f s)" % (n_re, order, time.perf_counter() - t0), flush=True)
assert order != "as given"
mv = device_cases(mat, n_re, ", re-ordered handle", False)
h = np.ones((n_re, m), order="F")
hp = h.ctypes.data_as(C.POINTER(C.c_double))
report("mv_from_host, re-ordered handle", n_re, m, timed(lambda: g.gcge_hip_mv_from_host(mv, 0, m, hp, n_re), 1, 3))
hip.ops.mv_destroy(mv, m)
hip.free_matrix(mat)
g.gcge_hip_spmm_reorder_mode(0)
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "n": n, "m": m, "n_reordered": n_re, "row_order": order, "results": results}, f, indent=1)
