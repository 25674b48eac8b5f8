"""Wall time of gcge_hip_mat_update_values_device on a handle that RE-ORDERED its rows, against the same update of the same matrix in its
natural order and against freeing the handle and creating the matrix again.  The matrix is the one bench.py's roofline_k1_permuted leg
generates: make_problem("sio2", G, K=K, R0=2.0, R1=5.0, seed=12345) under the random symmetric permutation of seed 20240601
(G = 128, K = 839 by default), uploaded through HipBackend.matrix:
    update, re-ordered        the permuted arrays, updatable=True: the gather through the entry map, then the update of the handle's form
    update, natural order     the generator's arrays, updatable=True: that update alone
    free + create, permuted   gcge_hip_mat_destroy + the upload of the permuted arrays (updatable=False), what a step costs without the update
    multigrid build / refresh hierarchies of 3 and of 2 levels over either handle: built, then gcge_hip_multigrid_refresh after an update
Updates: a new diagonal in every row; the stream is synchronised before and after (the call ends in a synchronise), one warm-up call,
then the median of 5.  The gather moves 20 bytes per entry (4 of map, 8 read, 8 written); its time is taken as the difference of the two
update medians, which run the same kernels on handles of the same form otherwise.
    python tools/mat_update_reordered_probe.py [G K [R0 R1]] [--out FILE]      (R0, R1: the atoms' radii, default 2.0 5.0)"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.sparse as sp
import torch
from gcge_amd import HipBackend, make_problem
from gcge_amd.lib import CSR, csr_arrays, mat_update_stats
import ctypes as C

argv = list(sys.argv[1:])
out_path = None
if "--out" in argv:
    i = argv.index("--out"); out_path = argv[i + 1]; del argv[i:i + 2]
G, K = (int(argv[0]), int(argv[1])) if len(argv) >= 2 else (128, 839)
R0, R1 = (float(argv[2]), float(argv[3])) if len(argv) >= 4 else (2.0, 5.0)
hip = HipBackend(); g = hip.g
results = {"device": torch.cuda.get_device_name(0), "G": G, "K": K, "R0": R0, "R1": R1}
IP, DP = C.POINTER(C.c_int), C.POINTER(C.c_double)


def say(key, value, text):
    results[key] = value
    print(text, flush=True)


def timed(fn, warm=1, reps=5):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def handle_of(arrays, updatable):
    rp, ci, va = arrays
    A = CSR(rp.size - 1, rp.size - 1, 0, va.size, rp.ctypes.data_as(IP), ci.ctypes.data_as(IP), va.ctypes.data_as(DP))
    torch.cuda.synchronize()
    t0 = time.perf_counter(); m = hip.matrix(A, updatable=updatable); hip.sync()
    return m, time.perf_counter() - t0


def new_diagonal(arrays):
    rp, ci, va = arrays
    rows = np.repeat(np.arange(rp.size - 1, dtype=np.int32), np.diff(rp))
    v = va.copy()
    d = rows == ci
    v[d] += np.random.default_rng(5).random(int(d.sum()))
    return torch.from_numpy(v).cuda()


def hierarchy_probe(tag, m, d_a, d_b):
    """hierarchies of 3 and of 2 levels over m: build time, then gcge_hip_multigrid_refresh after every one of 5 updates (d_a, d_b in turn)"""
    for levels in (3, 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter(); h = hip.multigrid(m, levels=levels); hip.sync(); t_build = time.perf_counter() - t0
        Ah = h.level_handles()[0]
        head, L = h._head(), h.num_levels
        say("multigrid_%s_L%d_build_s" % (tag, levels), t_build, "%s, %d levels: built in %.3f s; rows %s; forms %s; row orders %s" % (
            tag, L, t_build, [g.gcge_hip_mat_nrows(a) for a in Ah], [g.gcge_hip_mat_spmm_form(a).decode() for a in Ah],
            ["as given" if g.gcge_hip_mat_row_order(a).decode() == "as given" else "re-ordered" for a in Ah]))
        tr, rcs = [], []
        for k in range(5):
            assert g.gcge_hip_mat_update_values_device(m, nnz, (d_b if k % 2 else d_a).data_ptr()) == 0
            torch.cuda.synchronize()
            t0 = time.perf_counter(); rc = g.gcge_hip_multigrid_refresh(head.A_array, None, head.P_array, L); hip.sync(); tr.append(time.perf_counter() - t0)
            rcs.append(rc)
            if rc != 0:
                break
        say("multigrid_%s_L%d_refresh_rc" % (tag, levels), rcs, "%s, %d levels: gcge_hip_multigrid_refresh returned %s" % (tag, L, rcs))
        if rcs[-1] == 0:
            say("multigrid_%s_L%d_refresh_ms" % (tag, levels), [1e3 * x for x in tr], "%s, %d levels: refresh first %.3f ms, median of the other 4 %.3f ms" % (
                tag, L, 1e3 * tr[0], 1e3 * float(np.median(tr[1:]))))
        h.close()


t0 = time.perf_counter()
A0 = make_problem("sio2", G, K=K, R0=R0, R1=R1, seed=12345)[0]
nat = tuple(np.ascontiguousarray(a).copy() for a in csr_arrays(A0))
n, nnz = nat[0].size - 1, int(nat[2].size)
S = sp.csr_matrix((nat[2], nat[1], nat[0]), shape=(n, n))
p = np.random.default_rng(20240601).permutation(n)
ip = np.empty(n, dtype=np.int32); ip[p] = np.arange(n, dtype=np.int32)
Sp = S[p].tocsr(); Sp.indices = ip[Sp.indices]; Sp.has_sorted_indices = False; Sp.sort_indices()
per = (np.ascontiguousarray(Sp.indptr, dtype=np.int32), np.ascontiguousarray(Sp.indices, dtype=np.int32), np.ascontiguousarray(Sp.data, dtype=np.float64))
del S, Sp
say("n", n, "sio2 %d, K %d, R0 %g, R1 %g: n %d, nnz %d, generated and permuted in %.1f s" % (G, K, R0, R1, n, nnz, time.perf_counter() - t0))
results["nnz"] = nnz

# ---- natural order
m, t = handle_of(nat, True)
say("create_natural_updatable_s", t, "create, natural order, updatable: %.2f s (%s; %s)" % (t, g.gcge_hip_mat_spmm_form(m).decode(), g.gcge_hip_mat_row_order(m).decode()))
d_new, d_old = new_diagonal(nat), torch.from_numpy(nat[2]).cuda()
s0 = mat_update_stats()
tb = timed(lambda: g.gcge_hip_mat_update_values_device(m, nnz, d_new.data_ptr()))
assert mat_update_stats()[0] - s0[0] == 6, (s0, mat_update_stats())
say("update_natural_ms", [1e3 * x for x in tb], "update, natural order:   median %9.3f ms (min %9.3f, max %9.3f)" % tuple(1e3 * x for x in tb))
hierarchy_probe("natural", m, d_new, d_old)
hip.free_matrix(m); del d_new, d_old

# ---- re-ordered
m, t = handle_of(per, True)
form, order = g.gcge_hip_mat_spmm_form(m).decode(), g.gcge_hip_mat_row_order(m).decode()
say("create_permuted_updatable_s", t, "create, permuted, updatable: %.2f s (%s; %s)" % (t, form, order))
assert order != "as given"
nmap = int(g.gcge_hip_mat_entry_map(m))
say("entry_map_bytes", nmap, "bytes of entry map: %d (%.2f per entry); value maps %d" % (nmap, nmap / nnz, int(g.gcge_hip_mat_value_maps(m))))
d_new = new_diagonal(per)
s0 = mat_update_stats()
ta = timed(lambda: g.gcge_hip_mat_update_values_device(m, nnz, d_new.data_ptr()))
assert mat_update_stats()[0] - s0[0] == 6, (s0, mat_update_stats())
say("update_reordered_ms", [1e3 * x for x in ta], "update, re-ordered:      median %9.3f ms (min %9.3f, max %9.3f)" % tuple(1e3 * x for x in ta))
dt = ta[0] - tb[0]
say("gather_ms_by_difference", 1e3 * dt, "gather, by difference:   %9.3f ms, 20 bytes per entry: %.0f GB/s" % (1e3 * dt, 20.0 * nnz / dt / 1e9 if dt > 0 else float("nan")))

# ---- the hierarchy over the re-ordered handle, and over the natural-order one for comparison
d_old = torch.from_numpy(per[2]).cuda()
hierarchy_probe("reordered", m, d_new, d_old)
del d_old, d_new

# ---- free + create
ts = []
for _ in range(2):
    torch.cuda.synchronize()
    t0 = time.perf_counter(); hip.free_matrix(m); m, t = handle_of(per, False); ts.append(time.perf_counter() - t0)
assert g.gcge_hip_mat_entry_map(m) == 0
say("free_create_permuted_s", ts, "free + create, permuted, updatable=False: %.2f s, %.2f s" % tuple(ts))
hip.free_matrix(m)
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(results, f, indent=1)
