"""Wall time of gcge_hip_mat_update_values_device against gcge_hip_mat_create_device on the same device arrays, lap3d N^3:
    U        every value doubled: the value table is rewritten, the form stays
    V first  diag[r] += (7 r) % 5 on a fresh handle: the conversion to the "+values" form (allocates the per-row values)
    V again  the same values on the converted handle: the re-scatter
Both calls synchronise before they return, so a host clock round them times the work; `warm` calls first where a call can be repeated
on one handle, then the median of `reps`.  GB/s counts the bytes an update has to move: 8 nnz + 2 n read, 8 nnz + 64 noct written, and
64 n more where the per-row values are written (the check pass reads the values and columns once more on handles with a table: that
is the kernels' own traffic, not counted).
    python tools/mat_update_probe.py N [N ...] [--out FILE]
With --star G K the star case runs instead: make_problem("sio2", G, K=K, R0=2.0, R1=5.0) (G = 171, K = 2000 is BASELINE config 5's
matrix, as in tools/tile_probe.py), uploaded through gcge_hip_mat_create_csr:
    create, maps off / on     the upload with gcge_hip_mat_keep_value_maps 0 / 1 (the host analysis: star split, blocks, layers, pad-8)
    free + create             what an SCF step costs without the update: gcge_hip_mat_destroy + the upload of the new values
    update D / O              a new diagonal in every row / the creation values again, in place (GB/s counts 16 bytes per CSR entry only)
and the bytes of maps the handle holds.  A library without the switch (an earlier commit) runs the "maps off" rows only."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from gcge_amd import HipBackend, make_problem
from gcge_amd.lib import csr_arrays, mat_update_stats

argv = list(sys.argv[1:])
out_path = None
if "--out" in argv:
    i = argv.index("--out"); out_path = argv[i + 1]; del argv[i:i + 2]
star_case = None
if "--star" in argv:
    i = argv.index("--star"); star_case = (int(argv[i + 1]), int(argv[i + 2])); del argv[i:i + 3]
sizes = [int(a) for a in argv] or ([] if star_case else [128])
hip = HipBackend(); g = hip.g
results = []


def timed(fn, warm, reps):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def report(name, N, n, nnz, t, nbytes):
    gbs = nbytes / t[0] / 1e9 if nbytes else None
    results.append({"case": name, "N": N, "n": n, "nnz": nnz, "median_ms": 1e3 * t[0], "min_ms": 1e3 * t[1], "max_ms": 1e3 * t[2], "bytes": nbytes, "GBps": gbs})
    print("%-44s N %4d  median %10.3f ms  (min %10.3f, max %10.3f)  %s" % (name, N, 1e3 * t[0], 1e3 * t[1], 1e3 * t[2],
                                                                            "%8.1f GB/s" % gbs if gbs else ""), flush=True)


def star_probe(G, K):
    import ctypes as C
    t0 = time.perf_counter()
    A = make_problem("sio2", G, K=K, R0=2.0, R1=5.0)[0]
    rp, ci, va = csr_arrays(A)
    n, nnz = A.nrows, int(va.size)
    print("sio2 %d, K %d: n %d, nnz %d, generated in %.1f s" % (G, K, n, nnz, time.perf_counter() - t0), flush=True)
    has_switch = hasattr(g, "gcge_hip_mat_keep_value_maps")

    def create(on):
        if has_switch:
            g.gcge_hip_mat_keep_value_maps(1 if on else 0)
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter(); m = g.gcge_hip_mat_create_csr(C.byref(A)); t = time.perf_counter() - t0
        finally:
            if has_switch:
                g.gcge_hip_mat_keep_value_maps(0)
        assert m
        return C.c_void_p(m), t

    def one(name, ts, nbytes=0):
        report(name, G, n, nnz, (float(np.median(ts)), min(ts), max(ts)), nbytes)

    m, t_first = create(False)
    form = g.gcge_hip_mat_spmm_form(m).decode()
    print("form:", form, flush=True)
    ts = []
    for _ in range(2):                                             # free + create from the same values, maps off
        torch.cuda.synchronize()
        t0 = time.perf_counter(); g.gcge_hip_mat_destroy(m); m, t = create(False); ts.append(time.perf_counter() - t0)
    one("free + create, maps off (%s)" % form, ts)
    one("create, maps off", [t_first, t])
    g.gcge_hip_mat_destroy(m)
    if not has_switch:
        return
    ts, tc = [], []
    m, t = create(True); tc.append(t)
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter(); g.gcge_hip_mat_destroy(m); m, t = create(True); ts.append(time.perf_counter() - t0); tc.append(t)
    one("free + create, maps on", ts)
    one("create, maps on", tc)
    nmap = int(g.gcge_hip_mat_value_maps(m))
    print("bytes of maps: %d (%.2f per stored entry)" % (nmap, nmap / nnz), flush=True)
    results.append({"case": "bytes of maps", "N": G, "n": n, "nnz": nnz, "bytes": nmap})
    assert nmap > 0 and g.gcge_hip_mat_spmm_form(m).decode() == form
    d_va = torch.from_numpy(va).cuda()
    d_rp, d_ci = torch.from_numpy(rp).cuda(), torch.from_numpy(ci).cuda()
    rows = torch.repeat_interleave(torch.arange(n, device="cuda", dtype=torch.int32), (d_rp[1:] - d_rp[:-1]).to(torch.int64))
    diag = rows == d_ci
    d_d = d_va + torch.where(diag, torch.rand(n, dtype=torch.float64, device="cuda")[rows.to(torch.int64)], torch.zeros((), dtype=torch.float64, device="cuda"))
    del rows, d_rp, d_ci
    torch.cuda.synchronize()
    s0 = mat_update_stats()
    report("update D (a new diagonal)", G, n, nnz, timed(lambda: g.gcge_hip_mat_update_values_device(m, nnz, d_d.data_ptr()), 1, 5), 16 * nnz)
    report("update O (the creation values again)", G, n, nnz, timed(lambda: g.gcge_hip_mat_update_values_device(m, nnz, d_va.data_ptr()), 1, 5), 16 * nnz)
    s1 = mat_update_stats()
    assert s1[0] - s0[0] == 12 and s1[3] == s0[3], (s0, s1)
    g.gcge_hip_mat_destroy(m)


print("device:", torch.cuda.get_device_name(0), flush=True)
if star_case:
    star_probe(*star_case)
for N in sizes:
    rp, ci, va = csr_arrays(make_problem("lap3d", N)[0])
    n, nnz = rp.size - 1, int(va.size)
    d_rp, d_ci, d_va = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (rp, ci, va))
    del rp, ci, va
    rows = torch.repeat_interleave(torch.arange(n, device="cuda", dtype=torch.int32), (d_rp[1:] - d_rp[:-1]).to(torch.int64))
    diag = rows == d_ci
    d_u = d_va * 2.0
    d_v = d_va + torch.where(diag, ((7 * rows.to(torch.int64)) % 5).to(torch.float64), torch.zeros((), dtype=torch.float64, device="cuda"))
    # an SCF step proper: another diagonal in EVERY row (the device search gives up on it: more classes than a table holds)
    d_s = d_va + torch.where(diag, torch.rand(n, dtype=torch.float64, device="cuda")[rows.to(torch.int64)], torch.zeros((), dtype=torch.float64, device="cuda"))
    del rows, diag
    torch.cuda.synchronize()
    noct = n                                                       # rows of at most 7 entries: one octet each
    moved = 8 * nnz + 2 * n + 8 * nnz + 64 * noct

    made = []

    def create(vals=None):
        m = g.gcge_hip_mat_create_device(n, nnz, d_rp.data_ptr(), d_ci.data_ptr(), (d_va if vals is None else vals).data_ptr())
        assert m
        made.append(m)

    def drop():
        while made:
            g.gcge_hip_mat_destroy(made.pop())

    ts = []
    for _ in range(4):                                             # (the first call warms the kernels up)
        torch.cuda.synchronize()
        t0 = time.perf_counter(); create(); ts.append(time.perf_counter() - t0)
        drop()
    report("gcge_hip_mat_create_device", N, n, nnz, (float(np.median(ts[1:])), min(ts[1:]), max(ts[1:])), 0)
    ts = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter(); create(d_v); ts.append(time.perf_counter() - t0)
        drop()
    report("gcge_hip_mat_create_device, V values", N, n, nnz, (float(np.median(ts)), min(ts), max(ts)), 0)
    ts = []
    for _ in range(2 if N <= 128 else 1):                          # (this one goes through the host: seconds at 256^3)
        torch.cuda.synchronize()
        t0 = time.perf_counter(); create(d_s); ts.append(time.perf_counter() - t0)
        form_s = g.gcge_hip_mat_spmm_form(made[-1]).decode()
        drop()
    report("gcge_hip_mat_create_device, a diagonal per row (%s)" % form_s, N, n, nnz, (float(np.median(ts)), min(ts), max(ts)), 0)
    create(); m = made[-1]
    ts = []
    for k in range(3):                                             # the same values through the update: conversion first, then re-scatters
        torch.cuda.synchronize()
        t0 = time.perf_counter(); rc = g.gcge_hip_mat_update_values_device(m, nnz, d_s.data_ptr()); ts.append(time.perf_counter() - t0)
        assert rc == 0
    report("update, a diagonal per row (conversion; min = re-scatter)", N, n, nnz, (ts[0], min(ts), max(ts)), moved + 64 * n)
    drop()

    create(); m = made[-1]
    form0 = g.gcge_hip_mat_spmm_form(m).decode()
    s0 = mat_update_stats()
    report("update U (table rewrite, %s)" % form0, N, n, nnz, timed(lambda: g.gcge_hip_mat_update_values_device(m, nnz, d_u.data_ptr()), 2, 7), moved)
    s1 = mat_update_stats()
    assert s1[1] - s0[1] == 9 and g.gcge_hip_mat_spmm_form(m).decode() == form0, (s0, s1)
    drop()

    ts = []
    for k in range(4):                                             # a conversion happens once per handle: a fresh handle every time
        create(); m = made[-1]
        torch.cuda.synchronize()
        t0 = time.perf_counter(); rc = g.gcge_hip_mat_update_values_device(m, nnz, d_v.data_ptr()); ts.append(time.perf_counter() - t0)
        assert rc == 0
        if k < 3:
            drop()
    form1 = g.gcge_hip_mat_spmm_form(m).decode()
    assert form1.endswith("+values"), form1
    report("update V first (conversion to %s)" % form1, N, n, nnz, (float(np.median(ts[1:])), min(ts[1:]), max(ts[1:])), moved + 64 * n)
    s0 = mat_update_stats()
    report("update V again (re-scatter)", N, n, nnz, timed(lambda: g.gcge_hip_mat_update_values_device(m, nnz, d_v.data_ptr()), 2, 7), moved + 64 * n)
    s1 = mat_update_stats()
    assert s1[0] - s0[0] == 9 and s1[2] == s0[2] and s1[5] - s0[5] == 9 * 4, (s0, s1)
    drop()
    del d_rp, d_ci, d_va, d_u, d_v, d_s
    g.gcge_hip_pool_release()
    torch.cuda.empty_cache()
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "results": results}, f, indent=1)
