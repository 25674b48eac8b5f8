"""Per-rank cost of keeping a row slab and its slab hierarchy across a value update, against creating them again.

Two ranks sharing one GPU over gloo (the rehearsal of tests/test_dist.py: per-rank costs, NOT scaling results — both ranks' kernels queue
on the one device and the halo is staged through the host):

    for r in 0 1; do RANK=$r WORLD_SIZE=2 MASTER_ADDR=127.0.0.1 MASTER_PORT=29655 python tools/slab_update_probe.py 96 350 & done; wait

The SiO2-like matrix on N^3 (argv[1], default 96) with argv[2] atoms (default 350; R0 = 2, R1 = 5), two slabs of N / 2 planes, dense mode
as the library defaults.  Measured on every rank between a barrier and a device synchronisation, after one warm-up, REPS times, median
(min .. max) reported by rank 0 for both ranks:
  update     HipBackend.matrix_update_values(agree=comm) with values already on the device, alternating between two value sets
  re-create  gcge_hip_mat_destroy + hip_slab_matrix from host arrays (localisation, halo plan, analysis, upload)
  refresh    GCGE_AMGRefresh of a 3-level slab hierarchy after an update
  rebuild    GCGE_AMGDestroy + GCGE_AMGCreate of the same hierarchy (host-side coarsening, collective coarse slab construction)"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
REPS = 5


def main():
    import torch
    import torch.distributed as dist
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from gcge_amd import HipBackend, make_problem
    from gcge_amd import dist as gdist
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 96
    K = int(sys.argv[2]) if len(sys.argv) > 2 else 350
    assert world == 2 and N % 2 == 0
    plane, n_global = N * N, N ** 3
    part = [0, (N // 2) * plane, n_global]
    be = HipBackend(device=0)
    comm = gdist.install(be, dist, rank, world, stage_through_host=True)
    gdist.install_slab_factory(be, comm)

    def slab():
        return make_problem("sio2", N, row_begin=part[rank], row_end=part[rank + 1], K=K, R0=2.0, R1=5.0, seed=12345)[0]

    A = slab()
    n_loc, nnz = A.nrows, int(A.nnz)
    rp = np.ctypeslib.as_array(A.rowptr, shape=(n_loc + 1,)).astype(np.int64)
    grow = part[rank] + np.repeat(np.arange(n_loc), np.diff(rp))
    gcol = np.ctypeslib.as_array(A.colidx, shape=(nnz,)).astype(np.int64)
    val0 = np.ctypeslib.as_array(A.val, shape=(nnz,)).copy()
    dg = grow == gcol
    val1 = val0.copy()
    val1[dg] += 0.25 * (1.0 + grow[dg] % 11)                    # another potential: the diagonal alone
    d_vals = [torch.from_numpy(v).cuda() for v in (val1, val0)]
    del grow, gcol, dg

    def timed(fn, reps=REPS):
        fn()                                                    # warm-up
        ts = []
        for k in range(reps):
            be.sync(); dist.barrier()
            t0 = time.perf_counter()
            fn()
            be.sync()
            ts.append(time.perf_counter() - t0)
        return ts

    state = {"k": 0}
    mat = gdist.hip_slab_matrix(be, comm, A, n_global, part, cap_cols=64, updatable=True)
    form = be.g.gcge_hip_mat_spmm_form(mat).decode()

    def update():
        ok = be.matrix_update_values(mat, d_vals[state["k"] % 2], agree=comm)
        state["k"] += 1
        assert ok, "the slab declined"
    t_update = timed(update)

    def recreate():
        nonlocal mat
        be.free_matrix(mat)
        mat = gdist.hip_slab_matrix(be, comm, slab(), n_global, part, cap_cols=64, updatable=True)
    t_gen = timed(lambda: slab(), 3)                            # (the generator's share of re-creation: reported apart)
    t_recreate = timed(recreate, 3)

    hier = be.multigrid(mat, None, levels=3, block_size=8, refreshable=True)
    levels = hier.num_levels

    def refresh():
        update()
        be.sync()
        t0 = time.perf_counter()
        rc = be.h.GCGE_AMGRefresh(hier._amg, be.ops_handle)
        be.sync()
        state["refresh"] = time.perf_counter() - t0
        assert rc == 0, rc
    t_refresh = []
    refresh()
    for k in range(REPS):
        dist.barrier()
        refresh()
        t_refresh.append(state["refresh"])

    def rebuild():
        hier.close()
        hier._create()
    t_rebuild = timed(rebuild, 3)
    forms = [be.g.gcge_hip_mat_spmm_form(m).decode() for m in hier.level_handles()[0]]
    hier.close()
    be.free_matrix(mat)
    mine = dict(rank=rank, rows=n_loc, nnz=nnz, form=form, levels=levels, forms=forms, update=t_update, generate=t_gen, recreate=t_recreate,
                refresh=t_refresh, rebuild=t_rebuild)
    allr = [None] * world
    dist.all_gather_object(allr, mine)
    if rank == 0:
        fmt = lambda ts: "median %.4f s (min %.4f, max %.4f, n = %d)" % (float(np.median(ts)), min(ts), max(ts), len(ts))
        for m in allr:
            print("rank %d: %d rows, %d entries, level 0 %s, %d levels %s" % (m["rank"], m["rows"], m["nnz"], m["form"], m["levels"], m["forms"]))
            for key in ("update", "generate", "recreate", "refresh", "rebuild"):
                print("    %-9s %s" % (key, fmt(m[key])))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
