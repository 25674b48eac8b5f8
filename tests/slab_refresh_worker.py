"""Worker of tests/test_mg_refresh_slab.py: 2 or 3 ranks sharing cuda:0 over gloo (the rehearsal of tests/test_dist.py).

argv[1] = "refresh", argv[2] = the matrix:
  lap:NX,NY,NZ[:P1,P2,..]   the 7-point Laplacian, slabs of whole planes (row_partition, or cut on the planes named: an odd cut)
  sio2:16                   make_problem("sio2", 16, K=8, R0=1.5, R1=3.0), two slabs of 8 planes, dense mode 1: level 0 in star or block form
                            on both ranks, and rank 0's level 1 (256 rows, atom rows of 50 entries) in block form.  (The 40 atoms of
                            tests/dist_worker.py's sio2:16 leave the upper slab without a detectable grid, and MultiGridCreate on a row
                            slab aborts there by design; 8 atoms are the generator's setting of the plane-aligned slab tests.)
Every rank creates its slab with updatable=True, builds the slab hierarchy with refreshable=True (coarse slabs through this
transport's constructor), updates level 0 in place (a potential on the diagonal, entries away from the star's positions scaled) and calls
GCGE_AMGRefresh, which must return 0 on every rank.  Then a second slab and hierarchy are built fresh from the new values: every level's
CSR (gcge_hip_mat_to_csr) must be bit-identical, and one BlockAMG solve of 8 right-hand sides over the refreshed hierarchy bit-identical
to the same solve over the fresh one.

argv[1] = "disagree" (sio2:16, two ranks): rank 0 creates its level 0 WITHOUT updatable.  matrix_update_values(agree=comm) must be False on
both ranks although rank 1's library call accepted; both re-create their slabs from the new values and build the hierarchy, rank 0 again
without the switch: its coarse slab is a block form without maps, so Hierarchy.refresh() must be False on both ranks (rank 1's own
levels would have gone through) — and nobody hangs."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def main():
    mode, spec = sys.argv[1], sys.argv[2]
    import torch
    import torch.distributed as dist
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from gcge_amd import HipBackend
    from gcge_amd import dist as gdist
    from gcge_amd.lib import CSR, csr_to_scipy, host_lib, make_problem, mat_to_csr
    from helpers import bits, block_amg_solve, uniform
    h = host_lib()
    be = HipBackend(device=0)
    g = be.g
    comm = gdist.install(be, dist, rank, world, stage_through_host=True)
    gdist.install_slab_factory(be, comm)
    kind, _, rest = spec.partition(":")
    if kind == "sio2":
        g.gcge_hip_spmm_dense_mode(1)                             # small atoms: rows of >= 24 entries may seed a block
    if kind == "lap":
        dims_s, _, planes_s = rest.partition(":")
        dims = tuple(int(t) for t in dims_s.split(","))
        n_global, plane = dims[0] * dims[1] * dims[2], dims[0] * dims[1]
        part = [int(t) * plane for t in planes_s.split(",")] if planes_s else gdist.row_partition(n_global, world)
    else:
        N = int(rest)
        dims, n_global, plane = (N, N, N), N ** 3, N * N
        part = [0, (N // 2) * plane, n_global]
    assert len(part) == world + 1 and all(p % plane == 0 for p in part), part
    levels = 3

    def slab():
        A = CSR()
        if kind == "lap":
            assert h.gcge_problem_lap3d_box(dims[0], dims[1], dims[2], C.c_int64(part[rank]), C.c_int64(part[rank + 1]), C.byref(A)) == 0
        else:
            A, _ = make_problem("sio2", dims[0], row_begin=part[rank], row_end=part[rank + 1], K=8, R0=1.5, R1=3.0, seed=12345)
        return A

    A = slab()
    Sg = csr_to_scipy(A).tocsr()                                # global columns, the generator's entry order
    n_loc, nnz = A.nrows, int(A.nnz)
    rp = np.ctypeslib.as_array(A.rowptr, shape=(n_loc + 1,)).astype(np.int64)
    grow = part[rank] + np.repeat(np.arange(n_loc), np.diff(rp))
    gcol = np.ctypeslib.as_array(A.colidx, shape=(nnz,)).astype(np.int64).copy()
    val0 = np.ctypeslib.as_array(A.val, shape=(nnz,)).copy()
    xyz = lambda q: np.stack([q % dims[0], (q // dims[0]) % dims[1], q // plane], axis=1)
    d = xyz(gcol) - xyz(grow)
    star_pos = ((d != 0).sum(axis=1) == 1) & (np.abs(d).sum(axis=1) <= 6)
    val1 = val0.copy()
    dg = grow == gcol
    val1[dg] += 0.25 * (1.0 + grow[dg] % 11)                    # a potential on the diagonal
    val1[~dg & ~star_pos] *= 1.5                                # the atoms' entries away from the star; star positions keep their values

    def create(v, updatable):
        B = slab()
        np.ctypeslib.as_array(B.val, shape=(nnz,))[:] = v
        m = gdist.hip_slab_matrix(be, comm, B, n_global, part, cap_cols=64, updatable=updatable)
        return m, B                                              # (B's arrays must outlive nothing, but keep them to be safe)

    def level_csr(hier):
        out = []
        for m in hier.level_handles()[0]:
            out.append(tuple(np.array(a, copy=True) for a in mat_to_csr(m)))
        return out

    def solve(hier, mat):
        Ah, _, Ph = hier.level_handles()
        L = hier.num_levels
        Bm = uniform(41 + rank, (n_loc, 8)) - 0.5
        x, niter, res = block_amg_solve(be, Ah, Ph, Bm, np.zeros_like(Bm), [1] + [5, 5] + [4, 4] * (L - 1), [1e-2] + [1e-16] * (L - 1), [1e-14] + [1e-16] * (L - 1))
        return x

    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()
    forms = lambda hier: [g.gcge_hip_mat_spmm_form(m).decode() for m in hier.level_handles()[0]]

    if mode == "refresh":
        mat, keepA = create(val0, True)
        hier = be.multigrid(mat, None, levels=levels, block_size=8, refreshable=True)
        assert hier.num_levels >= 2, hier.num_levels
        f_before = forms(hier)
        before = level_csr(hier)
        assert be.matrix_update_values(mat, dev(val1), agree=comm) is True, "rank %d: the slab declined its new values" % rank
        rc = be.h.GCGE_AMGRefresh(hier._amg, be.ops_handle)
        assert rc == 0, "rank %d: GCGE_AMGRefresh returned %d" % (rank, rc)
        got = level_csr(hier)
        mat2, keepB = create(val1, False)
        fresh = be.multigrid(mat2, None, levels=levels, block_size=8, refreshable=False)
        want = level_csr(fresh)
        assert len(got) == len(want) == hier.num_levels
        for l, (a, b) in enumerate(zip(got, want)):
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), "rank %d level %d: another structure" % (rank, l)
            nd = int(np.sum(bits(a[2]) != bits(b[2])))
            assert nd == 0, "rank %d level %d: %d of %d values differ from the fresh hierarchy's" % (rank, l, nd, a[2].size)
            assert l == 0 or not np.array_equal(bits(a[2]), bits(before[l][2])), "level %d did not change at all" % l
        x_r, x_f = solve(hier, mat), solve(fresh, mat2)
        assert np.all(np.isfinite(x_r)) and np.array_equal(bits(x_r), bits(x_f)), "rank %d: the BlockAMG solve over the refreshed hierarchy differs from the fresh one's" % rank
        print("rank %d: levels %d, forms %s -> %s, fresh %s" % (rank, hier.num_levels, f_before, forms(hier), forms(fresh)), flush=True)
        if kind == "sio2" and rank == 0:
            assert any("spmm_star" in f or "spmm_dense" in f for f in f_before[1:]), ("no coarse slab with a star or dense form was refreshed", f_before)
        hier.close(); fresh.close()
        be.free_matrix(mat); be.free_matrix(mat2)
    else:
        assert world == 2 and kind == "sio2"
        upd = rank == 1                                          # rank 0 forgets the switch
        mat, keepA = create(val0, upd)
        f0 = g.gcge_hip_mat_spmm_form(mat).decode()
        assert "spmm_star" in f0 or "spmm_dense" in f0, (rank, f0)
        mine = be.matrix_update_values(mat, dev(val1))           # the library's own answer: this rank's alone
        assert mine is upd, (rank, mine)
        assert be.matrix_update_values(mat, dev(val1), agree=comm) is False, "rank %d: the ranks did not agree on the decline" % rank
        be.free_matrix(mat)
        # every rank frees and creates again, from the new values; rank 0 forgets the switch again, around MultiGridCreate too: its coarse
        # slab has a block form without maps and declines, rank 1's levels take their (same) values — GCGE_AMGRefresh agrees on level 1
        mat_new, keepB = create(val1, upd)
        hier = be.multigrid(mat_new, None, levels=levels, block_size=8, refreshable=upd)
        L0, fc = hier.num_levels, forms(hier)
        assert L0 >= 2 and (rank != 0 or "spmm_star" in fc[1] or "spmm_dense" in fc[1]), (rank, fc)
        local = g.gcge_hip_multigrid_refresh_check(hier._head().A_array, None, hier._head().P_array, L0)
        assert local == 0, (rank, local)
        ok = hier.refresh()
        assert ok is False, "rank %d: Hierarchy.refresh() returned %r over a hierarchy one rank cannot refresh" % (rank, ok)
        assert hier.num_levels == L0
        print("rank %d: level 0 %s, the library said %r, the ranks agreed on a decline; refresh() rebuilt on both" % (rank, f0, mine), flush=True)
        hier.close(); be.free_matrix(mat_new)
    dist.barrier()
    print("rank %d ok" % rank, flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
