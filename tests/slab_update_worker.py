"""Worker of tests/test_mat_update_slab.py::test_loopback_slab_updated_in_place_is_a_fresh_slab_bit_for_bit — one process, one GPU.

The loop-back slab of tests/rccl_loopback_worker.py (star_loopback): the lower slab of a two-slab matrix whose neighbour is this rank
itself, the halo moved by grouped ncclSend / ncclRecv from C (a world of ONE rank: gcge_hip_mat_set_halo_rccl with both virtual slabs
mapped to rank 0).  The operator is S[:, own] + S[:, halo] P with P the 0/1 matrix of the halo map.

argv[1]:
  sio2      the lower slab (12 planes) of make_problem("sio2", 24): spmm_star+spmm_dense+spmm_pad8
  ball      the lower slab of make_problem("sio2ball", 24), cut between grid lines, geometry named: the sweep's masked form
  lap       the lower slab (5 planes) of the 7-point Laplacian on 8 x 8 x 10: a value table, which a varying diagonal turns into "+values"
  lap_pad8  the same slab with gcge_hip_set_spmm_path(3): the pad-8 copy multiplies

For each: created with the value maps kept (updatable) from val0, updated to val1; with halo overlap 0 and 1 the products at widths 64 and
17 on odd column ranges must be BIT-IDENTICAL to those of a fresh slab handle created from val1, and within 1e-12 of scipy's loop-back
operator (entries of magnitude <= 20 against X in [-0.5, 0.5], rows of at most a few hundred entries: sums below 1e3, whose rounding
stays below 1e-13 x a few hundred).  The form string stays, but for the documented switch of a value table to "+values".  A second
update back to val0 reproduces the first products bit for bit.  For the star slabs also: a handle created WITHOUT the maps declines
(the product unchanged), and a changed star coefficient declines with nothing written (the product unchanged, bit for bit) — a
pattern or pad-8 slab needs no maps and has no pinned entry, so these two do not apply to it."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def main():
    which = sys.argv[1]
    os.environ["GCGE_COMM_KEEP_SINGLE"] = "1"
    import scipy.sparse as sp
    import torch
    torch.cuda.set_device(0)
    from gcge_amd import HipBackend
    from gcge_amd import dist as gdist
    from gcge_amd.lib import CSR, csr_to_scipy, host_lib, mat_update_form_stats, mat_update_stats
    from helpers import bits, uniform
    from slab_cases import G, dp_, ip_, scipy_rows, slab_of, values
    be = HipBackend(device=0)
    g = be.g
    comm = gdist.NativeComm(be, None, 0, 1)
    star = which in ("sio2", "ball")
    if star:
        from test_mat_update_forms import case
        g.gcge_hip_spmm_dense_mode(1)                             # small atoms: rows of >= 24 entries may seed a block
        c = case(which)
        n_loc = gdist.partition_lines(c.box, G, 2)[1] if which == "ball" else (G // 2) * G * G
        s = slab_of(c, 0, n_loc)
        val0, val1 = values(c, s, 0), values(c, s, 2)
        send_rows = np.ascontiguousarray(s.ghosts - n_loc, dtype=np.int32)       # halo row g is served by own row g - n_loc
    else:
        class Whole:
            pass
        h = host_lib()
        nx, ny, nz = 8, 8, 10
        A = CSR(); h.gcge_problem_lap3d_box(nx, ny, nz, C.c_int64(0), C.c_int64(-1), C.byref(A))
        c = Whole()
        c.S = csr_to_scipy(A).tocsr(); c.S.sort_indices()
        n = c.S.shape[0]
        rows = np.repeat(np.arange(n), np.diff(c.S.indptr))
        c.diag = rows == c.S.indices
        c.pinned = np.zeros(c.S.nnz, dtype=bool); c.free = ~c.diag; c.box = None; c.dims = None
        n_loc = (nz // 2) * nx * ny
        s = slab_of(c, 0, n_loc)
        val0 = np.ascontiguousarray(c.S.data[s.sel], dtype=np.float64)
        r_loc = np.repeat(np.arange(n_loc), np.diff(s.rp))
        val1 = val0.copy()
        val1[s.diag] += 0.25 * (1.0 + r_loc[s.diag] % 11)          # a potential on the diagonal: the classes of the table are no longer uniform
        send_rows = np.ascontiguousarray(s.ghosts - nx * ny, dtype=np.int32)     # the plane above is served by the slab's own last plane
        if which == "lap_pad8":
            g.gcge_hip_set_spmm_path(3)
    ng = int(s.ghosts.size)
    assert ng > 0 and send_rows.min() >= 0 and send_rows.max() < n_loc
    P = sp.csr_matrix((np.ones(ng), (np.arange(ng), send_rows)), shape=(ng, n_loc))

    def loopback(v):
        Sg = scipy_rows(s, v).tocsc()
        return (Sg[:, :n_loc] + Sg[:, s.ghosts] @ P).tocsr()

    def create(v, updatable):
        slab = (s.n_loc, s.ncols, s.n_global, 0, s.rp.ctypes.data_as(ip_), s.ci.ctypes.data_as(ip_), v.ctypes.data_as(dp_), s.ghosts.ctypes.data_as(ip_))
        with be._keeping_value_maps(updatable):
            if s.box_local is not None:
                m = g.gcge_hip_mat_create_local_ghosts_grid(*slab, G, G, G, s.box_local.ctypes.data_as(ip_))
            else:
                m = g.gcge_hip_mat_create_local_ghosts(*slab)
        assert m
        m = C.c_void_p(m)
        peer, scnt, rcnt = (C.c_int * 2)(0, 0), (C.c_int * 2)(0, ng), (C.c_int * 2)(0, ng)
        assert g.gcge_hip_mat_set_halo_rccl(m, s.n_global, 2, peer, scnt, rcnt, send_rows.ctypes.data_as(ip_), 64) == 0
        return m

    X = uniform(5, (n_loc, 70)) - 0.5
    RANGES = [(64, 1, 3), (17, 3, 5)]                             # width, first column of X, first column of Y: odd ranges

    def products(m):
        x = be.mv_from_numpy(m, X)
        y = be.ops.mv_create(70, m)
        out = []
        for overlap in (0, 1):
            g.gcge_hip_set_halo_overlap(overlap)
            for w, a, b in RANGES:
                be.ops.spmm(m, x, y, (a, b), (a + w, b + w))
                out.append(be.mv_to_numpy(y, n_loc, b, b + w))
        be.ops.mv_destroy(x, 70); be.ops.mv_destroy(y, 70)
        return out

    def same(p, q):
        return all(np.array_equal(bits(a), bits(b)) for a, b in zip(p, q))

    def near(p, S):
        worst = 0.0
        for k, Y in enumerate(p):
            w, a, _ = RANGES[k % len(RANGES)]
            worst = max(worst, float(np.max(np.abs(Y - S @ X[:, a:a + w]))))
        return worst

    last = {}

    def update(m, v):
        u0, f0_ = mat_update_stats(), mat_update_form_stats()
        ok = be.matrix_update_values(m, torch.from_numpy(v).cuda(), agree=comm)
        last["stats"] = ([a - b for a, b in zip(mat_update_stats(), u0)], [a - b for a, b in zip(mat_update_form_stats(), f0_)])
        return ok

    form = lambda m: g.gcge_hip_mat_spmm_form(m).decode()
    m = create(val0, True)
    f0 = form(m)
    want = {"sio2": "spmm_star+spmm_dense+spmm_pad8", "ball": "spmm_star+spmm_dense+spmm_pad8", "lap_pad8": "spmm_pad8"}.get(which)
    assert (f0 == want) if want else (f0.startswith("spmm_pattern") and not f0.endswith("+values")), f0
    if which == "ball":
        assert g.gcge_hip_mat_star_masked_form(m) == 3
    if star:
        assert g.gcge_hip_mat_value_maps(m) > 0, "a star slab created with the switch on keeps its value maps"
    p0 = products(m)
    e0 = near(p0, loopback(val0))
    assert e0 < 1e-12, e0
    assert update(m, val1) is True, ("the slab declined new values", last)
    f1 = form(m)
    assert f1 == (f0 + "+values" if which == "lap" else f0), (f0, f1)
    p1 = products(m)
    e1 = near(p1, loopback(val1))
    fresh = create(val1, False)
    pf = products(fresh)
    print("%s: form %s -> %s, fresh %s; distance to scipy %.2e before, %.2e after the update" % (which, f0, f1, form(fresh), e0, e1), flush=True)
    assert e1 < 1e-12, e1
    assert same(p1, pf), "the updated slab does not multiply like a fresh slab of the new values, bit for bit"
    assert not same(p1, p0)
    be.free_matrix(fresh)
    assert update(m, val0) is True
    assert same(products(m), p0), "the update back to the first values does not reproduce the first products"
    if star:
        plain = create(val0, False)
        assert g.gcge_hip_mat_value_maps(plain) == 0
        pp = products(plain)
        assert same(pp, p0)
        assert update(plain, val1) is False, "a star slab without value maps must decline"
        assert same(products(plain), pp), "a declined update wrote to the handle"
        be.free_matrix(plain)
        bad = val1.copy()
        pinned = np.flatnonzero(s.pinned)
        q = pinned[pinned.size // 2]
        bad[q] = np.nextafter(bad[q], 0.0)                        # another star coefficient in one entry
        assert update(m, bad) is False, "a changed star coefficient must decline"
        assert same(products(m), p0), "a declined update wrote to the handle"
    be.free_matrix(m)
    g.gcge_hip_set_spmm_path(0)
    comm.finalize()
    print("slab update ok: %s, %d rows, %d halo rows, form %s -> %s" % (which, n_loc, ng, f0, f1))


if __name__ == "__main__":
    main()
