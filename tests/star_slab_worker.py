"""Worker of tests/test_star_rows.py::test_loopback_slabs_exact — one process, one GPU, every slab case of tests/star_cases.py (or
those named on the command line).

The loop-back recipe of tests/slab_update_worker.py: a world of ONE rank (gcge_hip_mat_set_halo_rccl with both virtual slabs mapped
to rank 0) in which halo row g of a slab of rows [a, b) is served by own row (g - a) mod (b - a); the operator this defines is
S[:, own] + S[:, halo] P with P the 0/1 matrix of that map, formed by scipy on the same integer arrays (star_cases.loopback), and
every comparison is np.array_equal: Y, x.y and y.y.

Slabs of planes of the 16 x 16 x 40 grid, arm length 6: [0, 14) lower; [14, 26) middle with an empty interior; [13, 26) middle with
one interior plane; [2, 30) with a lower halo of 2 planes (zmin clipped to 0); [26, 40) upper; [14, 26) with arm length 3 (zmin = zs -
3 while the sweep reaches 6 planes and clamps).  A middle slab has both halo offsets and the plane shift nonzero, so X, Y, the
diagonal and the clean flags are all shifted.  And a lower and a middle slab of the sheared ellipsoid in 20 x 20 x 50, cut between
grid lines (the masked third form on a slab).

Each slab under both forms of the sweep (plane slabs; a masked slab has the third only), with halo overlap 0 and 1, at widths 64, 18
and 2 with column offsets, plain and with column sums, three times with fresh operands (a missing stream dependency shows as stale halo
planes).  Overlap 1 must raise the split counter of gcge_hip_star_product_stats exactly where gcge_hip_star_interior, restated in
star_cases.interior, says the slab has an interior; overlap 0 never; both must give the same bits.  The product counter is asserted
both ways: it rises by one for every operand the sweep takes, and stays put — as does the split counter — for the operands it
declines (an odd width, an odd first column of X or of Y, a width below 8 on an odd range), whose exact results come by the other
routes; x and y in one block on disjoint even ranges are taken and counted."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def main():
    os.environ["GCGE_COMM_KEEP_SINGLE"] = "1"
    import torch
    torch.cuda.set_device(0)
    import star_cases as sc
    from gcge_amd import HipBackend
    from gcge_amd import dist as gdist
    from helpers import IN_GUARD, OUT_BITS, OUT_GUARD, bits, draw
    from star_cases import STAR_R, ip_, dp_
    be = HipBackend(device=0)
    g = be.g
    comm = gdist.NativeComm(be, None, 0, 1)
    g.gcge_hip_spmm_dense_mode(1)
    RANGES = [(64, 0, 0), (18, 2, 4), (2, 2, 0)]                        # width, first column of X, first column of Y
    t_all = time.time()

    def stats():
        p, s = C.c_long(), C.c_long()
        g.gcge_hip_star_product_stats(C.byref(p), C.byref(s))
        return p.value, s.value

    names = sys.argv[1:] or list(sc.SLABS) + sc.MASKED_SLABS           # (some of the cases only: by name)
    for name in names:
        t0 = time.time()
        st, s, planes = sc.slab_case(name)
        n_loc, ng = s.n_loc, int(s.ghosts.size)
        S = sc.loopback(s)
        # (sums_form of mat_product.hip sends the sums of 16 .. 128 columns through the sweep where the rows average >= 2.5 octets: every slab here)
        assert np.sum(-(-np.diff(s.rp) // 8)) / n_loc >= 2.5, name
        slab = (s.n_loc, s.ncols, s.n_global, s.a, s.rp.ctypes.data_as(ip_), s.ci.ctypes.data_as(ip_), s.val.ctypes.data_as(dp_), s.ghosts.ctypes.data_as(ip_))
        if s.box_local is not None:
            mat = g.gcge_hip_mat_create_local_ghosts_grid(*slab, *st.dims, s.box_local.ctypes.data_as(ip_))
        else:
            mat = g.gcge_hip_mat_create_local_ghosts(*slab)
        assert mat, name
        mat = C.c_void_p(mat)
        peer, scnt, rcnt = (C.c_int * 2)(0, 0), (C.c_int * 2)(0, ng), (C.c_int * 2)(0, ng)
        assert g.gcge_hip_mat_set_halo_rccl(mat, s.n_global, 2, peer, scnt, rcnt, s.send_rows.ctypes.data_as(ip_), 64) == 0
        form = g.gcge_hip_mat_spmm_form(mat).decode()
        assert form.startswith("spmm_star"), (name, form)
        stt = (C.c_long * 8)()
        assert g.gcge_hip_mat_star_stats(mat, stt) == 1 and stt[4] == s.nclean and stt[5] == n_loc, (name, list(stt), s.nclean)
        nz = st.dims[2]
        if planes is not None:
            R = sc.SLABS[name][0]
            assert tuple(stt[:4]) == st.dims + (R,) and (stt[6], stt[7]) == planes and g.gcge_hip_mat_star_masked_form(mat) == 0, (name, list(stt))
            has_interior = sc.interior(planes[0], planes[1], nz, R)[0]
            forms = (3, 2)
        else:
            assert g.gcge_hip_mat_star_masked_form(mat) == 3, name
            plane = st.dims[0] * st.dims[1]
            zs, ze = int(st.box[s.a]) // plane, int(st.box[s.b - 1]) // plane + 1
            gz = st.box[s.ghosts] // plane
            assert (stt[6], stt[7]) == (zs, ze), (name, list(stt))
            has_interior = sc.interior(zs, ze, nz, STAR_R, True, int(np.any(gz == zs)), int(np.any(gz == ze - 1)))[0]
            forms = (3,)

        def block(data, c0, width, guard):
            host = np.full((n_loc, width), guard)
            host[:, c0:c0 + data.shape[1]] = data
            return be.mv_from_numpy(mat, host), host, width

        seen = {}
        for form_ in forms:
            g.gcge_hip_spmm_star_form(form_)
            for overlap in (0, 1):
                g.gcge_hip_set_halo_overlap(overlap)
                out, nprod = [], 0
                p0, s0 = stats()
                for rep in range(3):
                    X = draw(st.seed + 50 + rep, (n_loc, 64), False)
                    for m, a, b in RANGES:
                        Yr = np.ascontiguousarray(S @ X[:, :m])
                        for sums in (False, True):
                            bx = block(X[:, :m], a, a + m + 2, IN_GUARD)
                            by = block(np.full((n_loc, m), OUT_GUARD), b, b + m + 2, OUT_GUARD)
                            what = (name, "form", form_, "overlap", overlap, "rep", rep, "m", m, "sums", sums)
                            if sums:
                                dots, yy = np.full(m + 4, OUT_GUARD), np.full(m + 4, OUT_GUARD)
                                g.gcge_hip_spmm_dot2_mv(mat, bx[0], by[0], (C.c_int * 2)(a, b), (C.c_int * 2)(a + m, b + m), dots.ctypes.data + 16,
                                                        yy.ctypes.data + 16, be.ops_handle)
                                for nm, v, ref in (("x.y", dots, (X[:, :m] * Yr).sum(axis=0)), ("y.y", yy, (Yr * Yr).sum(axis=0))):
                                    assert np.array_equal(v[2:2 + m], ref), (what, nm, (v[2:2 + m] - ref)[:6].tolist())
                                    assert np.all(bits(v[:2]) == OUT_BITS) and np.all(bits(v[2 + m:]) == OUT_BITS), (what, nm, "guard")
                                out += [bits(dots).copy(), bits(yy).copy()]
                            else:
                                be.ops.spmm(mat, bx[0], by[0], (a, b), (a + m, b + m))
                            nprod += 1
                            gy, gx = be.mv_to_numpy(by[0], n_loc, 0, by[2]), be.mv_to_numpy(bx[0], n_loc, 0, bx[2])
                            assert np.array_equal(gy[:, b:b + m], Yr), (what, "Y", np.argwhere(gy[:, b:b + m] != Yr)[:4].tolist())
                            out.append(bits(np.ascontiguousarray(gy)).copy())
                            gy[:, b:b + m] = OUT_GUARD
                            assert np.array_equal(bits(np.ascontiguousarray(gy)), bits(by[1])), (what, "the columns of Y beside the operand")
                            assert np.array_equal(bits(np.ascontiguousarray(gx)), bits(bx[1])), (what, "X was written")
                            be.ops.mv_destroy(bx[0], bx[2]); be.ops.mv_destroy(by[0], by[2])
                p1, s1 = stats()
                assert p1 - p0 == nprod, (name, form_, overlap, "calls that take the sweep", p1 - p0, nprod)
                assert s1 - s0 == (nprod if overlap and has_interior else 0), (name, form_, overlap, "split products", s1 - s0, nprod, has_interior)
                # the declines: operands gcge_hip_star_spmm_part is documented to refuse (an odd width, an odd first column of X or of Y, a
                # width below 8 on an odd range) reach the result through the other routes — the same exact Y, the guards intact, and
                # NEITHER counter moves
                X = draw(st.seed + 60, (n_loc, 18), False)
                for m, a, b, sums in [(17, 0, 0, False), (16, 1, 2, False), (16, 2, 1, False), (6, 1, 0, False), (3, 0, 0, False), (17, 0, 0, True), (16, 1, 2, True)]:
                    what = (name, "form", form_, "overlap", overlap, "decline", m, a, b, "sums", sums)
                    Yr = np.ascontiguousarray(S @ X[:, :m])
                    bx = block(X[:, :m], a, a + m + 2, IN_GUARD)
                    by = block(np.full((n_loc, m), OUT_GUARD), b, b + m + 2, OUT_GUARD)
                    if sums:
                        dots, yy = np.full(m + 4, OUT_GUARD), np.full(m + 4, OUT_GUARD)
                        g.gcge_hip_spmm_dot2_mv(mat, bx[0], by[0], (C.c_int * 2)(a, b), (C.c_int * 2)(a + m, b + m), dots.ctypes.data + 16, yy.ctypes.data + 16, be.ops_handle)
                        for nm, v, ref in (("x.y", dots, (X[:, :m] * Yr).sum(axis=0)), ("y.y", yy, (Yr * Yr).sum(axis=0))):
                            assert np.array_equal(v[2:2 + m], ref), (what, nm, (v[2:2 + m] - ref)[:6].tolist())
                            assert np.all(bits(v[:2]) == OUT_BITS) and np.all(bits(v[2 + m:]) == OUT_BITS), (what, nm, "guard")
                    else:
                        be.ops.spmm(mat, bx[0], by[0], (a, b), (a + m, b + m))
                    gy, gx = be.mv_to_numpy(by[0], n_loc, 0, by[2]), be.mv_to_numpy(bx[0], n_loc, 0, bx[2])
                    assert np.array_equal(gy[:, b:b + m], Yr), (what, "Y", np.argwhere(gy[:, b:b + m] != Yr)[:4].tolist())
                    gy[:, b:b + m] = OUT_GUARD
                    assert np.array_equal(bits(np.ascontiguousarray(gy)), bits(by[1])), (what, "the columns of Y beside the operand")
                    assert np.array_equal(bits(np.ascontiguousarray(gx)), bits(bx[1])), (what, "X was written")
                    be.ops.mv_destroy(bx[0], bx[2]); be.ops.mv_destroy(by[0], by[2])
                    assert stats() == (p1, s1), (what, "a declined operand was counted as a product of the sweep", stats(), (p1, s1))
                # x and y in ONE block on disjoint even ranges: the entry refuses only d_x == d_y, so the sweep takes it — and is counted
                m, a = 16, 2
                b = a + m + 2
                Yr = np.ascontiguousarray(S @ X[:, :m])
                bx = block(X[:, :m], a, b + m + 2, IN_GUARD)
                be.ops.spmm(mat, bx[0], bx[0], (a, b), (a + m, b + m))
                gx = be.mv_to_numpy(bx[0], n_loc, 0, bx[2])
                assert np.array_equal(gx[:, b:b + m], Yr), (name, form_, overlap, "Y in X's block")
                gx[:, b:b + m] = IN_GUARD
                assert np.array_equal(gx, bx[1]), (name, form_, overlap, "X's block beside the result")
                be.ops.mv_destroy(bx[0], bx[2])
                assert stats() == (p1 + 1, s1 + (1 if overlap and has_interior else 0)), (name, form_, overlap, "one block", stats(), (p1, s1))
                seen[(form_, overlap)] = out
        first = seen[(forms[0], 0)]
        for key, out in seen.items():
            assert all(np.array_equal(u, v) for u, v in zip(first, out)), (name, key, "other bits than form %d without overlap" % forms[0])
        be.free_matrix(mat)
        print("%s: %d rows, %d halo rows, %s, interior %s, %.1f s" % (name, n_loc, ng, form, has_interior, time.time() - t0), flush=True)
    g.gcge_hip_spmm_star_form(3)
    g.gcge_hip_set_halo_overlap(1)
    g.gcge_hip_spmm_dense_mode(0)
    comm.finalize()
    print("star slabs ok: %d cases, %.1f s" % (len(names), time.time() - t_all))


if __name__ == "__main__":
    main()
