"""The plane sweep — spmm_star.hip: spmm_star2_kernel (second form), spmm_star3_kernel (third form, LDS-DMA strips) and
spmm_star3m_kernel (third form on masked grids), their launcher star_launch and the interior / boundary split of
gcge_hip_star_spmm_part — through the entries every caller uses (ops.spmm, gcge_hip_spmm_dot2_mv) on EXACT data: coefficients,
diagonals, planted entries and X are nonzero integers of magnitude <= 3 (stored zeros apart), so every product, every sum of six
neighbours and every column sum is an integer far below 2^53, the reference is scipy on the same arrays and every comparison is
np.array_equal — for Y and for both column sums (x.y and y.y).  tests/star_cases.py holds the matrices, the case table (each case
named for the branch it reaches) and the launch arithmetic restated (launch, pranges, masked_spans, interior, block_of).

Guards: the columns of X outside the operand hold 2^40, the columns of Y outside it the payload NaN of helpers.OUT_BITS, which must
come back bit for bit; X is compared bitwise after every call.

Slabs run in tests/star_slab_worker.py (one fresh process, a world of one rank whose halo rows are served by its own rows).

Rounding bound on real data (uniform - 0.5, all rows clean, test_real_data_stays_inside_the_derived_bound): the kernels form, per
arm position k, zsum, xsum and ysum (one addition each); with one coefficient set s6 = (zsum + xsum) + ysum (two more) and one fma
into the accumulator, which starts as the once-rounded product of the diagonal and the own value.  A neighbour's value thus passes
at most 3 additions and the fmas of k .. R: at most R + 3 roundings (the fmas beyond the arm length multiply by 0.0 and round
nothing); the diagonal term 1 + R.  With a set per axis a term passes its pair's addition and at most 3 R fmas: 1 + 3 R.  So
|result - ref| <= (count + 1) 2^-53 times the same expression over absolute values, count = R + 3 (one set) or 3 R + 1 (per axis);
the last unit covers the terms of second order and the longdouble reference's own rounding, as in test_pattern_rows.py.
"""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import star_cases as sc
from gcge_amd import abi
from gcge_amd.lib import hip_lib
from helpers import IN_GUARD, OUT_BITS, OUT_GUARD, bits
from star_cases import STAR_R, cdiv, ip_, dp_

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = np.longdouble(2.0) ** -53
WHOLE_NAMES = list(sc.WHOLE)
XCD_SMALL = "ragged_both_ways_31_planes"


# ---- 1. the premise and the builder, on the host -----------------------------------------------------------------------------------
def all_exact_cases():
    return [sc.whole(n) for n in WHOLE_NAMES + [sc.XCD_BIG[0]]] + [sc.masked(n) for n in sc.MASKED] + [sc.slab_grid(6), sc.slab_grid(3)]


def test_exactness_premise_and_builder():
    """every stored value an integer of magnitude <= 3, the diagonal and X nonzero (the rows without a stored diagonal and with a
    stored 0.0 apart); symmetric; planted rows below half of the rows; |A X| <= 9 x the longest row, the column sums below 2^53; the
    clean rows' product rebuilt from the neighbour table equals scipy's on the CSR arrays"""
    for st in all_exact_cases():
        S, n = st.S, st.n
        v = S.data
        assert np.all(v == np.round(v)) and np.all(np.abs(v) <= 3), st.name
        assert np.all(st.c == np.round(st.c)) and np.all(st.c != 0) and np.all(np.abs(st.c) <= 3)
        d = S.diagonal()
        nz = np.ones(n, dtype=bool)
        nz[st.nodiag] = nz[st.zerodiag] = False
        assert np.all(d[nz] != 0) and np.all(d[~nz] == 0)
        rows = np.repeat(np.arange(n), np.diff(S.indptr))
        stored_diag = np.zeros(n, dtype=bool)
        stored_diag[rows[rows == S.indices]] = True
        assert not stored_diag[st.nodiag].any() and stored_diag[st.zerodiag].all() and stored_diag.sum() == n - st.nodiag.size
        assert abs(S - S.T).nnz == 0 or abs(S - S.T).max() == 0, st.name
        assert 0 <= 2 * st.touched.size < n and st.nclean == n - st.touched.size
        X = st.X(8)
        assert np.all(X == np.round(X)) and np.all(X != 0) and np.all(np.abs(X) <= 3)
        longest = int(np.diff(S.indptr).max())
        assert longest <= 6 * STAR_R + 1 + 64
        Y = st.product(X)
        assert np.max(np.abs(Y)) <= 9 * longest and n * (9 * longest) ** 2 < 2 ** 53
        # the clean rows from the neighbour table, in int64
        Xi = X.astype(np.int64)
        W = st.diag.astype(np.int64)[:, None] * Xi
        for (a, k, sgn), j in st.nb.items():
            W += np.where((j >= 0)[:, None], int(st.c[a, k - 1]) * Xi[np.maximum(j, 0)], 0)
        clean = np.ones(n, dtype=bool)
        clean[st.touched] = False
        assert np.array_equal(W[clean], Y[clean]) and (st.touched.size == 0 or not np.array_equal(W[~clean], Y[~clean])), st.name
    # detection constraints of star_split.hip that the table respects
    for st in all_exact_cases():
        nx, ny, nz = st.dims
        assert st.n >= 2048 and nx > 2 * STAR_R and ny > 2 * STAR_R and nz >= 2 and (not st.masked or st.iso_on_device()), st.name
        assert max(st.arms) > 2 or st.block, (st.name, "rows of <= 16 entries alone would take the pattern form")
    assert not sc.whole("two_planes_arms_661").iso_on_device() and sc.whole("two_planes_arms_661").detected_arms() == (6, 6, 1)
    assert sc.whole("eight_planes").detected_arms() == (6, 6, 6) and sc.whole("two_planes_arm_1").detected_arms() == (1, 1, 1)


def selfcheck(st):
    g = hip_lib()
    out = (C.c_long * 12)()
    A, _ = st.csr()
    if st.masked:
        bad = g.gcge_hip_star_selfcheck_grid(A.nrows, A.rowptr, A.colidx, A.val, *st.dims, st.box.ctypes.data_as(ip_), out)
    else:
        bad = g.gcge_hip_star_selfcheck(A.nrows, A.ncols, A.rowptr, A.colidx, A.val, out)
    return bad, list(out[:5])


def test_every_case_is_accepted_by_its_selfcheck():
    """gcge_hip_star_selfcheck / _grid / _slab (host only): dims, arm length and the EXACT clean count of every whole, masked and slab
    case; the masked slabs through gcge_hip_value_maps_selfcheck_slab with the same values twice (the self-check that takes the box
    index of the local columns); 13 x 13 x 8 is refused (1352 rows)"""
    g = hip_lib()
    for st in all_exact_cases() + [sc.real_case(n) for n in sc.REAL]:
        bad, out = selfcheck(st)
        assert bad == 0 and out == list(st.dims) + [max(st.detected_arms()), st.nclean], (st.name, bad, out)
    assert sc.whole("one_ragged_patch_all_clean").nclean == 2197 and sc.whole("nine_planes").touched.size == 0
    small = sc.Star("refused", (13, 13, 8), (6, 6, 6), "iso", 3)
    assert selfcheck(small)[0] == -1
    plain = sc.Star("arm_2_no_planted_row", (13, 13, 48), (2, 2, 2), "iso", 4)
    assert selfcheck(plain) == (0, [13, 13, 48, 2, plain.n])
    out = (C.c_long * 12)()
    for name in sc.SLABS:
        st, s, (zs, ze) = sc.slab_case(name)
        R = sc.SLABS[name][0]
        bad = g.gcge_hip_star_selfcheck_slab(s.n_loc, s.ncols, s.a, s.n_global, s.ghosts.ctypes.data_as(ip_), s.rp.ctypes.data_as(ip_),
                                             s.ci.ctypes.data_as(ip_), s.val.ctypes.data_as(dp_), out)
        nz = st.dims[2]
        assert bad == 0 and list(out[:9]) == list(st.dims) + [R, s.nclean, zs, ze, max(0, zs - R), min(nz, ze + R)], (name, bad, list(out))
        assert (out[9] == -1) == (zs == 0) and (out[10] == -1) == (ze == nz) and np.unique(s.send_rows).size == s.send_rows.size
    o4 = (C.c_long * 4)()
    for name in sc.MASKED_SLABS:
        st, s, _ = sc.slab_case(name)
        bad = g.gcge_hip_value_maps_selfcheck_slab(s.n_loc, s.ncols, s.a, s.n_global, s.ghosts.ctypes.data_as(ip_), s.rp.ctypes.data_as(ip_),
                                                   s.ci.ctypes.data_as(ip_), s.val.ctypes.data_as(dp_), s.val.ctypes.data_as(dp_), 1, *st.dims,
                                                   s.box_local.ctypes.data_as(ip_), o4)
        assert bad == 0 and (o4[0] & 1) and s.n_loc >= 2048, (name, bad, list(o4))


def forms_of(st):
    """the forms of the sweep a whole case runs under: (form switch, third form taken)"""
    return [(3, True), (2, False)] if st.iso_on_device() else [(2, False)]


def test_the_case_table_reaches_the_branches():
    """star_launch, gcge_hip_star_interior and the plane ranges of the masked kernels restated: what the tables reach"""
    spans = {True: set(), False: set()}
    chunks = {True: {}, False: {}}
    for name in WHOLE_NAMES:
        st = sc.whole(name)
        for m, _, _ in sc.WHOLE[name][4] + sc.DOT_M:
            for _, third in forms_of(st):
                L = sc.launch(st.dims[0], st.dims[1], m, 0, st.dims[2], third)
                spans[third] |= {b - a for a, b in L["ranges"]}
                chunks[third].setdefault(L["zchunks"], set()).add(tuple(b - a for a, b in L["ranges"]))
    # every z1 - z0 class: Q - 1, Q, Q + 1, 2 Q + 1 of the unrolled bodies (14 steps in the second form, 15 in the third), short
    # ranges, and the planes per range of 2, 8, 9, 13 .. 16, 29 .. 31
    assert spans[False] >= {2, 8, 9, 13, 14, 15, 16, 29, 30, 31, 23, 24, 25} and spans[True] >= {2, 8, 9, 13, 14, 15, 16, 29, 30, 31, 23, 24, 25}
    for third in (True, False):
        assert set(chunks[third]) == {1, 2, 3}
        assert (24, 24) in chunks[third][2] and (25, 24) in chunks[third][2] and (25, 25, 23) in chunks[third][3]
    # several ranges x several patches x several passes
    L = sc.launch(33, 17, 34, 0, 49, True)
    assert (L["ntx"], L["nty"], L["npass"], L["zchunks"], L["zlen"]) == (3, 3, 3, 2, 25) and L["total"] == 54
    L = sc.launch(33, 17, 34, 0, 49, False)
    assert (L["ntx"], L["nty"], L["npass"], L["zchunks"]) == (3, 2, 5, 2)
    # patch edges: one ragged patch, exact patches, one point into the second patch column, ragged both ways
    assert sc.launch(13, 13, 2, 0, 13, True)["npatch"] == 2 and sc.launch(13, 13, 2, 0, 13, False)["npatch"] == 1
    assert sc.launch(16, 16, 2, 0, 16, False)["npatch"] == 1 and sc.launch(17, 24, 2, 0, 14, False)["npatch"] == 4
    assert sc.launch(33, 17, 2, 0, 31, True)["npatch"] == 9 and 33 % 16 == 1 and 17 % 8 == 1 and 17 % 16 == 1
    # planted rows in the last plane of a range and the first plane of the next
    st = sc.whole("two_ranges_of_24")
    assert {23, 24} <= set(st.co[2][st.touched].tolist()) and sc.launch(13, 13, 2, 0, 48, True)["ranges"] == [(0, 24), (24, 48)]
    # listed rows in a single patch (16 x 8: the first)
    st = sc.whole("single_patch_of_listed_rows")
    assert st.touched.size and np.all(st.co[0][st.touched] < 16) and np.all(st.co[1][st.touched] < 8)
    # arm lengths 1 .. 6 with one coefficient set, per-axis sets, one set on axes of different lengths
    assert {max(sc.whole(n).arms) for n in WHOLE_NAMES if sc.whole(n).iso_on_device()} == {1, 2, 3, 4, 5, 6}
    assert [sc.whole(n).arms for n in WHOLE_NAMES if not sc.whole(n).iso_on_device()] == [(3, 3, 3), (6, 6, 1), (4, 5, 6)]
    # the XCD order: 27 workgroups (the default permutes none), 270 (176 permuted, 94 behind)
    st, big = sc.whole(XCD_SMALL), sc.whole(sc.XCD_BIG[0])
    assert sc.launch(st.dims[0], st.dims[1], 34, 0, st.dims[2], True)["total"] == 27
    L = sc.launch(big.dims[0], big.dims[1], sc.XCD_BIG[5], 0, big.dims[2], True)
    assert (L["npatch"], L["zchunks"], L["npass"], L["total"]) == (15, 2, 9, 270)
    moved = [b for b in range(270) if sc.block_of(22, b, 270) != b]
    assert moved and max(moved) < 176 and all(sc.block_of(22, b, 27) == b for b in range(27))
    assert any(sc.block_of(1, b, 27) != b for b in range(27)) and any(sc.block_of(2, b, 27) != b for b in range(16)) and all(sc.block_of(2, b, 27) == b for b in range(16, 27))
    # masked grids: two ranges, short plane ranges in the corner patches, (patch, range) pairs without a plane: the zero-fill branch
    for third in (True, False):
        L, sp = sc.masked_spans(sc.masked("sheared_ellipsoid_20x20x50"), 34, third)
        assert L["zchunks"] == 2 and any(a >= b for a, b in sp) and any(0 < b - a < L["zlen"] for a, b in sp), (third, sp)
        L, sp = sc.masked_spans(sc.masked("ellipsoid_20x27x33"), 34, third)
        assert L["zchunks"] == 1 and all(a < b for a, b in sp) and len({b - a for a, b in sp}) > 1
    # slabs: empty and nonempty interiors, zmin clipped, a detected arm below STAR_R
    want = {"lower": (True, 0, 8), "middle_empty_interior": (False, 20, 20), "middle_one_interior_plane": (True, 19, 20),
            "lower_halo_of_2_planes": (True, 8, 24), "upper": (True, 32, 40), "middle_arm_3": (False, 20, 20)}
    for name, (R, zs, ze) in sc.SLABS.items():
        assert sc.interior(zs, ze, sc.SLAB_GRID[2], R) == want[name], name
    # a lower halo of fewer than R planes, beginning at plane 0 (zmin clipped); a detected arm below STAR_R on a middle slab
    R, zs, ze = sc.SLABS["lower_halo_of_2_planes"]
    s = sc.slab_case("lower_halo_of_2_planes")[1]
    assert 0 < zs < R and s.ghosts[0] == 0 and np.count_nonzero(s.ghosts < s.a) == zs * sc.SLAB_GRID[0] * sc.SLAB_GRID[1]
    R, zs, ze = sc.SLABS["middle_arm_3"]
    assert R < STAR_R and zs > R and ze + R < sc.SLAB_GRID[2]


def test_the_xcd_orders_are_permutations():
    """star_block_of restated: every setting maps the launch ids of a grid onto themselves one to one, for every total from 1 to 400"""
    for total in range(1, 401):
        for xcd in (0, 1, 2, 4, 11, 22):
            assert sorted(sc.block_of(xcd, b, total) for b in range(total)) == list(range(total)), (total, xcd)
    for total in (27, 270):
        assert [sc.block_of(0, b, total) for b in range(total)] == list(range(total))


# ---- 2. the device ------------------------------------------------------------------------------------------------------------------
class Dev:
    """guarded blocks and calls on one matrix handle"""

    def __init__(self, hip, st, mat, n=None):
        self.hip, self.g, self.st, self.mat, self.n = hip, hip.g, st, mat, st.n if n is None else n

    def block(self, data, s, width, guard):
        host = np.full((self.n, width), guard)
        host[:, s:s + data.shape[1]] = data
        mv = self.hip.mv_from_numpy(self.mat, host)
        return mv, host, width

    def got(self, blk):
        return self.hip.mv_to_numpy(blk[0], self.n, 0, blk[2])

    def free(self, *blks):
        for b in blks:
            self.hip.ops.mv_destroy(b[0], b[2])

    def stats(self):
        p, s = C.c_long(), C.c_long()
        self.g.gcge_hip_star_product_stats(C.byref(p), C.byref(s))
        return p.value, s.value

    def check(self, bx, by, s1, ref, what):
        gy, gx = self.got(by), self.got(bx)
        m = ref.shape[1]
        assert np.array_equal(gy[:, s1:s1 + m], ref), (what, "Y", np.argwhere(gy[:, s1:s1 + m] != ref)[:4].tolist())
        gy[:, s1:s1 + m] = by[1][:, s1:s1 + m]
        assert np.array_equal(bits(np.ascontiguousarray(gy)), bits(by[1])), (what, "the columns of Y beside the operand")
        assert np.array_equal(bits(np.ascontiguousarray(gx)), bits(bx[1])), (what, "X was written")
        return gy

    def spmm(self, X, Yref, m, s0, s1, what, same_block=False):
        """Y[:, s1 : s1 + m) = A X[:, s0 : s0 + m) through ops.spmm; returns the bits of the result"""
        if same_block:      # x and y in ONE block: X at s0, the result behind it
            s1 = s0 + m + 2
            bx = self.block(X[:, :m], s0, s1 + m + 2, IN_GUARD)
            self.hip.ops.spmm(self.mat, bx[0], bx[0], (s0, s1), (s0 + m, s1 + m))
            got = self.got(bx)
            assert np.array_equal(got[:, s1:s1 + m], Yref[:, :m]), (what, "Y in X's block")
            got[:, s1:s1 + m] = IN_GUARD
            assert np.array_equal(got, bx[1]), (what, "X's block beside the result")
            self.free(bx)
            return None
        bx = self.block(X[:, :m], s0, s0 + m + 2, IN_GUARD)
        by = self.block(np.full((self.n, m), OUT_GUARD), s1, s1 + m + 2, OUT_GUARD)
        self.hip.ops.spmm(self.mat, bx[0], by[0], (s0, s1), (s0 + m, s1 + m))
        self.check(bx, by, s1, Yref[:, :m], what)
        out = bits(np.ascontiguousarray(self.got(by))).copy()
        self.free(bx, by)
        return out

    def dot2(self, X, Yref, m, s0, s1, what):
        """the product with its column sums through gcge_hip_spmm_dot2_mv: Y, x.y and y.y exact; returns their bits"""
        bx = self.block(X[:, :m], s0, s0 + m + 2, IN_GUARD)
        by = self.block(np.full((self.n, m), OUT_GUARD), s1, s1 + m + 2, OUT_GUARD)
        dots, yy = np.full(m + 4, OUT_GUARD), np.full(m + 4, OUT_GUARD)
        self.g.gcge_hip_spmm_dot2_mv(self.mat, bx[0], by[0], (C.c_int * 2)(s0, s1), (C.c_int * 2)(s0 + m, s1 + m), dots.ctypes.data + 16,
                                     yy.ctypes.data + 16, self.hip.ops_handle)
        self.check(bx, by, s1, Yref[:, :m], what)
        Xm, Ym = X[:, :m], Yref[:, :m]
        for name, v, ref in (("x.y", dots, (Xm * Ym).sum(axis=0)), ("y.y", yy, (Ym * Ym).sum(axis=0))):
            assert np.array_equal(v[2:2 + m], ref), (what, name, np.argwhere(v[2:2 + m] != ref)[:4].tolist(), (v[2:2 + m] - ref)[:4].tolist())
            assert np.all(bits(v[:2]) == OUT_BITS) and np.all(bits(v[2 + m:]) == OUT_BITS), (what, name, "guard")
        out = np.concatenate([bits(np.ascontiguousarray(self.got(by))).ravel(), bits(dots), bits(yy)])
        self.free(bx, by)
        return out


def long_rows(S):
    """sums_form of mat_product.hip: on 16 .. 128 columns the sweep sums only where the rows average >= 2.5 octets"""
    return np.sum(cdiv(np.diff(S.indptr), 8)) / S.shape[0] >= 2.5


def restore(g):
    g.gcge_hip_spmm_star_form(3)
    g.gcge_hip_spmm_star_masked_third(1)
    g.gcge_hip_spmm_star_infer(1)
    g.gcge_hip_spmm_star_xcd(22)
    g.gcge_hip_spmm_dense_mode(0)


def upload_whole(hip, st):
    A, _ = st.csr()
    mat = hip.matrix(A)
    form = hip.g.gcge_hip_mat_spmm_form(mat).decode()
    stt = (C.c_long * 8)()
    assert form.startswith("spmm_star"), (st.name, form)
    assert hip.g.gcge_hip_mat_star_stats(mat, stt) == 1, st.name
    assert list(stt[:6]) == list(st.dims) + [max(st.detected_arms()), st.nclean, st.n], (st.name, list(stt))
    assert hip.g.gcge_hip_mat_star_masked_form(mat) == 0
    return mat


@pytest.mark.gpu
def test_the_nan_payload_survives_the_block_moves(hip):
    """the guards of this file rest on it: a block uploaded and downloaded keeps the payload NaN and 2^40 bit for bit"""
    st = sc.whole("one_ragged_patch_all_clean")
    mat = upload_whole(hip, st)
    try:
        d = Dev(hip, st, mat)
        for guard in (OUT_GUARD, IN_GUARD):
            b = d.block(st.X(4), 2, 8, guard)
            assert np.array_equal(bits(np.ascontiguousarray(d.got(b))), bits(b[1]))
            d.free(b)
    finally:
        hip.free_matrix(mat)


@pytest.mark.gpu
@pytest.mark.parametrize("name", WHOLE_NAMES)
def test_whole_grids_exact(hip, name):
    """every case of star_cases.WHOLE under every form it can take (one coefficient set: the third form and, under
    gcge_hip_spmm_star_form(2), the second; otherwise the second): plain products over the case's widths and column offsets, the
    product with column sums at widths 2, 30 and 64, the declines (an odd width, an odd first column of X or of Y, a width below 8 on
    an odd range, x and y in one block) with the same exact results and the guards intact.  The forms must agree bit for bit."""
    st = sc.whole(name)
    g = hip.g
    widths = sc.WHOLE[name][4]
    X = st.X(132)
    refs = {}

    def ref(m):
        if m not in refs:
            refs[m] = st.product(np.ascontiguousarray(X[:, :m]))
        return refs[m]
    seen = {}
    g.gcge_hip_spmm_dense_mode(1)
    mat = None
    try:
        mat = upload_whole(hip, st)
        d = Dev(hip, st, mat)
        for form, third in forms_of(st):
            g.gcge_hip_spmm_star_form(form)
            out = []
            for m, s0, s1 in widths:
                p0 = d.stats()[0]
                out.append(d.spmm(X, ref(m), m, s0, s1, (name, form, "spmm", m, s0, s1)))
                assert d.stats()[0] - p0 == 1, (name, form, m, "an even range must take the sweep")
            for m, s0, s1 in sc.DOT_M:
                p0 = d.stats()[0]
                out.append(d.dot2(X, ref(m), m, s0, s1, (name, form, "dot2", m, s0, s1)))
                swept = long_rows(st.S) or not 16 <= m <= 128
                assert d.stats()[0] - p0 == (1 if swept else 0), (name, form, m, "sums through the sweep", swept)
            for m, s0, s1 in [(17, 0, 0), (16, 1, 2), (16, 2, 1), (6, 1, 0), (3, 0, 0)]:
                p0 = d.stats()[0]
                d.spmm(X, ref(m), m, s0, s1, (name, form, "decline", m, s0, s1))
                assert d.stats()[0] == p0, (name, form, m, s0, s1, "an odd range is not counted as a product of the sweep")
            d.dot2(X, ref(17), 17, 0, 0, (name, form, "dot2 odd width"))
            d.dot2(X, ref(16), 16, 1, 2, (name, form, "dot2 odd column"))
            p0 = d.stats()[0]
            d.spmm(X, ref(16), 16, 2, 0, (name, form, "one block"), same_block=True)
            assert d.stats()[0] - p0 == 1, (name, form, "x and y in one block on disjoint even ranges: the sweep refuses only d_x == d_y")
            seen[form] = out
        if len(seen) == 2:
            for a, b in zip(seen[3], seen[2]):
                assert np.array_equal(a, b), (name, "the second and the third form differ in their bits")
    finally:
        if mat is not None:
            hip.free_matrix(mat)
        restore(g)


@pytest.mark.gpu
def test_all_rows_clean_takes_the_grid_form(hip):
    """13^3 with arm length 6 and no planted row: every row is clean on the device, the remainder is empty, and the handle still
    reports the grid form (dense_layers_host keeps it with a listed remainder or with none) — products and sums exact"""
    st = sc.whole("one_ragged_patch_all_clean")
    g = hip.g
    mat = None
    try:
        mat = upload_whole(hip, st)
        stt = (C.c_long * 8)()
        g.gcge_hip_mat_star_stats(mat, stt)
        assert stt[4] == stt[5] == st.n == 2197 and g.gcge_hip_mat_spmm_form(mat).decode().startswith("spmm_star")
        d = Dev(hip, st, mat)
        X = st.X(66)
        for m, s0, s1 in [(2, 0, 0), (64, 2, 0), (30, 0, 4)]:
            d.dot2(X, st.product(np.ascontiguousarray(X[:, :m])), m, s0, s1, ("all clean", m))
    finally:
        if mat is not None:
            hip.free_matrix(mat)
        restore(g)


@pytest.mark.gpu
@pytest.mark.parametrize("name,m", [(XCD_SMALL, 34), (sc.XCD_BIG[0], sc.XCD_BIG[5])])
def test_xcd_orders_agree_bit_for_bit(hip, name, m):
    """the third form under gcge_hip_spmm_star_xcd(0 / 1 / 2 / 22) on 27 workgroups (the default order is the identity, 1 and 2 are
    not) and on 270 (176 permuted by the default, 94 behind): the same bits, equal to the reference, products and sums"""
    st = sc.whole(name)
    g = hip.g
    assert st.iso_on_device() and long_rows(st.S)                   # the third form takes it, and the sums of any width go through the sweep
    mat = None
    try:
        g.gcge_hip_spmm_star_form(3)
        mat = upload_whole(hip, st)
        d = Dev(hip, st, mat)
        X = st.X(m)
        Y = st.product(X)
        first = None
        for xcd in (0, 1, 2, 22):
            g.gcge_hip_spmm_star_xcd(xcd)
            p0 = d.stats()[0]
            out = [d.spmm(X, Y, m, 2, 0, (name, "xcd", xcd)), d.dot2(X, Y, m, 0, 2, (name, "xcd", xcd, "dot2"))]
            assert d.stats()[0] - p0 == 2, (name, xcd, "both calls must take the sweep")
            first = first or out
            assert all(np.array_equal(a, b) for a, b in zip(first, out)), (name, xcd)
    finally:
        if mat is not None:
            hip.free_matrix(mat)
        restore(g)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(sc.MASKED))
def test_masked_grids_four_ways(hip, name):
    """a convex set of grid points in scan order: named geometry in the third form (line table), named geometry in the second form
    (point-wise map, gcge_hip_spmm_star_masked_third(0)), the geometry recovered at upload, and the recovery switched off (the other
    forms) — bit-identical and equal to the reference, products and sums"""
    st = sc.masked(name)
    g = hip.g
    A, _ = st.csr()
    X = st.X(66)
    g.gcge_hip_spmm_dense_mode(1)
    mats = []
    try:
        g.gcge_hip_spmm_star_infer(0)
        mp = hip.matrix(A)
        g.gcge_hip_spmm_star_infer(1)
        mh, mi = hip.matrix_grid(A, st.dims, st.box), hip.matrix(A)
        mats = [mp, mh, mi]
        assert g.gcge_hip_mat_spmm_form(mh).decode().startswith("spmm_star") and g.gcge_hip_mat_spmm_form(mi).decode().startswith("spmm_star")
        assert not g.gcge_hip_mat_spmm_form(mp).decode().startswith("spmm_star")
        stt = (C.c_long * 8)()
        assert g.gcge_hip_mat_star_stats(mh, stt) == 1 and list(stt[:6]) == list(st.dims) + [6, st.nclean, st.n], list(stt)
        assert g.gcge_hip_mat_star_masked_form(mh) == 3 and g.gcge_hip_mat_star_masked_form(mi) == 3 and g.gcge_hip_mat_star_masked_form(mp) == 0
        ways = [("named, third", mh, 1), ("named, second", mh, 0), ("recovered", mi, 1), ("no geometry", mp, 1)]
        first = None
        for what, mat, third in ways:
            g.gcge_hip_spmm_star_masked_third(third)
            if mat is mh:
                assert g.gcge_hip_mat_star_masked_form(mh) == (3 if third else 2)
            d = Dev(hip, st, mat)
            out = []
            for m, s0, s1 in sc.FEW_M + [(66, 0, 0)]:
                out.append(d.spmm(X, st.product(np.ascontiguousarray(X[:, :m])), m, s0, s1, (name, what, "spmm", m)))
            for m, s0, s1 in sc.DOT_M:
                p0 = d.stats()[0]
                out.append(d.dot2(X, st.product(np.ascontiguousarray(X[:, :m])), m, s0, s1, (name, what, "dot2", m)))
                assert d.stats()[0] - p0 == (1 if mat is not mp else 0), (name, what, m)
            first = first or out
            assert all(np.array_equal(a, b) for a, b in zip(first, out)), (name, what, "differs from the first way in its bits")
    finally:
        for mat in mats:
            hip.free_matrix(mat)
        restore(g)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(sc.REAL))
def test_real_data_stays_inside_the_derived_bound(hip, name):
    """uniform - 0.5 on all-clean matrices, every form once: |Y - ref| <= (count + 1) 2^-53 |A| |X| with the operation count of the
    header (derived from the kernels' code, not measured); a repeated call gives the same bits"""
    st = sc.real_case(name)
    g = hip.g
    A, _ = st.csr()
    R = max(st.arms)
    count = R + 3 if st.coef == "iso" else 3 * R + 1
    m = 34
    X = st.X(m)
    w, ab = st.product_ld(X)
    mat = None
    try:
        mat = hip.matrix_grid(A, st.dims, st.box) if st.masked else hip.matrix(A)
        stt = (C.c_long * 8)()
        assert g.gcge_hip_mat_spmm_form(mat).decode().startswith("spmm_star") and g.gcge_hip_mat_star_stats(mat, stt) == 1 and stt[4] == st.n
        d = Dev(hip, st, mat)
        for form in ([3, 2] if st.coef == "iso" else [2]):
            g.gcge_hip_spmm_star_form(form)
            g.gcge_hip_spmm_star_masked_third(1 if form == 3 else 0)
            outs = []
            for rep in range(2):
                bx = d.block(X, 2, m + 4, IN_GUARD)
                by = d.block(np.full((st.n, m), OUT_GUARD), 0, m + 2, OUT_GUARD)
                p0 = d.stats()[0]
                hip.ops.spmm(mat, bx[0], by[0], (2, 0), (2 + m, m))
                assert d.stats()[0] - p0 == 1
                got = d.got(by)
                err = np.abs(got[:, :m].astype(np.longdouble) - w)
                worst = float(np.max(err / np.maximum((count + 1) * U * ab, np.longdouble(1e-300))))
                print("%s form %d: worst error / bound = %.3f" % (name, form, worst))
                assert np.all(err <= (count + 1) * U * ab), (name, form, worst)
                assert np.all(bits(np.ascontiguousarray(got[:, m:])) == OUT_BITS)
                outs.append(bits(np.ascontiguousarray(got)).copy())
                d.free(bx, by)
            assert np.array_equal(outs[0], outs[1]), (name, form, "a repeated call gives other bits")
    finally:
        if mat is not None:
            hip.free_matrix(mat)
        restore(g)


# ---- 3. the slabs, one process ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_loopback_slabs_exact():
    """tests/star_slab_worker.py: see its docstring.  The worker's time limit is the guard against a hang; a time-out is a failure."""
    assert all("gcge_hip_" + n in abi.HIP for n in ("mat_create_local_ghosts", "mat_create_local_ghosts_grid", "mat_set_halo_rccl", "set_halo_overlap"))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    t0 = time.time()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "star_slab_worker.py")], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=300)
    print(p.stdout[-4000:])
    print("worker wall time %.1f s" % (time.time() - t0))
    assert p.returncode == 0, p.stdout[-4000:]
    assert "star slabs ok: %d cases" % (len(sc.SLABS) + len(sc.MASKED_SLABS)) in p.stdout, p.stdout[-2000:]
