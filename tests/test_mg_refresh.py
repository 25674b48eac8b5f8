"""A live multigrid hierarchy refreshed in place after its level 0 took new values (gcge_hip_multigrid_refresh in csrc/hip/multigrid.hip
over the values-only Galerkin kernel of csrc/hip/mg_device.hip; GCGE_AMGRefresh, HipBackend.multigrid, Hierarchy.refresh, eigsh(amg=...)):
the kernel against the host's product by bits, a refreshed hierarchy against a fresh one by bits and by exact products, what a decline
leaves behind, and the SCF-style loop over one handle and one hierarchy.

New values of the generic cases: v (1 + 0.125 ((r + c) mod 5)) plus a shift on the diagonal — symmetric, every factor a multiple of
1/8, no entry becomes zero, so the structure stays.  The SiO2-like matrices take real_values / integer_values of
tests/test_mat_update_forms.py, which leave the star's coefficients alone."""
import ctypes as C

import numpy as np
import pytest

from gcge_amd.lib import (CSR, hip_lib, host_lib, make_problem, mat_to_csr, mat_update_stats, mg_galerkin_device, mg_galerkin_values_device,
                          multigrid_graph_method, multigrid_refresh_stats)
from helpers import bits, csr_to_scipy
from test_mg_device import _galerkin_cases, _host_arrays, chain_with_hubs, empty_and_isolated, graph_agg, grid_agg, host_galerkin, permuted_lap3d, same_csr
from test_mat_update_forms import case as forms_case, create as forms_create, form, integer_values, real_values


def new_diagonal(rp, ci, v):
    """a potential on the diagonal, everything else as it is"""
    r = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    d = r == ci
    out = v.copy()
    out[d] += 0.25 * (1.0 + r[d] % 11)
    return out


def new_values(rp, ci, v, shift=0.5):
    r = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    out = v * (1.0 + 0.125 * ((r + ci) % 5)) + shift * (r == ci)
    assert np.all(out != 0.0)
    return out


def to_device(v):
    import torch
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).cuda()


# ---------------------------------------------------------------------------------------------- 1. the values kernel against the host
def _galerkin_setup(hip, name):
    """(handle, device rows, agg, nc, scale) of tests/test_mg_device.py::test_device_galerkin_is_the_host_galerkin_byte_for_byte"""
    if name.startswith("lap3d20"):
        A, _ = make_problem("lap3d", 20); scale = float(name.split("_")[-1]); mode = "grid"; dims = (20, 20, 20)
    elif name.startswith("fe3d12"):
        A, B = make_problem("fe3d", 12); dims = (12, 12, 12); mode = "grid"
        A, scale = (A, 0.5) if name.endswith("A") else (B, 1.0)
    elif name == "sio2_24":
        A, _ = make_problem("sio2", 24); scale = 0.5; mode = "grid"; dims = (24, 24, 24)
    elif name == "lap3d16_permuted_graph":
        (A, keep), scale, mode = permuted_lap3d(16), 0.5, "graph"
    elif name == "empty_isolated":
        (A, keep), scale, mode = empty_and_isolated(), 0.5, "graph"
    elif name == "hubs_pairs":
        (A, keep), scale, mode = chain_with_hubs("second"), 0.5, "pairs"
    else:
        A, _ = make_problem("lap3d", 9); scale = 0.5; mode = "one"
    m = hip.matrix(A)
    dev = mat_to_csr(m)
    if mode == "grid":
        agg, nc = grid_agg(dims)
    elif mode == "graph":
        agg, nc = graph_agg(dev)
    elif mode == "pairs":
        agg, nc = (np.arange(A.nrows) // 2).astype(np.int32), A.nrows // 2
    else:
        agg, nc = np.zeros(A.nrows, dtype=np.int32), 1
    return m, dev, agg, nc, scale


@pytest.mark.gpu
@pytest.mark.parametrize("name", _galerkin_cases() + ["hubs_pairs"])
def test_values_kernel_is_the_host_galerkin_of_the_new_values_by_bits(hip, name):
    """The cases of tests/test_mg_device.py, whose coarse rows hold at most 53 columns, and hubs_pairs: the chain with two hub rows of
    that file aggregated by pairs of rows, whose coarse rows 0 and 1 hold about 300 columns each — ranks beyond the 64 lanes."""
    m, dev, agg, nc, scale = _galerkin_setup(hip, name)
    m1 = None
    try:
        rp_c, ci_c, va_c = mg_galerkin_device(m, agg, nc, scale)             # the coarse structure, found once
        v1 = new_values(dev[0], dev[1], dev[2])
        A1, keep = _host_arrays(dev[0], dev[1], v1)
        m1 = hip.matrix(A1)
        same_csr(mat_to_csr(m1), (dev[0], dev[1], v1))                       # the same rows, the new values
        out = np.full(len(ci_c), np.nan)
        assert mg_galerkin_values_device(m1, agg, nc, scale, rp_c, ci_c, out) == 0
        ref = host_galerkin((dev[0], dev[1], v1), agg, nc, scale)
        same_csr((rp_c, ci_c, out), ref)
        assert not np.array_equal(bits(out), bits(va_c)) or len(out) == 0    # (the values did change)
        if name == "sio2_24":
            assert np.bincount(agg, weights=np.diff(dev[0])).max() > 4 * 64       # long coarse rows: several chunks of entries per row
        if name == "hubs_pairs":
            assert 2 * 64 < np.diff(rp_c).max() <= 512                        # more columns than lanes, inside the kernel's reach
        if name == "nc1":
            assert np.bincount(agg).max() > 64                                # batches of more than 64 member rows
    finally:
        hip.free_matrix(m)
        if m1 is not None:
            hip.free_matrix(m1)


@pytest.mark.gpu
def test_values_kernel_flags_a_structure_of_another_aggregate_map(hip):
    """lap3d 20 on its grid cells; the structure comes from that map, the call gets a map in which one fine row sits in a far cell: the
    entries that name that row fall on a coarse column their coarse rows do not hold."""
    m, dev, agg, nc, scale = _galerkin_setup(hip, "lap3d20_grid_0.5")
    try:
        rp_c, ci_c, va_c = mg_galerkin_device(m, agg, nc, scale)
        other = agg.copy()
        r0 = 20 * 20 * 9 + 20 * 9 + 9                                        # an interior point
        far = nc - 1
        assert far != agg[r0] and far not in ci_c[rp_c[agg[r0]]:rp_c[agg[r0] + 1]]
        other[r0] = far
        out = np.arange(len(ci_c), dtype=np.float64) + 0.25
        keep = out.copy()
        assert mg_galerkin_values_device(m, other, nc, scale, rp_c, ci_c, out) == 1
        assert np.array_equal(bits(out), bits(keep))
        assert mg_galerkin_values_device(m, agg, nc, scale, rp_c, ci_c, out) == 0          # and the right map still goes through
        assert np.array_equal(bits(out), bits(va_c))
    finally:
        hip.free_matrix(m)


# ---------------------------------------------------------------------------------------------- 2. a refreshed hierarchy is a fresh one
class Setup:
    """One case: arrays of A (and B), the two value sets of each, how a handle is made of values, levels, graph method"""


def _csr_handles(hip, arrays, values, updatable):
    A, keep = _host_arrays(arrays[0], arrays[1], values)
    return hip.matrix(A, updatable=updatable)


def setup_case(name, integer=False, levels=4):
    s = Setup()
    s.name, s.graph, s.levels, s.B = name, 0, levels, None
    if name in ("sio2", "ball"):
        c = forms_case(name)
        s.make = lambda hip, which, v, updatable: forms_create(hip, c, v, updatable)
        s.A = (integer_values(c, "O"), integer_values(c, "B")) if integer else (real_values(c, 0), real_values(c, 1))
        return s
    if name == "sio2_32":
        # level 1 (16^3 rows: a star of arm 3 and the coarsened atom blocks) takes the star and dense forms, which 12^3 rows do not;
        # level 2 (8^3) is pad-8 rows; level 3 (4^3, with levels=4) a pattern form whose 16-slot table takes uniform classes only
        arrays = csr_arrays_of(make_problem("sio2", 32)[0])
        s.A = (arrays[2], new_diagonal(*arrays))
    elif name == "lap3d16":
        arrays, s.levels = csr_arrays_of(make_problem("lap3d", 16)[0]), 3
    elif name == "fe3d12":
        A, B = make_problem("fe3d", 12)
        arrays, arraysB = csr_arrays_of(A), csr_arrays_of(B)
        # (the mass matrix has 19 entries per row: a value table of 16 slots, which takes new values in place only while the rows of
        # a class stay equal — gcge_hip.h; a factor keeps them so, and 1.25 v is exact)
        s.B = (arraysB[2], 1.25 * arraysB[2])
    else:
        # MIS-2 picks its aggregates from the off-diagonal values (strength of connection, the strongest neighbouring root), level by
        # level, and a refresh keeps the aggregates it has: it is the fresh hierarchy bit for bit when the new values leave every
        # off-diagonal alone — a coarse off-diagonal sums fine off-diagonals only —, so this case moves the diagonal
        A, keep = permuted_lap3d(16)
        arrays, s.graph = csr_arrays_of(A), 1
        s.A = (arrays[2], new_diagonal(*arrays))
    if name in ("lap3d16", "fe3d12"):
        s.A = (arrays[2], new_values(*arrays))
    if integer:             # small integers on the diagonal, the couplings as they are (-1): every product below is exact
        r = np.repeat(np.arange(len(arrays[0]) - 1), np.diff(arrays[0]))
        d = r == arrays[1]
        v0, v1 = arrays[2].copy(), arrays[2].copy()
        v0[d] = 6.0 + r[d] % 3
        v1[d] = 7.0 + (2 * r[d]) % 5
        s.A = (v0, v1)
    s.make = lambda hip, which, v, updatable: _csr_handles(hip, arrays if which == "A" else arraysB, v, updatable)
    return s


def csr_arrays_of(A):
    S = csr_to_scipy(A).tocsr()
    S.sort_indices()
    return S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data.astype(np.float64)


def snapshot(hip, h):
    g = hip_lib()
    Ah, Bh, Ph = h.level_handles()
    return {"L": len(Ah), "A": [mat_to_csr(a) for a in Ah[1:]], "B": [mat_to_csr(b) for b in Bh[1:]],
            "P": [mat_to_csr(p) for p in Ph], "PT": [mat_to_csr(p, transpose=True) for p in Ph],
            "form": [g.gcge_hip_mat_spmm_form(a).decode() for a in Ah], "order": [g.gcge_hip_mat_row_order(a).decode() for a in Ah],
            "handles": [a.value for a in Ah + Bh + Ph]}


def same_levels(a, b, keys=("A", "B", "P", "PT")):
    assert a["L"] == b["L"]
    for key in keys:
        assert len(a[key]) == len(b[key])
        for x, y in zip(a[key], b[key]):
            same_csr(x, y)


class Pair:
    """handles of V0 given V1 in place, their hierarchy built on V0, and fresh handles of V1 with their hierarchy"""

    def __init__(self, hip, s, refreshable=True, updatable=True):
        self.hip, self.s = hip, s
        self.before = multigrid_graph_method()
        multigrid_graph_method(s.graph)
        self.mats, self.hier = [], []
        try:
            self.mA = self._mat("A", s.A[0], updatable)
            self.mB = self._mat("B", s.B[0], updatable) if s.B is not None else None
            self.h = self._hier(self.mA, self.mB, refreshable)
            self.built = snapshot(hip, self.h)
            assert hip.matrix_update_values(self.mA, to_device(s.A[1]))
            if s.B is not None:
                assert hip.matrix_update_values(self.mB, to_device(s.B[1]))
            self.fA = self._mat("A", s.A[1], False)
            self.fB = self._mat("B", s.B[1], False) if s.B is not None else None
            self.fresh = snapshot(hip, self._hier(self.fA, self.fB, False))
        except BaseException:
            self.close()
            raise

    def _mat(self, which, v, updatable):
        m = self.s.make(self.hip, which, v, updatable)
        self.mats.append(m)
        return m

    def _hier(self, mA, mB, refreshable):
        h = self.hip.multigrid(mA, mB, levels=self.s.levels, block_size=8, refreshable=refreshable)
        self.hier.append(h)
        return h

    def close(self):
        multigrid_graph_method(self.before)
        for h in self.hier:
            h.close()
        for m in self.mats:
            self.hip.free_matrix(m)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


@pytest.mark.gpu
@pytest.mark.parametrize("name,min_levels", [("lap3d16", 3), ("fe3d12", 3), ("sio2", 3), ("ball", 3), ("lap3d16_permuted", 3), ("sio2_32", 3)])
def test_a_refreshed_hierarchy_is_a_fresh_hierarchy_by_bits(hip, name, min_levels):
    s = setup_case(name, levels=3 if name == "sio2_32" else 4)
    with Pair(hip, s) as p:
        assert p.built["L"] == p.fresh["L"] >= min_levels
        assert any(not np.array_equal(bits(x[2]), bits(y[2])) for x, y in zip(p.built["A"], p.fresh["A"]))     # the values moved
        r0 = multigrid_refresh_stats()
        head = p.h._head()
        assert hip.g.gcge_hip_multigrid_refresh(head.A_array, head.B_array if s.B is not None else None, head.P_array, p.h.num_levels) == 0
        r1 = multigrid_refresh_stats()
        L = p.built["L"]
        assert (r1[0] - r0[0], r1[1] - r0[1], r1[2] - r0[2]) == (1, 0, (L - 1) * (2 if s.B is not None else 1)), (r0, r1)
        assert 0 < r1[3] - r0[3] <= 8 * (L - 1) * (2 if s.B is not None else 1)       # a flag word per product and per checked update
        got = snapshot(hip, p.h)
        assert got["handles"] == p.built["handles"]                         # in place: the same handles
        same_levels(got, p.fresh)                                           # A, B by bits; P, P^T are those of the fresh build ...
        same_levels(got, p.built, keys=("P", "PT"))                         # ... and untouched
        # forms and row orders: those of the fresh hierarchy, but that a pattern level whose classes are no longer uniform keeps its
        # offsets table and takes values per row ("+values") where a fresh handle of such values finds no pattern form or the same one
        print(name, "forms refreshed", got["form"], "fresh", p.fresh["form"])
        if name == "sio2_32":
            assert "spmm_star" in got["form"][1] or "spmm_dense" in got["form"][1], got["form"]      # a coarse level that needs its maps
        assert got["order"] == p.fresh["order"] == p.built["order"]
        for l, (a, b, c) in enumerate(zip(got["form"], p.fresh["form"], p.built["form"])):
            assert a == b or (a.endswith("+values") and a[:-len("+values")] == c), (l, a, b, c)
        assert p.h.refresh() is True                                        # the Python route, once more on the same values
        same_levels(snapshot(hip, p.h), p.fresh)


def level_products(hip, Ah):
    """A_l X for an integer block X of 8 columns on every level, through MatDotMultiVec"""
    out = []
    for a in Ah:
        n = hip.g.gcge_hip_mat_nrows(a)
        X = np.random.default_rng(100 + n).integers(-4, 5, (n, 8)).astype(np.float64)
        xh, yh = hip.mv_from_numpy(a, X), hip.mv_from_numpy(a, np.full((n, 8), 3.0))
        hip.ops.spmm(a, xh, yh, (0, 0), (8, 8))
        out.append(hip.mv_to_numpy(yh, n, 0, 8))
        hip.ops.mv_destroy(xh, 8)
        hip.ops.mv_destroy(yh, 8)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sio2", "lap3d16"])
def test_products_through_a_refreshed_hierarchy_are_exact(hip, name):
    """mat_to_csr reads d_val only; the stored copies the products read (pad-8, tables, row values, star diagonal, blocks) are checked
    here: integer data, scale 0.5, so every coarse value of level l is a multiple of 2^-l and every product is exact in any order."""
    s = setup_case(name, integer=True)
    with Pair(hip, s) as p:
        assert p.h.refresh() is True
        got, fresh = level_products(hip, p.h.level_handles()[0]), level_products(hip, p.hier[1].level_handles()[0])
        assert len(got) == len(fresh) >= 3
        for l, (a, b) in enumerate(zip(got, fresh)):
            assert np.array_equal(bits(np.ascontiguousarray(a)), bits(np.ascontiguousarray(b))), l
        csr = [mat_to_csr(a) for a in p.h.level_handles()[0]]
        for l, ((rp, ci, va), y) in enumerate(zip(csr, got)):               # and they are the products of the matrices mat_to_csr shows
            import scipy.sparse as sp
            S = sp.csr_matrix((va, ci, rp), shape=(len(rp) - 1, len(rp) - 1))
            X = np.random.default_rng(100 + S.shape[0]).integers(-4, 5, (S.shape[0], 8)).astype(np.float64)
            assert np.array_equal(y, S @ X), l


# ---------------------------------------------------------------------------------------------- 3. declines
@pytest.mark.gpu
@pytest.mark.parametrize("why,refreshable,expect", [("no_value_maps", False, 1), ("table_of_16_slots", True, 3)])
def test_a_level_that_declines_ends_the_refresh_and_the_hierarchy_is_built_again(hip, why, refreshable, expect):
    """sio2 32 with a new diagonal, 4 levels of 32^3, 16^3, 8^3 and 4^3 rows; sio2 32 is the smallest of the generator's usual sizes
    whose level 1 takes a star or dense form (the 12^3 rows under sio2 24 stay pad-8 rows, which take any values).
      no_value_maps      the hierarchy is built WITHOUT value maps: level 1 declines every in-place update from the handle alone.
      table_of_16_slots  built with them, levels 1 and 2 are written; level 3 is a pattern form whose value table has 16 slots, and
                         the new values split its classes — a decline of gcge_hip_mat_update_values_device by design.
    The refresh returns the level; the levels below it are fresh, it and those above it as they were."""
    s = setup_case("sio2_32")
    with Pair(hip, s, refreshable=refreshable) as p:
        forms = p.built["form"]
        print(why, "forms", forms)
        assert p.built["L"] == 4
        assert "spmm_star" in forms[1] or "spmm_dense" in forms[1], forms
        assert forms[3].startswith("spmm_pattern") and not forms[3].endswith("+values"), forms
        head = p.h._head()
        r0, u0 = multigrid_refresh_stats(), mat_update_stats()
        rc = hip.g.gcge_hip_multigrid_refresh(head.A_array, None, head.P_array, p.h.num_levels)
        r1, u1 = multigrid_refresh_stats(), mat_update_stats()
        assert rc == expect, (rc, forms)
        assert u1[3] - u0[3] == 1 and (r1[0] - r0[0], r1[1] - r0[1], r1[2] - r0[2]) == (0, 1, rc - 1), (r0, r1, u0, u1)
        got = snapshot(hip, p.h)
        for l in range(1, p.built["L"]):                                    # coarse level l is entry l - 1
            same_csr(got["A"][l - 1], (p.fresh if l < rc else p.built)["A"][l - 1])
        assert not np.array_equal(bits(p.fresh["A"][rc - 1][2]), bits(p.built["A"][rc - 1][2]))     # (the two differ at that level)
        assert got["handles"] == p.built["handles"] and got["form"] == forms
        assert p.h.refresh() is False                                       # declines again, then destroys and builds again
        again = snapshot(hip, p.h)
        same_levels(again, p.fresh)
        assert again["form"] == p.fresh["form"] and again["order"] == p.fresh["order"]
        assert multigrid_refresh_stats()[1] - r1[1] == 1


@pytest.mark.gpu
def test_refresh_refuses_what_is_not_its_hierarchy(hip):
    arrays = csr_arrays_of(make_problem("lap3d", 16)[0])
    m = _csr_handles(hip, arrays, arrays[2], True)
    try:
        with hip.multigrid(m, levels=3, block_size=4) as h:
            head = h._head()
            before, r0 = snapshot(hip, h), multigrid_refresh_stats()
            foreign = (C.c_void_p * h.num_levels)(*[head.A_array[l] for l in range(h.num_levels)])         # the same handles in another array
            assert hip.g.gcge_hip_multigrid_refresh(foreign, None, head.P_array, h.num_levels) == -1
            assert hip.g.gcge_hip_multigrid_refresh(head.A_array, None, head.P_array, h.num_levels + 1) == -1
            assert hip.g.gcge_hip_multigrid_refresh(head.A_array, None, head.P_array, h.num_levels - 1) == -1
            assert multigrid_refresh_stats() == r0
            same_levels(snapshot(hip, h), before)
            assert hip.g.gcge_hip_multigrid_refresh(head.A_array, None, head.P_array, h.num_levels) == 0     # the same values: the same hierarchy
            same_levels(snapshot(hip, h), before)
    finally:
        hip.free_matrix(m)


# ---------------------------------------------------------------------------------------------- 4. the loop
@pytest.mark.gpu
def test_eigsh_over_three_potentials_on_one_handle_and_one_hierarchy(hip):
    """sio2 + t v on the diagonal, t = 0, 1, 2 (tests/test_mat_update_forms.py::test_eigsh_over_three_potentials_on_one_star_handle):
    one updatable handle, ONE hierarchy of 3 levels refreshed in place, warm starts; every step against eigsh on a fresh handle with a
    hierarchy built inside the solve (amg_levels=3).  Both solves stop a pair at ||r|| <= tol |lambda| and |lambda~ - lambda| <= ||r||
    for a unit eigenvector, so two converged solves of one matrix differ by at most 2 tol |lambda|."""
    import torch
    from gcge_amd import eigsh
    c = forms_case("sio2")
    k, tol = 4, 1e-8
    n = c.S.shape[0]
    pot = np.random.default_rng(23).random(n)
    dev = lambda v: tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (c.S.indptr.astype(np.int32), c.S.indices.astype(np.int32), v))
    m = hip.matrix_from_device(*dev(c.S.data), updatable=True)
    h = None
    try:
        h = hip.multigrid(m, levels=3, block_size=4)
        assert h.num_levels == 3 and h.block_size == 4 and h.A.value == m.value and h.M is None
        handles = snapshot(hip, h)["handles"]
        r0 = multigrid_refresh_stats()
        r = None
        for t in range(3):
            v = c.S.data.copy()
            v[c.diag] += 0.5 * t * pot
            if t:
                assert hip.matrix_update_values(m, torch.from_numpy(v).cuda())
                assert h.refresh() is True
            r = eigsh(m, k, X0=None if r is None else r.eigenvectors, tol=tol, amg=h, backend=hip)
            f = hip.matrix_from_device(*dev(v))
            try:
                rf = eigsh(f, k, tol=tol, amg_levels=3, backend=hip)
            finally:
                hip.free_matrix(f)
            lam, lamf = r.eigenvalues.cpu().numpy(), rf.eigenvalues.cpu().numpy()
            print("step", t, "iterations", r.iterations, rf.iterations, "max relative difference %.2e" % np.max(np.abs(lam - lamf) / np.abs(lamf)))
            assert r.converged >= k and rf.converged >= k
            assert np.all(np.abs(lam - lamf) <= 2.0 * tol * np.abs(lamf)), (lam, lamf)
        r1 = multigrid_refresh_stats()
        assert (r1[0] - r0[0], r1[1] - r0[1], r1[2] - r0[2]) == (2, 0, 4), (r0, r1)
        assert snapshot(hip, h)["handles"] == handles                       # the kept hierarchy was never built again
        # what eigsh refuses
        other = hip.matrix_from_device(*dev(c.S.data))
        try:
            with pytest.raises(ValueError):
                eigsh(m, k, tol=tol, amg=h, amg_levels=3, backend=hip)
            with pytest.raises(ValueError):
                eigsh(other, k, tol=tol, amg=h, backend=hip)
            with pytest.raises(ValueError):
                eigsh(dev(c.S.data), k, tol=tol, amg=h, backend=hip)
            with pytest.raises(ValueError):
                eigsh(m, k, tol=tol, amg=h, block_size=h.block_size + 1, backend=hip)
        finally:
            hip.free_matrix(other)
    finally:
        if h is not None:
            h.close()
        hip.free_matrix(m)
    with pytest.raises(ValueError):
        h.refresh()                                                         # a closed hierarchy


# ---------------------------------------------------------------------------------------------- 5. CPU
def test_amg_refresh_over_a_table_without_the_hook_returns_minus_one_and_changes_nothing(oracle):
    import pyoracle as po
    h = host_lib()
    A, _ = make_problem("lap3d", 8)
    mA = oracle.matrix(A)
    amg = C.c_void_p(h.GCGE_AMGCreate(mA, None, 3, 4, 1, 5, 4, 1e-2, oracle.ops_handle))
    assert amg.value
    try:
        L = C.cast(amg, C.POINTER(C.c_int * 8)).contents[6]                 # GCGE_AMG: three pointers, then num_levels
        assert L >= 2
        A_array = C.cast(C.cast(amg, C.POINTER(C.c_void_p)).contents.value, C.POINTER(C.c_void_p))

        def level_values():
            out = []
            for l in range(1, L):
                mat = C.cast(A_array[l], C.POINTER(po.OCcs)).contents
                nnz = mat.j_col[mat.ncols]
                out.append(np.ctypeslib.as_array(mat.data, (nnz,)).copy())
            return out
        before = level_values()
        assert h.GCGE_AMGRefresh(amg, oracle.ops_handle) == -1
        assert h.GCGE_AMGRefresh(None, oracle.ops_handle) == -1
        for a, b in zip(before, level_values()):
            assert np.array_equal(bits(a), bits(b))
    finally:
        h.GCGE_AMGDestroy(C.byref(amg), oracle.ops_handle)
