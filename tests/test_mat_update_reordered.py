"""New values, in place, for handles that RE-ORDERED their rows (csrc/hip/mat_upload.hip "row orders": the grid recovered from the star
couplings, or reverse Cuthill-McKee): created with updatable=True such a handle keeps its entry map (gcge_hip_mat_entry_map;
tests/test_entry_map.py checks the map on the host), gcge_hip_mat_update_values_device gathers the caller's values through it
(k_mv_gather_entries, csrc/hip/mat_values.hip) and runs the update of tests/test_mat_update.py / tests/test_mat_update_forms.py on the
result; gcge_hip_multigrid_refresh takes such a handle as level 0.  Those two files and tests/test_mg_refresh.py stay as they are.

Four matrices, each in a random numbering (the permuted() pattern of tests/test_reorder.py) and in sizes no other test uses — a live
matrix pins the row order of its size for later ones, and every handle made here is freed:
  lap3d   make_problem("lap3d", 15): 3375 rows, the 7-point star; the handle recovers the grid and takes a pattern form
  sio2    make_problem("sio2", 22, K=8, R0=1.5, R1=3.0, seed=12345): the 37-point star and atom blocks; star + blocks + pad-8
  ball    make_problem("sio2ball", 26, ...): the same on the grid points inside a sphere (a row map under the sweep)
  graph   tests/test_mg_graph.py::geometric_graph(3000): no grid anywhere, reverse Cuthill-McKee

Data is exact, as in tests/test_mat_update_forms.py: integer matrix entries assigned on the generator's STRUCTURE (one integer
coefficient per distance at star positions, the same on every axis, another integer at star positions whose generated value is not
the coefficient, small integers elsewhere, an integer diagonal) and integer X in [-4, 4]: products are compared
with S_new @ X by np.array_equal, the handle's CSR with that of a second handle by bits.  An entry at a star position whose creation
value equals the star's coefficient is pinned (include/gcge_hip.h); the diagonal and everything else is free."""
import functools

import numpy as np
import pytest

from gcge_amd.lib import ball_geometry, csr_to_scipy, make_problem, mat_to_csr, mat_update_stats, multigrid_refresh_stats
from helpers import bits, csr_from_scipy

WIDTHS = (7, 16, 64)
OFFSETS = (1, 3)                          # odd column offsets: columns [1, 1 + w) of X into columns [3, 3 + w) of Y
SIO2 = dict(K=8, R0=1.5, R1=3.0, seed=12345)
GEN = {"lap3d": ("lap3d", 15, {}), "sio2": ("sio2", 22, SIO2), "ball": ("sio2ball", 26, SIO2)}
NAMES = ("lap3d", "sio2", "ball", "graph")
FE = 25                                   # the generalised pair: make_problem("fe3d", 25)


@pytest.fixture()
def reorder_on(hip):
    hip.g.gcge_hip_spmm_reorder_mode(1)
    yield hip
    hip.g.gcge_hip_spmm_reorder_mode(0)


# ---- the matrices -----------------------------------------------------------------------------------------------------------------------
class Case:
    """S: the generator's matrix in ITS order (sorted CSR); rows / cols; masks diag, star, pinned, free and the (axis, dist) codes of the
    star positions; p: the random numbering the caller uses (caller row i = generator row p[i])"""


@functools.lru_cache(maxsize=None)
def case(name):
    c = Case()
    c.name = name
    if name == "graph":
        from test_mg_graph import geometric_graph
        c.S = geometric_graph(3000).tocsr()
    else:
        kind, G, kw = GEN[name]
        c.S = csr_to_scipy(make_problem(kind, G, **kw)[0]).tocsr()
    c.S.sort_indices()
    S = c.S
    n = S.shape[0]
    c.p = np.random.default_rng(17 + n).permutation(n)
    c.rows, c.cols = np.repeat(np.arange(n), np.diff(S.indptr)), S.indices
    c.diag = c.rows == c.cols
    c.star = np.zeros(S.nnz, dtype=bool)
    c.axis, c.dist = np.zeros(S.nnz, dtype=np.int64), np.zeros(S.nnz, dtype=np.int64)
    c.pinned = np.zeros(S.nnz, dtype=bool)
    if name != "graph":
        G = GEN[name][1]
        box = ball_geometry(G).astype(np.int64) if name == "ball" else np.arange(n, dtype=np.int64)
        xyz = np.stack([box % G, (box // G) % G, box // (G * G)], axis=1)
        d = xyz[c.cols] - xyz[c.rows]
        one = (d != 0).sum(axis=1) == 1
        c.axis = np.argmax(d != 0, axis=1)
        c.dist = np.abs(d).sum(axis=1)
        c.star = one & (c.dist >= 1) & (c.dist <= 6)
        for a in range(3):                                   # the star's coefficients: the value most entries of an (axis, distance) carry
            for k in range(1, 7):
                sel = c.star & (c.axis == a) & (c.dist == k)
                if sel.any():
                    vals, cnt = np.unique(bits(S.data[sel]), return_counts=True)
                    c.pinned |= sel & (bits(S.data) == vals[np.argmax(cnt)])
    c.free = ~c.pinned & ~c.diag
    return c


def integer_values(c, kind):
    """O: the creation values; D: another diagonal; B: another diagonal and another value in every free entry.  Symmetric; none is 0.
    The star is isotropic and its coefficients fall off with the distance: what gcge_hip_reorder_star_grid recovers a grid from
    (csrc/hip/reorder.hip: the distance-1 coefficient is the frequent off-diagonal value of largest magnitude)."""
    r, q = c.rows, c.cols
    coef = (20 - 2 * c.dist).astype(np.float64)                                                 # 18, 16 .. 8 at distance 1 .. 6
    bump = {"O": 0, "D": 0, "B": 1}[kind]
    v = -(1.0 + (r + q + bump) % 3)                                                             # -1 .. -3 elsewhere
    v = np.where(c.star, np.where(c.pinned, -coef, 1.0 + (r + q + bump) % 3), v)               # 1 .. 3 at star positions inside atom rows
    v = np.where(c.diag, 40.0 + (r + (3 if kind != "O" else 0)) % 7 + (5 * r) % 3 * (kind != "O"), v)
    return v.astype(np.float64)


def in_callers_order(S, v, p):
    """the matrix of S's structure with the values v, rows and columns numbered by p, ascending columns: what the caller holds"""
    import scipy.sparse as sp
    T = S.copy()
    T.data = np.ascontiguousarray(v, dtype=np.float64)
    Tp = sp.csr_matrix(T[p][:, p])
    Tp.sort_indices()
    assert Tp.nnz == S.nnz
    return Tp


@functools.lru_cache(maxsize=None)
def permuted(name, kind):
    c = case(name)
    return in_callers_order(c.S, integer_values(c, kind), c.p)


def callers_mask(c, mask):
    """a mask over the generator's entries as a mask over the caller's"""
    return in_callers_order(c.S, np.where(mask, 2.0, 1.0), c.p).data == 2.0


def create(hip, S, updatable):
    A, keep = csr_from_scipy(S)
    return hip.matrix(A, updatable=updatable)


def form(hip, m):
    return hip.g.gcge_hip_mat_spmm_form(m).decode()


def order(hip, m):
    return hip.g.gcge_hip_mat_row_order(m).decode()


_X = {}


def x_block(n):
    if n not in _X:
        _X[n] = np.random.default_rng(9 + n).integers(-4, 5, (n, OFFSETS[0] + max(WIDTHS))).astype(np.float64)
    return _X[n]


def products(hip, m, n):
    X, out = x_block(n), []
    a, b = OFFSETS
    for w in WIDTHS:
        xh, yh = hip.mv_from_numpy(m, X), hip.mv_from_numpy(m, np.full((n, b + w), 5.0))
        hip.ops.spmm(m, xh, yh, (a, b), (a + w, b + w))
        out.append(hip.mv_to_numpy(yh, n, b, b + w))
        hip.ops.mv_destroy(xh, X.shape[1])
        hip.ops.mv_destroy(yh, b + w)
    return out


def check_products(hip, m, S, what):
    n, X = S.shape[0], x_block(S.shape[0])
    a = OFFSETS[0]
    for w, y in zip(WIDTHS, products(hip, m, n)):
        want = S @ X[:, a:a + w]
        assert np.array_equal(y, want), (what, "width", w, np.argwhere(y != want)[:4].tolist())


def same_csr(x, y, what):
    for a, b in zip(x, y):
        assert a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)), what


def raw_update(hip, m, values):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(values, dtype=np.float64)).cuda()
    torch.cuda.synchronize()
    return hip.g.gcge_hip_mat_update_values_device(m, int(t.numel()), t.data_ptr())


def same_form_or_plus_values(now, before):
    return now == before or (now.endswith("+values") and now[:-len("+values")] == before)


# ---- 1. accepted updates ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_a_reordered_handle_takes_new_values_in_place(reorder_on, name):
    hip = reorder_on
    c = case(name)
    S0, SD, SB = permuted(name, "O"), permuted(name, "D"), permuted(name, "B")
    n, nnz = S0.shape[0], S0.nnz
    dg, pin, free = callers_mask(c, c.diag), callers_mask(c, c.pinned), callers_mask(c, c.free)
    for Snew, every_free in ((SD, False), (SB, True)):
        changed = bits(S0.data) != bits(Snew.data)
        assert np.all(changed[dg]) and not np.any(changed[pin]) and bool(np.all(changed[free])) == (every_free or not free.any())
    m = create(hip, S0, True)
    second = None
    try:
        f0 = form(hip, m)
        print(name, "rows", n, "entries", nnz, "form", f0, "row order:", order(hip, m))
        assert order(hip, m) != "as given"
        assert ("Cuthill" in order(hip, m)) == (name == "graph")
        assert hip.g.gcge_hip_mat_entry_map(m) == 4 * nnz
        check_products(hip, m, S0, "before")
        f = f0
        for step, Snew in enumerate((SD, SB, S0)):
            u0 = mat_update_stats()
            rc = raw_update(hip, m, Snew.data)
            du = tuple(b - a for a, b in zip(u0, mat_update_stats()))
            print(name, "update", "DBO"[step], "rc", rc, "stats", du, "form", form(hip, m))
            assert rc == 0
            assert du[0] + du[2] == 1 and du[3] == 0 and du[4] == 0 and 0 <= du[5] <= 4, du      # one accepted update, no decline
            assert same_form_or_plus_values(form(hip, m), f), (form(hip, m), f)
            f = form(hip, m)
            assert same_form_or_plus_values(f, f0) and hip.g.gcge_hip_mat_entry_map(m) == 4 * nnz
            check_products(hip, m, Snew, "after update %d" % step)
            second = create(hip, Snew, False)               # while m is alive: it adopts m's row order
            assert order(hip, second) == order(hip, m) and hip.g.gcge_hip_mat_entry_map(second) == 0
            same_csr(mat_to_csr(m), mat_to_csr(second), ("gcge_hip_mat_to_csr after update", step))
            hip.free_matrix(second)
            second = None
    finally:
        hip.free_matrix(m)
        if second is not None:
            hip.free_matrix(second)


# ---- 2. declines --------------------------------------------------------------------------------------------------------------------------
def check_decline(hip, m, n, values):
    before, csr0, f0 = products(hip, m, n), mat_to_csr(m), form(hip, m)
    u0 = mat_update_stats()
    rc = raw_update(hip, m, values)
    du = tuple(b - a for a, b in zip(u0, mat_update_stats()))
    assert rc == 1, rc
    assert du[:5] == (0, 0, 0, 1, 0) and 0 <= du[5] <= 4, du
    assert form(hip, m) == f0
    for w, a, b in zip(WIDTHS, before, products(hip, m, n)):
        assert np.array_equal(bits(np.ascontiguousarray(a)), bits(np.ascontiguousarray(b))), w
    same_csr(csr0, mat_to_csr(m), "gcge_hip_mat_to_csr after a decline")
    return du


@pytest.mark.gpu
def test_declines_write_nothing(reorder_on):
    hip = reorder_on
    c = case("sio2")
    S0, SB = permuted("sio2", "O"), permuted("sio2", "B")
    n = S0.shape[0]
    pin, dg = callers_mask(c, c.pinned), callers_mask(c, c.diag)
    npin = np.add.reduceat(pin.astype(np.int64), S0.indptr[:-1])
    clean = np.flatnonzero(npin == 36)                       # interior star rows
    assert clean.size
    r = clean[clean.size // 2]
    m = create(hip, S0, True)
    try:
        assert "spmm_star" in form(hip, m) and order(hip, m) != "as given" and hip.g.gcge_hip_mat_entry_map(m) == 4 * S0.nnz
        v1 = SB.data.copy()                                  # a pinned coefficient moved
        v1[S0.indptr[r] + np.flatnonzero(pin[S0.indptr[r]:S0.indptr[r + 1]])[-1]] += 1.0
        check_decline(hip, m, n, v1)
        v1 = SB.data.copy()                                  # a NaN on the diagonal
        v1[np.flatnonzero(dg)[n // 3]] = np.nan
        check_decline(hip, m, n, v1)
        check_products(hip, m, S0, "after the declines")
        assert raw_update(hip, m, SB.data) == 0              # and the handle still takes an update
        check_products(hip, m, SB, "an update after the declines")
    finally:
        hip.free_matrix(m)
    m = create(hip, S0, False)                               # the same handle without the switch: declined from the handle alone
    try:
        assert "spmm_star" in form(hip, m) and order(hip, m) != "as given"
        assert hip.g.gcge_hip_mat_entry_map(m) == 0 and hip.g.gcge_hip_mat_value_maps(m) == 0
        du = check_decline(hip, m, n, permuted("sio2", "D").data)
        assert du[5] == 0
        check_products(hip, m, S0, "without updatable")
    finally:
        hip.free_matrix(m)


# ---- 3. a generalised pair ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fe_pair():
    """fe3d in a random numbering, integer values on its structure: A's couplings -1 and a diagonal that moves, B's entries 1 and 8 and
    then twice that (B's rows hold more entries than 8 table slots: a value table takes uniform classes only, include/gcge_hip.h)"""
    A, B = make_problem("fe3d", FE)
    SA, SB = csr_to_scipy(A).tocsr(), csr_to_scipy(B).tocsr()
    SA.sort_indices(); SB.sort_indices()
    n = SA.shape[0]
    p = np.random.default_rng(17 + n).permutation(n)
    ra, rb = np.repeat(np.arange(n), np.diff(SA.indptr)), np.repeat(np.arange(n), np.diff(SB.indptr))
    a0 = np.where(ra == SA.indices, 6.0 + ra % 3, -1.0)
    a1 = np.where(ra == SA.indices, 7.0 + (2 * ra) % 5, -1.0)
    b0 = np.where(rb == SB.indices, 8.0, 1.0)
    return tuple(in_callers_order(S, v, p) for S, v in ((SA, a0), (SA, a1), (SB, b0), (SB, 2.0 * b0)))


@pytest.mark.gpu
def test_both_matrices_of_a_generalised_problem(reorder_on):
    hip = reorder_on
    A0, A1, B0, B1 = fe_pair()
    assert A0.nnz != B0.nnz
    mA = create(hip, A0, True)
    mB = None
    try:
        mB = create(hip, B0, True)                           # adopts A's order; its structure, and so its map, is its own
        print("fe3d", FE, "rows", A0.shape[0], "A:", form(hip, mA), "B:", form(hip, mB), "row order:", order(hip, mA))
        assert order(hip, mA) != "as given" and order(hip, mB) == order(hip, mA)
        assert hip.g.gcge_hip_mat_entry_map(mA) == 4 * A0.nnz and hip.g.gcge_hip_mat_entry_map(mB) == 4 * B0.nnz
        check_products(hip, mA, A0, "A before")
        check_products(hip, mB, B0, "B before")
        u0 = mat_update_stats()
        assert raw_update(hip, mA, A1.data) == 0 and raw_update(hip, mB, B1.data) == 0
        du = tuple(b - a for a, b in zip(u0, mat_update_stats()))
        assert du[0] + du[2] == 2 and du[3] == 0 and du[4] == 0, du
        check_products(hip, mA, A1, "A after")
        check_products(hip, mB, B1, "B after")
    finally:
        hip.free_matrix(mA)
        if mB is not None:
            hip.free_matrix(mB)


# ---- 4. the hierarchy follows -------------------------------------------------------------------------------------------------------------
def snapshot(hip, h):
    """(tests/test_mg_refresh.py::snapshot)"""
    Ah, Bh, Ph = h.level_handles()
    return {"L": len(Ah), "A": [mat_to_csr(a) for a in Ah[1:]], "P": [mat_to_csr(p) for p in Ph], "PT": [mat_to_csr(p, transpose=True) for p in Ph],
            "form": [form(hip, a) for a in Ah], "order": [order(hip, a) for a in Ah], "handles": [a.value for a in Ah + Bh + Ph]}


def build_hierarchy(hip, m, **kw):
    """Reorder mode 1 (the fixture's: every matrix without a fast form, whatever its size) is what re-orders the small level 0 of these
    tests; left on it would re-order small coarse levels as well, which a refresh refuses by design (a re-ordered coarse level contradicts
    its prolongation).  The hierarchy is built under the default mode, in which only matrices of 65 536 rows and more are candidates."""
    hip.g.gcge_hip_spmm_reorder_mode(0)
    try:
        return hip.multigrid(m, **kw)
    finally:
        hip.g.gcge_hip_spmm_reorder_mode(1)


def same_levels(a, b, keys=("A", "P", "PT")):
    assert a["L"] == b["L"]
    for key in keys:
        assert len(a[key]) == len(b[key])
        for l, (x, y) in enumerate(zip(a[key], b[key])):
            same_csr(x, y, (key, l))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["lap3d", "sio2"])
def test_a_hierarchy_over_a_reordered_level_0_is_refreshed_in_place(reorder_on, name):
    hip = reorder_on
    S0, SD = permuted(name, "O"), permuted(name, "D")
    m = create(hip, S0, True)
    h = fresh = None
    try:
        assert order(hip, m) != "as given"
        h = build_hierarchy(hip, m, levels=3)
        built = snapshot(hip, h)
        assert built["L"] == 3 and built["order"][0] != "as given" and all(o == "as given" for o in built["order"][1:]), built["order"]
        assert raw_update(hip, m, SD.data) == 0
        r0 = multigrid_refresh_stats()
        assert h.refresh() is True
        r1 = multigrid_refresh_stats()
        assert (r1[0] - r0[0], r1[1] - r0[1], r1[2] - r0[2]) == (1, 0, built["L"] - 1), (r0, r1)      # a full refresh, no rebuild
        got = snapshot(hip, h)
        assert got["handles"] == built["handles"]            # in place: the same handles
        assert any(not np.array_equal(bits(x[2]), bits(y[2])) for x, y in zip(got["A"], built["A"]))      # the values moved
        fresh = build_hierarchy(hip, m, levels=3)                # built on the updated handle
        want = snapshot(hip, fresh)
        print(name, "forms refreshed", got["form"], "fresh", want["form"])
        same_levels(got, want)
        same_levels(got, built, keys=("P", "PT"))
        assert got["order"] == want["order"] == built["order"]
    finally:
        for k in (h, fresh):
            if k is not None:
                k.close()
        hip.free_matrix(m)


# ---- 5. from torch ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_eigsh_on_a_reordered_handle_after_an_update(reorder_on):
    """lap3d 15 with the generator's values, then with a potential on the diagonal: the update takes a device tensor in the caller's
    entry order.  Each solve stops a pair at ||r|| <= tol |lambda|, and |lambda~ - lambda| <= ||r|| for a unit eigenvector, so a
    converged value lies within tol |lambda| of scipy's (shift-invert at 0: the lowest pairs to rounding)."""
    import scipy.sparse.linalg as sla
    import torch
    from gcge_amd import eigsh
    hip = reorder_on
    c = case("lap3d")
    k, tol = 4, 1e-8
    n = c.S.shape[0]
    S0 = in_callers_order(c.S, c.S.data, c.p)
    v1 = c.S.data.copy()
    v1[c.diag] += 0.5 * np.random.default_rng(23).random(n)
    S1 = in_callers_order(c.S, v1, c.p)
    m = create(hip, S0, True)
    h = None
    try:
        assert order(hip, m) != "as given" and hip.g.gcge_hip_mat_entry_map(m) == 4 * S0.nnz
        h = build_hierarchy(hip, m, levels=3, block_size=4)
        handles = snapshot(hip, h)["handles"]
        cold = eigsh(m, k, tol=tol, amg=h, backend=hip)
        assert hip.matrix_update_values(m, torch.from_numpy(S1.data).cuda())
        assert h.refresh() is True and snapshot(hip, h)["handles"] == handles
        warm = eigsh(m, k, X0=cold.eigenvectors, tol=tol, amg=h, backend=hip)
        for r, S in ((cold, S0), (warm, S1)):
            ref = np.sort(sla.eigsh(S.tocsc(), k=k, sigma=0.0, which="LM", return_eigenvectors=False))
            lam = r.eigenvalues.cpu().numpy()[:k]
            print("iterations", r.iterations, "max relative difference %.2e" % np.max(np.abs(lam - ref) / np.abs(ref)))
            assert r.converged >= k
            assert np.all(np.abs(lam - ref) <= tol * np.abs(ref)), (lam, ref)
        assert warm.iterations <= cold.iterations, (warm.iterations, cold.iterations)
    finally:
        if h is not None:
            h.close()
        hip.free_matrix(m)
