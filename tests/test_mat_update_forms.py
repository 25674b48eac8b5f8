"""New values, in place, for handles with a star or a dense form (gcge_hip_mat_update_values_device through csrc/hip/mat_values_forms.hip;
HipBackend.matrix(..., updatable=True)): the handle keeps where its stored values came from (csrc/hip/value_maps.h) and replays that on
the device.  tests/test_mat_update.py covers the pattern and pad-8 handles and stays as it is.

Four matrices:
  sio2      make_problem("sio2", 24): the 37-point star on 24^3 and the generator's default 8 atoms, two of which overlap — the split has
            two layers of blocks (asserted below through gcge_hip_value_maps_selfcheck's out[1]), so the maps of a later layer, which
            compose with the previous remainder's, are exercised.
  ball      make_problem("sio2ball", 24) with its geometry named (the masked grid: a row map under the sweep)
  star_only make_problem("sio2", 24, K=0): the 37-point star and a diagonal, no atom — every row is clean, the star's remainder and the
            block form under it are empty; the simplest real-space Hamiltonian (a Laplacian and a local potential): the diagonal alone
            can change
  cliques   the 300-row symmetric random structure of tests/test_mat_update.py::random300 plus three cliques: 40 x 40, 48 x 48 and one of
            37 rows and 33 columns (a block of 64 x 40 slots: pad rows and pad columns); no star, dense mode 1

Which entries may change is decided here from the structure and the creation values, the way include/gcge_hip.h states it: an entry at a
star position (its row and column differ along one axis by 1 .. 6 grid points) whose creation value equals the star's coefficient is
pinned; the diagonal and everything else is free.

GPU data is exact: integer matrix entries assigned on the generator's STRUCTURE (one small integer coefficient per axis and distance —
per distance only on the ball, whose sweep takes one coefficient set for all axes —, coefficient + 1 .. 3 at star positions inside atom
rows, small integers elsewhere, an integer diagonal) and integer X in [-4, 4]: every summation order is exact, "entry minus coefficient"
is exact, and products are compared with S_new @ X by np.array_equal."""
import ctypes as C
import functools

import numpy as np
import pytest

from gcge_amd.lib import ball_geometry, csr_to_scipy, hip_lib, make_problem, mat_device_stats, mat_to_csr, mat_update_form_stats, mat_update_stats
from helpers import bits, csr_from_scipy

WIDTHS = (7, 16, 64)
G = 24
SIO2 = dict(K=8, R0=1.5, R1=3.0)
NAMES = ("sio2", "ball", "cliques")
ALL_NAMES = NAMES + ("star_only",)
ip_, dp_ = C.POINTER(C.c_int), C.POINTER(C.c_double)


# ---- the matrices -----------------------------------------------------------------------------------------------------------------------
def cliques300():
    import scipy.sparse as sp
    from test_mat_update import random300
    S = random300().tolil()
    rng = np.random.default_rng(37)
    idx = rng.permutation(300)
    for lo, hi in ((0, 40), (40, 88)):                       # two symmetric cliques: rows = columns
        I = np.sort(idx[lo:hi])
        for i in I:
            for j in I:
                if i != j:
                    S[i, j] = -(1.0 + (i + j) % 3)
    R, Cc = np.sort(idx[88:125]), np.sort(idx[125:158])       # 37 rows that all hold the same 33 columns ...
    for i in R:
        for j in Cc:
            S[i, j] = -(1.0 + (i + 2 * j) % 3)
    for j in R[1:]:                                           # ... and the longest of them names the others (the search finds rows through a seed's columns)
        S[R[0], j] = -2.0
    S = S.tocsr()
    S.sort_indices()
    return S


class Case:
    """S: creation values as the generator made them (sorted CSR); star: bool mask of the entries at star positions and their
    (axis, distance) codes; pinned / diag masks; dims, box: the geometry to name (None: none)"""


@functools.lru_cache(maxsize=None)
def case(name):
    c = Case()
    c.name, c.dims, c.box, c.dense_mode = name, None, None, 0
    if name == "cliques":
        c.S, c.dense_mode = cliques300(), 1
    else:
        kw = dict(SIO2, K=0) if name == "star_only" else SIO2
        c.S = csr_to_scipy(make_problem("sio2ball" if name == "ball" else "sio2", G, **kw)[0]).tocsr()
        c.S.sort_indices()
    S = c.S
    n = S.shape[0]
    c.rows, c.cols = np.repeat(np.arange(n), np.diff(S.indptr)), S.indices
    c.diag = c.rows == c.cols
    c.star = np.zeros(S.nnz, dtype=bool)
    c.axis, c.dist = np.zeros(S.nnz, dtype=np.int64), np.zeros(S.nnz, dtype=np.int64)
    c.pinned = np.zeros(S.nnz, dtype=bool)
    if name != "cliques":
        box = ball_geometry(G).astype(np.int64) if name == "ball" else np.arange(n, dtype=np.int64)
        if name == "ball":
            c.dims, c.box = (G, G, G), box.astype(np.int32)
        xyz = np.stack([box % G, (box // G) % G, box // (G * G)], axis=1)
        d = xyz[c.cols] - xyz[c.rows]
        one = (d != 0).sum(axis=1) == 1
        c.axis = np.argmax(d != 0, axis=1)
        c.dist = np.abs(d).sum(axis=1)
        c.star = one & (c.dist >= 1) & (c.dist <= 6)
        for a in range(3):                                   # the star's coefficients: the value most entries of an (axis, distance) carry
            for k in range(1, 7):
                sel = c.star & (c.axis == a) & (c.dist == k)
                vals, cnt = np.unique(bits(S.data[sel]), return_counts=True)
                c.pinned |= sel & (bits(S.data) == vals[np.argmax(cnt)])
    c.free = ~c.pinned & ~c.diag
    return c


def real_values(c, step):
    """the generator's values with a potential on the diagonal and the free entries scaled: step 0 is the creation matrix"""
    v = c.S.data.copy()
    if step:
        v[c.diag] += 0.25 * step * (1.0 + (c.rows[c.diag] % 11))
        v[c.free] *= 1.0 + 0.25 * step
    return v


def integer_values(c, kind):
    """O: the creation values; D: another diagonal; B: another diagonal and another value in every free entry"""
    r, q = c.rows, c.cols
    coef = (1 + c.dist + (0 if c.name == "ball" else 2 * c.axis)).astype(np.float64)          # 2 .. 11, the same for +k and -k
    bump = {"O": 0, "D": 0, "B": 1}[kind]
    v = -(1.0 + (r + q + bump) % 3)                                                             # -1 .. -3 elsewhere
    v = np.where(c.star, np.where(c.pinned, -coef, -coef + 1.0 + (r + q + bump) % 3), v)
    v = np.where(c.diag, 40.0 + (r + (3 if kind != "O" else 0)) % 7 + (5 * r) % 3 * (kind != "O"), v)
    return v.astype(np.float64)


def with_values(c, v):
    S = c.S.copy()
    S.data = np.ascontiguousarray(v, dtype=np.float64)
    return S


def S_nnz_bytes(c):
    """bytes of maps of a star whose remainder is empty: 1 per CSR entry, 4 per row"""
    return c.S.nnz + 4 * c.S.shape[0]


# ---- CPU: the maps replayed on the host --------------------------------------------------------------------------------------------------
def selfcheck(c, v0, v1):
    g = hip_lib()
    S = c.S
    rp, ci = np.ascontiguousarray(S.indptr, dtype=np.int32), np.ascontiguousarray(S.indices, dtype=np.int32)
    v0, v1 = np.ascontiguousarray(v0, dtype=np.float64), np.ascontiguousarray(v1, dtype=np.float64)
    out = (C.c_long * 4)()
    a = (S.shape[0], rp.ctypes.data_as(ip_), ci.ctypes.data_as(ip_), v0.ctypes.data_as(dp_), v1.ctypes.data_as(dp_), c.dense_mode)
    if c.box is not None:
        bad = g.gcge_hip_value_maps_selfcheck_grid(*a, c.dims[0], c.dims[1], c.dims[2], c.box.ctypes.data_as(ip_), out)
    else:
        bad = g.gcge_hip_value_maps_selfcheck(*a, out)
    return bad, list(out)


@pytest.mark.parametrize("values", ["real", "integer"])
@pytest.mark.parametrize("name", ALL_NAMES)
def test_maps_replayed_on_the_host_reproduce_the_new_rows(name, values):
    c = case(name)
    v0, v1 = (real_values(c, 0), real_values(c, 2)) if values == "real" else (integer_values(c, "O"), integer_values(c, "B"))
    changed = bits(v0) != bits(v1)
    assert np.all(changed[c.diag]) and np.all(changed[c.free]) and not np.any(changed[c.pinned])
    bad, out = selfcheck(c, v0, v1)
    print(name, values, "differing entries", bad, "forms", out[0], "layers", out[1], "pinned", out[2], "bytes of maps", out[3])
    assert bad == 0, (bad, out)
    assert out[0] == {"cliques": 2, "star_only": 1}.get(name, 3) and out[3] > 0, out
    assert out[2] == int(c.pinned.sum()), (out, int(c.pinned.sum()))
    if name == "star_only":
        assert out[1] == 0 and not np.any(c.free) and out[3] == S_nnz_bytes(c), out            # no block, nothing free: pins, diagonal sources
    if name == "sio2":
        assert out[1] >= 2, out                               # a second layer of blocks: the maps compose
    if name == "cliques":
        assert out[1] == 1 and out[3] >= 4 * (64 * 40 + 64 * 40 + 64 * 48), out     # 37 x 33 -> 64 x 40 slots, 40 x 40 -> 64 x 40, 48 x 48 -> 64 x 48
    assert selfcheck(c, v0, v0)[0] == 0                       # the identity update


def test_the_setter_returns_the_setting_it_replaces():
    g = hip_lib()
    assert g.gcge_hip_mat_keep_value_maps(1) == 0 and g.gcge_hip_mat_keep_value_maps(1) == 1 and g.gcge_hip_mat_keep_value_maps(0) == 1
    assert g.gcge_hip_mat_keep_value_maps(0) == 0


@pytest.mark.parametrize("name", ["sio2", "ball"])
def test_a_changed_pinned_entry_is_a_decline_on_the_host(name):
    c = case(name)
    v0 = real_values(c, 0)
    S = c.S
    npin = np.add.reduceat(c.pinned.astype(np.int64), S.indptr[:-1])
    nfree = np.add.reduceat(c.free.astype(np.int64), S.indptr[:-1])
    clean = np.flatnonzero((npin == 36) & (nfree == 0))       # an interior star row: nothing but the star and a diagonal
    mixed = np.flatnonzero((npin > 0) & (nfree > 0))          # a row inside an atom that still carries star entries
    assert clean.size and mixed.size
    for r in (clean[clean.size // 2], mixed[mixed.size // 2]):
        q = S.indptr[r] + np.flatnonzero(c.pinned[S.indptr[r]:S.indptr[r + 1]])[0]
        v1 = real_values(c, 1)
        v1[q] = np.nextafter(v1[q], 0.0)
        assert selfcheck(c, v0, v1)[0] == -2, r
    v1 = real_values(c, 1)
    v1[np.flatnonzero(c.diag)[5]] = np.nan
    assert selfcheck(c, v0, v1)[0] == -2


def test_no_form_no_maps():
    c = Case()
    c.S, c.dense_mode, c.box = csr_to_scipy(make_problem("lap3d", 6)[0]).tocsr(), 0, None
    c.S.sort_indices()
    assert selfcheck(c, c.S.data, c.S.data * 2.0)[0] == -1


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------------
def create(hip, c, v, updatable, device=False):
    import torch
    S = with_values(c, v)
    hip.g.gcge_hip_spmm_dense_mode(c.dense_mode)
    try:
        if c.box is not None:
            A, keep = csr_from_scipy(S)
            return hip.matrix_grid(A, c.dims, c.box, updatable=updatable)
        if device:
            t = tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data))
            return hip.matrix_from_device(*t, updatable=updatable)
        A, keep = csr_from_scipy(S)
        return hip.matrix(A, updatable=updatable)
    finally:
        hip.g.gcge_hip_spmm_dense_mode(0)


def form(hip, m):
    return hip.g.gcge_hip_mat_spmm_form(m).decode()


def form_stats(hip, m):
    out = (C.c_double * 12)()
    hip.g.gcge_hip_mat_form_stats(m, out)
    return tuple(out)


_X = {}


def x_block(n):
    if n not in _X:
        _X[n] = np.random.default_rng(9 + n).integers(-4, 5, (n, max(WIDTHS))).astype(np.float64)
    return _X[n]


def products(hip, m, n):
    X, out = x_block(n), []
    for w in WIDTHS:
        xh, yh = hip.mv_from_numpy(m, X[:, :w]), hip.mv_from_numpy(m, np.full((n, w), 5.0))
        hip.ops.spmm(m, xh, yh, (0, 0), (w, w))
        out.append(hip.mv_to_numpy(yh, n, 0, w))
        hip.ops.mv_destroy(xh, w)
        hip.ops.mv_destroy(yh, w)
    return out


def check_products(hip, m, S, what):
    n, X = S.shape[0], x_block(S.shape[0])
    for w, y in zip(WIDTHS, products(hip, m, n)):
        assert np.array_equal(y, S @ X[:, :w]), (what, "width", w, np.argwhere(y != S @ X[:, :w])[:4].tolist())
    rp, ci, va = mat_to_csr(m)
    assert np.array_equal(rp, S.indptr) and np.array_equal(ci, S.indices) and np.array_equal(bits(va), bits(S.data)), (what, "gcge_hip_mat_to_csr")


def raw_update(hip, m, values):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(values, dtype=np.float64)).cuda()
    torch.cuda.synchronize()
    return hip.g.gcge_hip_mat_update_values_device(m, int(t.numel()), t.data_ptr())


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["D", "B"])
@pytest.mark.parametrize("name", NAMES)
def test_accepted_updates(hip, name, kind):
    c = case(name)
    S0, S1 = with_values(c, integer_values(c, "O")), with_values(c, integer_values(c, kind))
    changed = bits(S0.data) != bits(S1.data)
    assert np.all(changed[c.diag]) and not np.any(changed[c.pinned]) and bool(np.all(changed[c.free])) == (kind == "B")
    m = create(hip, c, S0.data, True)
    try:
        f0, fs0 = form(hip, m), form_stats(hip, m)
        assert ("spmm_star" in f0) == (name != "cliques") and "spmm_dense" in f0 and f0.endswith("spmm_pad8"), f0
        nbytes = hip.g.gcge_hip_mat_value_maps(m)
        assert nbytes > 0
        check_products(hip, m, S0, "before")
        for step, Snew in enumerate((S1, S0)):
            u0, f_0, d0 = mat_update_stats(), mat_update_form_stats(), mat_device_stats()
            rc = raw_update(hip, m, Snew.data)
            u1, f_1 = mat_update_stats(), mat_update_form_stats()
            du, df = tuple(b - a for a, b in zip(u0, u1)), tuple(b - a for a, b in zip(f_0, f_1))
            print(name, kind, "step", step, f0, "bytes of maps", nbytes, "update stats", du, "form stats", df)
            assert rc == 0
            assert form(hip, m) == f0 and form_stats(hip, m) == fs0 and hip.g.gcge_hip_mat_value_maps(m) == nbytes
            assert du[:5] == (1, 0, 0, 0, 0) and 0 <= du[5] <= 4, du                 # kept, no decline; at most one flag word came back
            assert df == ((1, 0, 0, 0) if name != "cliques" else (0, 1, 0, 0)), df
            assert mat_device_stats() == d0
            check_products(hip, m, Snew, "after update %d" % step)
    finally:
        hip.free_matrix(m)


@pytest.mark.gpu
def test_a_star_without_blocks_takes_a_new_diagonal(hip):
    """every row clean: the block form under the star has no slot at all, the handle still holds maps (pins, diagonal sources) and
    takes a new diagonal; a changed star entry declines.  A switch the caller turned on survives a creation with updatable=True."""
    c = case("star_only")
    S0, S1 = with_values(c, integer_values(c, "O")), with_values(c, integer_values(c, "D"))
    assert np.all((bits(S0.data) != bits(S1.data)) == c.diag) and not np.any(c.free)
    assert hip.g.gcge_hip_mat_keep_value_maps(1) == 0
    try:
        m = create(hip, c, S0.data, True)
        assert hip.g.gcge_hip_mat_keep_value_maps(1) == 1                      # still on: restored, not switched off
    finally:
        hip.g.gcge_hip_mat_keep_value_maps(0)
    try:
        f0 = form(hip, m)
        assert "spmm_star" in f0, f0
        assert hip.g.gcge_hip_mat_value_maps(m) == S_nnz_bytes(c), (hip.g.gcge_hip_mat_value_maps(m), S_nnz_bytes(c))
        check_products(hip, m, S0, "before")
        for step, Snew in enumerate((S1, S0)):
            u0, g0 = mat_update_stats(), mat_update_form_stats()
            assert raw_update(hip, m, Snew.data) == 0
            du = tuple(b - a for a, b in zip(u0, mat_update_stats()))
            assert du[:5] == (1, 0, 0, 0, 0) and du[5] <= 4, du
            assert tuple(b - a for a, b in zip(g0, mat_update_form_stats())) == (1, 0, 0, 0)
            assert form(hip, m) == f0
            check_products(hip, m, Snew, "after update %d" % step)
        v1 = S1.data.copy()
        v1[np.flatnonzero(c.pinned)[c.S.nnz // 3]] += 1.0
        check_decline(hip, m, c, v1, 4, (0, 0, 1, 0))
        check_products(hip, m, S0, "after the decline")
    finally:
        hip.free_matrix(m)


def fused_cg(hip, m, Bm, iters):
    """one fused block-CG call of exactly `iters` iterations from x0 = 0 (a rate no residual reaches)"""
    g = hip.g
    n, nrhs = Bm.shape
    g.gcge_hip_bpcg_setup(hip.ops_handle, iters, 1e-300, 0.0, b"abs")
    try:
        b, x = hip.mv_from_numpy(m, Bm), hip.mv_from_numpy(m, np.zeros((n, nrhs)))
        hip.ops.multi_linear_solver(m, b, x, (0, 0), (nrhs, nrhs))
        it = C.c_int()
        g.gcge_hip_bpcg_stats(None, None, C.byref(it))
        out = hip.mv_to_numpy(x, n, 0, nrhs)
        hip.ops.mv_destroy(b, nrhs)
        hip.ops.mv_destroy(x, nrhs)
    finally:
        g.gcge_hip_bpcg_setup(hip.ops_handle, 30, 1e-2, 1e-14, b"abs")
    return out, it.value


@pytest.mark.gpu
def test_an_updated_handle_is_a_fresh_handle_bit_for_bit(hip):
    """sio2 with the generator's own (non-integer) values: a potential on the diagonal, the free entries times 1.25 — a fresh split of
    the new values has the same structure, so products and a fused-CG call through the updated handle equal those through a handle
    created from the new values, with the switch on AND off (the maps do not change the forms)."""
    from helpers import uniform
    c = case("sio2")
    v0, v1 = real_values(c, 0), real_values(c, 1)
    n = c.S.shape[0]
    Bm = uniform(73, (n, 16)) - 0.5
    m = create(hip, c, v0, True)
    fresh = []
    try:
        assert raw_update(hip, m, v1) == 0
        assert np.array_equal(bits(mat_to_csr(m)[2]), bits(v1))
        pm, (xm, itm) = products(hip, m, n), fused_cg(hip, m, Bm, 8)
        assert itm == 8 and np.all(np.isfinite(xm))
        for updatable in (True, False):
            f = create(hip, c, v1, updatable)
            fresh.append(f)
            assert form(hip, f) == form(hip, m) and form_stats(hip, f) == form_stats(hip, m)
            assert (hip.g.gcge_hip_mat_value_maps(f) > 0) == updatable
            if updatable:
                assert hip.g.gcge_hip_mat_value_maps(f) == hip.g.gcge_hip_mat_value_maps(m)
            for w, a, b in zip(WIDTHS, pm, products(hip, f, n)):
                assert np.array_equal(bits(a), bits(b)), ("updatable", updatable, "width", w)
            xf, itf = fused_cg(hip, f, Bm, 8)
            assert itf == 8 and np.array_equal(bits(np.ascontiguousarray(xm)), bits(np.ascontiguousarray(xf))), ("fused CG, updatable", updatable)
    finally:
        hip.free_matrix(m)
        for f in fresh:
            hip.free_matrix(f)


def check_decline(hip, m, c, values, moved_at_most, form_delta):
    n = c.S.shape[0]
    before, csr0, f0, fs0 = products(hip, m, n), mat_to_csr(m), form(hip, m), form_stats(hip, m)
    u0, g0, d0 = mat_update_stats(), mat_update_form_stats(), mat_device_stats()
    rc = raw_update(hip, m, values)
    u1, g1 = mat_update_stats(), mat_update_form_stats()
    assert rc == 1, rc
    du = tuple(b - a for a, b in zip(u0, u1))
    assert du[:5] == (0, 0, 0, 1, 0) and 0 <= du[5] <= moved_at_most, du
    assert tuple(b - a for a, b in zip(g0, g1)) == form_delta, (g0, g1)
    assert mat_device_stats() == d0 and form(hip, m) == f0 and form_stats(hip, m) == fs0
    for w, a, b in zip(WIDTHS, before, products(hip, m, n)):
        assert np.array_equal(bits(a), bits(b)), w
    for a, b in zip(csr0, mat_to_csr(m)):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sio2", "ball"])
def test_declines_write_nothing(hip, name):
    c = case(name)
    S = c.S
    v0 = integer_values(c, "O")
    npin = np.add.reduceat(c.pinned.astype(np.int64), S.indptr[:-1])
    nfree = np.add.reduceat(c.free.astype(np.int64), S.indptr[:-1])
    clean, block = np.flatnonzero((npin == 36) & (nfree == 0)), np.flatnonzero((npin > 0) & (nfree > 50))
    assert clean.size and block.size
    m = create(hip, c, v0, True)
    try:
        for r in (clean[clean.size // 2], block[block.size // 2]):             # a pinned entry of a clean row, of a block row
            v1 = integer_values(c, "B")
            q = S.indptr[r] + np.flatnonzero(c.pinned[S.indptr[r]:S.indptr[r + 1]])[-1]
            v1[q] += 1.0
            check_decline(hip, m, c, v1, 4, (0, 0, 1, 0))
        v1 = integer_values(c, "B")
        v1[np.flatnonzero(c.diag)[S.shape[0] // 3]] = np.nan
        check_decline(hip, m, c, v1, 4, (0, 0, 0, 1))
        check_products(hip, m, with_values(c, v0), "after the declines")
        assert raw_update(hip, m, integer_values(c, "B")) == 0                 # and the handle still takes an update
        check_products(hip, m, with_values(c, integer_values(c, "B")), "an update after the declines")
    finally:
        hip.free_matrix(m)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL_NAMES)
def test_a_handle_without_maps_declines_from_the_handle_alone(hip, name):
    c = case(name)
    v0 = integer_values(c, "O")
    m = create(hip, c, v0, False)
    try:
        assert ("spmm_star" in form(hip, m)) == (name != "cliques") and "spmm_dense" in form(hip, m), form(hip, m)
        assert hip.g.gcge_hip_mat_value_maps(m) == 0
        check_decline(hip, m, c, integer_values(c, "D"), 0, (0, 0, 0, 0))
    finally:
        hip.free_matrix(m)


@pytest.mark.gpu
def test_a_tile_form_declines_even_with_maps(hip):
    c = case("cliques")
    v0 = integer_values(c, "O")
    hip.g.gcge_hip_spmm_tile_mode(1)
    m = None
    try:
        m = create(hip, c, v0, True)
        print("form with the tile path on:", form(hip, m), "bytes of maps", hip.g.gcge_hip_mat_value_maps(m))
        assert "spmm_tile" in form(hip, m), form(hip, m)
        assert hip.g.gcge_hip_mat_value_maps(m) > 0                          # the maps are there: it is the tile form that declines
        check_decline(hip, m, c, integer_values(c, "D"), 0, (0, 0, 0, 0))
    finally:
        hip.g.gcge_hip_spmm_tile_mode(0)
        if m is not None:
            hip.free_matrix(m)


@pytest.mark.gpu
def test_eigsh_over_three_potentials_on_one_star_handle(hip):
    """sio2 + t v on the diagonal, t = 0, 1, 2: one handle from matrix_from_device(updatable=True), warm starts; every step against eigsh
    on a fresh handle of the same values.  Both solves stop a pair at ||r|| <= tol |lambda| (tol = 1e-8) and |lambda~ - lambda| <=
    ||r|| for a unit eigenvector, so two converged solves of one matrix differ by at most 2 tol |lambda|."""
    import torch
    from gcge_amd import eigsh
    c = case("sio2")
    k, tol = 4, 1e-8
    n = c.S.shape[0]
    pot = np.random.default_rng(23).random(n)
    dev = lambda v: tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (c.S.indptr.astype(np.int32), c.S.indices.astype(np.int32), v))
    m = hip.matrix_from_device(*dev(c.S.data), updatable=True)
    try:
        assert "spmm_star" in form(hip, m) and hip.g.gcge_hip_mat_value_maps(m) > 0
        g0, u0 = mat_update_form_stats(), mat_update_stats()
        r = None
        for t in range(3):
            v = c.S.data.copy()
            v[c.diag] += 0.5 * t * pot
            if t:
                assert hip.matrix_update_values(m, torch.from_numpy(v).cuda())
            r = eigsh(m, k, X0=None if r is None else r.eigenvectors, tol=tol, backend=hip)
            f = hip.matrix_from_device(*dev(v))
            try:
                rf = eigsh(f, k, tol=tol, backend=hip)
            finally:
                hip.free_matrix(f)
            lam, lamf = r.eigenvalues.cpu().numpy(), rf.eigenvalues.cpu().numpy()
            print("step", t, "iterations", r.iterations, rf.iterations, "max relative difference %.2e" % np.max(np.abs(lam - lamf) / np.abs(lamf)))
            assert r.converged >= k and rf.converged >= k
            assert np.all(np.abs(lam - lamf) <= 2.0 * tol * np.abs(lamf)), (lam, lamf)
        g1, u1 = mat_update_form_stats(), mat_update_stats()
        assert tuple(b - a for a, b in zip(g0, g1)) == (2, 0, 0, 0), (g0, g1)
        assert u1[3] == u0[3]
    finally:
        hip.free_matrix(m)
