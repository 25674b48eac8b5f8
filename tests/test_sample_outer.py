"""gcge_hip_csr_sample_outer (csrc/hip/sample_outer.hip: one kernel template, sample_outer<LPE, CPL, MULTI>) over ROW STRUCTURES, column
counts and layouts, through its raw-pointer entry, on EXACT data: the entries of U, V and w are nonzero integers of magnitude <= 3
and k <= 258, so every product is an integer of magnitude <= 27, every sum one of magnitude <= 27 * 258 * |alpha| < 2^32, and any
order of summation gives the same double.  The reference is numpy on the same arrays and the comparison np.array_equal: a column
that is dropped, taken twice or read from the neighbouring row or entry changes an output by a nonzero integer (up to
cancellation, which the three weights, alpha and the 2^40 beside the operands make unlikely in every case at once).
(test_refusals_and_the_premise checks the premise on the host.)

U and V sit in blocks with 2^40 in the columns beside the operand and in the rows behind it; the output in a vector filled with a
payload NaN that must come back bit for bit round the nnz entries.

Row structures (TABLE, built once): uniform lengths 0, 1, 7, 27, 64, 65, 300, mixed tables with empty rows first, last and between
long rows at the row counts 1, 2, 63, 64, 65, 257, matrices of empty rows only.  Columns are unsorted, repeat inside a row and hit
the first and the last row of V; V has as many rows as U ("square": U and V may be one block), 3 n + 1 or (n - 1) // 3.
Column counts K: the issue's 1, 2, 3, 8, 31, 32, 33, 64, 65, 127, 128, 129, 258 and 16, without which two of the sixteen kernels
would not be launched.  Layouts: ld == k (a block of its own), even ld > k on a 16-byte origin, an origin one double off, odd ld;
d_w NULL and given; alpha 1, -1, 2.

The launch arithmetic, restated in so_branch / piece_features and checked in test_the_case_table_reaches_the_branches:
  gcge_hip_csr_sample_outer   CPL = 2 (16-byte loads) when ldu and ldv are even and U and V start on 16 bytes, else 1;
                              LPE = the power of two >= ceil(k / CPL), at most 64; MULTI (chunks of 64 CPL columns) when k > 64 CPL.
  sample_outer                a wave takes 16 rows and cuts their entries into G = 64 / LPE contiguous pieces of ceil(total / G)
                              entries; a group walks its piece row by row in batches of 4 entries and stores every LPE results
                              (and what is left at the piece's end) at once; a block is 4 waves.
"""
import numpy as np
import pytest

from gcge_amd import abi
from helpers import IN_GUARD, LAYOUTS, OUT_GUARD, Block, bits, check_vec, draw, out_vec, uniform

ROWS = [1, 2, 63, 64, 65, 257]
UNIFORM = [0, 1, 7, 27, 64, 65, 300]
K = [1, 2, 3, 8, 16, 31, 32, 33, 64, 65, 127, 128, 129, 258]
ISSUE_K = [1, 2, 3, 8, 31, 32, 33, 64, 65, 127, 128, 129, 258]
MIX = [0, 0, 70, 0, 3, 300, 2, 8, 64, 1, 0, 129, 7, 9, 50, 6, 0, 65, 4, 16, 0, 0, 5, 27, 17, 63, 15]
WMAX = 258
ALPHAS = [1.0, -1.0, 2.0]
ROWS_PER_WAVE, UNROLL = 16, 4
TIGHT = "tight"                                      # the layout ld == k; the others are helpers.LAYOUTS
ALL_LAYOUTS = [TIGHT] + LAYOUTS
U_ROUND = 2.0 ** -53


def cdiv(a, b):
    return -(-a // b)


# ---- the patterns -----------------------------------------------------------------------------------------------------------------
class Pattern:
    """One row structure with its data: CSR arrays, U (nrows x WMAX), V (ncols x WMAX), w (WMAX)"""

    def __init__(self, name, lens, shape, seed):
        lens = np.asarray(lens, dtype=np.int64)
        n = lens.size
        self.name, self.nrows, self.shape, self.lens, self.seed = name, n, shape, lens, seed
        self.ncols = {"square": n, "wide": 3 * n + 1, "tall": max(1, (n - 1) // 3)}[shape]
        self.rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        nnz = self.nnz = int(self.rowptr[-1])
        rng = np.random.default_rng(seed)
        col = rng.integers(0, self.ncols, nnz)                     # unsorted; repeats happen and are forced below
        first = self.rowptr[:-1][lens >= 2][::2]
        col[first + 1] = col[first]                                # a repeated column at the head of every other row of >= 2 entries
        if nnz:
            col[0], col[nnz // 2], col[-1] = 0, self.ncols - 1, self.ncols - 1     # the first and the last row of V
        self.col = col.astype(np.int32)
        self.row_of = np.repeat(np.arange(n), lens)
        self.U, self.V, self.w = draw(seed + 1, (n, WMAX), False), draw(seed + 2, (self.ncols, WMAX), False), draw(seed + 3, (WMAX,), False)
        self._ref = {}

    def ref(self, k, weighted, same=False):
        """sum_c w_c U[i, c] V[j, c] over the entries (alpha = 1; V = U with same), computed once"""
        key = (k, weighted, same)
        if key not in self._ref:
            V = self.U if same else self.V
            w = self.w[:k] if weighted else np.ones(k)
            self._ref[key] = np.einsum("ec,ec,c->e", self.U[self.row_of, :k], V[self.col, :k], w) if self.nnz else np.zeros(0)
        return self._ref[key]


def build_table():
    t, seed = [], 7000
    shapes = ("square", "wide", "tall")
    for i, ln in enumerate(UNIFORM):                               # every uniform length at two row counts (300: the small ones)
        for j in (0, 1):
            n = ROWS[(2 * i + 3 * j + 2) % len(ROWS)] if ln < 300 else (2, 65)[j]
            seed += 10
            t.append(Pattern("len%d_n%d" % (ln, n), [ln] * n, shapes[(i + j) % 3], seed))
    for i, n in enumerate(ROWS):                                   # every row count with mixed lengths, square and one other shape
        for k, shape in enumerate(("square", shapes[1 + i % 2])):
            lens = [MIX[(q + 5 * i + 3 * k) % len(MIX)] for q in range(n)]
            if n >= 3:
                lens[0], lens[1], lens[-1] = 0, 0, 0               # empty rows first and last (the pattern puts them between long rows)
            seed += 10
            t.append(Pattern("mix_n%d_%s" % (n, shape), lens, shape, seed))
    for n, shape in ((1, "square"), (65, "wide"), (257, "square")):
        seed += 10
        t.append(Pattern("empty_n%d" % n, [0] * n, shape, seed))
    return t


TABLE = build_table()
BY_NAME = {a.name: a for a in TABLE}
MIXED = BY_NAME["mix_n65_square"]


# ---- the launch arithmetic restated -------------------------------------------------------------------------------------------------
def takes_pairs(lu, lv, k):
    """16-byte loads: both leading dimensions even, both origins on 16 bytes (helpers.Block: gl columns in front, ld of parity
    layout[1]; a block of its own starts on an allocation)"""
    def ok(layout):
        return k % 2 == 0 if layout == TIGHT else (layout[0] % 2 == 0 and layout[1] == 0)
    return ok(lu) and ok(lv)


def so_branch(k, pairs):
    """(LPE, CPL, MULTI, chunks) of gcge_hip_csr_sample_outer"""
    cpl = 2 if pairs else 1
    need = cdiv(k, cpl)
    lpe = 1
    while lpe < min(need, 64):
        lpe *= 2
    return lpe, cpl, need > 64, cdiv(k, 64 * cpl) if need > 64 else 1


def piece_features(lens, lpe):
    """what the groups of the waves of 16 rows meet when they walk their pieces"""
    f = set()
    G = 64 // lpe
    lens = np.asarray(lens)
    for r0 in range(0, len(lens), ROWS_PER_WAVE):
        w = lens[r0:r0 + ROWS_PER_WAVE]
        ends = np.concatenate([[0], np.cumsum(w)])
        tot = int(ends[-1])
        if len(w) < ROWS_PER_WAVE:
            f.add("short_wave")
        if tot == 0:
            f.add("all_empty")
            continue
        per = cdiv(tot, G)
        for g in range(G):
            gs, ge = min(tot, g * per), min(tot, g * per + per)
            if gs >= ge:
                f.add("idle_group")
                continue
            if g > 0 and gs not in ends:
                f.add("piece_starts_inside_a_row")
            if ge - gs >= lpe:
                f.add("full_store")
            if (ge - gs) % lpe:
                f.add("partial_store")
            rows = [r for r in range(len(w)) if ends[r] < ge and ends[r + 1] > gs]
            if any(w[r] == 0 for r in range(rows[0], rows[-1])):
                f.add("empty_rows_inside_a_piece")
            if len(rows) > 1:
                f.add("rows_change_inside_a_piece")
            for r in rows:
                seg = min(ends[r + 1], ge) - max(ends[r], gs)
                f.add("masked_batch" if seg % UNROLL else "whole_batches")
                if seg > UNROLL:
                    f.add("several_batches")
        if G > 1 and any(x > per for x in w):
            f.add("row_over_several_groups")
    return f


# ---- 1. the refusals, the premise and the table's reach, on the host ------------------------------------------------------------------
def test_refusals_and_the_premise():
    """every refusal returns -1 from the loaded library without a device (nothing is dereferenced: the pointers are made up), nrows == 0
    returns 0; the data are nonzero integers of magnitude <= 3, the float64 reference equals the same sums in int64 and stays far
    below 2^32"""
    from gcge_amd.lib import hip_lib
    fn = hip_lib().gcge_hip_csr_sample_outer
    p = 4096                                                        # (never read: the arguments are refused on the host)
    good = dict(nrows=5, rp=p, ci=p, u=p, ldu=8, v=p, ldv=8, k=8, w=p, alpha=1.0, out=p)

    def call(**kw):
        a = dict(good, **kw)
        return fn(a["nrows"], a["rp"], a["ci"], a["u"], a["ldu"], a["v"], a["ldv"], a["k"], a["w"], a["alpha"], a["out"], None)
    assert call(nrows=-1) == -1 and call(k=0) == -1 and call(k=-3) == -1 and call(ldu=7) == -1 and call(ldv=7) == -1
    for name in ("rp", "ci", "u", "v", "out"):
        assert call(**{name: None}) == -1, name
    assert call(nrows=0) == 0 and call(nrows=0, rp=None, ci=None, u=None, v=None, out=None, w=None) == 0
    assert call(nrows=0, k=0) == -1 and call(nrows=0, ldu=7) == -1 and call(nrows=-1, rp=None) == -1
    for a in TABLE:
        for x in (a.U, a.V, a.w):
            assert np.all(x == np.round(x)) and np.all(np.abs(x) <= 3) and np.all(x != 0)
        assert a.col.size < 3 or (a.col.min() == 0 and a.col.max() == a.ncols - 1)
        for k in (1, 33, 258):
            ri = np.einsum("ec,ec,c->e", a.U[a.row_of, :k].astype(np.int64), a.V[a.col, :k].astype(np.int64), a.w[:k].astype(np.int64))
            assert np.array_equal(a.ref(k, True), ri) and np.max(np.abs(ri), initial=0) <= 27 * k
    assert 27 * WMAX * max(abs(x) for x in ALPHAS) < 2 ** 32 and max(K) <= WMAX and set(K) >= set(ISSUE_K)
    rows_of = lambda a: [a.col[a.rowptr[r]:a.rowptr[r + 1]] for r in range(a.nrows)]
    assert any(np.any(np.diff(c) < 0) for c in rows_of(MIXED)) and any(np.unique(c).size < c.size for c in rows_of(MIXED))
    assert {a.nrows for a in TABLE} >= set(ROWS) and {int(l) for a in TABLE for l in a.lens} >= set(UNIFORM)
    for ln in UNIFORM:
        assert sum(1 for a in TABLE if a.lens.size and np.all(a.lens == ln)) >= 2, ln
    for a in TABLE:
        if a.name.startswith("mix") and a.nrows >= 63:
            nz = np.nonzero(a.lens)[0]
            assert a.lens[0] == 0 and a.lens[-1] == 0 and np.any(a.lens[nz[0]:nz[-1]] == 0) and a.lens.max() == 300


def test_the_case_table_reaches_the_branches():
    """the launch arithmetic of sample_outer.hip restated: every one of the sixteen kernels is launched, and under every LPE the
    table meets what a piece can meet"""
    # the dispatch: K x layouts reach every (LPE, CPL, MULTI)
    seen = {so_branch(k, takes_pairs(lu, lv, k))[:3] for k in K for lu in ALL_LAYOUTS for lv in ALL_LAYOUTS}
    want = {(l, c, False) for l in (1, 2, 4, 8, 16, 32, 64) for c in (1, 2)} | {(64, 1, True), (64, 2, True)}
    assert seen == want, (want - seen, seen - want)
    assert so_branch(128, True) == (64, 2, False, 1) and so_branch(129, True) == (64, 2, True, 2) and so_branch(258, True) == (64, 2, True, 3)
    assert so_branch(64, False) == (64, 1, False, 1) and so_branch(65, False) == (64, 1, True, 2) and so_branch(258, False) == (64, 1, True, 5)
    assert so_branch(3, True) == (2, 2, False, 1) and so_branch(33, True) == (32, 2, False, 1) and so_branch(31, False) == (32, 1, False, 1)
    # an odd k with pairs reads one double past the operand and must drop it; a chunk that ends inside the lanes
    assert any(k % 2 and takes_pairs(LAYOUTS[0], LAYOUTS[0], k) for k in K) and 258 % 128 == 2 and 129 % 128 == 1 and 65 % 64 == 1
    # the layouts: pairs lost through U alone, through V alone, an odd origin, an odd ld; ld == k with an even and an odd k
    assert takes_pairs(LAYOUTS[0], LAYOUTS[0], 7) and not takes_pairs(LAYOUTS[1], LAYOUTS[0], 8) and not takes_pairs(LAYOUTS[0], LAYOUTS[2], 8)
    assert takes_pairs(TIGHT, TIGHT, 8) and not takes_pairs(TIGHT, TIGHT, 3) and not takes_pairs(TIGHT, LAYOUTS[3], 8)
    assert {(gl % 2, par) for gl, par in LAYOUTS} == {(0, 0), (1, 0), (0, 1), (1, 1)}
    # the pieces
    for lpe in (1, 2, 4, 8, 16, 32, 64):
        seen = set()
        for a in TABLE:
            seen |= piece_features(a.lens, lpe)
        need = {"short_wave", "all_empty", "full_store", "partial_store", "empty_rows_inside_a_piece", "rows_change_inside_a_piece",
                "masked_batch", "whole_batches", "several_batches"}
        if lpe == 1:
            need -= {"partial_store"}                                # (every entry is stored alone)
        if lpe < 64:
            need |= {"idle_group", "piece_starts_inside_a_row", "row_over_several_groups"}
        assert seen >= need, (lpe, need - seen)
    # rows much longer than a wave; one wave, one block (4 waves of 16 rows), more than one block
    assert max(int(a.lens.max(initial=0)) for a in TABLE) == 300 and {cdiv(cdiv(n, ROWS_PER_WAVE), 4) for n in ROWS} == {1, 2, 5}
    assert {cdiv(n, ROWS_PER_WAVE) for n in ROWS} >= {1, 4, 5, 17}


# ---- 2. the library -------------------------------------------------------------------------------------------------------------------
class Lib:
    def __init__(self, hip):
        import torch
        self.torch, self.hip, self.g = torch, hip, hip.g
        self.st = hip.g.gcge_hip_stream()
        self.devs = {}

    def ints(self, a):
        a = np.ascontiguousarray(a, dtype=np.int32)
        return self.torch.from_numpy(a if a.size else np.zeros(1, dtype=np.int32)).cuda()

    def dev(self, a):
        if id(a) not in self.devs:
            self.devs[id(a)] = (self.ints(a.rowptr), self.ints(a.col))
        return self.devs[id(a)]

    def operand(self, data, layout):
        """(keep-alive, pointer, ld, check that nothing was written): helpers.Block, or for ld == k a block of its own with guard
        rows behind it"""
        if layout != TIGHT:
            b = Block(self.torch, data, layout, IN_GUARD)
            return b, b.ptr, b.ld, b.unchanged
        host = np.full((data.shape[0] + 3, data.shape[1]), IN_GUARD)
        host[:data.shape[0]] = data
        t = self.torch.from_numpy(host).cuda()

        def unchanged(what):
            assert np.array_equal(bits(t.cpu().numpy()), bits(host)), (what, "an input block was written")
        return t, t.data_ptr(), data.shape[1], unchanged

    def weights(self, w):
        if w is None:
            return None, None
        t = self.torch.from_numpy(np.ascontiguousarray(w)).cuda()
        return t, t.data_ptr()

    def call(self, *args, expect=0):
        self.torch.cuda.synchronize()
        assert "gcge_hip_csr_sample_outer" in abi.HIP
        rc = self.g.gcge_hip_csr_sample_outer(*args)
        self.hip.sync()
        assert rc == expect, rc


@pytest.fixture(scope="module")
def lib(hip):
    return Lib(hip)


def run(lib, a, k, lu, lv, weighted, alpha, same=False, data=None):
    """one call on pattern a; data: (U, V, w, reference, bound) instead of the pattern's exact data"""
    rp, ci = lib.dev(a)
    U, V, w, ref, bound = data if data is not None else (a.U, a.U if same else a.V, a.w, None, None)
    ku, pu, ldu, u_same = lib.operand(U[:, :k], lu)
    if same:
        kv, pv, ldv, v_same = ku, pu, ldu, u_same
    else:
        kv, pv, ldv, v_same = lib.operand(V[:, :k], lv)
    kw, pw = lib.weights(w[:k] if weighted else None)
    out = out_vec(lib.torch, a.nnz)
    lib.call(a.nrows, rp.data_ptr(), ci.data_ptr(), pu, ldu, pv, ldv, k, pw, alpha, out[1], lib.st)
    what = (a.name, k, lu, lv, weighted, alpha, same)
    check_vec(out, alpha * a.ref(k, weighted, same) if ref is None else ref, what, bound)
    u_same(what)
    v_same(what)
    return out[0].cpu().numpy()


def pick(i, pool):
    return pool[i % len(pool)]


# ---- 3. the GPU tests -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k", K)
def test_every_row_structure(lib, k):
    """every pattern of the table at this column count; the layouts of U and V, the weights and alpha cycle independently"""
    ki = K.index(k)
    for ai, a in enumerate(TABLE):
        run(lib, a, k, pick(ai + ki, ALL_LAYOUTS), pick(ai // 5 + 2 * ki + 1, ALL_LAYOUTS), (ai + ki) % 3 != 0, pick(ai + ki // 2, ALPHAS))


@pytest.mark.gpu
@pytest.mark.parametrize("k", K)
def test_every_pair_of_layouts(lib, k):
    """the mixed 65-row table under the 25 combinations of U and V layouts: pairs lost through an odd ldu, an odd ldv, an odd origin
    of U or of V, each alone and together, and ld == k"""
    for i, lu in enumerate(ALL_LAYOUTS):
        for j, lv in enumerate(ALL_LAYOUTS):
            run(lib, MIXED, k, lu, lv, (i + j) % 2 == 0, pick(i + 2 * j, ALPHAS))


@pytest.mark.gpu
def test_u_and_v_the_same_block(lib):
    """d_u == d_v on the square patterns, in every layout"""
    square = [a for a in TABLE if a.shape == "square"]
    assert len(square) >= 8
    for ai, a in enumerate(square):
        for ki, k in enumerate(K):
            lay = pick(ai + ki, ALL_LAYOUTS)
            run(lib, a, k, lay, lay, (ai + ki) % 2 == 0, pick(ai + ki, ALPHAS), same=True)


@pytest.mark.gpu
def test_no_weights_and_every_alpha(lib):
    """d_w NULL and given under every alpha, with and without pairs, in one chunk and in several"""
    for k in (7, 64, 129):
        for lay in (LAYOUTS[0], LAYOUTS[3]):
            for weighted in (False, True):
                for alpha in ALPHAS:
                    run(lib, MIXED, k, lay, lay, weighted, alpha)


@pytest.mark.gpu
def test_two_runs_give_the_same_bits(lib):
    """real-valued U, V, w in (-1/2, 1/2): two runs agree bit for bit — on every branch of the dispatch — and each is within
    (k + 4) u |alpha| sum_c |w_c u_ic v_jc| of the sum formed in longdouble (two roundings per term, k - 1 additions in whatever
    order, one for alpha, one for the reference's own rounding to double: k + 3, first order)"""
    a = BY_NAME["mix_n257_square"]
    U, V, w = uniform(91, (a.nrows, WMAX)) - 0.5, uniform(92, (a.ncols, WMAX)) - 0.5, uniform(93, (WMAX,)) - 0.5
    for k in (3, 16, 33, 64, 128, 258):
        terms = (U[a.row_of, :k] * V[a.col, :k] * w[:k]).astype(np.longdouble)
        ref, bound = (-2.0 * terms.sum(axis=1)).astype(np.float64), (2.0 * (k + 4) * U_ROUND * np.abs(terms).sum(axis=1)).astype(np.float64)
        for lay in (LAYOUTS[0], LAYOUTS[2]):
            first = run(lib, a, k, lay, lay, True, -2.0, data=(U, V, w, ref, bound))
            second = run(lib, a, k, lay, lay, True, -2.0, data=(U, V, w, ref, bound))
            assert np.array_equal(bits(first), bits(second)), (k, lay)


@pytest.mark.gpu
def test_backend_sample_outer(hip):
    """HipBackend.sample_outer: int64 indices, a V whose rows are contiguous inside a wider tensor, a column slice of a transposed
    tensor (one copy), weights and alpha; host tensors raise TypeError, shapes that do not belong together ValueError"""
    import torch
    a = MIXED
    k = 33
    crow, col = torch.from_numpy(a.rowptr.astype(np.int64)).cuda(), torch.from_numpy(a.col.astype(np.int64)).cuda()
    U = torch.from_numpy(a.U).cuda()[:, :k]                          # rows contiguous, stride WMAX
    Vt = torch.from_numpy(np.ascontiguousarray(a.V[:, :k].T)).cuda().T      # columns contiguous
    w = torch.from_numpy(a.w[:k].copy()).cuda()
    got = hip.sample_outer(crow, col, U, Vt, weights=w, alpha=2.0)
    assert got.dtype == torch.float64 and got.shape == (a.nnz,) and np.array_equal(got.cpu().numpy(), 2.0 * a.ref(k, True))
    got = hip.sample_outer(crow.to(torch.int32), col.to(torch.int32), U.contiguous(), U.contiguous())
    assert np.array_equal(got.cpu().numpy(), a.ref(k, False, same=True))
    empty = hip.sample_outer(torch.zeros(4, dtype=torch.int64).cuda(), col[:0], U[:3], Vt)
    assert empty.shape == (0,)
    with pytest.raises(TypeError):
        hip.sample_outer(crow, col, U.cpu(), Vt)
    with pytest.raises(TypeError):
        hip.sample_outer(crow.cpu(), col, U, Vt)
    with pytest.raises(ValueError):
        hip.sample_outer(crow, col, U, Vt[:, :k - 1])
    with pytest.raises(ValueError):
        hip.sample_outer(crow[:-1], col, U, Vt)
    with pytest.raises(ValueError):
        hip.sample_outer(crow, col, U, Vt, weights=w[:-1])
