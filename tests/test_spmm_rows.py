"""The two generic sparse products — gcge_hip_csr_spmm (spmm.hip: spmm_stream, spmm_wave_row, spmm_subwave<1..32>) and
gcge_hip_pad8_spmm / gcge_hip_pad8_spmm_dot (spmm_pad8.hip: one kernel template as plain, grid-stride, scheduled, listed-row and
fused-dot kernel) — over ROW STRUCTURES, through their raw-pointer entries, on EXACT data: matrix values and X entries are nonzero
integers of magnitude <= 3 (plus stored zeros and pads placed on purpose), a row holds at most 200 entries, so every product and
partial sum is an integer of magnitude <= 1800 and any order of summation gives the same double.  The reference is scipy on the same
arrays and the comparison np.array_equal: an entry that is dropped, taken twice or added to the neighbouring row changes an output
by a nonzero integer.  (test_exactness_of_the_case_table checks that premise on the host.)

X sits in a block with 2^40 in the rows behind it and in the columns on both sides; Y in a block filled with a payload NaN (the
kernels never read Y unless they add to listed rows) that must come back bit for bit round the operand — with listed rows also in
the rows that are not listed, on a -1 return in the whole block.

Row structures (TABLE, built once): uniform lengths, mixed tables with empty rows first, last and between long rows, matrices of
empty rows only, and per rows-per-wave value an "edge" table whose waves end their entry stream on a multiple of 64 and one entry
(pad-8: one octet) behind it, hold a row that spans three 64-entry reloads, a row that ends exactly on a reload, and a short last
wave.  Columns are unsorted, repeat inside a row, and hit the first and the last row of X.  Shapes: square, wide (3 n + 1
columns), tall (n = 3 ncols + 1 where the row count allows it, (n - 1) // 3 columns otherwise).  Pads of a pad-8 row name the
row's own column where X has such a row and the last row of X otherwise (the contract in the header of spmm_pad8.hip).
test_the_case_table_reaches_the_branches restates the launch arithmetic of both files and asserts what the table reaches.

Thresholds, each from the launch code:
  spmm.hip gcge_hip_csr_spmm      m > 64 with 16-byte pairs (even ldx, ldy, 16-byte origins): passes of min(m, 128) & ~1 columns, two
                                  per lane; else m > 32: passes of min(m, 64), one per lane; else spmm_subwave<LPR>, LPR = the power of
                                  two >= m.  65 = 64 (two per lane) + 1; 193 = 128 + 64 + 1; without pairs 193 = 64 + 64 + 64 + 1.
  spmm.hip launch_stream          a block = 4 waves of rpw rows, nb = cdiv(n, 4 rpw); xcd_group G > 1 pads the grid to a multiple of
                                  8 G; a chunk map at least nb long replaces the grid by its length.
  spmm.hip spmm_stream            64 entries per reload, BATCH (8 / 16 / 32) per step.
  spmm.hip spmm_wave_row          the first 64 entries of a row in steps of 8 plus a masked tail, then chunks of 64.
  spmm.hip spmm_subwave           steps of 4 entries plus a tail.
  spmm_pad8.hip gcge_hip_pad8_spmm   passes of min(m, col_pass or 128) columns; LPR = 64 / 32 / 16 / 8 lanes per entry at
                                  m > 64 / 32 / 16 / else, G = 64 / LPR entries per step, nsteps = cnt / G per reload of cnt <= 64
                                  padded entries, BATCH (4 / 8 / 16) steps in flight; nchunks = cdiv(n, 4 rpw), grid = min(nchunks,
                                  gridcap) or the schedule's; adding lists with acc_early: rpw = min(rpw, 4).
  spmm_pad8.hip gcge_hip_pad8_spmm_dot   rpw = 4, grid = min(cdiv(n, 16), 8192): blocks stride from n > 131072.
"""

import numpy as np
import pytest

from gcge_amd import abi
from helpers import IN_GUARD, LAYOUTS, OUT_GUARD, Block, bits, check_vec, draw, out_vec

UNIFORM = [0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 128, 129, 200]
ROWS = [1, 2, 3, 5, 15, 16, 17, 63, 64, 65, 127, 129, 257]
MIX = [0, 0, 70, 0, 3, 129, 2, 8, 64, 1, 0, 200, 7, 9, 50, 6, 0, 65, 4, 16, 0, 0, 5, 128, 17, 63, 15]
EDGE_RPW = [1, 2, 4, 8, 16, 32, 64]
CSR_RPW = [4, 8, 16, 32, 64]
P8_RPW = [1, 2, 4, 8, 16, 64]
CSR_M = [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64, 65, 66, 127, 128, 129, 130, 193, 258]
CSR_NARROW = [m for m in CSR_M if m <= 32]          # spmm_subwave: no tuning reaches it
CSR_WIDE = [m for m in CSR_M if m > 32]
P8_M = [2, 4, 14, 16, 18, 32, 34, 64, 66, 128, 130, 258]
DOT_M = [2, 16, 18, 34, 66, 128]
DOT_ROWS_LARGE = [131071, 131072, 131073, 131089]
WMAX = 258                                           # X and the reference are drawn once per matrix at this width
MAX_LEN = 200
EVEN = (2, 0)                                        # the layout pad-8 takes: even ld; its origins: 0, 2 or 4 columns in front
P8_GL = [2, 0, 4]
U = np.longdouble(2.0) ** -53                        # unit roundoff; the bounds are formed in longdouble, like the differences


def cdiv(a, b):
    return -(-a // b)


# ---- the matrices -----------------------------------------------------------------------------------------------------------------
class Mat:
    """One row structure with its data: CSR arrays, the pad-8 arrays by the rule of mat_upload.hip, X (ncols x WMAX) and A X."""

    def __init__(self, name, lens, shape, seed, width=WMAX):
        lens = np.asarray(lens, dtype=np.int64)
        n = lens.size
        self.name, self.nrows, self.shape, self.lens, self.seed, self.width = name, n, shape, lens, seed, width
        self.ncols = {"square": n, "wide": 3 * n + 1, "tall": max(1, (n - 1) // 3)}[shape]
        self.rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        nnz = int(self.rowptr[-1])
        rng = np.random.default_rng(seed)
        col = rng.integers(0, self.ncols, nnz)                     # unsorted; repeats happen and are forced below
        row_of = np.repeat(np.arange(n), lens)
        first = self.rowptr[:-1][lens >= 2][::2]
        col[first + 1] = col[first]                                # a repeated column at the head of every other row of >= 2 entries
        if nnz:
            col[0], col[nnz // 2], col[-1] = 0, self.ncols - 1, self.ncols - 1     # the first and the last row of X
        self.col = col.astype(np.int32)
        self.val = draw(seed + 1, (nnz,), False)
        self.val[5::11] = 0.0                                      # stored zeros
        self.row_of = row_of
        # pad-8: every row padded to a multiple of 8 entries with (a valid row of X — its own column where there is one —, 0.0)
        octs = (lens + 7) // 8
        self.orp = np.concatenate([[0], np.cumsum(octs)]).astype(np.int32)
        self.pcol = np.repeat(np.minimum(np.arange(n), self.ncols - 1), 8 * octs).astype(np.int32)
        self.pval = np.zeros(8 * int(self.orp[-1]))
        dest = 8 * self.orp[:-1].astype(np.int64)[row_of] + (np.arange(nnz) - self.rowptr[:-1].astype(np.int64)[row_of])
        self.pcol[dest] = self.col
        self.pval[dest] = self.val
        self._cache = {}

    def scipy(self, val=None):
        import scipy.sparse as sp
        return sp.csr_matrix((self.val if val is None else val, self.col, self.rowptr), shape=(self.nrows, self.ncols))

    def get(self, key, make):
        if key not in self._cache:
            self._cache[key] = make()
        return self._cache[key]

    def X(self, real=False):
        return self.get(("X", real), lambda: draw(self.seed + 2, (self.ncols, self.width), real))

    def ref(self):
        """A X on the exact data (float64 holds it exactly)"""
        return self.get("ref", lambda: np.ascontiguousarray(self.scipy() @ self.X()))

    def val_real(self):
        def make():
            v = draw(self.seed + 3, (self.val.size,), True)
            v[5::11] = 0.0
            return v
        return self.get("val_real", make)

    def ref_real(self):
        """(A X, |A| |X|) in longdouble on the real-valued data, row by row"""
        def make():
            v, X = self.val_real(), self.X(True)
            vl, Xl = v.astype(np.longdouble), X.astype(np.longdouble)
            out, ab = np.zeros((self.nrows, self.width), dtype=np.longdouble), np.zeros((self.nrows, self.width), dtype=np.longdouble)
            for r in range(self.nrows):
                s, e = self.rowptr[r], self.rowptr[r + 1]
                out[r] = (vl[s:e, None] * Xl[self.col[s:e]]).sum(axis=0)
                ab[r] = (np.abs(vl[s:e, None]) * np.abs(Xl[self.col[s:e]])).sum(axis=0)
            return out, ab
        return self.get("ref_real", make)


def edge_lens(rpw):
    """waves of rpw rows: 64 entries; 65; 72 (pad-8: one octet more); a row over three reloads and a total of 192; an empty first row, a row that ends on the
    first reload with entries behind it, an empty row inside; three rows"""
    base = [64 // rpw] * rpw
    w3 = ([10, 140, 42] + [0] * rpw)[:max(rpw, 3)]
    w4 = ([0, 64, 0, 5] + [1] * rpw)[:max(rpw, 4)]
    return base + base[:-1] + [base[-1] + 1] + base[:-1] + [base[-1] + 8] + w3 + w4 + [7, 0, 9]


def build_table():
    t, seed = [], 1000
    shapes = ("square", "wide", "tall")
    for i, ln in enumerate(UNIFORM):                               # every uniform length at two row counts
        for j in (0, 1):
            n = ROWS[(2 * i + 7 * j + 3) % len(ROWS)]
            seed += 10
            t.append(Mat("len%d_n%d" % (ln, n), [ln] * n, shapes[(i + j) % 3], seed))
    for i, n in enumerate(ROWS):                                   # every row count with mixed lengths, in every shape
        for k, shape in enumerate(shapes):
            lens = [MIX[(q + 5 * i + 3 * k) % len(MIX)] for q in range(n)]
            if n >= 3:
                lens[0], lens[1], lens[-1] = 0, 0, 0               # empty rows first and last (the pattern puts them between long rows)
            seed += 10
            t.append(Mat("mix_n%d_%s" % (n, shape), lens, shape, seed))
    for n, shape in ((5, "square"), (65, "wide"), (257, "tall")):
        seed += 10
        t.append(Mat("empty_n%d" % n, [0] * n, shape, seed))
    for i, rpw in enumerate(EDGE_RPW):
        seed += 10
        t.append(Mat("edge%d" % rpw, edge_lens(rpw), shapes[i % 3], seed))
    return t


TABLE = build_table()
BY_NAME = {a.name: a for a in TABLE}
MIXED = [BY_NAME["mix_n129_square"], BY_NAME["mix_n65_wide"], BY_NAME["mix_n127_tall"]]
# the fused product's matrices: X is a slab of own0 + n rows and more, the product's own rows start at own0 (square + 40 columns)
DOT_OWN0 = [0, 37]


class DotMat(Mat):
    """n rows over a slab of n + 40 rows of X"""

    def __init__(self, n, seed, large):
        lens = [1 + (q * 5) % 8 for q in range(n)] if large else [MIX[(q + n + 1) % len(MIX)] for q in range(n)]
        Mat.__init__(self, "dot_n%d" % n, lens, "square", seed, width=16 if large else 128)

    # (columns drawn in [0, n): rows of the slab; the slab itself is n + 40 rows so that own0 = 37 fits)
    def X(self, real=False):
        return self.get(("X", real), lambda: draw(self.seed + 2, (self.nrows + 40, self.width), real))

    def scipy(self, val=None):
        import scipy.sparse as sp
        return sp.csr_matrix((self.val if val is None else val, self.col, self.rowptr), shape=(self.nrows, self.nrows + 40))


DOT_SMALL = [DotMat(n, 5000 + n, False) for n in (1, 5, 16, 17)]


# ---- the launch arithmetic restated (checked on the host below) -------------------------------------------------------------------
def csr_passes(m, pairs):
    """the column passes of gcge_hip_csr_spmm: [(kernel, columns per lane or lanes per row, width)]"""
    out = []
    while m > 0:
        if m > 32:
            w, k = ((min(m, 128) & ~1), ("wide", 2)) if pairs and m > 64 else (min(m, 64), ("wide", 1))
        else:
            lpr = 1
            while lpr < m:
                lpr *= 2
            w, k = m, ("subwave", lpr)
        out.append(k + (w,))
        m -= w
    return out


def p8_passes(m, col_pass=0):
    """[(LPR, width)] of gcge_hip_pad8_spmm"""
    out = []
    while m > 0:
        w = min(m, col_pass if col_pass > 0 else 128)
        out.append((64 if w > 64 else 32 if w > 32 else 16 if w > 16 else 8, w))
        m -= w
    return out


def wave_features(lens, rpw, reload=64, behind=1):
    """what the waves of rpw rows meet when they walk their rows' entries as one stream in reloads of 64 (pad-8: lens already padded)"""
    f = set()
    n = len(lens)
    for row0 in range(0, n, rpw):
        w = np.asarray(lens[row0:row0 + rpw])
        nr, ends = len(w), np.concatenate([[0], np.cumsum(w)])
        tot = int(ends[-1])
        if nr < rpw:
            f.add("short_wave")
        if nr == 64:
            f.add("lane63")
        if tot == 0:
            f.add("all_empty")
            continue
        nz = np.nonzero(w)[0]
        if w[0] == 0:
            f.add("leading")
        if w[-1] == 0:
            f.add("trailing")
        if np.any(w[nz[0]:nz[-1]] == 0):
            f.add("interior")
        for i in nz:
            if ends[i + 1] % reload == 0 and ends[i + 1] < tot:
                f.add("row_ends_on_reload")
            if (ends[i + 1] - 1) // reload - ends[i] // reload >= 2:
                f.add("three_reloads")
        if tot % reload == 0:
            f.add("stream_ends_on_64")
        if tot % reload == behind:
            f.add("one_behind")
    return f


def stream_grid(n, rpw, group, map_len=0):
    """(chunks, blocks launched) of launch_stream / launch_wave_row"""
    nb = cdiv(n, 4 * rpw)
    grid = nb if group <= 1 else cdiv(nb, 8 * group) * 8 * group
    return nb, (map_len if map_len >= nb and map_len > 0 else grid)


# ---- 1. the premise and the table's reach, on the host ----------------------------------------------------------------------------
def test_exactness_of_the_case_table():
    """every value a nonzero integer of magnitude <= 3 (stored zeros apart), at most 200 entries per row, so |y| <= 1800 and the fused
    product's sums stay below 3 * 1800 * n < 2^53; the float64 reference equals the same product in int64; the pad-8 arrays hold the
    CSR entries in order, pads of weight 0 on a valid row of X, and give the same product"""
    for a in TABLE + DOT_SMALL:
        assert a.lens.max(initial=0) <= MAX_LEN and a.nrows >= 1 and a.ncols >= 1
        v, X = a.val, a.X()
        assert np.all(v == np.round(v)) and np.all(np.abs(v) <= 3) and np.all(X == np.round(X)) and np.all(np.abs(X) <= 3) and np.all(X != 0)
        assert np.all((v == 0) == (np.arange(v.size) % 11 == 5))
        ri = a.scipy(v.astype(np.int64)) @ X.astype(np.int64)
        assert np.array_equal(a.ref(), ri) and np.max(np.abs(ri), initial=0) <= 9 * MAX_LEN
        assert a.col.size < 3 or (a.col.min() == 0 and a.col.max() == a.ncols - 1)
        import scipy.sparse as sp
        assert a.pcol.size == 8 * a.orp[-1] and np.all((a.pcol >= 0) & (a.pcol < a.ncols))
        P = sp.csr_matrix((a.pval, a.pcol, 8 * a.orp.astype(np.int64)), shape=a.scipy().shape)
        assert np.array_equal(P @ X, a.ref())
        pads = np.ones(a.pval.size, dtype=bool)
        pads[8 * a.orp[:-1].astype(np.int64)[a.row_of] + (np.arange(a.val.size) - a.rowptr[:-1].astype(np.int64)[a.row_of])] = False
        assert np.all(a.pval[pads] == 0) and pads.sum() == a.pval.size - a.val.size
    assert any(np.any(np.diff(a.col[a.rowptr[r]:a.rowptr[r + 1]]) < 0) for a in MIXED for r in range(a.nrows))          # unsorted
    assert any(np.unique(a.col[a.rowptr[r]:a.rowptr[r + 1]]).size < a.lens[r] for a in MIXED for r in range(a.nrows))   # repeated
    assert 3 * 9 * MAX_LEN * max(DOT_ROWS_LARGE) < 2 ** 53
    assert {a.nrows for a in TABLE} >= set(ROWS) and {int(l) for a in TABLE for l in a.lens} >= set(UNIFORM)
    assert {(a.nrows, a.ncols) for a in TABLE if a.shape == "tall"} >= {(16, 5), (64, 21), (127, 42)}
    assert {(a.nrows, a.ncols) for a in TABLE if a.shape == "wide"} >= {(n, 3 * n + 1) for n in ROWS}


def test_the_case_table_reaches_the_branches():
    """the launch arithmetic of spmm.hip and spmm_pad8.hip restated: what the table meets under every rows-per-wave value"""
    lens_all = {int(l) for a in TABLE for l in a.lens}
    stream_need = {"leading", "interior", "trailing", "all_empty", "row_ends_on_reload", "three_reloads", "short_wave",
                   "stream_ends_on_64", "one_behind"}
    for rpw in CSR_RPW:                                             # spmm_stream
        seen = set()
        for a in TABLE:
            seen |= wave_features(a.lens, rpw)
        assert seen >= stream_need | ({"lane63"} if rpw == 64 else set()), (rpw, stream_need - seen)
        edge = BY_NAME["edge%d" % rpw]
        assert wave_features(edge.lens, rpw) >= {"stream_ends_on_64", "one_behind", "three_reloads", "row_ends_on_reload", "short_wave"}
    assert lens_all >= {7, 8, 9, 63, 64, 65, 128, 129} and lens_all >= set(range(10))        # spmm_wave_row, spmm_subwave
    # xcd_group pads the grid; the map replaces it
    assert stream_grid(257, 4, 2) == (17, 32) and stream_grid(257, 4, 3) == (17, 24) and stream_grid(257, 16, 1, 13) == (5, 13)
    assert any(stream_grid(a.nrows, rpw, g)[1] > stream_grid(a.nrows, rpw, g)[0] for a in TABLE for rpw in CSR_RPW for g in (2, 3))
    # the column splitter
    assert csr_passes(65, True) == [("wide", 2, 64), ("subwave", 1, 1)] and csr_passes(65, False) == [("wide", 1, 64), ("subwave", 1, 1)]
    assert csr_passes(129, True) == [("wide", 2, 128), ("subwave", 1, 1)] and csr_passes(130, True) == [("wide", 2, 128), ("subwave", 2, 2)]
    assert csr_passes(193, True) == [("wide", 2, 128), ("wide", 2, 64), ("subwave", 1, 1)]
    assert csr_passes(193, False) == [("wide", 1, 64)] * 3 + [("subwave", 1, 1)]
    assert csr_passes(258, True) == [("wide", 2, 128), ("wide", 2, 128), ("subwave", 2, 2)]
    assert {k[1] for m in CSR_NARROW for k in csr_passes(m, False)} == {1, 2, 4, 8, 16, 32}
    assert {k[:2] for m in CSR_WIDE for p in (True, False) for k in csr_passes(m, p)} >= {("wide", 1), ("wide", 2)}
    # pad-8: every LPR; rows of 0, 1, 7, 8, 9, 17 octets; per rows-per-wave value the stream edges in padded entries
    assert {l for m in P8_M for l, _ in p8_passes(m)} == {8, 16, 32, 64} and {l for m in DOT_M for l, _ in p8_passes(m)} == {8, 16, 32, 64}
    assert p8_passes(130, 64) == [(32, 64), (32, 64), (8, 2)] and p8_passes(258) == [(64, 128), (64, 128), (8, 2)]
    assert {cdiv(l, 8) for l in lens_all} >= {0, 1, 7, 8, 9, 17}
    for rpw in P8_RPW:
        seen = set()
        for a in TABLE:
            seen |= wave_features(8 * ((a.lens + 7) // 8), rpw, behind=8)
        need = {"all_empty", "stream_ends_on_64", "one_behind", "three_reloads"}       # (one_behind: one octet)
        need |= ({"short_wave", "row_ends_on_reload", "leading", "trailing"} if rpw >= 2 else set()) | ({"interior"} if rpw >= 3 else set())
        assert seen >= need, (rpw, need - seen)
    # BATCH tails: steps per reload (cnt / G, cnt a multiple of 8 up to 64) that are no multiple of the batch, for every G
    for lpr in (8, 16, 32, 64):
        steps = {min(64, 8 * cdiv(l, 8)) * lpr // 64 for l in lens_all if l}
        for batch in (4, 8, 16):
            # (cnt is a multiple of 8, so nsteps is one of lpr / 8: a batch that divides lpr / 8 never meets a tail)
            assert any(s % batch for s in steps) == (batch > lpr // 8) and any(s % batch == 0 for s in steps) == (batch <= lpr), (lpr, batch)
    # grid caps, schedules and the fused product's cap
    assert any(cdiv(a.nrows, 4 * rpw) > cap for a in TABLE for rpw in P8_RPW for cap in (1, 3, 8))
    assert cdiv(131072, 16) == 8192 and cdiv(131073, 16) == 8193 and all(n % 16 for n in (131071, 131073, 131089)) and 131089 - 131072 > 16
    assert {n % 16 != 0 for n in (1, 5, 16, 17)} == {True, False}


# ---- 2. the library ---------------------------------------------------------------------------------------------------------------
class Lib:
    def __init__(self, hip):
        import torch
        self.torch, self.hip, g = torch, hip, hip.g
        self.g = g
        self.st = g.gcge_hip_stream()
        self.keep, self.devs = [], {}

    def defaults(self):
        g = self.g
        g.gcge_hip_spmm_tune(16, 1, 0)
        g.gcge_hip_spmm_variant(1, 16)
        g.gcge_hip_spmm_set_chunk_map(None, 0)
        g.gcge_hip_spmm_pad8_tune(0, 0, 0, 0)          # automatic again: batch 8, store 1, the widest pass
        g.gcge_hip_spmm_pad8_gridcap(0)
        g.gcge_hip_spmm_pad8_schedule(None, 0, 0, 0)
        g.gcge_hip_spmm_pad8_row_map(None)
        g.gcge_hip_spmm_pad8_acc_early(1)
        g.gcge_hip_set_spmm_path(0)
        self.hip.sync()
        self.keep, self.devs = [], {}

    def ints(self, a):
        a = np.ascontiguousarray(a, dtype=np.int32)
        return self.torch.from_numpy(a if a.size else np.zeros(1, dtype=np.int32)).cuda()

    def dev(self, a, real=False):
        """device copies of a matrix's arrays, kept until the test ends (nothing on the device outlives a test)"""
        def make():
            val, pval = a.val, a.pval
            if real:
                val = a.val_real()
                pval = np.zeros_like(a.pval)
                pval[8 * a.orp[:-1].astype(np.int64)[a.row_of] + (np.arange(val.size) - a.rowptr[:-1].astype(np.int64)[a.row_of])] = val
            f = lambda v: self.torch.from_numpy(np.ascontiguousarray(v) if v.size else np.zeros(1)).cuda()
            t = {"rowptr": self.ints(a.rowptr), "col": self.ints(a.col), "val": f(val), "orp": self.ints(a.orp), "pcol": self.ints(a.pcol), "pval": f(pval)}
            return {k: v.data_ptr() for k, v in t.items()}, t
        key = (id(a), real)
        if key not in self.devs:
            self.devs[key] = make()
        return self.devs[key][0]

    def call(self, name, *args, expect=0):
        self.torch.cuda.synchronize()
        assert "gcge_hip_" + name in abi.HIP, name          # a name composed here escapes test_abi's source scan
        rc = getattr(self.g, "gcge_hip_" + name)(*args)
        self.hip.sync()
        assert rc == expect, (name, rc)

    def block(self, data, layout, guard=IN_GUARD, gl=None):
        return Block(self.torch, data, layout, guard, gl)

    def chunk_map(self, nb, seed):
        """a permutation of the chunk ids with -1 slots, longer than nb"""
        rng = np.random.default_rng(seed)
        m = np.full(2 * nb + 3, -1, dtype=np.int32)
        m[rng.permutation(2 * nb + 3)[:nb]] = rng.permutation(nb)
        t = self.ints(m)
        self.keep.append(t)
        self.g.gcge_hip_spmm_set_chunk_map(t.data_ptr(), m.size)

    def schedule(self, nchunks, rpw, seed, jx=2):
        """8 lists (one per XCD) that hold every chunk id once among -1 slots, for a grid of 8 jx blocks"""
        rng = np.random.default_rng(seed)
        ln = cdiv(cdiv(nchunks, 8) + 2, jx) * jx
        s = np.full(8 * ln, -1, dtype=np.int32)
        s[rng.permutation(8 * ln)[:nchunks]] = rng.permutation(nchunks)
        t = self.ints(s)
        self.keep.append(t)
        self.g.gcge_hip_spmm_pad8_schedule(t.data_ptr(), ln, rpw, 8 * jx)


@pytest.fixture(scope="module")
def lib_(hip):
    return Lib(hip)


@pytest.fixture
def lib(lib_):
    """every knob at its default before the test and — whether the test passed or not — behind it"""
    lib_.defaults()
    yield lib_
    lib_.defaults()


def lay(i, pool=LAYOUTS):
    return pool[i % len(pool)]


def y_block(lib, n, m, layout, gl=None):
    return lib.block(np.full((n, m), OUT_GUARD), layout, OUT_GUARD, gl)


def run_csr(lib, a, m, lx, ly, real=False):
    d = lib.dev(a, real)
    bx, by = lib.block(a.X(real)[:, :m], lx), y_block(lib, a.nrows, m, ly)
    lib.call("csr_spmm", a.nrows, d["rowptr"], d["col"], d["val"], bx.ptr, bx.ld, by.ptr, by.ld, m, lib.st)
    what = ("csr_spmm", a.name, m, lx, ly)
    if real:
        ref, ab = a.ref_real()
        by.check(ref[:, :m], what, (a.lens[:, None] + 2) * U * ab[:, :m])
    else:
        by.check(a.ref()[:, :m], what)
    bx.unchanged(what)
    return bx, by


def run_p8(lib, a, m, lx=0, ly=0, real=False):
    """lx, ly: which of the even origins X and Y start on"""
    d = lib.dev(a, real)
    bx, by = lib.block(a.X(real)[:, :m], EVEN, gl=P8_GL[lx % 3]), y_block(lib, a.nrows, m, EVEN, P8_GL[ly % 3])
    lib.call("pad8_spmm", a.nrows, d["orp"], d["pcol"], d["pval"], bx.ptr, bx.ld, by.ptr, by.ld, m, lib.st)
    what = ("pad8_spmm", a.name, m, lx, ly)
    if real:
        ref, ab = a.ref_real()
        by.check(ref[:, :m], what, (a.lens[:, None] + 2) * U * ab[:, :m])
    else:
        by.check(a.ref()[:, :m], what)
    bx.unchanged(what)
    return bx, by


# ---- 3. gcge_hip_csr_spmm ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_csr_narrow_columns_over_the_table(lib):
    """spmm_subwave<1 .. 32>: every row structure at every narrow width, the layouts of X and Y cycling independently"""
    for ai, a in enumerate(TABLE):
        for mi, m in enumerate(CSR_NARROW):
            run_csr(lib, a, m, lay(ai + mi), lay(ai // 4 + mi // 4 + 1))


# (variant, batch, rows per wave, nt stores, xcd group, chunk map)
CSR_CONFIGS = [(1, 16, 16, 0, 1, 0), (1, 8, 4, 1, 2, 0), (1, 32, 8, 0, 3, 0), (1, 16, 32, 1, 1, 1), (1, 8, 64, 0, 1, 0),
               (1, 32, 64, 1, 2, 1), (1, 8, 16, 0, 3, 1), (1, 32, 4, 0, 1, 1), (1, 16, 8, 1, 2, 0),
               (0, 16, 4, 0, 1, 0), (0, 16, 8, 1, 2, 0), (0, 16, 16, 0, 3, 1), (0, 16, 32, 1, 1, 1), (0, 16, 64, 0, 2, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", CSR_CONFIGS, ids=lambda c: "v%d-b%d-rpw%d-nt%d-xcd%d-map%d" % c)
def test_csr_wide_columns_over_the_table(lib, cfg):
    """spmm_stream (variant 1) and spmm_wave_row (variant 0; 64 rows per wave fall back to 16 there): every row structure at three
    of the wide widths — which three moves with the structure and the configuration — and all of them on the mixed tables"""
    variant, batch, rpw, nt, group, use_map = cfg
    ci = CSR_CONFIGS.index(cfg)
    lib.g.gcge_hip_spmm_variant(variant, batch)
    lib.g.gcge_hip_spmm_tune(rpw, group, nt)
    eff = rpw if variant == 1 or rpw != 64 else 16
    for ai, a in enumerate(TABLE):
        if use_map:
            lib.chunk_map(cdiv(a.nrows, 4 * eff), ai + ci)
        ms = CSR_WIDE if a in MIXED else [CSR_WIDE[(ai + ci + 4 * k) % len(CSR_WIDE)] for k in range(3)]
        for mi, m in enumerate(ms):
            run_csr(lib, a, m, lay(ai + mi + ci), lay((ai + ci) // 4 + mi // 4))
        lib.keep = []


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [1, 0])
def test_csr_column_splitter(lib, variant):
    """every width under the 16 combinations of X and Y layouts: pairs lost through an odd ldx, an odd ldy, an odd origin of X or of
    Y, each alone and together"""
    lib.g.gcge_hip_spmm_variant(variant, 16)
    a = MIXED[0]
    for m in CSR_M:
        for lx in LAYOUTS:
            for ly in LAYOUTS:
                run_csr(lib, a, m, lx, ly)


# ---- 4. gcge_hip_pad8_spmm --------------------------------------------------------------------------------------------------------
# (rows per wave, batch, store, col_pass, gridcap, schedule); rows per wave 0: automatic (8 here: nothing has called the ops table's choice)
P8_CONFIGS = [(0, 8, 1, 0, 0, 0), (1, 4, 0, 0, 0, 0), (2, 8, 1, 64, 0, 0), (4, 16, 2, 0, 1, 0), (8, 4, 1, 0, 3, 0), (16, 8, 0, 64, 8, 0),
              (64, 16, 1, 0, 0, 0), (4, 8, 1, 0, 0, 1), (1, 16, 2, 64, 0, 1), (16, 4, 0, 0, 0, 1), (2, 16, 0, 0, 3, 0), (64, 4, 2, 64, 1, 0)]


def p8_setup(lib, cfg, a, seed):
    rpw, batch, store, col_pass, cap, sched = cfg
    if rpw:
        lib.g.gcge_hip_spmm_pad8_tune(rpw, batch, store, col_pass)
    lib.g.gcge_hip_spmm_pad8_gridcap(cap)
    if sched:
        lib.schedule(cdiv(a.nrows, 4 * rpw), rpw, seed)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", P8_CONFIGS, ids=lambda c: "rpw%d-b%d-st%d-pass%d-cap%d-sched%d" % c)
def test_pad8_over_the_table(lib, cfg):
    """every row structure at three widths — which three moves with the structure and the configuration —, all widths on the mixed
    tables; X and Y start 0, 2 or 4 columns into their blocks"""
    ci = P8_CONFIGS.index(cfg)
    for ai, a in enumerate(TABLE):
        p8_setup(lib, cfg, a, ai + ci)
        ms = P8_M if a in MIXED else [P8_M[(ai + ci + 4 * k) % len(P8_M)] for k in range(3)]
        for mi, m in enumerate(ms):
            run_p8(lib, a, m, ai + mi, ai // 3 + ci)
        lib.keep = []


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [4, 8, 16])
def test_pad8_every_width_and_batch(lib, batch):
    """every LPR (8 / 16 / 32 / 64 lanes per entry: the reduction across 8 / 4 / 2 / 1 groups) with every batch, whose tail re-reads
    the last step with weight 0, on rows of 0 .. 25 octets; 128- and 64-column passes"""
    for col_pass in (0, 64):
        for rpw in (1, 8):
            lib.g.gcge_hip_spmm_pad8_tune(rpw, batch, 1, col_pass)
            for a in MIXED + [BY_NAME["edge8"]]:
                for m in P8_M:
                    run_p8(lib, a, m, m // 2 + rpw, m // 4)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["set-early", "set-late", "add-early", "add-late"])
def test_pad8_listed_rows(lib, mode):
    """a matrix given as a list of rows of a longer Y: = and += (the ACC kernel with rows per wave clamped to 4, and the read at the
    end of each row); the rows of Y that are not listed keep their payload NaN"""
    add, early = mode.startswith("add"), mode.endswith("early")
    lib.g.gcge_hip_spmm_pad8_acc_early(1 if early else 0)
    for ci, (rpw, batch, store) in enumerate([(1, 4, 0), (4, 8, 1), (8, 16, 2), (2, 8, 1)]):
        lib.g.gcge_hip_spmm_pad8_tune(rpw, batch, store, 0)
        for ai, a in enumerate(TABLE):
            if ai % 4 != ci and a not in MIXED:
                continue
            d = lib.dev(a)
            rng = np.random.default_rng(ai + 77)
            ny = 2 * a.nrows + 3
            rows = rng.permutation(ny)[:a.nrows]                   # the listed rows' places in Y, in no order
            tmap = lib.ints(rows)
            for mi in range(3):
                m = P8_M[(ai + ci + 4 * mi) % len(P8_M)]
                Y0 = np.full((ny, m), OUT_GUARD)
                old = draw(ai + mi, (a.nrows, m), False)
                if add:
                    Y0[rows] = old
                bx, by = lib.block(a.X()[:, :m], EVEN), lib.block(Y0, EVEN, OUT_GUARD)
                (lib.g.gcge_hip_spmm_pad8_row_map_add if add else lib.g.gcge_hip_spmm_pad8_row_map)(tmap.data_ptr())
                lib.call("pad8_spmm", a.nrows, d["orp"], d["pcol"], d["pval"], bx.ptr, bx.ld, by.ptr, by.ld, m, lib.st)
                lib.g.gcge_hip_spmm_pad8_row_map(None)
                what = ("pad8_spmm listed", mode, a.name, m, rpw)
                got = by.dev.cpu().numpy()
                op = got[:ny, by.gl:by.gl + m]
                ref = a.ref()[:, :m] + (old if add else 0)
                assert np.array_equal(op[rows], ref), (what, np.argwhere(op[rows] != ref)[:4].tolist())
                got[rows, by.gl:by.gl + m] = by.host[rows, by.gl:by.gl + m]
                assert np.array_equal(bits(got), bits(by.host)), (what, "a row that is not listed, or a guard, was written")
                bx.unchanged(what)


@pytest.mark.gpu
def test_pad8_declines_and_leaves_y_alone(lib):
    """the five ways to -1: an odd width, an odd ldx, an odd ldy, X or Y off a 16-byte boundary"""
    a = MIXED[0]
    d = lib.dev(a)
    E, O_ORIGIN, O_LD = (2, 0), (1, 0), (2, 1)
    for m, lx, ly in ((17, E, E), (16, O_LD, E), (16, E, O_LD), (16, O_ORIGIN, E), (16, E, O_ORIGIN)):
        bx, by = lib.block(a.X()[:, :m], lx), y_block(lib, a.nrows, m, ly)
        assert (m % 2, bx.ld % 2, by.ld % 2, bx.ptr % 16, by.ptr % 16).count(0) == 4
        lib.call("pad8_spmm", a.nrows, d["orp"], d["pcol"], d["pval"], bx.ptr, bx.ld, by.ptr, by.ld, m, lib.st, expect=-1)
        by.unchanged(("pad8_spmm declines", m, lx, ly))
        out = out_vec(lib.torch, m)
        lib.call("pad8_spmm_dot", a.nrows, d["orp"], d["pcol"], d["pval"], bx.ptr, bx.ld, by.ptr, by.ld, m, out[1], lib.st, 0, expect=-1)
        by.unchanged(("pad8_spmm_dot declines", m, lx, ly))
        assert np.all(bits(out[0].cpu().numpy()) == bits(np.array([OUT_GUARD]))[0])


@pytest.mark.gpu
def test_pad8_tune_refuses_odd_and_wide_passes(lib):
    """an odd col_pass is refused (its last pair would store a column beyond m, into the guard), one above 128 as well (a wave covers
    128 columns).  The last step calls tune(0, ..), which by the code clears the hand-tuned flag and restores batch 8 / store 1 /
    pass 0 whatever the other arguments say; the product is exact under every setting, so this test sees only that the call leaves a
    working state — neither the restored values nor that gcge_hip_spmm_pad8_auto chooses again can be observed through the entry
    points (the reset is pinned by reading gcge_hip_spmm_pad8_tune, not by this test)"""
    a = MIXED[0]
    lib.g.gcge_hip_spmm_pad8_tune(2, 4, 0, 64)
    lib.g.gcge_hip_spmm_pad8_tune(2, 4, 0, 33)                     # refused: the pass stays 64
    run_p8(lib, a, 130)
    lib.g.gcge_hip_spmm_pad8_tune(2, 4, 0, 130)                    # refused as well (a wave covers 128 columns)
    run_p8(lib, a, 258)
    lib.g.gcge_hip_spmm_pad8_tune(0, 16, 2, 64)                    # everything back, whatever the other arguments say
    run_p8(lib, a, 258)


@pytest.mark.gpu
def test_pad8_schedule_with_an_unusable_grid_is_not_installed(lib):
    """a schedule whose grid is no positive multiple of 8 (12: slots nobody walks; 4: gridDim.x >> 3 == 0) is refused by
    gcge_hip_spmm_pad8_schedule — a line on stderr says so — and the product runs unscheduled, exact"""
    for grid in (12, 4):
        for a in MIXED:
            lib.g.gcge_hip_spmm_pad8_tune(4, 8, 1, 0)
            nchunks = cdiv(a.nrows, 16)
            s = np.full(8 * nchunks, -1, dtype=np.int32)           # a schedule that names NO chunk: followed, it would leave Y unwritten
            t = lib.ints(s)
            lib.g.gcge_hip_spmm_pad8_schedule(t.data_ptr(), nchunks, 4, grid)
            for m in (16, 66):
                run_p8(lib, a, m)
            lib.g.gcge_hip_spmm_pad8_schedule(None, 0, 0, 0)


# ---- 5. gcge_hip_pad8_spmm_dot ----------------------------------------------------------------------------------------------------
def run_dot(lib, a, m, own0, real=False):
    d = lib.dev(a, real)
    n = a.nrows
    bx, by, out = lib.block(a.X(real)[:, :m], EVEN), y_block(lib, n, m, EVEN), out_vec(lib.torch, m)
    lib.call("pad8_spmm_dot", n, d["orp"], d["pcol"], d["pval"], bx.ptr, bx.ld, by.ptr, by.ld, m, out[1], lib.st, own0)
    what = ("pad8_spmm_dot", a.name, m, own0)
    own = a.X(real)[own0:own0 + n, :m]
    if real:
        ref, ab = a.ref_real()
        by.check(ref[:, :m], what, (a.lens[:, None] + 2) * U * ab[:, :m])
        check_vec(out, (own.astype(np.longdouble) * ref[:, :m]).sum(axis=0), what,
                  (n + 2 + int(a.lens.max()) + 2) * U * (np.abs(own.astype(np.longdouble)) * ab[:, :m]).sum(axis=0))
    else:
        by.check(a.ref()[:, :m], what)
        check_vec(out, (own * a.ref()[:, :m]).sum(axis=0), what)
    bx.unchanged(what)
    return bx, by, out


@pytest.mark.gpu
@pytest.mark.parametrize("own0", DOT_OWN0)
def test_pad8_dot_small_rows(lib, own0):
    """Y and the column sums sum_r X[own0 + r, j] Y[r, j], exact, at every LPR; 1, 5, 16, 17 rows (the clamped loads of a wave's own
    rows of X where n is no multiple of 16) of mixed lengths"""
    for a in DOT_SMALL:
        for m in DOT_M:
            run_dot(lib, a, m, own0)


@pytest.mark.gpu
@pytest.mark.parametrize("n", DOT_ROWS_LARGE)
def test_pad8_dot_grid_cap(lib, n):
    """8192 blocks of 16 rows: from 131073 rows blocks stride and a block's partial sum collects a second chunk; one-octet rows,
    16 columns"""
    a = DotMat(n, 6000 + n % 100, True)
    for own0 in DOT_OWN0:
        run_dot(lib, a, 16, own0)


# ---- 6. real data: the rounding bound, the same bits twice, pad-8 == CSR where both are one fma chain -----------------------------
@pytest.mark.gpu
def test_rounding_bound_same_bits_and_pad8_equals_csr(lib):
    """uniform - 0.5 against longdouble: |Y - ref| <= (len_r + 2) 2^-53 (|A| |X|)_r (len_r products fused into len_r additions, in
    any order); a second run gives the same bits; at G == 1 (65 .. 128 columns) pad-8 and the CSR stream kernel are the same fma
    chain in entry order (a pad adds 0 x = +-0 to the sum, which changes no bit of it), so their results are equal bit for bit.
    The fused product's sums: n terms that each carry the (len_r + 2) u of Y, in any order: (n + 2 + max len + 2) u sum |x| (|A| |X|)."""
    a = MIXED[0]
    for m in (2, 16, 18, 34, 66, 128):
        bx, by = run_p8(lib, a, m, real=True)
        first = by.dev.cpu().numpy().copy()
        d = lib.dev(a, True)
        lib.call("pad8_spmm", a.nrows, d["orp"], d["pcol"], d["pval"], bx.ptr, bx.ld, by.ptr, by.ld, m, lib.st)
        assert np.array_equal(bits(first), bits(by.dev.cpu().numpy())), ("pad8_spmm twice", m)
        if m > 64:
            _, cy = run_csr(lib, a, m, EVEN, EVEN, real=True)
            assert np.array_equal(bits(first), bits(cy.dev.cpu().numpy())), ("pad-8 against CSR at G == 1", m)
    for m in (1, 5, 17, 33, 64, 65, 130):
        for lx, ly in ((LAYOUTS[0], LAYOUTS[0]), (LAYOUTS[3], LAYOUTS[1])):
            for variant in (1, 0):
                lib.g.gcge_hip_spmm_variant(variant, 16)
                bx, by = run_csr(lib, a, m, lx, ly, real=True)
                first = by.dev.cpu().numpy().copy()
                d = lib.dev(a, True)
                lib.call("csr_spmm", a.nrows, d["rowptr"], d["col"], d["val"], bx.ptr, bx.ld, by.ptr, by.ld, m, lib.st)
                assert np.array_equal(bits(first), bits(by.dev.cpu().numpy())), ("csr_spmm twice", m, variant)
    b = DOT_SMALL[-1]
    for m in DOT_M:
        bx, by, out = run_dot(lib, b, m, 37, real=True)
        again = out_vec(lib.torch, m)
        d = lib.dev(b, True)
        lib.call("pad8_spmm_dot", b.nrows, d["orp"], d["pcol"], d["pval"], bx.ptr, bx.ld, by.ptr, by.ld, m, again[1], lib.st, 37)
        assert np.array_equal(bits(out[0].cpu().numpy()), bits(again[0].cpu().numpy())), ("pad8_spmm_dot twice", m)


# ---- 7. through the ops table ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_ops_table_takes_pad8_and_csr_on_a_matrix_without_a_form(lib, hip):
    """a symmetric matrix of mixed row lengths (1 .. ~150 entries, integer values) through hip.matrix and ops.spmm with the generic
    kernels alone (path 3): even column ranges of >= 16 columns go to pad-8 — mat_upload.hip's own pad-8 copy —, an odd origin or
    fewer than 16 columns to the CSR kernels; exact against scipy, the other columns of Y untouched"""
    import scipy.sparse as sp
    from helpers import csr_from_scipy
    n, rng = 301, np.random.default_rng(42)
    dens = np.where(np.arange(n) % 29 == 3, 0.45, np.where(np.arange(n) % 7 == 1, 0.0, 0.015))
    mask = np.triu(rng.random((n, n)) < np.maximum(dens[:, None], dens[None, :]) * (np.minimum(dens[:, None], dens[None, :]) > 0), 1)
    Uv = np.where(mask, draw(43, (n, n), False), 0.0)
    S = sp.csr_matrix(Uv + Uv.T + np.diag(draw(44, (n,), False)))
    lens = np.diff(S.indptr)
    assert lens.min() == 1 and lens.max() <= MAX_LEN and lens.max() > 64 and np.unique(lens).size > 12 and (S != S.T).nnz == 0
    A, keep = csr_from_scipy(S)
    g = hip.g
    mh = hip.matrix(A)
    try:
        g.gcge_hip_set_spmm_path(3)
        assert g.gcge_hip_mat_spmm_form(mh).decode() == "spmm_pad8"
        X, Y0 = draw(45, (n, 72), False), draw(46, (n, 72), False)
        xh = hip.mv_from_numpy(mh, X)
        for m, s0, s1 in [(64, 0, 0), (16, 2, 4), (34, 4, 2), (66, 6, 0), (18, 2, 2), (9, 1, 3), (15, 0, 0), (1, 5, 8), (2, 0, 2), (16, 1, 2), (17, 0, 0), (40, 3, 1)]:
            yh = hip.mv_from_numpy(mh, Y0)
            hip.ops.spmm(mh, xh, yh, (s0, s1), (s0 + m, s1 + m))
            got = hip.mv_to_numpy(yh, n, 0, 72)
            want = Y0.copy()
            want[:, s1:s1 + m] = S @ X[:, s0:s0 + m]
            assert np.array_equal(got, want), ("ops.spmm", m, s0, s1, np.argwhere(got != want)[:4].tolist())
            hip.ops.mv_destroy(yh, 72)
        hip.ops.mv_destroy(xh, 72)
    finally:
        g.gcge_hip_set_spmm_path(0)
        hip.free_matrix(mh)
