"""The pattern-table product and its CG passes — spmm_pattern.hip: spmm_pattern_kernel (plain), spmm_pattern_chain_kernel (chain) and
spmm_pattern_chain2_kernel (chain + line exchange), and the ring sweep of spmm_ring.hip where it takes their calls — through the raw
entries gcge_hip_pattern_spmm_vals / gcge_hip_pattern_cg_vals, on hand-built tables and EXACT data: table values, X, R, P, Q, B and all
coefficients (alpha, beta, the previous beta, scale, lambda) are nonzero integers of magnitude <= 3 (stored zeros apart), a row has at
most 16 slots, so |A x| <= 144, every updated entry is at most 3 * 144 + 12 + 9 in magnitude, every column sum below 2^18 * nrows: any
order of summation gives the same double and the comparison is np.array_equal for Y, R, PNEW, the stored B AND the sums
(test_exactness_premise_and_builder checks that premise, and the tables against scipy, on the host).

Guards: X in a block with 2^40 in the rows before and behind the matrix and in the columns beside the operand (a read outside the
table's reach shows as a huge value); every output in a block of the payload NaN that must come back bit for bit round the operand —
for a row strip also in the rows of the matrix outside the strip; read-only operands are compared bitwise after every call.

The matrices (build): row r of an nrows x nrows matrix takes value class r % classes and the ordered offset list; a slot whose column
leaves the matrix becomes (0.0, offset 0); distinct rows are numbered by first occurrence into pid (16 bit) and a table of
{double val; long off}.  Slot order as documented in spmm_pattern.hip: generic any; chain (span2 == -1) slots 0, 1, 2 = -S, 0, +S;
chain2 (span2 == -L) additionally slots 3, 4 = -L, +L; ring tables exactly [-S, 0, +S, -L, +L, -1, +1].  The streamed-values form
has the table of the offsets alone and rowval[8 r + slot].  A row strip [r0, r1) is called as spmm_rows (mat_product.hip) calls it:
d_pid + r0, x + r0 ldx, nrows = r1 - r0, the same table.

Thresholds, each from the launch code of spmm_pattern.hip (restated in test_the_case_table_reaches_the_branches):
  plain    a tile = 4 slices of 8 rows, one per wave, `line` rows apart (8: 32 consecutive rows); ntiles = cdiv(cdiv(n, line), 4) *
           line / 8; grid = min(forced grid rounded up to 8, or 1024 while span / 32 < 256, ntiles); block b walks tiles b, b + G, ..:
           cnt = cdiv(ntiles - b, G), two per loop trip — an odd cnt runs one surplus half trip, row_of clamps to the last tile and to
           nrows - 1.  Forced grids 8 and 16: cnt 1 up to 257 rows, 2 / 3 / 5 in front of 1 / 2 / 4 at 257 / 513 / 1029, 3 at 763.
  chain    lanes per row lpr = the tuned 8 / 16 / 32, halved while 2 lpr > the columns rounded up to 16 or span % (256 / lpr) != 0; a
           pass = 2 lpr columns, a tile 256 / lpr rows, grid = min(span / tile, cdiv(n, tile)), cnt = cdiv(ntl - b, grid), four per trip.
  chain2   nw = the largest of 16, 8, 4 (capped by the tuning) with span % (nw L) == 0, n >= nw L and — the strip rule,
           chain2_waves — n % (nw L) == 0 or the ragged last group not the first tile of a block; grid = min(span / (8 nw),
           cdiv(cdiv(n, L), nw) * L / 8); tile t = (group q = t / (L / 8), slice a); cnt as above, four per trip; tiles permuted over
           the XCDs when grid % 8 == 0 (runs 1) / grid % 32 == 0 (runs 2).
  passes   16 columns; all passes in one launch (gridDim.y) while passes > 1 and grid * waves <= 16 * merge (256 by default).
  ring     near > 0, lt 7, nw >= 4, cg modes 2 and 4 (products with gcge_hip_spmm_ring_product): n % 8 == 0, d_pid on 16 bytes, the
           chain2 rule on the ragged group, grid % (L / 8) == 0 where grid < tiles; products also tiles * nw * 8 == n.

Rounding bound on real data (uniform - 0.5): a row's product is lt terms, one product and lt - 1 fused additions: lt roundings; the
update behind it adds at most two (mode 3 / 7: r_new = fma(-alpha, w, r), p_new = fma(cb, p, cr r_new) with cr in {0, 1} exact; mode 7
first forms r = fma(-beta', q, p), a third rounding on a path that has none of the product's; mode 6 / 8: fl(scale x), then the
difference).  So every path to an entry carries at most lt + 2 roundings, and |result - ref| <= (lt + 3) 2^-53 times the same
expression formed from absolute values; the last unit covers the terms of second order ((lt + 2)^2 2^-106) and the longdouble
reference's own rounding (2^-64 per operation).
"""

import numpy as np
import pytest

from gcge_amd import abi
from helpers import GR, IN_GUARD, OUT_BITS, OUT_GUARD, bits, check_vec, draw, out_vec

GF = 4                                               # guard rows in front of a block (even: an odd ld alone leaves row 0 on 16 bytes)
CW = 50                                              # widths: chain2 and plain kernels up to 50 columns, the chain kernel up to 130
CHW = 130
U = np.longdouble(2.0) ** -53
PASS_M = [2, 14, 16, 18, 30, 32, 34, 50]
CHAIN_M = [2, 16, 18, 32, 34, 64, 66, 130]
PLAIN_ROWS = [1, 7, 8, 9, 31, 32, 33, 255, 256, 257, 513, 763, 1029]
C2_GEOM = [(8, 32, 4), (8, 64, 8), (8, 128, 16), (16, 256, 16), (24, 576, 8), (8, 64, 4)]     # (L, S, nw)
CG_MODES = [2, 3, 4, 5, 6, 7, 8]
FLAGS = ["all", "none", "third", "pass"]


def cdiv(a, b):
    return -(-a // b)


# ---- the matrices -----------------------------------------------------------------------------------------------------------------
class Pat:
    """One matrix: pid / table (and the offsets-only table with rowval), the scipy CSR reference, X and A X."""

    def __init__(self, name, n, offs, lt, classes, seed, span, span2, width=CW):
        assert len(offs) <= lt and len(set(offs)) == len(offs)
        self.name, self.n, self.offs, self.lt, self.seed, self.span, self.span2, self.width = name, n, list(offs), lt, seed, span, span2, width
        k = len(offs)
        cls = draw(seed, (classes, k), False)
        if classes > 1:
            cls[classes - 1, k - 1] = 0.0                           # a stored zero on a live offset
        r = np.arange(n)
        self.off = np.zeros((n, lt), dtype=np.int64)                # slots behind the list: (0.0, 0)
        self.val = np.zeros((n, lt))
        for t, o in enumerate(offs):
            ok = (r + o >= 0) & (r + o < n)
            self.off[:, t] = np.where(ok, o, 0)
            self.val[:, t] = np.where(ok, cls[r % classes, t], 0.0)
        self.pid, self.tab = self._number(np.concatenate([self.val.view(np.int64), self.off], axis=1), self.val, self.off)
        self.pid_o, self.tab_o = self._number(self.off, np.zeros_like(self.val), self.off)
        self.rowval = np.zeros((n, 8))
        if lt <= 8:
            self.rowval[:, :lt] = self.val
        self._cache = {}

    @staticmethod
    def _number(key, val, off):
        """distinct rows of key numbered by first occurrence: (pid uint16, table of npat * lt {double; long})"""
        _, first, inv = np.unique(key, axis=0, return_index=True, return_inverse=True)
        order = np.argsort(first)                                   # unique's ids -> ids by first occurrence
        rank = np.empty_like(order)
        rank[order] = np.arange(order.size)
        pid = rank[inv.ravel()]
        rows = first[order]
        tab = np.zeros(rows.size * val.shape[1], dtype=[("val", "<f8"), ("off", "<i8")])
        tab["val"], tab["off"] = val[rows].ravel(), off[rows].ravel()
        assert rows.size < 65536
        return pid.astype(np.uint16), tab

    @property
    def npat(self):
        return self.tab.size // self.lt

    def scipy(self, val=None):
        import scipy.sparse as sp
        r = np.repeat(np.arange(self.n), self.lt)
        v = (self.val if val is None else val).ravel()
        return sp.coo_matrix((v, (r, r + self.off.ravel())), shape=(self.n, self.n)).tocsr()

    def get(self, key, make):
        if key not in self._cache:
            self._cache[key] = make()
        return self._cache[key]

    def data(self, k, real=False, shape=None):
        """the k-th operand of this matrix (0: X; 1: R / Q; 2: B; 3 ..: coefficient vectors), drawn once"""
        return self.get(("data", k, real), lambda: draw(self.seed + 10 + k, shape or (self.n, self.width), real))

    def tab_real(self):
        """uniform - 0.5 in place of the table's nonzero values (npat x lt)"""
        return self.get("tab_real", lambda: np.where(self.tab["val"].reshape(-1, self.lt) != 0, draw(self.seed + 5, (self.npat, self.lt), True), 0.0))

    def val_real(self):
        return self.get("val_real", lambda: self.tab_real()[self.pid])

    def prod(self, real=False):
        """(A X, |A| |X|) over all rows: float64 from scipy on the exact data, longdouble slot by slot on the real data"""
        def make():
            X = self.data(0, real)
            if not real:
                return np.ascontiguousarray(self.scipy() @ X), None
            v, Xl, r = self.val_real().astype(np.longdouble), X.astype(np.longdouble), np.arange(self.n)
            w, ab = np.zeros(X.shape, dtype=np.longdouble), np.zeros(X.shape, dtype=np.longdouble)
            for t in range(self.lt):
                w += v[:, t, None] * Xl[r + self.off[:, t]]
                ab += np.abs(v[:, t, None]) * np.abs(Xl[r + self.off[:, t]])
            return w, ab
        return self.get(("prod", real), make)


GEN_OFFS = {7: [5, -1, 0, 17, -9, 1, -40], 8: [0, -3, 3, -64, 64, 11, -1, 2],
            16: [0, 1, -1, 2, -2, 8, -8, 9, -9, 24, -24, 64, -64, 65, -65, 7]}


def chain_offs(S, lt):
    return [-S, 0, S] + [-1, 1, 3, -7, 9, -2, 2, 5, -5, 11, -11, 13, -13][:lt - 3 - (lt == 16)]     # lt 16: one padded slot


def chain2_offs(L, S, lt):
    return [-S, 0, S, -L, L, -1, 1] + [2, -3, 3, -2, 5, -5, L + 1, -L - 1][:max(0, lt - 7 - (lt == 16))]


def c2_rows(L, S, nw):
    """k nw L + r for the residues named in the issue, k moving so that the trip counts take every value mod 4; nw L and nw L - 1"""
    grp = nw * L
    rs = [0, 1, 7, 8, L - 1, L, L + 1, (nw - 1) * L + 3]
    rows = [(1 + (i + i // 4) % 4 + (S // grp if i % 2 else 0)) * grp + r for i, r in enumerate(rs)]
    return sorted(set(rows + [grp, grp - 1, S + grp + 5, 3 * S + 2 * grp + L + 1]))


def build_tables():
    plain, chain, chain2 = [], [], []
    seed = 100
    for i, n in enumerate(PLAIN_ROWS):
        for j, lt in enumerate((7, 8, 16)):
            seed += 20
            offs = GEN_OFFS[lt]
            plain.append(Pat("gen%d_n%d" % (lt, n), n, offs, lt, 3 + (i + j) % 3, seed, max(abs(o) for o in offs), sorted(abs(o) for o in offs)[-3]))
    for S in (32, 64, 256):
        for i, n in enumerate([S + 1, 2 * S - 1, 3 * S - 5, 4 * S, 4 * S + 1, 5 * S, 300 if S < 256 else 6 * S + 77, 7 * S + 5]):
            seed += 20
            lt = (7, 8, 16)[(i + S // 32) % 3]
            chain.append(Pat("chain%d_S%d_n%d" % (lt, S, n), n, chain_offs(S, lt), lt, 2 + i % 3, seed, S, -1, width=CHW))
    for gi, (L, S, nw) in enumerate(C2_GEOM):
        for i, n in enumerate(c2_rows(L, S, nw)):
            seed += 20
            lt = (7, 8, 16)[(i + gi) % 3]
            chain2.append(Pat("c2_%d_L%d_S%d_w%d_n%d" % (lt, L, S, nw, n), n, chain2_offs(L, S, lt), lt, 2 + i % 4, seed, S, -L))
    big = [Pat("c2_7_L8_S256_n2507", 2507, chain2_offs(8, 256, 7), 7, 3, 7001, 256, -8),
           Pat("c2_16_L8_S512_n1301", 1301, chain2_offs(8, 512, 16), 16, 2, 7041, 512, -8),
           Pat("c2_8_L8_S1024_n3113", 3113, chain2_offs(8, 1024, 8), 8, 4, 7021, 1024, -8)]
    return plain, chain, chain2, big


PLAIN, CHAIN, CHAIN2, BIG = build_tables()
BY_NAME = {a.name: a for a in PLAIN + CHAIN + CHAIN2 + BIG}
# ring tables: exactly [-S, 0, +S, -L, +L, -1, +1]
RING = [Pat("ring_L16_S256_n4096", 4096, chain2_offs(16, 256, 7), 7, 3, 8001, 256, -16),
        Pat("ring_L8_S64_n512", 512, chain2_offs(8, 64, 7), 7, 2, 8021, 64, -8),
        Pat("ring_L8_S64_n1540", 1540, chain2_offs(8, 64, 7), 7, 3, 8041, 64, -8)]
# the matrix of the strip hole: 104 rows, L = 8, S = 64 (and a longer one for strips behind S + nw L)
HOLE = Pat("c2_7_L8_S64_n104", 104, chain2_offs(8, 64, 7), 7, 3, 9001, 64, -8)
LONG = Pat("c2_8_L8_S64_n700", 700, chain2_offs(8, 64, 8), 8, 4, 9021, 64, -8)


# ---- the launch arithmetic restated ------------------------------------------------------------------------------------------------
def plain_geom(n, span, forced, line=8):
    """(tiles, grid, [cnt of every block]) of the plain kernel"""
    ntiles = cdiv(cdiv(n, line), 4) * (line // 8)
    if forced > 0:
        g = cdiv(forced, 8) * 8
    elif span // 32 < 256:
        g = 1024
    else:
        raise AssertionError("no case of this file has a span that long")
    g = min(g, ntiles)
    return ntiles, g, [cdiv(ntiles - b, g) for b in range(g)]


def chain_geom(n, S, m, tuned):
    lpr = tuned
    while lpr > 8 and (2 * lpr > cdiv(m, 16) * 16 or S % (256 // lpr) != 0):
        lpr //= 2
    tr = 256 // lpr
    ntl = cdiv(n, tr)
    g = min(S // tr, ntl)
    return lpr, g, [cdiv(ntl - b, g) for b in range(g)]


def chain2_waves(n, S, L, lt, cap=16):
    """the launcher's choice of waves per block, 0: the chain or the plain kernel"""
    if not (L >= 8 and L % 8 == 0 and lt >= 5):
        return 0
    cand = cap
    while cand >= 4:
        if S % (cand * L) == 0 and n >= cand * L:
            nb = min(S // (8 * cand), cdiv(cdiv(n, L), cand) * (L // 8))
            if n % (cand * L) == 0 or (n // (cand * L)) * (L // 8) >= nb:
                return cand
        cand //= 2
    return 0


def chain2_geom(n, S, L, nw, xcd=2):
    """(grid, tiles, [cnt per block], permuted) of the chain2 kernel"""
    ntl = cdiv(cdiv(n, L), nw) * (L // 8)
    g = min(S // (8 * nw), ntl)
    perm = list(range(g))
    if xcd == 2 and g % 32 == 0:
        perm = [(b & ~31) | ((b & 7) << 2) | ((b >> 3) & 3) for b in range(g)]
    elif xcd == 1 and g % 8 == 0:
        perm = [(b & 7) * (g >> 3) + (b >> 3) for b in range(g)]
    assert sorted(perm) == list(range(g))
    return g, ntl, [cdiv(ntl - b0, g) for b0 in perm], perm != list(range(g))


def merged(m, grid, waves, merge=256):
    return cdiv(m, 16) > 1 and grid * waves <= 16 * merge


def ring_takes(n, S, L, nw, pid_aligned, product=False):
    """gcge_hip_ring_pass's geometry checks (the LDS budget is met by every table of this file: 3 planes ahead or 2)"""
    if nw < 4 or n % 8 or n < 8 or not pid_aligned:
        return False
    g, ntl, _, _ = chain2_geom(n, S, L, nw)
    if n % (nw * L) != 0 and (n // (nw * L)) * (L // 8) < g:
        return False
    if product and ntl * nw * 8 != n:
        return False
    return not (g < ntl and g % (L // 8))


# ---- 1. the premise, the builder and the table's reach, on the host ----------------------------------------------------------------
def test_exactness_premise_and_builder():
    """values and operands nonzero integers of magnitude <= 3 (stored zeros and slots outside the matrix apart), at most 16 slots: |A x|
    <= 144, updated entries <= 3 * 144 + 12 + 9, sums of squares below 2^18 per row; the table (both forms) times X equals the CSR
    product in int64; the slot layouts are the documented ones"""
    for a in PLAIN + CHAIN + CHAIN2 + BIG + RING + [HOLE, LONG]:
        assert a.lt in (7, 8, 16) and len(a.offs) <= 16 and a.pid.dtype == np.uint16 and a.tab.size == a.npat * a.lt
        X = a.data(0)
        for k in range(3):
            d = a.data(k)
            assert np.all(d == np.round(d)) and np.all(np.abs(d) <= 3) and np.all(d != 0)
        v = a.val
        assert np.all(v == np.round(v)) and np.all(np.abs(v) <= 3)
        r = np.arange(a.n)
        inside = np.zeros((a.n, a.lt), dtype=bool)
        for t, o in enumerate(a.offs):
            inside[:, t] = (r + o >= 0) & (r + o < a.n)
        assert np.all(a.off[~inside] == 0) and np.all(v[~inside] == 0) and np.all(a.off[inside] == np.broadcast_to(np.array(a.offs + [0] * (a.lt - len(a.offs))), (a.n, a.lt))[inside])
        assert np.count_nonzero(v[inside] == 0) <= cdiv(a.n, 2)                                               # the stored zero of the last class
        Xi = X.astype(np.int64)
        for pid, tab, vals in ((a.pid, a.tab, None), (a.pid_o, a.tab_o, a.rowval)):
            if vals is not None and a.lt > 8:
                continue
            off = tab["off"].reshape(-1, a.lt)[pid]
            tv = tab["val"].reshape(-1, a.lt)[pid] if vals is None else vals[:, :a.lt]
            assert vals is None or np.all(tab["val"] == 0)
            Y = np.zeros(X.shape, dtype=np.int64)
            for t in range(a.lt):
                Y += tv[:, t, None].astype(np.int64) * Xi[r + off[:, t]]
            ref = a.scipy(a.val.astype(np.int64)) @ Xi
            assert np.array_equal(Y, ref) and np.array_equal(a.prod()[0], ref) and np.max(np.abs(ref)) <= 144
            first = np.unique(pid, return_index=True)[1]
            assert np.all(np.diff(first) > 0) and pid.max() == tab.size // a.lt - 1                        # numbered by first occurrence
        assert 3 * 144 + 12 + 9 < 512 and (3 * 144 + 12) ** 2 < 2 ** 18 and 2 ** 18 * a.n < 2 ** 53
        if a.span2 < 0:
            assert a.offs[:3] == [-a.span, 0, a.span] and a.span % 32 == 0
        if a.span2 <= -8:
            assert a.offs[3:5] == [a.span2, -a.span2]
    for a in RING + [HOLE]:
        assert a.lt == 7 and a.offs == [-a.span, 0, a.span, a.span2, -a.span2, -1, 1]
    assert any(a.npat != a.tab_o.size // a.lt for a in PLAIN)       # the two forms number the rows differently
    assert sum(np.any((a.val == 0) & (a.off != 0)) for a in PLAIN + CHAIN + CHAIN2) > 60      # stored zeros on live offsets


def test_the_case_table_reaches_the_branches():
    """the launch arithmetic of spmm_pattern.hip restated (plain_geom, chain_geom, chain2_waves, chain2_geom, merged, ring_takes): what
    the tables of this file reach under the knobs the tests turn"""
    # plain kernel, grids forced to 8 and 16: the pipeline iterates; odd and even trip counts, blocks with different ones, ragged tiles
    seen = set()
    for n in PLAIN_ROWS:
        for forced in (8, 16):
            nt, g, cnts = plain_geom(n, 64, forced)
            seen |= set(cnts)
            if n <= 256:
                assert max(cnts) == 1
    assert seen >= {1, 2, 3, 4, 5}
    assert plain_geom(513, 64, 8)[2] == [3] + [2] * 7 and plain_geom(763, 64, 8)[2] == [3] * 8 and plain_geom(1029, 64, 8)[2] == [5] + [4] * 7
    assert plain_geom(257, 64, 8)[2] == [2] + [1] * 7 and all(n % 32 for n in (513, 763, 1029)) and plain_geom(1029, 64, 0)[1] == 33
    assert plain_geom(763, 64, 8, 16)[:2] == (24, 8) and plain_geom(763, 64, 8, 64)[:2] == (24, 8) and plain_geom(257, 64, 8, 64) == (16, 8, [2] * 8)
    assert {a.lt for a in PLAIN} == {7, 8, 16} and {a.n for a in PLAIN} == set(PLAIN_ROWS)
    # chain kernel: every lpr, one and several blocks, every trip count mod 4, the fallback of lpr on narrow widths
    for S in (32, 64, 256):
        for tuned in (8, 16, 32):
            mods, grids = set(), set()
            for a in CHAIN:
                if a.span == S:
                    lpr, g, cnts = chain_geom(a.n, S, 130, tuned)
                    assert lpr == tuned
                    mods |= {c % 4 for c in cnts}
                    grids.add(g)
            assert mods == {0, 1, 2, 3}, (S, tuned, mods)
            assert (S == 32 and tuned == 8) == (grids == {1})
    assert [chain_geom(300, 64, m, 32)[0] for m in CHAIN_M] == [8, 8, 16, 16, 16, 32, 32, 32]
    assert [chain_geom(300, 64, m, 16)[0] for m in CHAIN_M] == [8, 8, 16, 16, 16, 16, 16, 16]
    # chain2: every geometry with its wave count, every trip count mod 4, the rule on the ragged group, smaller wave counts
    for L, S, nw in C2_GEOM:
        mods, kinds = set(), set()
        for a in CHAIN2:
            if (a.span, -a.span2) != (S, L) or ("_w%d_" % nw) not in a.name:
                continue
            for cap in (16, 8, 4):
                w = chain2_waves(a.n, S, L, a.lt, cap)
                kinds.add(w)
                if w == min(nw, cap):
                    mods |= {c % 4 for c in chain2_geom(a.n, S, L, w)[2]}
        assert mods == {0, 1, 2, 3} and nw in kinds and 0 in kinds, (L, S, nw, mods, kinds)
        assert chain2_waves(nw * L, S, L, 7) == nw and chain2_waves(nw * L - 1, S, L, 7) in (0, nw // 2, nw // 4)
    assert chain2_geom(700, 64, 8, 4)[0] == 2 and chain2_geom(4 * 192, 576, 24, 8)[0] == 9 and chain2_geom(4096, 256, 16, 16)[0] == 2
    # the XCD maps: grids of 8 and 32 blocks, permuted under runs 1 (and 2 at 32)
    # (a grid of exactly 8 takes the branch of runs 1, whose map is then the identity; 16 blocks are the smallest it permutes)
    assert chain2_waves(2507, 256, 8, 7, 4) == 4 and chain2_geom(2507, 256, 8, 4, 1)[::3] == (8, False) and chain2_geom(2507, 256, 8, 4, 2)[3] is False
    assert chain2_waves(1301, 512, 8, 16, 4) == 4 and chain2_geom(1301, 512, 8, 4, 1)[::3] == (16, True) and chain2_geom(1301, 512, 8, 4, 2)[3] is False
    assert chain2_waves(3113, 1024, 8, 8, 4) == 4 and chain2_geom(3113, 1024, 8, 4, 2)[::3] == (32, True) and chain2_geom(3113, 1024, 8, 4, 1)[3] is True
    assert {c % 4 for x in (0, 1, 2) for c in chain2_geom(2507, 256, 8, 4, x)[2]} | {c % 4 for c in chain2_geom(3113, 1024, 8, 4, 2)[2]} >= {0, 1, 2, 3}
    # the strip hole: 40 rows from row 64 of 104 would be two blocks of 4 waves, block 1 starting on rows 32..39 with wave 1 clamped
    assert chain2_geom(40, 64, 8, 4)[:2] == (2, 2) and chain2_waves(40, 64, 8, 7) == 0 and chain2_waves(32, 64, 8, 7) == 4
    assert chain2_waves(64 + 32 + 9, 64, 8, 8) == 8 and chain2_waves(64, 64, 8, 7) == 8 and chain2_waves(63, 64, 8, 7) == 0
    # column passes: merged by default at every size here, apart with merge 0
    assert all(merged(m, 32, 16) == (m > 16) for m in PASS_M) and not any(merged(m, 32, 16, 0) for m in PASS_M)
    assert [cdiv(m, 16) for m in PASS_M] == [1, 1, 1, 2, 2, 2, 3, 4]
    # ring
    assert ring_takes(4096, 256, 16, 16, True, True) and ring_takes(512, 64, 8, 8, True, True) and ring_takes(1544 - 8, 64, 8, 8, True)
    assert not ring_takes(1540, 64, 8, 8, True) and not ring_takes(512, 64, 8, 8, False) and not ring_takes(40, 64, 8, 4, True)
    assert ring_takes(512 + 24, 256, 16, 16, True) and not ring_takes(512 + 24, 256, 16, 16, True, True)


# ---- 2. the library and the guarded operands ---------------------------------------------------------------------------------------
class RBlock:
    """rows of a matrix (GF guard rows in front, GR behind) x ld columns filled with `guard`; the operand at [0, rows) x [gl, gl + cols)
    — for an output only the rows [r0, r1) of it, the other rows keep the guard"""

    def __init__(self, torch, data, guard, gl=2, odd_ld=False, r0=0, r1=None, whole=False):
        rows, cols = data.shape
        r1 = rows if r1 is None else r1
        self.rows, self.cols, self.gl, self.guard, self.r0, self.r1 = rows, cols, gl, guard, r0, r1
        self.ld = gl + cols + 2
        if (self.ld % 2 == 1) != odd_ld:
            self.ld += 1
        self.host = np.full((GF + rows + GR, self.ld), guard)
        if whole:                                                   # X: every row of the matrix, the pointer on row r0
            self.host[GF:GF + rows, gl:gl + cols] = data
        else:
            self.host[GF + r0:GF + r1, gl:gl + cols] = data[r0:r1]
        self.dev = torch.from_numpy(self.host).cuda()
        self.ptr = self.dev.data_ptr() + 8 * ((GF + r0) * self.ld + gl)

    def got(self):
        return self.dev.cpu().numpy()

    def check(self, ref, what, bound=None):
        """rows [r0, r1) of the operand == ref (or within bound of it), everything else bit for bit what it was"""
        got = self.got()
        op = got[GF + self.r0:GF + self.r1, self.gl:self.gl + self.cols]
        if bound is None:
            assert np.array_equal(op, ref), (what, "operand", np.argwhere(op != ref)[:4].tolist())
        else:
            err = np.abs(op.astype(np.longdouble) - ref)
            assert np.all(err <= bound), (what, float(np.max(err / np.maximum(bound, np.longdouble(1e-300)))))
        got[GF + self.r0:GF + self.r1, self.gl:self.gl + self.cols] = self.host[GF + self.r0:GF + self.r1, self.gl:self.gl + self.cols]
        assert np.array_equal(bits(got), bits(self.host)), (what, "guard", np.argwhere(bits(got) != bits(self.host))[:4].tolist())

    def unchanged(self, what):
        assert np.array_equal(bits(self.got()), bits(self.host)), (what, "a block that is only read, or a whole output on a decline, was written")


class Lib:
    def __init__(self, hip):
        import torch
        self.torch, self.hip, g = torch, hip, hip.g
        self.g = g
        self.st = g.gcge_hip_stream()
        self.devs = {}

    def defaults(self):
        g = self.g
        g.gcge_hip_spmm_pattern_tune(0)
        g.gcge_hip_spmm_pattern_tune_line(8)
        g.gcge_hip_spmm_chain_tune(8)
        g.gcge_hip_spmm_chain2_tune(16)
        g.gcge_hip_spmm_chain2_xcd(2)
        g.gcge_hip_spmm_pass_merge(256)
        g.gcge_hip_cg_pass_streams(0)
        g.gcge_hip_spmm_ring_tune(1, 3)
        g.gcge_hip_spmm_ring_product(0)
        g.gcge_hip_spmm_ring_wide(0)
        g.gcge_hip_spmm_ring_xcd(2)
        self.hip.sync()
        self.devs = {}

    def dev(self, a, vals, real):
        """device copies of (pid, table, rowval), kept until the test ends; 16 spare entries behind each"""
        def make():
            t = self.torch
            pid, tab = (a.pid_o, a.tab_o) if vals else (a.pid, a.tab)
            if real and not vals:
                tab = tab.copy()
                tab["val"] = a.tab_real().ravel()
            rv = a.val_real() if real else a.val
            rowval = np.zeros((a.n + 2, 8))
            rowval[:a.n, :min(a.lt, 8)] = rv[:, :8]
            keep = [t.from_numpy(np.concatenate([pid, np.zeros(16, dtype=np.uint16)]).view(np.int16)).cuda(),
                    t.from_numpy(np.concatenate([tab, np.zeros(16, dtype=tab.dtype)]).view(np.int64)).cuda(), t.from_numpy(rowval).cuda()]
            return {"pid": keep[0].data_ptr(), "tab": keep[1].data_ptr(), "rowval": keep[2].data_ptr() if vals else None, "npat": tab.size // a.lt}, keep
        key = (id(a), vals, real)
        if key not in self.devs:
            self.devs[key] = make()
        return self.devs[key][0]

    def cvec(self, data, dtype=np.float64):
        """a coefficient vector with two guard entries in front and 16 behind: (tensor, pointer of element 0)"""
        g = IN_GUARD if dtype == np.float64 else 1
        host = np.concatenate([[g, g] if dtype == np.float64 else [g] * 4, np.asarray(data), [g] * 16]).astype(dtype)
        dev = self.torch.from_numpy(host).cuda()
        return dev, dev.data_ptr() + 16, host

    def call(self, name, *args, expect=0):
        self.torch.cuda.synchronize()
        assert "gcge_hip_pattern_" + name in abi.HIP, name          # a name composed here escapes test_abi's source scan
        rc = getattr(self.g, "gcge_hip_pattern_" + name)(*args)
        self.hip.sync()
        assert rc == expect, (name, rc, expect)


@pytest.fixture(scope="module")
def lib_(hip):
    return Lib(hip)


@pytest.fixture
def lib(lib_):
    """every knob at its default before the test and — whether the test passed or not — behind it"""
    lib_.defaults()
    yield lib_
    lib_.defaults()


def flags_of(kind, m):
    f = np.ones(m, dtype=np.int32)
    if kind == "none":
        f[:] = 0
    elif kind == "third":
        f[1::3] = 0
    elif kind == "pass":
        f[(16 if m >= 32 else 0):(32 if m >= 32 else 16)] = 0          # one whole 16-column pass
    return f


def run(lib, a, mode, m, r0=0, r1=None, vals=False, near=0, real=False, flag="all", alone=False, xgl=2, yy=True, again=None):
    """one call of the entry for `mode` on rows [r0, r1) of a, every result checked (exact data: np.array_equal; real data: the bound
    of the header); again: the dict a former call returned — the outputs must have the same bits.  Returns {name: bits}"""
    n = a.n
    r1 = n if r1 is None else r1
    nr, lt = r1 - r0, a.lt
    d = lib.dev(a, vals, real)
    T = lib.torch
    what = (a.name, "mode", mode, "m", m, "rows", r0, r1, "vals", vals, "near", near, "real", real, flag, alone)
    Xf = a.data(0, real)[:, :m]
    bx = RBlock(T, Xf, IN_GUARD, gl=xgl, r0=r0, r1=r1, whole=True)
    wf, abf = a.prod(real)
    w = wf[r0:r1, :m]
    ab = abf[r0:r1, :m] if real else None
    LD = np.longdouble if real else np.float64
    X = Xf[r0:r1].astype(LD)
    eps = (lt + 3) * U
    pid, rowval = d["pid"] + 2 * r0, (d["rowval"] + 64 * r0 if vals else None)
    nearv = max(abs(o) for o in a.offs) if near else 0
    geo = (d["tab"], d["npat"], lt, a.span, a.span2)
    ro, outs, sums = [bx], {}, {}
    dots = out_vec(T, m)

    def done(blocks, dref, yref=None, dyy=None):
        for name, (blk, ref, bound) in blocks.items():
            blk.check(ref, what + (name,), bound)
            outs[name] = bits(blk.got()).copy()
        for b in ro:
            b.unchanged(what)
        if not real:
            check_vec(dots, dref, what + ("sums",))
            if dyy is not None:
                check_vec(dyy, yref, what + ("sums yy",))
        else:   # finite, and the guards round them
            gd = dots[0].cpu().numpy()
            assert np.all(np.isfinite(gd[2:2 + m])) and np.all(bits(gd[:2]) == OUT_BITS) and np.all(bits(gd[2 + m:]) == OUT_BITS), what
        outs["sums"] = bits(dots[0].cpu().numpy()).copy()
        if dyy is not None:
            outs["sums yy"] = bits(dyy[0].cpu().numpy()).copy()
        if again is not None:
            for k, v in outs.items():
                assert np.array_equal(v, again[k]), (what, k, "not the same bits")
        return outs

    def out(r0_=r0, gl=2):
        return RBlock(T, np.full((n, m), OUT_GUARD), OUT_GUARD, gl=gl, r0=r0_, r1=r1)

    if mode <= 1:
        by = out()
        dyy = out_vec(T, m) if (mode == 1 and yy) else None
        lib.call("spmm_vals", nr, pid, *geo, bx.ptr, bx.ld, by.ptr, by.ld, m, dots[1] if mode == 1 else None, dyy[1] if dyy else None, lib.st, nearv, rowval)
        if mode == 0:
            assert np.all(bits(dots[0].cpu().numpy()) == OUT_BITS), what
            by.check(w, what, eps * ab if real else None)
            bx.unchanged(what)
            outs["Y"] = bits(by.got()).copy()
            if again is not None:
                assert np.array_equal(outs["Y"], again["Y"]), (what, "not the same bits")
            return outs
        return done({"Y": (by, w, eps * ab if real else None)}, (X * w).sum(axis=0), (w * w).sum(axis=0), dyy)

    def cg(r, pnew, alpha=None, beta=None, flg=None, b=None, dyy=None):
        lib.call("cg_vals", mode, nr, pid, *geo, bx.ptr, bx.ld, r.ptr if r else None, r.ld if r else 0, pnew.ptr if pnew else None, pnew.ld if pnew else 0, m,
                 alpha, beta, flg, dots[1], dyy, lib.st, b.ptr if isinstance(b, RBlock) else b, b.ld if isinstance(b, RBlock) else 0, nearv, rowval)

    coef = lambda k: a.data(3 + k, real, (CHW,))[:m]
    if mode == 2:
        dyy = out_vec(T, m) if yy else None
        cg(None, None, dyy=dyy[1] if dyy else None)
        return done({}, (X * w).sum(axis=0), (w * w).sum(axis=0), dyy)
    if mode == 4:
        lam = lib.cvec(coef(0))
        cg(None, None, alpha=lam[1])
        q = w - coef(0).astype(LD) * X
        assert np.array_equal(bits(lam[0].cpu().numpy()), bits(lam[2])), what
        return done({}, (q * q).sum(axis=0))
    if mode in (3, 7):
        f = flags_of(flag, m)
        al, be, fl = lib.cvec(coef(0)), lib.cvec(coef(1)), lib.cvec(f, np.int32)
        alc, cb, cr = np.where(f, coef(0), 0.0).astype(LD), np.where(f, coef(1), 1.0).astype(LD), f.astype(LD)
        Rf = a.data(1, real)[:, :m]
        R = Rf[r0:r1].astype(LD)
        pn = out(gl=4)
        if mode == 3:
            rb = RBlock(T, Rf, OUT_GUARD, r0=r0, r1=r1)
            cg(rb, pn, al[1], be[1], fl[1])
            rn = R - alc * w
            rab = np.abs(R) + np.abs(alc) * ab if real else None
            blocks = {"R": (rb, rn, eps * rab if real else None)}
        else:
            qb = RBlock(T, Rf, IN_GUARD, r0=r0, r1=r1)              # p_{k-1}: read only
            bp = lib.cvec(coef(2))
            ro.append(qb)
            cg(qb, pn, al[1], be[1], fl[1], b=bp[1])
            bpv = coef(2).astype(LD)
            rn = (X - bpv * R) - alc * w
            rab = np.abs(X) + np.abs(bpv) * np.abs(R) + np.abs(alc) * ab if real else None
            blocks = {}
            assert np.array_equal(bits(bp[0].cpu().numpy()), bits(bp[2])), what
        pref = cr * rn + cb * X
        blocks["PNEW"] = (pn, pref, eps * (cr * rab + np.abs(cb) * np.abs(X)) if real else None)
        for v in (al, be, fl):
            assert np.array_equal(v[0].cpu().numpy().view(np.uint8), v[2].view(np.uint8)), what
        res = done(blocks, (cr * rn * rn).sum(axis=0))
        if not real:   # retired columns: R as it was, PNEW a copy of X, bit for bit
            ret = np.nonzero(f == 0)[0]
            gp = pn.got()[GF + r0:GF + r1, 4:4 + m]
            assert np.array_equal(bits(np.ascontiguousarray(gp[:, ret])), bits(np.ascontiguousarray(Xf[r0:r1][:, ret]))), what
            if mode == 3:
                gr = rb.got()[GF + r0:GF + r1, 2:2 + m]
                assert np.array_equal(bits(np.ascontiguousarray(gr[:, ret])), bits(np.ascontiguousarray(Rf[r0:r1][:, ret]))), what
        return res
    # modes 5, 6, 8
    rb = out()
    pn = rb if alone else out(gl=4)
    sc = lib.cvec(coef(0))
    if mode == 5:
        Bf = a.data(2, real)[:, :m]
        bb = RBlock(T, Bf, IN_GUARD, gl=4, r0=r0, r1=r1)
        ro.append(bb)
        cg(rb, pn, b=bb)
        B = Bf[r0:r1].astype(LD)
        bab = np.abs(B)
    else:
        bb = out(gl=6) if mode == 8 else None
        cg(rb, pn, alpha=sc[1], b=bb)
        B = coef(0).astype(LD) * X
        bab = np.abs(B)
        assert np.array_equal(bits(sc[0].cpu().numpy()), bits(sc[2])), what
    rn = B - w
    bound = eps * (bab + ab) if real else None
    blocks = {"R": (rb, rn, bound)}
    if not alone:
        blocks["PNEW"] = (pn, rn, bound)
    if mode == 8:   # the stored right-hand side: the once-rounded product itself
        blocks["B"] = (bb, (coef(0) * Xf[r0:r1]) if real else B, np.zeros(B.shape, dtype=np.longdouble) if real else None)
    return done(blocks, (rn * rn).sum(axis=0))


def cyc(seq, i):
    return seq[i % len(seq)]


def strips_of(a, i):
    """the whole matrix and, where it is long enough, a strip with odd ends inside it"""
    return [(0, a.n)] + ([(2 * (i % 5) + 3, a.n - 2 * (i % 3) - 1)] if a.n >= 31 and i % 2 else [])


# ---- 3. the plain kernel -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1] + CG_MODES)
def test_plain_kernel_over_row_counts(lib, mode):
    """span2 >= 0 (and chain-layout tables with streamed values or in a CG mode, which the launcher sends here), the grid forced to 8 and
    16 so that the double-buffered walk iterates; lines of 8, 16 and 64; lt 7, 8, 16; table and streamed values; odd-ended strips"""
    k = 0
    for ai, a in enumerate(PLAIN):
        for forced in (8, 16):
            k += 1
            lib.g.gcge_hip_spmm_pattern_tune(forced)
            lib.g.gcge_hip_spmm_pattern_tune_line(cyc([8, 8, 16, 64], k))
            for r0, r1 in strips_of(a, k):
                run(lib, a, mode, cyc(PASS_M, k + ai), r0, r1, vals=(a.lt <= 8 and k % 3 == 0), flag=cyc(FLAGS, k), alone=(k % 4 == 1), xgl=cyc([2, 4], k))
    lib.g.gcge_hip_spmm_pattern_tune_line(8)
    for k, a in enumerate(CHAIN + [HOLE, LONG]):                   # chain-layout tables on the plain kernel
        if a.lt > 8 and mode <= 1:
            continue
        lib.g.gcge_hip_spmm_pattern_tune(cyc([8, 16, 0], k))
        lib.g.gcge_hip_spmm_chain2_tune(0)                          # (chain2 tables: no line exchange)
        S = a.span
        rows = [(0, a.n)] + ([(S, min(a.n - 3, 3 * S + 9))] if a.n > 2 * S + 8 else [])
        for r0, r1 in rows:
            run(lib, a, mode, cyc(PASS_M, k), r0, r1, vals=(a.lt <= 8 and (mode <= 1 or k % 2 == 0)), flag=cyc(FLAGS, k))


# ---- 4. the chain kernel -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("lpr", [8, 16, 32])
def test_chain_kernel_over_row_counts(lib, lpr):
    """span2 == -1, modes 0 and 1: S = 32, 64, 256, trip counts of every value mod 4 with ragged ends, pass widths 16 / 32 / 64 with a
    narrow last pass and the fallback of the lanes per row; strips from a multiple of S"""
    lib.g.gcge_hip_spmm_chain_tune(lpr)
    for k, a in enumerate(CHAIN):
        S = a.span
        rows = [(0, a.n)] + ([(S, 3 * S + 9), (2 * S, a.n - 5)] if a.n > 4 * S else [])
        for r0, r1 in rows:
            ms = CHAIN_M if a.n in (300, 6 * S + 77) and r0 == 0 else [cyc(CHAIN_M, k + j * 3 + r0) for j in range(2)]
            for j, m in enumerate(ms):
                run(lib, a, (k + j) % 2, m, r0, r1, yy=(j % 2 == 0))


# ---- 5. the chain2 kernel ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1] + CG_MODES)
def test_chain2_kernel_over_row_counts(lib, mode):
    """span2 == -L: every geometry of C2_GEOM at row counts k nw L + r, the wave count as found and forced down to 8 and 4, the three
    XCD maps; lt 7, 8, 16; table and streamed values"""
    k = 0
    for ai, a in enumerate(CHAIN2):
        found = set()
        for cap in (16, 8, 4):
            w = chain2_waves(a.n, a.span, -a.span2, a.lt, cap)
            if w in found:                                          # (the same launch as under the larger cap)
                continue
            found.add(w)
            k += 1
            lib.g.gcge_hip_spmm_chain2_tune(cap)
            lib.g.gcge_hip_spmm_chain2_xcd(k % 3)
            run(lib, a, mode, cyc(PASS_M, k + ai), vals=(a.lt <= 8 and k % 3 == 1), flag=cyc(FLAGS, k), alone=(k % 4 == 1), xgl=cyc([2, 4], k))


@pytest.mark.gpu
@pytest.mark.parametrize("xcd", [0, 1, 2])
def test_chain2_xcd_tile_maps(lib, xcd):
    """grids of 8 (S = 256), 16 (S = 512) and 32 blocks (S = 1024) of 4 waves: the permutations of runs 1 (grid % 8 == 0) and 2
    (grid % 32 == 0), every mode, merged passes and single ones"""
    lib.g.gcge_hip_spmm_chain2_tune(4)
    lib.g.gcge_hip_spmm_chain2_xcd(xcd)
    for ai, a in enumerate(BIG):
        for k, mode in enumerate([0, 1] + CG_MODES):
            lib.g.gcge_hip_spmm_pass_merge(cyc([256, 0], k + ai))
            run(lib, a, mode, cyc([16, 34, 50, 2], k + ai + xcd), vals=(a.lt <= 8 and k % 2 == 1), flag=cyc(FLAGS, k + xcd), alone=(k % 2 == 0))


# ---- 6. row strips -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1] + CG_MODES)
def test_row_strips_on_chain2_tables(lib, mode):
    """strips that begin on a multiple of S and end inside the matrix: 40 rows of 104 (L = 8, S = 64: with 4 waves block 1 would start on
    the ragged group, its wave 0 taking X[nrows - 1] from the clamped wave 1 for its +L row — chain2_waves keeps the exchange off it),
    multiples and non-multiples of nw L, a strip longer than S + nw L with a ragged end; every wave count"""
    for cap in (16, 8, 4):
        lib.g.gcge_hip_spmm_chain2_tune(cap)
        for vals in (False, True):
            run(lib, HOLE, mode, 16, 64, 104, vals=vals, flag="third")
            run(lib, HOLE, mode, 18, 0, 40, vals=vals, flag="third")
            run(lib, HOLE, mode, 16, 0, 64, vals=vals)
        for k, (r0, r1) in enumerate([(64, 64 + 32), (64, 64 + 40), (64, 64 + 64 + 32 + 13), (128, 128 + 96), (64, 64 + 70), (192, 192 + 320 + 27), (0, 64 + 35), (64, 699)]):
            run(lib, LONG, mode, cyc(PASS_M, k + cap), r0, r1, vals=(k % 2 == 0), flag=cyc(FLAGS, k), alone=(k % 2 == 1))
        for a in BIG:
            S = a.span
            run(lib, a, mode, 18, S, 2 * S + 4 * 8 * 3 + 5, flag="pass")


# ---- 7. column passes: merged, apart, on side streams ------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["plain", "chain2"])
def test_column_passes_merged_apart_and_on_side_streams(lib, kernel):
    """2 .. 50 columns, real data: the passes in one launch (merge 256), apart (merge 0) and apart on 2 and 4 side streams give the
    same bits — results and sums; and the exact data under each setting"""
    a = BY_NAME["gen8_n763"] if kernel == "plain" else LONG
    if kernel == "plain":
        lib.g.gcge_hip_spmm_pattern_tune(8)
    for real in (True, False):
        for k, m in enumerate(PASS_M):
            for mode in [1] + CG_MODES:
                kw = dict(real=real, flag=cyc(FLAGS, k + mode), vals=(k % 2 == 1))
                lib.g.gcge_hip_spmm_pass_merge(256)
                lib.g.gcge_hip_cg_pass_streams(0)
                first = run(lib, a, mode, m, **kw)
                lib.g.gcge_hip_spmm_pass_merge(0)
                for streams in (0, 2, 4):
                    if streams and (mode == 1 or not real):
                        continue
                    lib.g.gcge_hip_cg_pass_streams(streams)
                    run(lib, a, mode, m, again=first, **kw)


# ---- 8. the ring ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1, 2, 4])
def test_ring_takes_or_declines_with_the_same_results(lib, mode):
    """near > 0 on [-S, 0, +S, -L, +L, -1, +1] tables: whether gcge_hip_ring_pass takes the call (gcge_hip_spmm_ring_launches counts the
    passes) or declines — nrows % 8 != 0, d_pid off 16 bytes, the ring switched off — the exact results are the same"""
    g = lib.g
    g.gcge_hip_spmm_ring_product(1)
    cases = []
    for a in RING:
        S, L = a.span, -a.span2
        cases += [(a, 0, a.n), (a, S, min(a.n, 5 * S)), (a, S, min(a.n, 4 * S + 24)), (a, S + 4, S + 4 + 2 * S), (a, 2 * S, 4 * S - 3)]
    for k, (a, r0, r1) in enumerate(cases):
        S, L = a.span, -a.span2
        for m in (16, 34):
            for on in (1, 0):
                g.gcge_hip_spmm_ring_tune(on, 3 - k % 2)
                nw = chain2_waves(r1 - r0, S, L, 7)
                takes = bool(on) and ring_takes(r1 - r0, S, L, nw, (2 * r0) % 16 == 0, product=mode <= 1)
                n0 = g.gcge_hip_spmm_ring_launches()
                run(lib, a, mode, m, r0, r1, near=1)
                took = g.gcge_hip_spmm_ring_launches() - n0
                assert took == (cdiv(m, 16) if takes else 0), (a.name, mode, r0, r1, m, on, took, takes)
    taken = [ring_takes(r1 - r0, a.span, -a.span2, chain2_waves(r1 - r0, a.span, -a.span2, 7), (2 * r0) % 16 == 0) for a, r0, r1 in cases]
    assert any(taken) and not all(taken)


# ---- 9. declines and empty calls ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_declines_leave_every_output_alone(lib):
    """every -1 of gcge_hip_pattern_spmm_vals / gcge_hip_pattern_cg_vals: no block and no sum is written"""
    T = lib.torch
    a = BY_NAME["gen7_n257"]
    ch = next(c for c in CHAIN if c.lt == 7)
    n, m = a.n, 16
    d, dv = lib.dev(a, False, False), lib.dev(a, True, False)
    geo = lambda dd=d, lt=7, npat=None, span=a.span, span2=a.span2: (dd["pid"], dd["tab"], dd["npat"] if npat is None else npat, lt, span, span2)
    big = T.zeros(700 * 16 * 2, dtype=T.float64).cuda()             # a table of up to 700 patterns of 16 slots (never read)

    def blocks(odd=None, off=None):
        """x, y / r, pnew, b with one of them on an odd ld or an odd origin"""
        mk = lambda name, guard, gl: RBlock(T, a.data(0)[:, :m] if guard == IN_GUARD else np.full((n, m), OUT_GUARD), guard,
                                           gl=gl + (1 if off == name else 0), odd_ld=(odd == name))
        return {"x": mk("x", IN_GUARD, 2), "r": mk("r", OUT_GUARD, 2), "p": mk("p", OUT_GUARD, 4), "b": mk("b", OUT_GUARD, 6)}

    def spmm(B, expect=-1, g=None, ncols=m, rowval=None, dots=True):
        dd = out_vec(T, m)
        lib.call("spmm_vals", n, *(g or geo()), B["x"].ptr, B["x"].ld, B["r"].ptr, B["r"].ld, ncols, dd[1] if dots else None, None, lib.st, 0, rowval, expect=expect)
        if expect == -1:
            for blk in B.values():
                blk.unchanged(("spmm declines", ncols))
            assert np.all(bits(dd[0].cpu().numpy()) == OUT_BITS)

    co = lib.cvec(a.data(3, False, (CHW,))[:m])
    fl = lib.cvec(np.ones(m, dtype=np.int32), np.int32)

    def cg(mode, B, expect=-1, g=None, ncols=m, alpha=True, b="blk", dots=True, r="r", p="p", x="x", rowval=None, nrows=n):
        dd, dy = out_vec(T, m), out_vec(T, m)
        bptr = {"blk": B["b"].ptr, "vec": co[1], None: None, "x": B["x"].ptr, "r": B["r"].ptr, "p": B["p"].ptr}[b]
        lib.call("cg_vals", mode, nrows, *(g or geo()), B[x].ptr, B[x].ld, B[r].ptr, B[r].ld, B[p].ptr, B[p].ld, ncols, co[1] if alpha else None, co[1], fl[1],
                 dd[1] if dots else None, dy[1], lib.st, bptr, B["b"].ld, 0, rowval, expect=expect)
        for blk in B.values():
            blk.unchanged(("cg declines", mode))
        return dd, dy

    def untouched(v):
        assert np.all(bits(v[0].cpu().numpy()) == OUT_BITS)

    # the product
    spmm(blocks(), ncols=15)
    for name in ("x", "r"):
        spmm(blocks(odd=name))
        spmm(blocks(off=name))
    spmm(blocks(), g=(d["pid"], big.data_ptr(), 586, 7, a.span, a.span2))
    spmm(blocks(), g=(d["pid"], big.data_ptr(), 257, 16, a.span, a.span2))
    assert 585 * 7 * 16 <= 64 * 1024 < 586 * 7 * 16 and 256 * 16 * 16 <= 64 * 1024 < 257 * 16 * 16
    spmm(blocks(), g=geo(lt=16), rowval=dv["rowval"])
    for lt in (6, 9, 15, 17, 0):
        spmm(blocks(), g=geo(lt=lt))
    dch = lib.dev(ch, False, False)
    spmm(blocks(), g=(dch["pid"], dch["tab"], dch["npat"], 7, 48, -1))          # a chain table whose span is no multiple of 32
    # the CG passes
    for mode in (0, 1, 9, -1):
        untouched(cg(mode, blocks())[0])
    for mode in CG_MODES:
        untouched(cg(mode, blocks(), ncols=15)[0])
        untouched(cg(mode, blocks(odd="x"))[0])
        untouched(cg(mode, blocks(off="x"))[0])
        cg(mode, blocks(), dots=False)
        untouched(cg(mode, blocks(), g=(d["pid"], big.data_ptr(), 586, 7, a.span, a.span2))[0])
        untouched(cg(mode, blocks(), g=geo(lt=16), rowval=dv["rowval"])[0])
        untouched(cg(mode, blocks(), g=geo(lt=9))[0])
    for mode in (3, 5, 6, 7, 8):
        for name in ("r", "p"):
            untouched(cg(mode, blocks(odd=name), b="vec" if mode == 7 else "blk")[0])
            untouched(cg(mode, blocks(off=name), b="vec" if mode == 7 else "blk")[0])
        untouched(cg(mode, blocks(), p="x", b="vec" if mode == 7 else "blk")[0])               # pnew == x
    for mode in (3, 5, 6, 8):
        untouched(cg(mode, blocks(), r="x")[0])                                                # r == x
    untouched(cg(7, blocks(), p="r", b="vec")[0])                                              # mode 7: pnew == r
    for mode in (6, 8):
        untouched(cg(mode, blocks(), alpha=False)[0])
    for mode in (5, 7, 8):
        untouched(cg(mode, blocks(), b=None)[0])
    for mode in (5, 8):
        untouched(cg(mode, blocks(odd="b"))[0])
        untouched(cg(mode, blocks(off="b"))[0])
    for b in ("x", "r", "p"):
        untouched(cg(8, blocks(), b=b)[0])                                                     # mode 8: b its own block


@pytest.mark.gpu
def test_the_largest_table_is_taken(lib):
    """585 patterns of 7 slots (65520 bytes of LDS) and 256 of 16 slots: the tables just below the 64 KiB the entries refuse above"""
    for name, npat in (("gen7_n257", 585), ("gen16_n257", 256)):
        a = BY_NAME[name]
        assert a.npat < npat
        d = lib.dev(a, False, False)
        T = lib.torch
        tab = np.concatenate([a.tab, np.tile(a.tab[:a.lt], npat - a.npat)])
        t = T.from_numpy(tab.view(np.int64)).cuda()
        bx = RBlock(T, a.data(0)[:, :16], IN_GUARD)
        by = RBlock(T, np.full((a.n, 16), OUT_GUARD), OUT_GUARD)
        lib.call("spmm_vals", a.n, d["pid"], t.data_ptr(), npat, a.lt, a.span, a.span2, bx.ptr, bx.ld, by.ptr, by.ld, 16, None, None, lib.st, 0, None)
        by.check(a.prod()[0][:, :16], (name, npat))


def guards_kept(v, what):
    got = v[0].cpu().numpy()
    assert np.all(bits(got[:2]) == OUT_BITS) and np.all(bits(got[2 + v[2]:]) == OUT_BITS), (what, "guard round the sums")


@pytest.mark.gpu
def test_no_rows_and_no_columns(lib):
    """nrows == 0 and ncols == 0 return 0 and write no block; with no rows the sums are 0 (gcge_hip_resid_sq's rule), with no columns
    nothing at all is written"""
    T = lib.torch
    a = BY_NAME["gen7_n257"]
    d = lib.dev(a, False, False)
    m = 16
    geo = (d["pid"], d["tab"], d["npat"], 7, a.span, a.span2)
    co = lib.cvec(a.data(3, False, (CHW,))[:m])
    fl = lib.cvec(np.ones(m, dtype=np.int32), np.int32)
    for nrows, ncols in ((0, m), (a.n, 0), (0, 0), (-3, m)):
        bx = RBlock(T, a.data(0)[:, :m], IN_GUARD)
        outs = [RBlock(T, np.full((a.n, m), OUT_GUARD), OUT_GUARD, gl=gl) for gl in (2, 4, 6)]
        for both in (True, False):
            dd, dy = out_vec(T, m), out_vec(T, m)
            lib.call("spmm_vals", nrows, *geo, bx.ptr, bx.ld, outs[0].ptr, outs[0].ld, ncols, dd[1], dy[1] if both else None, lib.st, 0, None)
            zero = np.zeros(m) if ncols > 0 else np.full(m, OUT_GUARD)
            for v, z in ((dd, zero), (dy, zero if both else np.full(m, OUT_GUARD))):
                assert np.array_equal(bits(v[0].cpu().numpy()[2:2 + m]), bits(z)), ("spmm_vals", nrows, ncols, both)
                guards_kept(v, ("spmm_vals guards", nrows, ncols))
        for mode in CG_MODES:
            dd, dy = out_vec(T, m), out_vec(T, m)
            lib.call("cg_vals", mode, nrows, *geo, bx.ptr, bx.ld, outs[0].ptr, outs[0].ld, outs[1].ptr, outs[1].ld, ncols, co[1], co[1], fl[1], dd[1], dy[1], lib.st,
                     outs[2].ptr if mode != 7 else co[1], outs[2].ld, 0, None)
            zero = np.zeros(m) if ncols > 0 else np.full(m, OUT_GUARD)
            assert np.array_equal(bits(dd[0].cpu().numpy()[2:2 + m]), bits(zero)), ("cg_vals", mode, nrows, ncols)
            assert np.array_equal(bits(dy[0].cpu().numpy()[2:2 + m]), bits(zero if mode == 2 else np.full(m, OUT_GUARD))), ("cg_vals yy", mode, nrows, ncols)
            guards_kept(dd, ("cg_vals guards", mode))
        for b in outs + [bx]:
            b.unchanged(("no rows / no columns", nrows, ncols))


# ---- 10. real data -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["plain", "chain", "chain2"])
def test_real_data_bound_same_bits_and_the_formed_rhs(lib, kernel):
    """uniform - 0.5 at one ragged size per kernel: Y and the updated blocks within (lt + 3) 2^-53 of the longdouble reference (header);
    the same call twice gives the same bits; mode 6 equals mode 5 fed with B = fl(scale X) formed in numpy, bit for bit, and mode 8
    stores exactly that B"""
    if kernel == "plain":
        lib.g.gcge_hip_spmm_pattern_tune(8)
        mats = [BY_NAME["gen7_n763"], BY_NAME["gen8_n763"], BY_NAME["gen16_n763"]]
    elif kernel == "chain":
        mats = [next(a for a in CHAIN if a.n == 300 and a.span == 64)]
    else:
        mats = [LONG, BIG[0], next(a for a in CHAIN2 if a.lt == 16 and a.n > 300)]
    for a in mats:
        modes = [0, 1] if kernel == "chain" else [0, 1] + CG_MODES
        for k, m in enumerate((18, 34) if kernel != "chain" else (18, 66, 130)):
            for mode in modes:
                if kernel == "chain":
                    lib.g.gcge_hip_spmm_chain_tune(cyc([8, 16, 32], k))
                kw = dict(real=True, flag=cyc(FLAGS[2:], k + mode), vals=(a.lt <= 8 and (k + mode) % 2 == 1), r1=a.n - 3 * k)
                first = run(lib, a, mode, m, **kw)
                run(lib, a, mode, m, again=first, **kw)
            if kernel == "chain":
                continue
            # mode 5 fed with fl(scale X)
            r1 = a.n - 3 * k
            six, eight = run(lib, a, 6, m, real=True, r1=r1), run(lib, a, 8, m, real=True, r1=r1)
            X, sc = a.data(0, True)[:, :m], a.data(3, True, (CHW,))[:m]
            saved = a._cache[("data", 2, True)] if ("data", 2, True) in a._cache else None
            B = np.zeros((a.n, a.width))
            B[:, :m] = sc * X
            a._cache[("data", 2, True)] = B
            try:
                five = run(lib, a, 5, m, real=True, r1=r1)
            finally:
                if saved is None:
                    del a._cache[("data", 2, True)]
                else:
                    a._cache[("data", 2, True)] = saved
            for name in ("R", "PNEW", "sums"):
                assert np.array_equal(six[name], five[name]) and np.array_equal(eight[name], five[name]), (a.name, m, name, "mode 6 / 8 against mode 5")
