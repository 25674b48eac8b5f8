"""The dense block kernels (gram_mfma.hip, lincomb_mfma.hip, the panel / column kernels of vec_kernels.hip) over row counts,
through their raw-pointer entry points, on EXACT data: every operand holds nonzero integers of magnitude <= 3, coefficients and
scale factors are integers (mgs_step's s a power of two), so every product and partial sum is an integer far below 2^53 and any
order of summation, on FMA or MFMA and split over any number of chunks, gives the same double.  The reference is plain numpy and the
comparison np.array_equal: a row that is dropped, counted twice or taken from the wrong chunk, or a column taken from the wrong
place, changes an output by a nonzero integer.  (test_exactness_of_the_case_table checks that premise on the host.)

Every operand sits in a block larger than itself — GR rows behind nrows, one or two columns on either side inside ld.  Input blocks
carry 2^40 there (finite: both panel-update forms let clamped columns meet zero coefficients); a guard that leaks into a sum shifts
it by a multiple of 2^40.  Output blocks carry a NaN with a payload of its own, which must come back bit for bit.

Row thresholds, each derived from the launch code (cdiv = rounding-up division):

  gcge_hip_gram          nchunks = max(64, 512 / (gy tj)), rpc = max(64, cdiv(cdiv(n, nchunks), 64) 64): rpc leaves 64 at
                         n > 64 nchunks — (64, 64): gy tj = 1, 512 chunks, T = 32768; (512, 128): gy = tj = 2, 128 chunks, T = 8192;
                         (320, 129): gy tj = 15, the floor of 64 chunks, T = 4096.  At T + 1 / T + 5 rpc = 128 and the last chunk
                         holds 1 / 5 rows (T is a multiple of 128).
  gram_tile_kernel       a wave's macro-step count cnt = cdiv(rows of the chunk / (4 MS) - rpart, 4 / TIB): GRAM_CNT below, the
                         coverage of {0, 1, 2, 3, >= 4} under every MS and TIB is asserted on the host.
  panel_geometry         (panel_dot1, mgs_step) nb = min(2048, cdiv(n, 16 rpi)), rpi = 256 / tpc = 4 at 33 .. 64 columns:
                         capped at n > 2048 * 64 = 131072; behind it rpb = cdiv(cdiv(n, 2048), 4) 4 = 68: 131105 = 1928 * 68 + 1
                         and 131109 leave the last block 1 and 5 rows.
  gcge_hip_rank1_update  nb = min(4096, cdiv(n, 16 rpi)): capped at n > 4096 * 64 = 262144 at 33 .. 64 columns; the kernel's slab
                         = cdiv(cdiv(n, 4096), 4) 4 = 68 behind it: 262209 = 3856 * 68 + 1, 262213.
  coldots / coldots2 / resid_sq   nb = min(2048, cdiv(n, 256)), rpb = cdiv(cdiv(n, nb), 4) 4: capped at n > 524288; behind it
                         rpb = 260: 524421 = 2017 * 260 + 1, 524425.
  lc_launch, staged      rf = 2 (128-row blocks) at n >= 128 * 256 * 8 = 262144 for 97 .. 128 columns, or 33 .. 64 with k >= 128,
                         where the direct form is not taken (odd ldx): 262145 / 262149 leave the last block 1 / 5 rows.
  gcge_hip_lincomb_norms chunk = max(16, cdiv(4 cdiv(n, 128), 1024)) leaves 16 at n > 524288; 128-row blocks: 524289, 524293.
  gcge_hip_axpby         the row kernels from n >= 1024 (16-byte lanes or edge lanes), the element kernels below and at odd ld.
  gcge_hip_colscale1     nb = min(4096, cdiv(n, 1024)): capped at n > 4194304, where every thread has exactly four rows.
"""

import numpy as np
import pytest

from gcge_amd import abi
from helpers import (EVEN_LD, IN_GUARD, LAYOUTS, OUT_BITS, OUT_GUARD, Block, bits, check_vec, draw, out_vec, vec)

SMALL = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 33, 63, 64, 65, 127, 128, 129, 255, 257, 1023, 1024, 1025]
GRAM_SHAPES = [(1, 2), (3, 5), (16, 16), (17, 64), (64, 64), (65, 33), (128, 70), (129, 64), (192, 64), (256, 64), (320, 17),
               (384, 64), (512, 128)]
GRAM_THRESH = [((64, 64), 32768), ((512, 128), 8192), ((320, 129), 4096)]
# (k, m) -> rows: TIB = 4, 2, 1 (the tile count of k is 4, 2, 3); see gram_cnts
GRAM_CNT = [((256, 64), [3, 4, 7, 8, 12, 15, 16, 24, 32, 48, 63, 64, 65]),
            ((128, 70), [3, 4, 8, 12, 16, 24, 32, 48, 64, 65, 16480]),
            ((129, 129), [3, 4, 8, 16, 24, 32, 48, 64, 4192, 8193, 12289])]
LC_SHAPES = [(1, 1), (2, 16), (9, 17), (33, 33), (40, 64), (131, 65), (64, 80), (200, 96), (255, 128)]
LC_STAGED2 = [(3, 97), (128, 40)]         # shapes that take two row fragments per wave in the staged form
LC_COPY_SHAPES = [(9, 17), (40, 64), (200, 96)]
PANEL_COLS = [1, 2, 3, 17, 32, 33, 64]
COL_M = [1, 7, 64, 65]
AXPBY_M = [1, 9, 64, 127]
AXPBY_MODES = [(2.0, 0.0, True), (-3.0, 2.0, True), (0.0, -2.0, False)]   # y = a x; y = a x + b y; y = b y (no x)


def around(T, *tails):
    return [T - 1, T, T + 1] + list(tails)


# kernel -> [(rows, [shape, ...])]: every small row with every shape (the blocks are tiny), every threshold row with the shapes
# that reach its threshold
CASES = {
    "gram": [(n, GRAM_SHAPES) for n in SMALL] + [(n, [s]) for s, T in GRAM_THRESH for n in around(T, T + 5)],
    "lincomb": [(n, LC_SHAPES) for n in SMALL] + [(n, LC_STAGED2) for n in around(262144, 262149)],
    "lincomb_norms": [(n, [(9, 33), (2, 64)]) for n in SMALL] + [(n, [(2, 33), (2, 64)]) for n in around(524288, 524293)],
    "lincomb_copy": [(n, [(k, m, nc) for k, m in LC_COPY_SHAPES for nc in (1, 16, 63)]) for n in SMALL],
    "panel_dot1": [(n, PANEL_COLS + [65, 130]) for n in SMALL] + [(n, [33, 64]) for n in around(131072, 131105, 131109)],
    "rank1_update": [(n, PANEL_COLS) for n in SMALL] + [(n, [33, 64]) for n in around(262144, 262209, 262213)],
    "mgs_step": [(n, PANEL_COLS) for n in SMALL] + [(n, [33, 64]) for n in around(131072, 131105, 131109)],
    "coldots": [(n, COL_M) for n in SMALL] + [(n, [7, 64]) for n in around(524288, 524421, 524425)],
    "coldots2": [(n, COL_M) for n in SMALL] + [(n, [7, 64]) for n in around(524288, 524421, 524425)],
    "resid_sq": [(n, COL_M) for n in SMALL] + [(n, [7, 64]) for n in around(524288, 524421, 524425)],
    "colscale": [(n, COL_M) for n in SMALL],
    "colscale1": [(n, [1]) for n in SMALL] + [(n, [1]) for n in around(4194304, 4194309)],
    "axpby": [(n, AXPBY_M) for n in SMALL + [1029]],
}


def case_ids(kernel):
    return [pytest.param(n, shapes, id="n%d" % n) for n, shapes in CASES[kernel]]


# ---- the launchers' arithmetic restated (which rows are threshold rows; checked on the host below) ---------------------------
def cdiv(a, b):
    return -(-a // b)


def gram_geometry(n, k, m):
    ti, tj = cdiv(k, 64), cdiv(m, 64)
    tib = 4 if ti % 4 == 0 else (2 if ti % 2 == 0 else 1)
    nch = max(64, 512 // (cdiv(ti, tib) * tj))
    rpc = max(64, cdiv(cdiv(n, nch), 64) * 64)
    return tib, nch, rpc


def gram_cnts(n, k, m, ms):
    """min(cnt, 4) of every wave of every chunk"""
    tib, _, rpc = gram_geometry(n, k, m)
    rp, out = 4 // tib, set()
    for rows in {min(rpc, n), n - (cdiv(n, rpc) - 1) * rpc}:
        for part in range(rp):
            out.add(min(4, max(0, cdiv(rows // (4 * ms) - part, rp))))
    return out


def pow2_at_least(v, cap=64):
    t = 1
    while t < v and t < cap:
        t *= 2
    return t


def slab_rows(kernel, n, cols):
    """rows per block of the launch as (rows per block, the cap on the block count, blocks before the cap)"""
    if kernel in ("panel_dot1", "mgs_step", "rank1_update"):
        rpi, cap = 256 // pow2_at_least(cols), 4096 if kernel == "rank1_update" else 2048
        nb = cdiv(n, 16 * rpi)
        return cdiv(cdiv(n, max(1, min(cap, nb))), rpi) * rpi, cap, nb
    nb = cdiv(n, 256)                       # coldots, coldots2, resid_sq
    return cdiv(cdiv(n, min(2048, nb)), 4) * 4, 2048, nb


# ---- the operations in plain numpy, written so that they take float64, int64, longdouble or absolute values alike ------------
def f_gram(Q, P):
    return Q.T @ P


def f_lincomb(X, Cf, Y, beta):
    if X.dtype == np.longdouble and X.shape[1] <= 4:   # (numpy multiplies longdouble matrices one scalar at a time)
        XC = sum(X[:, j:j + 1] * Cf[j] for j in range(X.shape[1]))
    else:
        XC = X @ Cf
    return XC + (Y * beta if beta is not None else 0)


def f_coldots(X, Y):
    return (X * Y).sum(axis=0)


def f_resid(W, X, neg_lambda):
    return ((W + X * neg_lambda) ** 2).sum(axis=0)


def f_mgs(xk, Y, s, c):
    q = xk * s
    Yn = Y + np.outer(q, c)
    return q, Yn, (Yn * Yn[:, :1]).sum(axis=0)


# the unit roundoff of the bounds (t + 2) U |expression|; the absolute expressions are formed in float64, whose own rounding
# (a relative (t + 2) 2^-53 of the bound) the factor behind it covers
U = 2.0 ** -53 * (1 + 2.0 ** -30)


def ld_(a):
    return None if a is None else np.asarray(a).astype(np.longdouble)


def ab_(a):
    return None if a is None else np.abs(np.asarray(a, dtype=np.float64))


class Lib:
    def __init__(self, hip):
        import torch
        self.torch, self.hip, g = torch, hip, hip.g
        self.g = g
        self.st = g.gcge_hip_stream()

    def call(self, name, *args, expect=0):
        self.torch.cuda.synchronize()
        assert "gcge_hip_" + name in abi.HIP, name          # a name composed here escapes test_abi's source scan
        rc = getattr(self.g, "gcge_hip_" + name)(*args, self.st)
        self.hip.sync()
        assert rc == expect, (name, rc)

    def block(self, data, layout, guard=IN_GUARD, gl=None):
        return Block(self.torch, data, layout, guard, gl)


@pytest.fixture(scope="module")
def lib(hip):
    return Lib(hip)


def lay(i, pool=LAYOUTS):
    return pool[i % len(pool)]


# ---- one call of each kernel: data, launch, comparison.  real: uniform - 0.5 against longdouble within the derived bound --------
def run_gram(lib, n, k, m, li, real=False, seed=100):
    Q, P = draw(seed + 1, (n, k), real), draw(seed + 2, (n, m), real)
    bq, bp, out = lib.block(Q, lay(li)), lib.block(P, lay(li // 4 + li + 1)), out_vec(lib.torch, k * m)
    lib.call("gram", n, bq.ptr, bq.ld, k, bp.ptr, bp.ld, m, out[1])
    what = ("gram", n, k, m, li)
    if real:
        check_vec(out, f_gram(ld_(Q), ld_(P)), what, (n + 2) * U * f_gram(ab_(Q), ab_(P)))
    else:
        check_vec(out, f_gram(Q, P), what)
    if n <= 2000:
        bq.unchanged(what); bp.unchanged(what)
    return bq, bp, out


def lc_operands(lib, n, k, m, li, real, beta_mode, seed, xpool=LAYOUTS, nan_y=False):
    X, Cf, Y = draw(seed + 1, (n, k), real), draw(seed + 2, (k, m), real), draw(seed + 3, (n, m), real)
    beta = None
    if beta_mode:
        beta = draw(seed + 4, (m,), real)
        beta[:3] = [0.0, 1.0, -2.0][:min(3, m)]
    bx = lib.block(X, lay(li, xpool))
    by = lib.block(np.full((n, m), np.nan) if nan_y else Y, lay(li // 4 + 1), OUT_GUARD)
    return X, Cf, Y, beta, bx, by, vec(lib.torch, Cf), (vec(lib.torch, beta) if beta_mode else (None, None, 0))


def lc_check(by, X, Cf, Y, beta, what, real):
    if real:   # k products, the scaled old value, k additions: k + 1 terms
        by.check(f_lincomb(ld_(X), ld_(Cf), ld_(Y), ld_(beta)), what, (X.shape[1] + 3) * U * f_lincomb(ab_(X), ab_(Cf), ab_(Y), ab_(np.ones(Y.shape[1]) if beta is None else beta)))
    else:
        by.check(f_lincomb(X, Cf, Y, beta), what)


def run_lincomb(lib, n, k, m, li, beta_mode, real=False, seed=200, nan_y=False):
    X, Cf, Y, beta, bx, by, vc, vb = lc_operands(lib, n, k, m, li, real, beta_mode, seed, nan_y=nan_y)
    lib.call("lincomb", n, bx.ptr, bx.ld, k, vc[1], m, vb[1], by.ptr, by.ld)
    what = ("lincomb", n, k, m, li, beta_mode)
    lc_check(by, X, Cf, Y, beta, what, real)
    if n <= 2000:
        bx.unchanged(what)


def run_lincomb_copy(lib, n, k, m, ncopy, li, beta_mode, seed=300):
    X, Cf, Y, beta, bx, by, vc, vb = lc_operands(lib, n, k, m, li, False, beta_mode, seed)
    S = draw(seed + 5, (n, ncopy), False)
    bs, bd = lib.block(S, lay(li // 2)), lib.block(np.full((n, ncopy), OUT_GUARD), lay(li // 3 + 1), OUT_GUARD)
    lib.call("lincomb_copy", n, bx.ptr, bx.ld, k, vc[1], m, vb[1], by.ptr, by.ld, bs.ptr, bs.ld, bd.ptr, bd.ld, ncopy)
    what = ("lincomb_copy", n, k, m, ncopy, li)
    lc_check(by, X, Cf, Y, beta, what, False)
    bd.check(S, what)
    bx.unchanged(what); bs.unchanged(what)


def run_lincomb_norms(lib, n, k, m, li, beta_mode, real=False, seed=400):
    X, Cf, Y, beta, bx, by, vc, vb = lc_operands(lib, n, k, m, li, real, beta_mode, seed, xpool=EVEN_LD)   # the direct form
    out = out_vec(lib.torch, m)
    lib.call("lincomb_norms", n, bx.ptr, bx.ld, k, vc[1], m, vb[1], by.ptr, by.ld, out[1])
    what = ("lincomb_norms", n, k, m, li, beta_mode)
    lc_check(by, X, Cf, Y, beta, what, real)
    if real:   # n squares of values that carry (k + 3) u each, twice in a square
        yl = f_lincomb(ld_(X), ld_(Cf), ld_(Y), ld_(beta))
        ya = f_lincomb(ab_(X), ab_(Cf), ab_(Y), ab_(np.ones(m) if beta is None else beta))
        check_vec(out, (yl ** 2).sum(axis=0), what, (n + 2 + 2 * (k + 3)) * U * (ya ** 2).sum(axis=0))
    else:
        check_vec(out, (f_lincomb(X, Cf, Y, beta) ** 2).sum(axis=0), what)
    return bx, by, vc, vb, out


def run_panel_dot1(lib, n, k, li, real=False, seed=500):
    X, y = draw(seed + 1, (n, k), real), draw(seed + 2, (n, 1), real)
    bx, by, out = lib.block(X, lay(li)), lib.block(y, lay(li // 4 + 2)), out_vec(lib.torch, k)
    lib.call("panel_dot1", n, bx.ptr, bx.ld, k, by.ptr, by.ld, out[1])
    what = ("panel_dot1", n, k, li)
    if real:
        check_vec(out, f_coldots(ld_(X), ld_(y)), what, (n + 2) * U * f_coldots(ab_(X), ab_(y)))
    else:
        check_vec(out, f_coldots(X, y), what)
    if n <= 2000:
        bx.unchanged(what); by.unchanged(what)


def run_rank1(lib, n, m, li, beta_mode, real=False, seed=600):
    x, c, Y = draw(seed + 1, (n, 1), real), draw(seed + 2, (m,), real), draw(seed + 3, (n, m), real)
    beta = None
    if beta_mode:
        beta = draw(seed + 4, (m,), real)
        beta[:3] = [0.0, 1.0, -2.0][:min(3, m)]
    bx, by = lib.block(x, lay(li)), lib.block(Y, lay(li // 4 + 3), OUT_GUARD)
    vc, vb = vec(lib.torch, c), (vec(lib.torch, beta) if beta_mode else (None, None, 0))
    lib.call("rank1_update", n, bx.ptr, bx.ld, vc[1], vb[1], by.ptr, by.ld, m)
    what = ("rank1_update", n, m, li, beta_mode)
    b1 = np.ones(m) if beta is None else beta
    if real:   # a product and a fused multiply-add
        by.check(f_lincomb(ld_(x), ld_(c[None, :]), ld_(Y), ld_(b1)), what, 4 * U * f_lincomb(ab_(x), ab_(c[None, :]), ab_(Y), ab_(b1)))
    else:
        by.check(f_lincomb(x, c[None, :], Y, b1), what)
    if n <= 2000:
        bx.unchanged(what)


def run_mgs(lib, n, w, li, real=False, seed=700):
    V, c, s = draw(seed + 1, (n, 1 + w), real), draw(seed + 2, (w,), real), 2.0
    bv, vc, out = lib.block(V, lay(li), OUT_GUARD), vec(lib.torch, c), out_vec(lib.torch, w)
    lib.call("mgs_step", n, bv.ptr, bv.ld, s, vc[1], w, out[1])
    what = ("mgs_step", n, w, li)
    if real:   # x s is exact; one rounding per updated value, n products of two such values
        q, Yn, dots = f_mgs(ld_(V[:, 0]), ld_(V[:, 1:]), np.longdouble(s), ld_(c))
        _, Ya, da = f_mgs(ab_(V[:, 0]), ab_(V[:, 1:]), s, ab_(c))
        bv.check(np.column_stack([q, Yn]), what, 3 * U * np.column_stack([np.abs(q), Ya]))
        check_vec(out, dots, what, (n + 2 + 2) * U * da)
    else:
        q, Yn, dots = f_mgs(V[:, 0], V[:, 1:], s, c)
        bv.check(np.column_stack([q, Yn]), what)
        check_vec(out, dots, what)
    return bv, out


def run_coldots(lib, n, m, li, real=False, seed=800, two=False):
    X, Y = draw(seed + 1, (n, m), real), draw(seed + 2, (n, m), real)
    bx, by, out = lib.block(X, lay(li)), lib.block(Y, lay(li // 4 + 1)), out_vec(lib.torch, 2 * m if two else m)
    lib.call("coldots2" if two else "coldots", n, bx.ptr, bx.ld, by.ptr, by.ld, m, out[1])
    what = ("coldots2" if two else "coldots", n, m, li)
    cat = (lambda a, b: np.concatenate([f_coldots(a, b), f_coldots(b, b)])) if two else f_coldots
    if real:
        check_vec(out, cat(ld_(X), ld_(Y)), what, (n + 2) * U * cat(ab_(X), ab_(Y)))
    else:
        check_vec(out, cat(X, Y), what)
    if n <= 2000:
        bx.unchanged(what); by.unchanged(what)
    return bx, by, out


def run_resid(lib, n, m, li, real=False, seed=900):
    W, X, lam = draw(seed + 1, (n, m), real), draw(seed + 2, (n, m), real), draw(seed + 3, (m,), real)
    bw, bx, vl, out = lib.block(W, lay(li)), lib.block(X, lay(li // 4 + 2)), vec(lib.torch, lam), out_vec(lib.torch, m)
    lib.call("resid_sq", n, bw.ptr, bw.ld, bx.ptr, bx.ld, m, vl[1], out[1])
    what = ("resid_sq", n, m, li)
    if real:   # n squares of differences that carry one rounding each
        check_vec(out, f_resid(ld_(W), ld_(X), -ld_(lam)), what, (n + 2 + 2) * U * f_resid(ab_(W), ab_(X), ab_(lam)))
    else:
        check_vec(out, f_resid(W, X, -lam), what)
    if n <= 2000:
        bw.unchanged(what); bx.unchanged(what)


def run_colscale(lib, n, m, li, real=False, seed=1000):
    Y, s = draw(seed + 1, (n, m), real), draw(seed + 2, (m,), real)
    by, vs = lib.block(Y, lay(li), OUT_GUARD), vec(lib.torch, s)
    lib.call("colscale", n, by.ptr, by.ld, m, vs[1])
    if real:
        by.check(ld_(Y) * ld_(s), ("colscale", n, m, li), 3 * U * np.abs(ld_(Y) * ld_(s)))
    else:
        by.check(Y * s, ("colscale", n, m, li))


def run_colscale1(lib, n, li, real=False, seed=1100):
    y, s = draw(seed + 1, (n, 1), real), -3.0
    by = lib.block(y, lay(li), OUT_GUARD, gl=0 if n > 100000 else None)    # the large rows: no column in front
    lib.call("colscale1", n, by.ptr, by.ld, s)
    if real:
        by.check(ld_(y) * np.longdouble(s), ("colscale1", n, li), 3 * U * np.abs(ld_(y) * np.longdouble(s)))
    else:
        by.check(y * s, ("colscale1", n, li))


def run_axpby(lib, n, m, li, mode, real=False, seed=1200):
    alpha, beta, use_x = AXPBY_MODES[mode]
    X, Y = draw(seed + 1, (n, m), real), draw(seed + 2, (n, m), real)
    bx, by = lib.block(X, lay(li)), lib.block(Y, lay(li // 4 + li + 1), OUT_GUARD)
    lib.call("axpby", n, alpha, bx.ptr if use_x else None, bx.ld, beta, by.ptr, by.ld, m)
    what = ("axpby", n, m, li, mode)
    f = lambda x, y, a, b: (a * x if use_x else 0) + (b * y if beta != 0.0 else 0)
    if real:
        by.check(f(ld_(X), ld_(Y), np.longdouble(alpha), np.longdouble(beta)), what, 4 * U * f(ab_(X), ab_(Y), abs(alpha), abs(beta)))
    else:
        by.check(f(X, Y, alpha, beta), what)
    if n <= 2000:
        bx.unchanged(what)


# ---- 1. the premise, on the host --------------------------------------------------------------------------------------------
def test_exactness_of_the_case_table():
    """rows x the largest term stays below 2^53 for every case; below 2000 rows the float64 reference equals the same expression in
    int64; the threshold rows named in the header are what the launchers' arithmetic gives; the Gram rows reach every macro-step
    count under every MS and TIB."""
    q = lambda shape, seed: draw(seed, shape, False)
    i64 = lambda a: a.astype(np.int64)
    for kernel, cases in CASES.items():
        for n, shapes in cases:
            for si, sh in enumerate(shapes):
                k = sh[0] if isinstance(sh, tuple) else sh
                term = {"gram": 9, "lincomb": 9 * k + 9, "lincomb_copy": 9 * k + 9, "lincomb_norms": (9 * k + 9) ** 2,
                        "panel_dot1": 9, "rank1_update": 18, "mgs_step": 441, "coldots": 9, "coldots2": 9, "resid_sq": 144,
                        "colscale": 9, "colscale1": 9, "axpby": 15}[kernel]
                rows = 1 if kernel in ("lincomb", "lincomb_copy", "rank1_update", "colscale", "colscale1", "axpby") else n
                assert rows * term < 2 ** 53, (kernel, n, sh)
                if n >= 2000 or si > 2:
                    continue
                if kernel == "gram":
                    a, b = q((n, sh[0]), 1), q((n, sh[1]), 2)
                    assert np.array_equal(f_gram(a, b), f_gram(i64(a), i64(b)))
                elif kernel in ("lincomb", "lincomb_copy", "lincomb_norms"):
                    a, c, y, be = q((n, sh[0]), 1), q((sh[0], sh[1]), 2), q((n, sh[1]), 3), q((sh[1],), 4)
                    r, ri = f_lincomb(a, c, y, be), f_lincomb(i64(a), i64(c), i64(y), i64(be))
                    assert np.array_equal(r, ri) and np.array_equal((r ** 2).sum(axis=0), (ri ** 2).sum(axis=0))
                    assert np.max(np.abs(ri)) <= 9 * k + 9
                elif kernel == "mgs_step":
                    v, c = q((n, 1 + sh), 1), q((sh,), 2)
                    for got, ref in zip(f_mgs(v[:, 0], v[:, 1:], 2.0, c), f_mgs(i64(v[:, 0]), i64(v[:, 1:]), 2, i64(c))):
                        assert np.array_equal(got, ref)
                    assert np.max(np.abs(f_mgs(i64(v[:, 0]), i64(v[:, 1:]), 2, i64(c))[1])) <= 21
                elif kernel in ("panel_dot1", "coldots", "coldots2", "resid_sq"):
                    a, b, lam = q((n, sh), 1), q((n, sh), 2), q((sh,), 3)
                    assert np.array_equal(f_coldots(a, b), f_coldots(i64(a), i64(b)))
                    assert np.array_equal(f_resid(a, b, -lam), f_resid(i64(a), i64(b), -i64(lam)))
    d = draw(7, (1000, 9), False)
    assert np.all(d != 0) and np.all(np.abs(d) <= 3) and np.all(d == np.round(d)) and set(np.unique(d)) == {-3, -2, -1, 1, 2, 3}
    # the threshold rows
    for (k, m), T in GRAM_THRESH:
        assert gram_geometry(T, k, m)[2] == 64 and gram_geometry(T + 1, k, m)[2] == 128 and T % 128 == 0
    for kernel, T, t1, t5 in (("panel_dot1", 131072, 131105, 131109), ("mgs_step", 131072, 131105, 131109),
                              ("rank1_update", 262144, 262209, 262213), ("coldots", 524288, 524421, 524425)):
        for cols in (33, 64):
            per, cap, nb = slab_rows(kernel, T, cols)
            assert nb == cap and slab_rows(kernel, T + 1, cols)[2] == cap + 1      # the cap starts to bind behind T
            for n, tail in ((t1, 1), (t5, 5)):
                per = slab_rows(kernel, n, cols)[0]
                assert n - (cdiv(n, per) - 1) * per == tail, (kernel, n, per)
    nw = lambda n: 4 * cdiv(n, 128)
    assert cdiv(nw(524288), 1024) == 16 and cdiv(nw(524289), 1024) == 17
    assert cdiv(4194304, 1024) == 4096 and 128 * 256 * 8 == 262144
    # the Gram's macro-step counts
    for (k, m), rows in GRAM_CNT:
        for ms in (1, 2, 4):
            seen = set()
            for n in rows:
                seen |= gram_cnts(n, k, m, ms)
            assert seen == {0, 1, 2, 3, 4}, (k, m, ms, seen)
    assert [gram_geometry(64, k, m)[0] for (k, m), _ in GRAM_CNT] == [4, 2, 1]
    assert sorted({(cdiv(k, 64), gram_geometry(64, k, m)[0]) for k, m in GRAM_SHAPES[-3:]}) == [(5, 1), (6, 2), (8, 4)]


# ---- 3 / 4. the row ladder, per kernel --------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n,shapes", case_ids("gram"))
def test_gram_rows(lib, n, shapes):
    for si, (k, m) in enumerate(shapes):
        run_gram(lib, n, k, m, si + n)


@pytest.mark.gpu
@pytest.mark.parametrize("ms", [1, 2, 4])
def test_gram_macro_step_counts(lib, ms):
    """a wave's macro-step count 0, 1, 2, 3 and >= 4 (pair loop, odd remainder, clamped prefetch) under every MS and TIB"""
    try:
        lib.g.gcge_hip_gram_tune(ms)
        for (k, m), rows in GRAM_CNT:
            for n in rows:
                run_gram(lib, n, k, m, n + ms)
        if ms != 2:                                   # the small rows of the ladder under the other macro-steps
            for n in (1, 5, 9, 17, 33, 65, 129):
                for si, (k, m) in enumerate(GRAM_SHAPES):
                    run_gram(lib, n, k, m, si + n)
    finally:
        lib.g.gcge_hip_gram_tune(2)


@pytest.mark.gpu
@pytest.mark.parametrize("n,shapes,tune", [pytest.param(n, shapes, tune, id="n%d-tune%d" % (n, tune)) for tune in (0, 3)
                                           for n, shapes in CASES["lincomb"] if tune == 0 or n < 100000])   # (odd ldx: staged under either)
def test_lincomb_rows(lib, n, shapes, tune):
    """default: the direct form for panels of >= 33 columns on even ld, the staged form otherwise; 3: the direct form for narrow
    panels too.  beta absent and a vector that holds 0, 1 and -2."""
    try:
        lib.g.gcge_hip_lincomb_tune(tune)
        for si, (k, m) in enumerate(shapes):
            for beta_mode in (0, 1):
                li = si + n + beta_mode
                if n > 100000:
                    li = 2 + (si + n) % 2             # odd ldx: the staged form, two row fragments from 262144 rows
                    if beta_mode != si % 2:
                        continue
                run_lincomb(lib, n, k, m, li, beta_mode)
    finally:
        lib.g.gcge_hip_lincomb_tune(0)


@pytest.mark.gpu
@pytest.mark.parametrize("tune", [0, 3])
def test_lincomb_never_reads_y_without_beta(lib, tune):
    try:
        lib.g.gcge_hip_lincomb_tune(tune)
        for n in (5, 129, 1025):
            for k, m in LC_SHAPES:
                for li in range(4):
                    run_lincomb(lib, n, k, m, li, 0, nan_y=True)
    finally:
        lib.g.gcge_hip_lincomb_tune(0)


@pytest.mark.gpu
@pytest.mark.parametrize("tune", [0, 3])
@pytest.mark.parametrize("n,shapes", case_ids("lincomb_copy"))
def test_lincomb_copy_rows(lib, n, shapes, tune):
    try:
        lib.g.gcge_hip_lincomb_tune(tune)
        for si, (k, m, ncopy) in enumerate(shapes):
            run_lincomb_copy(lib, n, k, m, ncopy, si + n, si % 2)
    finally:
        lib.g.gcge_hip_lincomb_tune(0)


@pytest.mark.gpu
@pytest.mark.parametrize("n,shapes", case_ids("lincomb_norms"))
def test_lincomb_norms_rows(lib, n, shapes):
    for si, (k, m) in enumerate(shapes):
        run_lincomb_norms(lib, n, k, m, si + n, (si + n) % 2)


@pytest.mark.gpu
@pytest.mark.parametrize("n,shapes", case_ids("panel_dot1"))
def test_panel_dot1_rows(lib, n, shapes):
    for si, k in enumerate(shapes):
        run_panel_dot1(lib, n, k, si + n)


@pytest.mark.gpu
@pytest.mark.parametrize("n,shapes", case_ids("rank1_update"))
def test_rank1_update_rows(lib, n, shapes):
    for si, m in enumerate(shapes):
        for beta_mode in ((0, 1) if n < 100000 else ((si + n) % 2,)):
            run_rank1(lib, n, m, si + n, beta_mode)


@pytest.mark.gpu
@pytest.mark.parametrize("n,shapes", case_ids("mgs_step"))
def test_mgs_step_rows(lib, n, shapes):
    for si, w in enumerate(shapes):
        run_mgs(lib, n, w, si + n)


@pytest.mark.gpu
@pytest.mark.parametrize("n,shapes", case_ids("coldots"))
def test_coldots_rows(lib, n, shapes):
    for si, m in enumerate(shapes):
        run_coldots(lib, n, m, si + n)


@pytest.mark.gpu
@pytest.mark.parametrize("n,shapes", case_ids("coldots2"))
def test_coldots2_rows(lib, n, shapes):
    for si, m in enumerate(shapes):
        run_coldots(lib, n, m, si + n, two=True)


@pytest.mark.gpu
@pytest.mark.parametrize("n,shapes", case_ids("resid_sq"))
def test_resid_sq_rows(lib, n, shapes):
    for si, m in enumerate(shapes):
        run_resid(lib, n, m, si + n)


@pytest.mark.gpu
@pytest.mark.parametrize("n,shapes", case_ids("colscale"))
def test_colscale_rows(lib, n, shapes):
    for si, m in enumerate(shapes):
        run_colscale(lib, n, m, si + n)


@pytest.mark.gpu
@pytest.mark.parametrize("n,shapes", case_ids("colscale1"))
def test_colscale1_rows(lib, n, shapes):
    for li in (range(4) if n < 100000 else (0,)):    # one column, ld 2, at the large rows
        run_colscale1(lib, n, li)


@pytest.mark.gpu
@pytest.mark.parametrize("n,shapes", case_ids("axpby"))
def test_axpby_rows(lib, n, shapes):
    """odd ld or fewer than 1024 rows: the element kernels; from 1024 rows the row kernels (16-byte lanes, edge lanes)"""
    for si, m in enumerate(shapes):
        for mode in range(3):
            for li in range(4):
                run_axpby(lib, n, m, li + 4 * ((si + mode) % 4), mode)


def partials(lib, nb, cols):
    """the first nb x cols doubles of the partial-sum workspace (copied out by the library's own axpby)"""
    ws = lib.g.gcge_hip_partial_ws(1)                 # (no larger than what it holds: the same allocation)
    t = lib.torch.zeros((nb, cols), dtype=lib.torch.float64, device="cuda")
    lib.call("axpby", nb, 1.0, ws, cols, 0.0, t.data_ptr(), cols, cols)
    return t.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [129, 1025, 131072, 131073, 131105])
def test_panel_partial_sums_follow_the_slab_geometry(lib, n):
    """What panel_dot1 and mgs_step leave in the workspace, one row of sums per block, is the sums over the slabs panel_geometry
    describes — rows [b rpb, (b + 1) rpb), rpb a multiple of the rpi rows a block walks per step, the same for both kernels.
    Exact data: a slab boundary that moves changes a block's sums by integers (the totals would not notice)."""
    for li, cols in enumerate((33, 64)):
        rpb = slab_rows("panel_dot1", n, cols)[0]
        nb = cdiv(n, rpb)
        starts = np.arange(nb) * rpb
        X, y = draw(1301, (n, cols), False), draw(1302, (n, 1), False)
        bx, by, out = lib.block(X, lay(li)), lib.block(y, lay(li + 2)), out_vec(lib.torch, cols)
        lib.call("panel_dot1", n, bx.ptr, bx.ld, cols, by.ptr, by.ld, out[1])
        assert np.array_equal(partials(lib, nb, cols), np.add.reduceat(X * y, starts, axis=0)), ("panel_dot1", n, cols, rpb)
        V, c = draw(1303, (n, 1 + cols), False), draw(1304, (cols,), False)
        bv, vc, out = lib.block(V, lay(li + 1), OUT_GUARD), vec(lib.torch, c), out_vec(lib.torch, cols)
        lib.call("mgs_step", n, bv.ptr, bv.ld, 2.0, vc[1], cols, out[1])
        Yn = f_mgs(V[:, 0], V[:, 1:], 2.0, c)[1]
        assert np.array_equal(partials(lib, nb, cols), np.add.reduceat(Yn * Yn[:, :1], starts, axis=0)), ("mgs_step", n, cols, rpb)


# ---- 5. rounding, once per kernel: real-valued data against longdouble, the bound (t + 2) 2^-53 of the absolute expression ----------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [129, 32773])
def test_gram_rounding_and_same_bits_on_a_second_run(lib, n):
    for li, (k, m) in enumerate([(3, 5), (17, 64)] if n > 1000 else GRAM_SHAPES):
        bq, bp, out = run_gram(lib, n, k, m, li, real=True)
        again = out_vec(lib.torch, k * m)
        lib.call("gram", n, bq.ptr, bq.ld, k, bp.ptr, bp.ld, m, again[1])
        assert np.array_equal(bits(out[0].cpu().numpy()), bits(again[0].cpu().numpy())), ("gram", n, k, m)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [129, 262149])
def test_lincomb_rounding(lib, n):
    for tune in ((0,) if n > 1000 else (0, 3)):
        try:
            lib.g.gcge_hip_lincomb_tune(tune)
            for si, (k, m) in enumerate([(3, 97)] if n > 1000 else LC_SHAPES):
                for li in ((2,) if n > 1000 else range(4)):
                    run_lincomb(lib, n, k, m, li, 1, real=True)
        finally:
            lib.g.gcge_hip_lincomb_tune(0)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [129, 524293])
def test_lincomb_norms_rounding_and_same_bits_on_a_second_run(lib, n):
    for li, (k, m) in enumerate([(2, 33)] if n > 1000 else [(9, 33), (40, 64)]):
        bx, by, vc, vb, out = run_lincomb_norms(lib, n, k, m, li, 0, real=True)    # beta absent: the second run sees the same operands
        again = out_vec(lib.torch, m)
        lib.call("lincomb_norms", n, bx.ptr, bx.ld, k, vc[1], m, vb[1], by.ptr, by.ld, again[1])
        assert np.array_equal(bits(out[0].cpu().numpy()), bits(again[0].cpu().numpy())), ("lincomb_norms", n, k, m)
        if n < 1000:
            run_lincomb_norms(lib, n, k, m, li, 1, real=True)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [129, 131109])
def test_mgs_step_rounding_and_dots_equal_panel_dot1(lib, n):
    for li, w in enumerate([33] if n > 1000 else PANEL_COLS):
        bv, out = run_mgs(lib, n, w, li, real=True)
        sep = out_vec(lib.torch, w)
        lib.call("panel_dot1", n, bv.ptr + 8, bv.ld, w, bv.ptr + 8, bv.ld, sep[1])     # the updated panel against its first column
        assert np.array_equal(bits(out[0].cpu().numpy()), bits(sep[0].cpu().numpy())), ("mgs_step", n, w)
        run_panel_dot1(lib, n, w, li, real=True)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [129, 524425])
def test_column_sums_rounding_and_coldots2_equals_two_coldots(lib, n):
    for li, m in enumerate([7] if n > 1000 else COL_M):
        bx, by, two = run_coldots(lib, n, m, li, real=True, two=True)
        xy, yy = out_vec(lib.torch, m), out_vec(lib.torch, m)
        lib.call("coldots", n, bx.ptr, bx.ld, by.ptr, by.ld, m, xy[1])
        lib.call("coldots", n, by.ptr, by.ld, by.ptr, by.ld, m, yy[1])
        both = np.concatenate([xy[0].cpu().numpy()[2:2 + m], yy[0].cpu().numpy()[2:2 + m]])
        assert np.array_equal(bits(two[0].cpu().numpy()[2:2 + 2 * m]), bits(both)), ("coldots2", n, m)
        run_coldots(lib, n, m, li + 1, real=True)
        run_resid(lib, n, m, li, real=True)


@pytest.mark.gpu
@pytest.mark.parametrize("big", [False, True], ids=["rows129", "threshold_rows"])
def test_elementwise_rounding(lib, big):
    for li, m in enumerate([33] if big else PANEL_COLS):
        run_rank1(lib, 262213 if big else 129, m, li, 1, real=True)
    for li, m in enumerate(COL_M):
        run_colscale(lib, 1029 if big else 129, m, li, real=True)
    for li, m in enumerate(AXPBY_M):
        for mode in range(3):
            run_axpby(lib, 1029 if big else 129, m, li, mode, real=True)
    run_colscale1(lib, 4194309 if big else 129, 0, real=True)


# ---- 6. zero rows ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_zero_rows_give_zeros(lib):
    """every reducing entry zeroes its output for an empty slab (its sums then go into a reduction across ranks);
    gcge_hip_lincomb_norms declines with 1 and leaves its output alone"""
    t = lib.torch
    A, B, c = lib.block(draw(1, (4, 64), False), (2, 0)), lib.block(draw(2, (4, 64), False), (2, 0)), vec(t, draw(3, (64 * 64,), False))
    for m in (1, 7, 64):
        for name, ln, args in (("gram", m * m, (0, A.ptr, A.ld, m, B.ptr, B.ld, m)),
                               ("coldots", m, (0, A.ptr, A.ld, B.ptr, B.ld, m)),
                               ("coldots2", 2 * m, (0, A.ptr, A.ld, B.ptr, B.ld, m)),
                               ("panel_dot1", m, (0, A.ptr, A.ld, m, B.ptr, B.ld)),
                               ("resid_sq", m, (0, A.ptr, A.ld, B.ptr, B.ld, m, c[1]))):
            out = out_vec(t, ln)
            lib.call(name, *args, out[1])
            check_vec(out, np.zeros(ln), (name, "zero rows", m))
        out = out_vec(t, m)
        lib.call("mgs_step", 0, A.ptr, A.ld, 2.0, c[1], m, out[1])
        check_vec(out, np.zeros(m), ("mgs_step", "zero rows", m))
    Y, out = lib.block(draw(4, (4, 64), False), (2, 0), OUT_GUARD), out_vec(t, 64)
    lib.call("lincomb_norms", 0, A.ptr, A.ld, 8, c[1], 64, None, Y.ptr, Y.ld, out[1], expect=1)
    assert np.all(bits(out[0].cpu().numpy()) == OUT_BITS)
    A.unchanged("zero rows"); B.unchanged("zero rows")
    Y.check(draw(4, (4, 64), False), "zero rows")
