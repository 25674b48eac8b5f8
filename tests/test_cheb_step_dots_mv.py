"""The Chebyshev step with its two column sums on matrix handles (gcge_hip_cheb_step_dots_mv, csrc/hip/mat_product.hip;
GCGE_BACKEND.cheb_step_dots):

    out[:, o0..o0+m) = alpha (A y[:, y0..) - c y[:, y0..)) - beta z[:, z0..) ,   oo_j = sum_r out[r, o0 + j]^2 ,   oy_j = sum_r out[r, o0 + j] y[r, y0 + j]

on the handle of lap3d 8^3, m in {2, 6}, windows at columns 0 and 1 of wider blocks, with and without GCGE_CHEB_NO_FUSE.  The call must
take exactly gcge_hip_cheb_step_mv's decisions: gcge_hip_cheb_step_dots_stats moves as gcge_hip_cheb_stats does for the same operands,
and out is bit for bit what that call writes.  Whether a matrix as small as 8^3 takes the fused pass is the step's own decision
(gcge_hip_cg_recompute_pays; tests/test_cheb_step.py pins it from 16^3 upwards), so the same cases run on 16^3 as well, where the even
window at column 0 is known to take the fused pass, here followed by gcge_hip_cheb_dots, and GCGE_CHEB_NO_FUSE=1 the sweep with the sums
inside.
Data: exact (integers of magnitude <= 3, powers of two: out equals numpy's, and the sums, of at most 4096 terms below 2^16 in multiples
of 2^-8, are exact too) and uniform (the sums within (n + 2) 2^-53 sum |terms| of a long double sum over the stored values, the bound
tests/test_cheb_dots.py derives)."""
import ctypes as C

import numpy as np
import pytest

from gcge_amd.lib import cheb_stats, cheb_step_dots_stats, csr_to_scipy, make_problem
from helpers import bits, draw
from test_pcg_sweeps import POW2

SENTINEL = -12345.0


@pytest.fixture(scope="module")
def laps(hip):
    """{N: (scipy matrix, handle)} for lap3d 8 and 16"""
    out = {}
    for N in (8, 16):
        A, _ = make_problem("lap3d", N)
        out[N] = (csr_to_scipy(A), hip.matrix(A))
    yield out
    for S, m in out.values():
        hip.free_matrix(m)


def moved(s0, s1):
    return tuple(b - a for a, b in zip(s0, s1))


def same(a, b):
    return np.array_equal(bits(np.ascontiguousarray(a)), bits(np.ascontiguousarray(b)))


def both_steps(hip, S, mat, m, col, seed, real, beta_zero=False):
    """gcge_hip_cheb_step_mv and gcge_hip_cheb_step_dots_mv on equal blocks of col + m + 2 columns, the windows at column `col`:
    (blocks before, blocks after the plain step, after the step with sums, oo, oy, scalars, how each call's stats moved)"""
    n, w = S.shape[0], col + m + 2
    Y, Z, O = (np.asfortranarray(draw(seed + k, (n, w), real)) for k in range(3))
    a, c, b = (0.37, 5.3, 0.81) if real else (float(v) for v in POW2[np.random.default_rng(seed + 3).integers(0, len(POW2), 3)])
    if beta_zero:
        b = 0.0
    oo, oy = np.full(m + 2, SENTINEL), np.full(m + 2, SENTINEL)
    blocks = [hip.mv_from_numpy(mat, v) for v in (Y, Z, O, Y, Z, O)]
    try:
        my, mz, mo, my2, mz2, mo2 = blocks
        s0, d0 = cheb_stats(), cheb_step_dots_stats()
        rc1 = hip.g.gcge_hip_cheb_step_mv(mat, my, col, None if beta_zero else mz, col, mo, col, m, a, c, b)
        s1, d1 = cheb_stats(), cheb_step_dots_stats()
        rc2 = hip.g.gcge_hip_cheb_step_dots_mv(mat, my2, col, None if beta_zero else mz2, col, mo2, col, m, a, c, b,
                                               C.c_void_p(oo.ctypes.data + 8), C.c_void_p(oy.ctypes.data + 8))
        s2, d2 = cheb_stats(), cheb_step_dots_stats()
        hip.sync()
        got = [hip.mv_to_numpy(v, n, 0, w) for v in blocks]
    finally:
        for v in blocks:
            hip.ops.mv_destroy(v, w)
    assert rc1 == 0 and rc2 == 0
    assert moved(d0, d1) == (0, 0, 0) and moved(s1, s2) == (0, 0, 0)                     # each call counts in its own stats only
    assert oo[0] == SENTINEL and oo[-1] == SENTINEL and oy[0] == SENTINEL and oy[-1] == SENTINEL
    return (Y, Z, O), got[:3], got[3:], oo[1:-1], oy[1:-1], (a, c, b), moved(s0, s1), moved(d1, d2)


def check(S, m, col, real, before, plain, dots, oo, oy, scal):
    (Y, Z, O), (a, c, b) = before, scal
    win = slice(col, col + m)
    assert same(dots[2], plain[2])                                                      # out: the bits of gcge_hip_cheb_step_mv, window and all
    assert same(dots[0], Y) and same(dots[1], Z)
    assert same(dots[2][:, :col], O[:, :col]) and same(dots[2][:, col + m:], O[:, col + m:])
    out = dots[2][:, win]
    if not real:
        ref = a * (S @ Y[:, win] - c * Y[:, win]) - (b * Z[:, win] if b != 0.0 else 0.0)
        assert np.array_equal(out, ref)
    ld = lambda v: np.asarray(v, dtype=np.longdouble)
    n = S.shape[0]
    for name, sums, terms in (("oo", oo, ld(out) * ld(out)), ("oy", oy, ld(out) * ld(Y[:, win]))):
        err = np.abs(ld(sums) - np.sum(terms, axis=0))
        bound = (n + 2) * 2.0 ** -53 * np.sum(np.abs(np.asarray(terms, dtype=np.float64)), axis=0)
        assert np.all(err <= bound), (name, float((err / bound).max()))
        if not real:
            assert np.array_equal(sums, np.sum(np.asarray(terms, dtype=np.float64), axis=0)), name


def test_the_exact_sums_are_exact():
    """the premise for the integer data: |A y| <= 36, out is a multiple of 2^-4 of magnitude <= 4 (36 + 4 * 3) + 4 * 3 = 204, so a term
    of either sum is a multiple of 2^-8 below 2^16 and 4096 of them stay below 2^28: 36 bits"""
    assert 4 * (36 + 4 * 3) + 4 * 3 == 204 and 204 ** 2 < 2 ** 16 and 16 ** 3 * 2 ** 16 == 2 ** 28 and 28 + 8 < 53


@pytest.mark.gpu
@pytest.mark.parametrize("real", [False, True])
@pytest.mark.parametrize("col", [0, 1])
@pytest.mark.parametrize("m", [2, 6])
@pytest.mark.parametrize("N", [8, 16])
def test_the_slot_takes_the_steps_decisions_and_writes_its_bits(hip, laps, N, m, col, real, monkeypatch):
    S, mat = laps[N]
    seed = 3100 + 100 * N + 10 * m + col
    before, plain, dots, oo, oy, scal, ds, dd = both_steps(hip, S, mat, m, col, seed, real)
    assert ds == dd and ds in ((1, 0, 0), (0, 1, 0)), (N, m, col, ds, dd)                 # the step's own decision, whatever it is
    if N == 16:                                   # an even width on an even column of a matrix whose product pays twice: fused
        assert dd == ((1, 0, 0) if col == 0 else (0, 1, 0)), (N, m, col, dd)
    if col == 1:
        assert dd == (0, 1, 0), (N, m, col, dd)
    check(S, m, col, real, before, plain, dots, oo, oy, scal)
    monkeypatch.setenv("GCGE_CHEB_NO_FUSE", "1")
    before2, plain2, dots2, oo2, oy2, scal2, ds2, dd2 = both_steps(hip, S, mat, m, col, seed, real)
    assert ds2 == dd2 == (0, 1, 0), (N, m, col, ds2, dd2)
    check(S, m, col, real, before2, plain2, dots2, oo2, oy2, scal2)
    if not real:
        assert same(dots2[2], dots[2]) and np.array_equal(oo2, oo) and np.array_equal(oy2, oy)      # exact data: the two paths agree


@pytest.mark.gpu
@pytest.mark.parametrize("N", [8, 16])
def test_first_step_without_z(hip, laps, N):
    S, mat = laps[N]
    before, plain, dots, oo, oy, scal, ds, dd = both_steps(hip, S, mat, 6, 0, 3900 + N, False, beta_zero=True)
    assert ds == dd == (0, 1, 0) and scal[2] == 0.0
    check(S, 6, 0, False, before, plain, dots, oo, oy, scal)


@pytest.mark.gpu
def test_mismatched_blocks_are_declined_with_nothing_written(hip, laps):
    S, mat = laps[8]
    S16, mat16 = laps[16]
    n = S.shape[0]
    data = [np.asfortranarray(draw(3950 + k, (n, 10), False)) for k in range(3)]
    other = np.asfortranarray(draw(3959, (S16.shape[0], 10), False))
    my, mz, mo = (hip.mv_from_numpy(mat, b) for b in data)
    mw = hip.mv_from_numpy(mat16, other)
    oo, oy = np.full(8, SENTINEL), np.full(8, SENTINEL)
    po, py = C.c_void_p(oo.ctypes.data), C.c_void_p(oy.ctypes.data)
    f = hip.g.gcge_hip_cheb_step_dots_mv
    try:
        for args in ((mat, my, 0, mz, 0, my, 0, 6, 1.0, 1.0, 1.0, po, py),       # out is y
                     (mat, my, 0, mz, 0, mz, 0, 6, 1.0, 1.0, 1.0, po, py),       # out is z
                     (mat, my, 0, my, 0, mo, 0, 6, 1.0, 1.0, 1.0, po, py),       # z is y
                     (mat, my, 0, None, 0, mo, 0, 6, 1.0, 1.0, 1.0, po, py),     # beta != 0 without z
                     (mat, my, 6, mz, 0, mo, 0, 6, 1.0, 1.0, 1.0, po, py),       # windows outside a block
                     (mat, my, 0, mz, 6, mo, 0, 6, 1.0, 1.0, 1.0, po, py),
                     (mat, my, 0, mz, 0, mo, -1, 6, 1.0, 1.0, 1.0, po, py),
                     (mat, my, 0, mz, 0, mo, 0, 0, 1.0, 1.0, 1.0, po, py),       # no columns
                     (None, my, 0, mz, 0, mo, 0, 6, 1.0, 1.0, 1.0, po, py),
                     (mat, mw, 0, mz, 0, mo, 0, 6, 1.0, 1.0, 1.0, po, py),       # blocks of another row count
                     (mat, my, 0, mw, 0, mo, 0, 6, 1.0, 1.0, 1.0, po, py),
                     (mat, my, 0, mz, 0, mw, 0, 6, 1.0, 1.0, 1.0, po, py),
                     (mat16, my, 0, mz, 0, mo, 0, 6, 1.0, 1.0, 1.0, po, py),     # a matrix of another row count
                     (mat, my, 0, mz, 0, mo, 0, 6, 1.0, 1.0, 1.0, None, py),     # no place for the sums
                     (mat, my, 0, mz, 0, mo, 0, 6, 1.0, 1.0, 1.0, po, None)):
            d0, s0 = cheb_step_dots_stats(), cheb_stats()
            assert f(*args) == -1, args[2:11]
            assert moved(d0, cheb_step_dots_stats()) == (0, 0, 1) and moved(s0, cheb_stats()) == (0, 0, 0), args[2:11]
        hip.sync()
        for v, b in zip((my, mz, mo), data):
            assert same(hip.mv_to_numpy(v, n, 0, 10), b)
        assert same(hip.mv_to_numpy(mw, S16.shape[0], 0, 10), other)
        assert np.all(oo == SENTINEL) and np.all(oy == SENTINEL)
    finally:
        for v in (my, mz, mo, mw):
            hip.ops.mv_destroy(v, 10)
