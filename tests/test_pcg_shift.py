"""The shift sweep of GCGE_PCGSolveDeflated's operator (gcge_hip_pcg_shift, csrc/hip/pcg_sweeps.hip) through its raw-pointer entry
point, on EXACT data as tests/test_pcg_sweeps.py: the blocks hold nonzero integers of magnitude <= 3 and the shifts are powers of two,
so w - shift q, its product with p and every sum are exact in any order and the comparison with numpy is np.array_equal.

    w[:, j] -= shift_j q[:, j] ;  pw_j = sum_r p[r, j] w_new[r, j]        for the flagged columns; the others keep the bits of w, pw_j = 0

q is a block of its own (B p) or p itself (the same pointer: the row is read once).  Every operand sits in a helpers.Block with
guards round it; w carries NaN guards that must come back bit for bit, p and q must not be written.  The four layouts and the
widths take the 16-byte lanes ((even, even), even width) and the scalar lanes (everything else); rows 1, 255 / 257, 4099 as there."""
import numpy as np
import pytest

from helpers import IN_GUARD, LAYOUTS, OUT_GUARD, Block, bits, draw
from test_pcg_sweeps import COLS, POW2, ROWS, Lib, coefs, flags_for, ptr


@pytest.fixture(scope="module")
def lib(hip):
    return Lib(hip)


def run_shift(lib, n, m, layout, seed, q_is_p):
    P, Q, W = (draw(seed + k, (n, m), False) for k in range(3))
    shift, flag = coefs(m, seed + 3), flags_for(m, seed + 4, (0, 1))
    bp, bw = Block(lib.torch, P, layout, IN_GUARD), Block(lib.torch, W, layout, OUT_GUARD)
    bq = bp if q_is_p else Block(lib.torch, Q, layout, IN_GUARD)
    if q_is_p:
        Q = P
    pw = np.full(m, -1.0)
    lib.call("pcg_shift", n, bp.ptr, bp.ld, bq.ptr, bq.ld, bw.ptr, bw.ld, m, ptr(shift), ptr(flag), ptr(pw))
    on = flag != 0
    wn = np.where(on, W - shift * Q, W)
    what = ("pcg_shift", n, m, layout, "q is p" if q_is_p else "q apart")
    bw.check(wn, what)                              # (flagged columns shifted, the others and the guards bit for bit what they were)
    bp.unchanged(what); bq.unchanged(what)
    assert np.array_equal(pw, np.where(on, (P * wn).sum(axis=0), 0.0)), what
    return pw


def test_the_data_is_exact():
    """the premise: the largest sum, 4099 rows of 3 (3 + 4 * 3), is an integer multiple of 2^-2 far below 2^53"""
    assert 4099 * 3 * (3 + 4 * 3) * 4 < 2 ** 53
    assert np.abs(POW2).max() == 4.0 and np.abs(POW2).min() == 0.25


@pytest.mark.gpu
@pytest.mark.parametrize("q_is_p", [False, True])
@pytest.mark.parametrize("n", ROWS)
def test_pcg_shift_rows(lib, n, q_is_p):
    for m in COLS:
        for li, layout in enumerate(LAYOUTS):
            a = run_shift(lib, n, m, layout, 500 * m + li, q_is_p)
            b = run_shift(lib, n, m, layout, 500 * m + li, q_is_p)
            assert np.array_equal(bits(a), bits(b))                 # the sums of two runs: the same bits


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [LAYOUTS[0], LAYOUTS[3]])
def test_sums_of_inexact_data_are_the_same_bits_on_every_run(lib, layout):
    """uniform data, where the order of summation shows: the partial sums are added in a fixed order (both kernels)"""
    n, m = 4099, 8
    P, Q, W = (draw(600 + k, (n, m), True) for k in range(3))
    shift, flag = np.linspace(0.3, 1.7, m), np.ones(m, dtype=np.int32)
    out = []
    for _ in range(2):
        bp, bq, bw = Block(lib.torch, P, layout, IN_GUARD), Block(lib.torch, Q, layout, IN_GUARD), Block(lib.torch, W, layout, OUT_GUARD)
        pw = np.zeros(m)
        lib.call("pcg_shift", n, bp.ptr, bp.ld, bq.ptr, bq.ld, bw.ptr, bw.ld, m, ptr(shift), ptr(flag), ptr(pw))
        out.append((pw, bw.dev.cpu().numpy()))
    assert np.array_equal(bits(out[0][0]), bits(out[1][0])) and np.array_equal(bits(out[0][1]), bits(out[1][1]))
    # against numpy: w_new is one fused rounding there and two here, a sum of n terms in any order is within (n - 1) eps sum |terms|
    eps = np.finfo(np.float64).eps
    wn = W - shift * Q
    w_bound = 2 * eps * (np.abs(W) + np.abs(shift * Q))
    assert np.all(np.abs(out[0][1][:n, layout[0]:layout[0] + m] - wn) <= w_bound)
    assert np.all(np.abs(out[0][0] - (P * wn).sum(axis=0)) <= (n + 2) * eps * (np.abs(P) * np.abs(wn)).sum(axis=0) + (np.abs(P) * w_bound).sum(axis=0))
