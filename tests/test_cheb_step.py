"""One step of a Chebyshev filter on matrix handles (gcge_hip_cheb_step_mv, csrc/hip/mat_product.hip):

    out[:, o0..o0+m) = alpha (A y[:, y0..) - c y[:, y0..)) - beta z[:, z0..)

on EXACT data: lap3d's integer stencil (6 and -1), y and z nonzero integers of magnitude <= 3, alpha, c, beta powers of two from POW2.
Then |A y| <= 36, -alpha c - 1 is exact, and every term of either path — the fused one forms (y - beta z + alpha (A y)) + (-alpha c - 1) y,
at most 159 + 51 in magnitude in multiples of 2^-4 — is exact: both paths must equal numpy's alpha (A y - c y) - beta z with
np.array_equal, and so each other.  The windows sit inside wider blocks whose other columns must come back bit for bit.

The fused path needs a matrix whose product is worth forming twice (gcge_hip_cg_recompute_pays: the chain + line-exchange layout).  The
smallest lap3d that has it is found by asking the handles from 16^3 upwards: 16^3 (test_smallest_fused_size states it)."""
import numpy as np
import pytest

from gcge_amd.lib import cheb_stats, csr_to_scipy, make_problem
from helpers import bits, draw
from test_pcg_sweeps import POW2

FUSED_N = 16           # the size the search below finds
U = np.longdouble(2.0) ** -53


def smallest_fused_size(hip):
    for N in range(16, 64):
        A, _ = make_problem("lap3d", N)
        m = hip.matrix(A)
        pays = hip.g.gcge_hip_cg_recompute_pays(m)
        hip.free_matrix(m)
        if pays == 1:
            return N
    return None


@pytest.fixture(scope="module")
def lap(hip):
    A, _ = make_problem("lap3d", FUSED_N)
    S = csr_to_scipy(A)
    assert np.array_equal(S.data, np.round(S.data)) and np.abs(S.data).max() == 6.0          # the integer stencil
    m = hip.matrix(A)
    yield S, m
    hip.free_matrix(m)


def step(hip, S, mat, m, col, seed, z_mode="data", scalars=None, real=False, same_block=None):
    """One call on blocks of col + m + 2 columns with the windows at column `col`; returns (return code, the three blocks as numpy before,
    the out block after, alpha, c, beta).  z_mode "null": beta = 0 and z = NULL."""
    n, w = S.shape[0], col + m + 2
    Y, Z, O = (np.asfortranarray(draw(seed + k, (n, w), real)) for k in range(3))
    a, c, b = scalars if scalars is not None else (float(v) for v in POW2[np.random.default_rng(seed + 3).integers(0, len(POW2), 3)])
    if z_mode == "null":
        b = 0.0
    my, mz, mo = hip.mv_from_numpy(mat, Y), hip.mv_from_numpy(mat, Z), hip.mv_from_numpy(mat, O)
    try:
        if same_block == "out is y":
            rc = hip.g.gcge_hip_cheb_step_mv(mat, my, col, mz, col, my, col, m, a, c, b)
        elif same_block == "out is z":
            rc = hip.g.gcge_hip_cheb_step_mv(mat, my, col, mz, col, mz, col, m, a, c, b)
        elif same_block == "z is y":
            rc = hip.g.gcge_hip_cheb_step_mv(mat, my, col, my, col, mo, col, m, a, c, b)
        else:
            rc = hip.g.gcge_hip_cheb_step_mv(mat, my, col, None if z_mode == "null" else mz, col, mo, col, m, a, c, b)
        hip.sync()
        got = [hip.mv_to_numpy(v, n, 0, w) for v in (my, mz, mo)]
    finally:
        for v in (my, mz, mo):
            hip.ops.mv_destroy(v, w)
    return rc, (Y, Z, O), got, (a, c, b)


def check_exact(S, m, col, before, got, scal):
    (Y, Z, O), (a, c, b) = before, scal
    ref = O.copy()
    ref[:, col:col + m] = a * (S @ Y[:, col:col + m] - c * Y[:, col:col + m]) - (b * Z[:, col:col + m] if b != 0.0 else 0.0)
    assert np.array_equal(got[2], ref), np.argwhere(got[2] != ref)[:4].tolist()                   # the window, and the columns round it
    assert np.array_equal(bits(np.ascontiguousarray(got[0])), bits(np.ascontiguousarray(Y)))
    assert np.array_equal(bits(np.ascontiguousarray(got[1])), bits(np.ascontiguousarray(Z)))


@pytest.mark.gpu
def test_smallest_fused_size(hip):
    assert smallest_fused_size(hip) == FUSED_N


@pytest.mark.gpu
@pytest.mark.parametrize("m", [2, 8, 16, 64])
def test_fused_and_sweep_paths_equal_numpy(hip, lap, m, monkeypatch):
    S, mat = lap
    s0 = cheb_stats()
    rc, before, got, scal = step(hip, S, mat, m, 2, 31 * m)
    s1 = cheb_stats()
    assert rc == 0 and (s1[0] - s0[0], s1[1] - s0[1], s1[2] - s0[2]) == (1, 0, 0), (s0, s1)       # fused
    check_exact(S, m, 2, before, got, scal)
    monkeypatch.setenv("GCGE_CHEB_NO_FUSE", "1")
    rc, before2, got2, scal2 = step(hip, S, mat, m, 2, 31 * m)
    s2 = cheb_stats()
    assert rc == 0 and (s2[0] - s1[0], s2[1] - s1[1], s2[2] - s1[2]) == (0, 1, 0), (s1, s2)       # the same handle: product + sweep
    check_exact(S, m, 2, before2, got2, scal2)
    assert np.array_equal(bits(np.ascontiguousarray(got[2])), bits(np.ascontiguousarray(got2[2])))


@pytest.mark.gpu
@pytest.mark.parametrize("m,col", [(1, 2), (7, 2), (2, 1), (8, 3), (16, 1), (64, 1)])
def test_odd_widths_and_origins_take_the_sweep_path(hip, lap, m, col):
    S, mat = lap
    s0 = cheb_stats()
    rc, before, got, scal = step(hip, S, mat, m, col, 57 * m + col)
    s1 = cheb_stats()
    assert rc == 0 and (s1[0] - s0[0], s1[1] - s0[1], s1[2] - s0[2]) == (0, 1, 0), (s0, s1)
    check_exact(S, m, col, before, got, scal)


@pytest.mark.gpu
@pytest.mark.parametrize("m", [2, 7, 64])
def test_first_step_takes_the_sweep_path_and_reads_no_z(hip, lap, m):
    S, mat = lap
    s0 = cheb_stats()
    rc, before, got, scal = step(hip, S, mat, m, 2, 77 * m, z_mode="null")
    s1 = cheb_stats()
    assert rc == 0 and scal[2] == 0.0 and (s1[0] - s0[0], s1[1] - s0[1], s1[2] - s0[2]) == (0, 1, 0), (s0, s1)
    check_exact(S, m, 2, before, got, scal)


@pytest.mark.gpu
@pytest.mark.parametrize("alias", ["out is y", "out is z", "z is y"])
def test_aliased_blocks_are_declined_with_nothing_written(hip, lap, alias):
    S, mat = lap
    s0 = cheb_stats()
    rc, (Y, Z, O), got, scal = step(hip, S, mat, 8, 2, 91, same_block=alias)
    s1 = cheb_stats()
    assert rc == -1 and (s1[0] - s0[0], s1[1] - s0[1], s1[2] - s0[2]) == (0, 0, 1), (s0, s1)
    for g, b in zip(got, (Y, Z, O)):
        assert np.array_equal(bits(np.ascontiguousarray(g)), bits(np.ascontiguousarray(b)))


@pytest.mark.gpu
def test_column_ranges_outside_a_block_are_declined(hip, lap):
    S, mat = lap
    rc, (Y, Z, O), got, scal = step(hip, S, mat, 8, 2, 93)              # (a valid call first: the blocks' width is col + m + 2 = 12)
    assert rc == 0
    n = S.shape[0]
    my, mz, mo = (hip.mv_from_numpy(mat, np.asfortranarray(draw(95 + k, (n, 12), False))) for k in range(3))
    try:
        assert hip.g.gcge_hip_cheb_step_mv(mat, my, 6, mz, 2, mo, 2, 8, 1.0, 1.0, 1.0) == -1
        assert hip.g.gcge_hip_cheb_step_mv(mat, my, 2, mz, 2, mo, -1, 8, 1.0, 1.0, 1.0) == -1
        assert hip.g.gcge_hip_cheb_step_mv(None, my, 2, mz, 2, mo, 2, 8, 1.0, 1.0, 1.0) == -1
    finally:
        for v in (my, mz, mo):
            hip.ops.mv_destroy(v, 12)


@pytest.fixture(scope="module")
def sio2(hip):
    """make_problem("sio2", 12): (scipy matrix, the same as a dense long double array, |A|, the handle)"""
    A, _ = make_problem("sio2", 12)
    S = csr_to_scipy(A)
    mat = hip.matrix(A)
    yield S, S.toarray().astype(np.longdouble), abs(S), mat
    hip.free_matrix(mat)


@pytest.mark.gpu
@pytest.mark.parametrize("m", [2, 7, 16])
def test_sio2_handle_takes_the_sweep_path_within_the_rounding_bound(hip, sio2, m):
    """make_problem("sio2", 12) — no pattern table: the star / dense / pad-8 forms — with uniform data, against the product in long
    double.  Bound: the product's, (row length + 2) 2^-53 |A| |y| as tests/test_spmm_rows.py has it, times |alpha|, plus the sweep's three
    roundings 3 eps (|alpha| (|A y| + |c y|) + |beta z|) with |A y| <= |A| |y|."""
    S, Sl, Sa, mat = sio2
    form = hip.g.gcge_hip_mat_spmm_form(mat).decode()
    s0 = cheb_stats()
    rc, (Y, Z, O), got, (a, c, b) = step(hip, S, mat, m, 2, 11 * m, scalars=(0.37, 5.3, 0.81), real=True)
    s1 = cheb_stats()
    assert rc == 0 and "pattern" not in form and (s1[0] - s0[0], s1[1] - s0[1]) == (0, 1), (form, s0, s1)
    ld = lambda v: np.asarray(v, dtype=np.longdouble)
    y, z = Y[:, 2:2 + m], Z[:, 2:2 + m]
    ref = ld(a) * (Sl @ ld(y) - ld(c) * ld(y)) - ld(b) * ld(z)
    absAy = Sa @ np.abs(y)
    lens = np.diff(S.indptr)[:, None]
    bound = abs(a) * (lens + 2) * U * absAy + 3 * 2 * U * (abs(a) * (absAy + abs(c) * np.abs(y)) + abs(b) * np.abs(z))
    err = np.abs(ld(got[2][:, 2:2 + m]) - ref)
    print(form, "max error / bound:", float((err / bound).max()))
    assert np.all(err <= bound), (form, float((err / bound).max()))
    assert np.array_equal(bits(np.ascontiguousarray(got[2][:, :2])), bits(np.ascontiguousarray(O[:, :2])))
    assert np.array_equal(bits(np.ascontiguousarray(got[2][:, 2 + m:])), bits(np.ascontiguousarray(O[:, 2 + m:])))
