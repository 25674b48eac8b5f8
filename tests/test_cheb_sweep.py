"""The sweep of one step of a Chebyshev filter (gcge_hip_cheb_sweep, csrc/hip/cheb_sweeps.hip) through its raw-pointer entry point, on
EXACT data as tests/test_pcg_shift.py: the blocks hold nonzero integers of magnitude <= 3 and alpha, c, beta are powers of two, so

    out <- alpha (out - c y) - beta z

is exact whatever the order of its roundings and the comparison with numpy is np.array_equal.  out sits in a helpers.Block with NaN
guards that must come back bit for bit, y and z in blocks that must not be written.  The four layouts and the widths take the 16-byte
lanes ((even, even), even width) and the scalar lanes (everything else); rows 1, 255 / 257, 4099 as there.  beta == 0 (a filter's
first step) must not read z: it is NaN-filled, or NULL."""
import numpy as np
import pytest

from helpers import IN_GUARD, LAYOUTS, OUT_GUARD, Block, bits, draw
from test_pcg_sweeps import COLS, POW2, ROWS, Lib, ptr  # noqa: F401


@pytest.fixture(scope="module")
def lib(hip):
    return Lib(hip)


def scalars(seed, with_beta=True):
    a, c, b = POW2[np.random.default_rng(seed).integers(0, len(POW2), 3)]
    return float(a), float(c), float(b) if with_beta else 0.0


def run_sweep(lib, n, m, layout, seed, z_mode="data"):
    """z_mode: "data" (beta != 0), "nan" (beta == 0, z holds NaN), "null" (beta == 0, z == NULL)"""
    O, Y, Z = (draw(seed + k, (n, m), False) for k in range(3))
    alpha, c, beta = scalars(seed + 3, z_mode == "data")
    bo, by = Block(lib.torch, O, layout, OUT_GUARD), Block(lib.torch, Y, layout, IN_GUARD)
    bz = None if z_mode == "null" else Block(lib.torch, Z if z_mode == "data" else np.full((n, m), np.nan), layout, IN_GUARD)
    lib.call("cheb_sweep", n, bo.ptr, bo.ld, by.ptr, by.ld, bz.ptr if bz is not None else None, bz.ld if bz is not None else 0, m, alpha, c, beta)
    ref = alpha * (O - c * Y) - (beta * Z if z_mode == "data" else 0.0)
    what = ("cheb_sweep", n, m, layout, z_mode, alpha, c, beta)
    assert not np.isnan(ref).any()
    bo.check(ref, what)                              # (the result, and the guards bit for bit what they were)
    by.unchanged(what)
    if bz is not None:
        assert np.array_equal(bits(bz.dev.cpu().numpy()), bits(bz.host)), (what, "z was written")


def test_the_data_is_exact():
    """the premise: every intermediate is a multiple of 2^-6 below 2^7 — the smallest product of two coefficients is 2^-4, the largest
    result 4 (3 + 4 * 3) + 4 * 3 = 72"""
    assert np.abs(POW2).max() == 4.0 and np.abs(POW2).min() == 0.25
    assert np.abs(POW2).min() ** 2 >= 2.0 ** -6
    assert 4 * (3 + 4 * 3) + 4 * 3 < 2 ** 7


@pytest.mark.gpu
@pytest.mark.parametrize("n", ROWS)
def test_cheb_sweep_rows(lib, n):
    for m in COLS:
        for li, layout in enumerate(LAYOUTS):
            run_sweep(lib, n, m, layout, 700 * m + li)


@pytest.mark.gpu
@pytest.mark.parametrize("z_mode", ["nan", "null"])
@pytest.mark.parametrize("n", ROWS)
def test_first_step_does_not_read_z(lib, n, z_mode):
    for m in COLS:
        for li, layout in enumerate(LAYOUTS):
            run_sweep(lib, n, m, layout, 900 * m + li, z_mode)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [LAYOUTS[0], LAYOUTS[3]])
def test_inexact_data_same_bits_on_every_run_and_three_roundings(lib, layout):
    """uniform data: two runs give the same bits; against numpy each entry is within 3 eps (|alpha| (|out| + |c y|) + |beta z|), which
    covers the three roundings u = fma(-c, y, out), beta z, fma(alpha, u, -(beta z)) and numpy's own"""
    n, m = 4099, 8
    O, Y, Z = (draw(800 + k, (n, m), True) for k in range(3))
    alpha, c, beta = 0.37, 5.3, 0.81
    out = []
    for _ in range(2):
        bo, by, bz = Block(lib.torch, O, layout, OUT_GUARD), Block(lib.torch, Y, layout, IN_GUARD), Block(lib.torch, Z, layout, IN_GUARD)
        lib.call("cheb_sweep", n, bo.ptr, bo.ld, by.ptr, by.ld, bz.ptr, bz.ld, m, alpha, c, beta)
        out.append(bo.dev.cpu().numpy())
    assert np.array_equal(bits(out[0]), bits(out[1]))
    eps = np.finfo(np.float64).eps
    ref = alpha * (O - c * Y) - beta * Z
    bound = 3 * eps * (abs(alpha) * (np.abs(O) + np.abs(c * Y)) + np.abs(beta * Z))
    bo.check(ref, ("cheb_sweep", "uniform", layout), bound)
