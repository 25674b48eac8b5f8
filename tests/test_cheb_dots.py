"""The sweep of a Chebyshev step with its two column sums, and the sums alone (gcge_hip_cheb_sweep_dots, gcge_hip_cheb_dots,
csrc/hip/cheb_sweeps.hip) through the raw-pointer entry points, on EXACT data as tests/test_cheb_accum.py: the blocks hold nonzero
integers of magnitude <= 3 and alpha, c, beta are powers of two from POW2, so

    out <- alpha (out - c y) - beta z ,   oo_j = sum_r out_new[r, j]^2 ,   oy_j = sum_r out_new[r, j] y[r, j]

are exact whatever the order of the roundings and of the additions, and the comparison with numpy is np.array_equal — for out also with
what gcge_hip_cheb_sweep writes on a copy.  out sits in a helpers.Block with NaN guards that must come back bit for bit, y, z and t in
blocks that must not be written; the sums come back in host arrays with a sentinel at each end.  The four layouts and the widths take
the 16-byte lanes ((even, even), even width) and the scalar lanes (everything else); rows 1, 255 / 257 (one workgroup, two), 4099."""
import ctypes as C

import numpy as np
import pytest

from helpers import IN_GUARD, LAYOUTS, OUT_GUARD, Block, bits, draw
from test_pcg_sweeps import COLS, POW2, ROWS, Lib  # noqa: F401

SENTINEL = -12345.0


@pytest.fixture(scope="module")
def lib(hip):
    return Lib(hip)


class Sums:
    """two host arrays of m doubles for the sums, a sentinel in front of and behind each"""

    def __init__(self, m):
        self.m = m
        self.a, self.b = np.full(m + 2, SENTINEL), np.full(m + 2, SENTINEL)
        self.pa, self.pb = (C.c_void_p(v.ctypes.data + 8) for v in (self.a, self.b))

    def get(self, what):
        for v in (self.a, self.b):
            assert v[0] == SENTINEL and v[-1] == SENTINEL, (what, "a sum was written outside its m entries")
        return self.a[1:-1].copy(), self.b[1:-1].copy()

    def untouched(self):
        return np.all(self.a == SENTINEL) and np.all(self.b == SENTINEL)


def scalars(seed, with_beta=True):
    a, c, b = POW2[np.random.default_rng(seed).integers(0, len(POW2), 3)]
    return float(a), float(c), float(b) if with_beta else 0.0


def run_sweep_dots(lib, n, m, layout, seed, z_mode="data"):
    """z_mode: "data" (beta != 0), "nan" (beta == 0, z holds NaN), "null" (beta == 0, z == NULL)"""
    O, Y, Z = (draw(seed + k, (n, m), False) for k in range(3))
    alpha, c, beta = scalars(seed + 3, z_mode == "data")
    what = ("cheb_sweep_dots", n, m, layout, z_mode, alpha, c, beta)
    bo, bo2, by = Block(lib.torch, O, layout, OUT_GUARD), Block(lib.torch, O, layout, OUT_GUARD), Block(lib.torch, Y, layout, IN_GUARD)
    bz = None if z_mode == "null" else Block(lib.torch, Z if z_mode == "data" else np.full((n, m), np.nan), layout, IN_GUARD)
    zp, zl = (bz.ptr, bz.ld) if bz is not None else (None, 0)
    s = Sums(m)
    lib.call("cheb_sweep_dots", n, bo.ptr, bo.ld, by.ptr, by.ld, zp, zl, m, alpha, c, beta, s.pa, s.pb)
    lib.call("cheb_sweep", n, bo2.ptr, bo2.ld, by.ptr, by.ld, zp, zl, m, alpha, c, beta)
    ref = alpha * (O - c * Y) - (beta * Z if z_mode == "data" else 0.0)
    assert not np.isnan(ref).any()
    bo.check(ref, what)                              # (the result, and the guards bit for bit what they were)
    assert np.array_equal(bits(bo.dev.cpu().numpy()), bits(bo2.dev.cpu().numpy())), (what, "not the bits of gcge_hip_cheb_sweep")
    by.unchanged(what)
    if bz is not None:
        bz.unchanged(what)
    oo, oy = s.get(what)
    assert np.array_equal(oo, np.sum(ref * ref, axis=0)), (what, "oo", oo, np.sum(ref * ref, axis=0))
    assert np.array_equal(oy, np.sum(ref * Y, axis=0)), (what, "oy", oy, np.sum(ref * Y, axis=0))


def run_dots(lib, n, m, layout, seed):
    T, Y = (draw(seed + k, (n, m), False) for k in range(2))
    what = ("cheb_dots", n, m, layout)
    bt, by = Block(lib.torch, T, layout, IN_GUARD), Block(lib.torch, Y, layout, IN_GUARD)
    s = Sums(m)
    lib.call("cheb_dots", n, bt.ptr, bt.ld, by.ptr, by.ld, m, s.pa, s.pb)
    bt.unchanged(what)
    by.unchanged(what)
    tt, ty = s.get(what)
    assert np.array_equal(tt, np.sum(T * T, axis=0)), (what, "tt")
    assert np.array_equal(ty, np.sum(T * Y, axis=0)), (what, "ty")


def test_the_data_is_exact():
    """the premise: out_new is a multiple of 2^-6 of magnitude <= 4 (3 + 4 * 3) + 4 * 3 = 72 (tests/test_cheb_sweep.py), so every
    term out_new^2 is a multiple of 2^-12 of magnitude <= 72^2 and every term out_new y a multiple of 2^-6 of magnitude <= 216; a sum
    of at most 4099 of them, in any order and with any partial sums, is a multiple of 2^-12 below 4099 * 5184 < 2^25: 37 bits, far
    inside the 53 of a double.  numpy's own sums are exact for the same reason."""
    assert np.abs(POW2).max() == 4.0 and np.abs(POW2).min() == 0.25 and np.all(np.log2(np.abs(POW2)) == np.round(np.log2(np.abs(POW2))))
    for s in range(8):
        v = draw(s, (64, 8), False)
        assert np.array_equal(v, np.round(v)) and np.abs(v).max() <= 3 and np.abs(v).min() >= 1
    assert 4 * (3 + 4 * 3) + 4 * 3 == 72 and np.abs(POW2).min() ** 2 == 2.0 ** -4 and max(ROWS) == 4099
    assert max(ROWS) * 72 ** 2 < 2 ** 25 and 25 + 12 < 53
    worst = np.full((max(ROWS), 1), 72.0 - 2.0 ** -6)
    assert float(np.sum(worst * worst)) == max(ROWS) * (72.0 - 2.0 ** -6) ** 2      # (no rounding at the largest magnitudes)


@pytest.mark.gpu
@pytest.mark.parametrize("n", ROWS)
def test_sweep_dots_rows(lib, n):
    for m in COLS:
        for li, layout in enumerate(LAYOUTS):
            run_sweep_dots(lib, n, m, layout, 2100 * m + li)


@pytest.mark.gpu
@pytest.mark.parametrize("z_mode", ["nan", "null"])
@pytest.mark.parametrize("n", ROWS)
def test_first_step_does_not_read_z(lib, n, z_mode):
    for m in COLS:
        for li, layout in enumerate(LAYOUTS):
            run_sweep_dots(lib, n, m, layout, 2300 * m + li, z_mode)


@pytest.mark.gpu
@pytest.mark.parametrize("n", ROWS)
def test_dots_rows(lib, n):
    for m in COLS:
        for li, layout in enumerate(LAYOUTS):
            run_dots(lib, n, m, layout, 2500 * m + li)


def sum_bound(n, terms):
    return (n + 2) * 2.0 ** -53 * np.sum(np.abs(np.asarray(terms, dtype=np.float64)), axis=0)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [LAYOUTS[0], LAYOUTS[3]])
def test_inexact_data_same_bits_on_every_run_and_the_sums_error(lib, layout):
    """uniform data at n = 4099, m = 8: two runs give the same bits, in out and in all four sums.  Against a long double reference
    over the values the kernel stored, every sum is within (n + 2) 2^-53 sum |terms|: each term enters by one fma (one rounding of a
    partial sum that sum |terms| bounds), a column's n terms pass through at most n such additions whatever the tree of thread, lane
    and workgroup sums, and the two spare units cover the reference's own rounding to double."""
    n, m = 4099, 8
    O, Y, Z = (draw(2800 + k, (n, m), True) for k in range(3))
    alpha, c, beta = 0.37, 5.3, 0.81
    runs = []
    for _ in range(2):
        bo, by, bz = Block(lib.torch, O, layout, OUT_GUARD), Block(lib.torch, Y, layout, IN_GUARD), Block(lib.torch, Z, layout, IN_GUARD)
        s, s2 = Sums(m), Sums(m)
        lib.call("cheb_sweep_dots", n, bo.ptr, bo.ld, by.ptr, by.ld, bz.ptr, bz.ld, m, alpha, c, beta, s.pa, s.pb)
        lib.call("cheb_dots", n, bo.ptr, bo.ld, by.ptr, by.ld, m, s2.pa, s2.pb)
        runs.append((bo.dev.cpu().numpy(),) + s.get("uniform") + s2.get("uniform"))
    for a, b in zip(*runs):
        assert np.array_equal(bits(a), bits(b))
    got = runs[0][0][:n, bo.gl:bo.gl + m]
    eps = np.finfo(np.float64).eps
    assert np.all(np.abs(got - (alpha * (O - c * Y) - beta * Z)) <= 3 * eps * (abs(alpha) * (np.abs(O) + np.abs(c * Y)) + np.abs(beta * Z)))
    ld = lambda v: np.asarray(v, dtype=np.longdouble)
    for name, sums, terms in (("oo", runs[0][1], ld(got) * ld(got)), ("oy", runs[0][2], ld(got) * ld(Y)),
                              ("tt", runs[0][3], ld(got) * ld(got)), ("ty", runs[0][4], ld(got) * ld(Y))):
        err, bound = np.abs(ld(sums) - np.sum(terms, axis=0)), sum_bound(n, terms)
        print(name, layout, "max error / bound:", float((err / bound).max()))
        assert np.all(err <= bound), (name, float((err / bound).max()))


@pytest.mark.gpu
def test_bad_arguments_return_minus_one_with_nothing_touched(lib):
    n, m, layout = 257, 8, LAYOUTS[0]
    O, Y, Z = (draw(2900 + k, (n, m), False) for k in range(3))
    bo, by, bz = Block(lib.torch, O, layout, OUT_GUARD), Block(lib.torch, Y, layout, IN_GUARD), Block(lib.torch, Z, layout, IN_GUARD)
    s = Sums(m)
    f, g = lib.g.gcge_hip_cheb_sweep_dots, lib.g.gcge_hip_cheb_dots
    lib.torch.cuda.synchronize()
    assert f(n, bo.ptr, bo.ld, bo.ptr, bo.ld, bz.ptr, bz.ld, m, 1.0, 1.0, 1.0, s.pa, s.pb, lib.st) == -1          # out == y
    assert f(n, bo.ptr, bo.ld, by.ptr, by.ld, bo.ptr, bo.ld, m, 1.0, 1.0, 1.0, s.pa, s.pb, lib.st) == -1          # out == z
    assert f(n, None, bo.ld, by.ptr, by.ld, bz.ptr, bz.ld, m, 1.0, 1.0, 1.0, s.pa, s.pb, lib.st) == -1            # NULL out
    assert f(n, bo.ptr, bo.ld, None, by.ld, bz.ptr, bz.ld, m, 1.0, 1.0, 1.0, s.pa, s.pb, lib.st) == -1            # NULL y
    assert f(n, bo.ptr, bo.ld, by.ptr, by.ld, None, 0, m, 1.0, 1.0, 1.0, s.pa, s.pb, lib.st) == -1                # NULL z with beta != 0
    assert f(-1, bo.ptr, bo.ld, by.ptr, by.ld, bz.ptr, bz.ld, m, 1.0, 1.0, 1.0, s.pa, s.pb, lib.st) == -1         # n < 0
    assert f(n, bo.ptr, bo.ld, by.ptr, by.ld, bz.ptr, bz.ld, -1, 1.0, 1.0, 1.0, s.pa, s.pb, lib.st) == -1         # m < 0
    assert f(n, bo.ptr, bo.ld, by.ptr, by.ld, bz.ptr, bz.ld, m, 1.0, 1.0, 1.0, None, s.pb, lib.st) == -1          # NULL oo
    assert f(n, bo.ptr, bo.ld, by.ptr, by.ld, bz.ptr, bz.ld, m, 1.0, 1.0, 1.0, s.pa, None, lib.st) == -1          # NULL oy
    assert g(n, None, bo.ld, by.ptr, by.ld, m, s.pa, s.pb, lib.st) == -1
    assert g(n, bo.ptr, bo.ld, None, by.ld, m, s.pa, s.pb, lib.st) == -1
    assert g(-1, bo.ptr, bo.ld, by.ptr, by.ld, m, s.pa, s.pb, lib.st) == -1
    assert g(n, bo.ptr, bo.ld, by.ptr, by.ld, -1, s.pa, s.pb, lib.st) == -1
    assert g(n, bo.ptr, bo.ld, by.ptr, by.ld, m, None, s.pb, lib.st) == -1
    assert g(n, bo.ptr, bo.ld, by.ptr, by.ld, m, s.pa, None, lib.st) == -1
    assert s.untouched()
    assert f(n, bo.ptr, bo.ld, by.ptr, by.ld, bz.ptr, bz.ld, 0, 1.0, 1.0, 1.0, s.pa, s.pb, lib.st) == 0           # nothing to do
    assert g(n, bo.ptr, bo.ld, by.ptr, by.ld, 0, s.pa, s.pb, lib.st) == 0
    assert s.untouched()
    assert f(0, bo.ptr, bo.ld, by.ptr, by.ld, bz.ptr, bz.ld, m, 1.0, 1.0, 1.0, s.pa, s.pb, lib.st) == 0           # no rows: the sums are 0
    oo, oy = s.get("n == 0")
    assert np.all(oo == 0.0) and np.all(oy == 0.0)
    lib.hip.sync()
    for b in (bo, by, bz):
        b.unchanged("bad arguments")
