"""The sums of a band-pass Chebyshev filter (gcge_hip_cheb_accum, csrc/hip/cheb_sweeps.hip) through the raw-pointer entry point, on
EXACT data as tests/test_cheb_sweep.py: the blocks hold nonzero integers of magnitude <= 3 and mu_a, mu_b are powers of two, so

    acc <- [acc +] mu_a ta + mu_b tb

is exact whatever the order of its roundings and the comparison with numpy is np.array_equal.  acc sits in a helpers.Block with NaN
guards that must come back bit for bit, ta and tb in blocks that must not be written.  The four layouts and the widths take the
16-byte lanes ((even, even), even width) and the scalar lanes (everything else); rows 1, 255 / 257, 4099 as there.  The init form must
not read acc (it is NaN-filled), the one-term form gets tb == NULL."""
import numpy as np
import pytest

from helpers import IN_GUARD, LAYOUTS, OUT_GUARD, Block, bits, draw
from test_pcg_sweeps import COLS, POW2, ROWS, Lib  # noqa: F401


@pytest.fixture(scope="module")
def lib(hip):
    return Lib(hip)


def scalars(seed):
    a, b = POW2[np.random.default_rng(seed).integers(0, len(POW2), 2)]
    return float(a), float(b)


def accum(lib, bc, ba, bb, mu_a, mu_b, n, m, init):
    lib.call("cheb_accum", n, bc.ptr, bc.ld, ba.ptr, ba.ld, mu_a, bb.ptr if bb is not None else None, bb.ld if bb is not None else 0, mu_b, m,
             init)


def run_accum(lib, n, m, layout, seed, init=False, two=True):
    """init: acc holds NaN and must not be read; two=False: tb == NULL (mu_b is passed as NaN: it must be ignored)"""
    Cc, Ta, Tb = (draw(seed + k, (n, m), False) for k in range(3))
    mu_a, mu_b = scalars(seed + 3)
    bc = Block(lib.torch, np.full((n, m), np.nan) if init else Cc, layout, OUT_GUARD)
    ba, bb = Block(lib.torch, Ta, layout, IN_GUARD), Block(lib.torch, Tb, layout, IN_GUARD) if two else None
    accum(lib, bc, ba, bb, mu_a, mu_b if two else float("nan"), n, m, 1 if init else 0)
    ref = (0.0 if init else Cc) + mu_a * Ta + (mu_b * Tb if two else 0.0)
    what = ("cheb_accum", n, m, layout, "init" if init else "add", "two terms" if two else "one term", mu_a, mu_b)
    assert not np.isnan(ref).any()
    bc.check(ref, what)                              # (the result, and the guards bit for bit what they were)
    ba.unchanged(what)
    if bb is not None:
        bb.unchanged(what)


def test_the_data_is_exact():
    """the premise: every intermediate is a multiple of 2^-2 of magnitude <= 3 + 4 * 3 + 4 * 3 = 27, far inside 2^53 multiples"""
    assert np.abs(POW2).max() == 4.0 and np.abs(POW2).min() == 0.25 and np.all(np.log2(np.abs(POW2)) == np.round(np.log2(np.abs(POW2))))
    for s in range(8):
        v = draw(s, (64, 8), False)
        assert np.array_equal(v, np.round(v)) and np.abs(v).max() <= 3 and np.abs(v).min() >= 1
    assert 3 + 4 * 3 + 4 * 3 == 27 and 27 * 4 < 2 ** 53


@pytest.mark.gpu
@pytest.mark.parametrize("n", ROWS)
def test_two_terms_onto_acc(lib, n):
    for m in COLS:
        for li, layout in enumerate(LAYOUTS):
            run_accum(lib, n, m, layout, 1100 * m + li)


@pytest.mark.gpu
@pytest.mark.parametrize("n", ROWS)
def test_init_does_not_read_acc(lib, n):
    for m in COLS:
        for li, layout in enumerate(LAYOUTS):
            run_accum(lib, n, m, layout, 1300 * m + li, init=True)


@pytest.mark.gpu
@pytest.mark.parametrize("init", [False, True])
@pytest.mark.parametrize("n", ROWS)
def test_one_term_with_tb_null(lib, n, init):
    for m in COLS:
        for li, layout in enumerate(LAYOUTS):
            run_accum(lib, n, m, layout, 1500 * m + li, init=init, two=False)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [LAYOUTS[0], LAYOUTS[3]])
def test_inexact_data_same_bits_on_every_run_and_two_roundings(lib, layout):
    """uniform data: two runs give the same bits; against a long double reference every entry is within
    3 * 2^-53 (|acc| + |mu_a ta| + |mu_b tb|): the two roundings, s = fma(mu_a, ta, acc) and fma(mu_b, tb, s), are each at most 2^-53
    times a value that this sum bounds, and the third unit covers the reference's own."""
    n, m = 4099, 8
    Cc, Ta, Tb = (draw(1000 + k, (n, m), True) for k in range(3))
    mu_a, mu_b = 0.37, -0.81
    out = []
    for _ in range(2):
        bc, ba, bb = Block(lib.torch, Cc, layout, OUT_GUARD), Block(lib.torch, Ta, layout, IN_GUARD), Block(lib.torch, Tb, layout, IN_GUARD)
        accum(lib, bc, ba, bb, mu_a, mu_b, n, m, 0)
        out.append(bc.dev.cpu().numpy())
    assert np.array_equal(bits(out[0]), bits(out[1]))
    ld = lambda v: np.asarray(v, dtype=np.longdouble)
    ref = ld(Cc) + ld(mu_a) * ld(Ta) + ld(mu_b) * ld(Tb)
    bound = 3 * 2.0 ** -53 * (np.abs(Cc) + np.abs(mu_a * Ta) + np.abs(mu_b * Tb))
    got = ld(out[1][:n, bc.gl:bc.gl + m])
    err = np.abs(got - ref)
    print("max error / bound:", float((err / bound).max()))
    assert np.all(err <= bound), float((err / bound).max())
    bc.check(np.asarray(ref, dtype=np.float64), ("cheb_accum", "uniform", layout), bound)      # (and the guards)


@pytest.mark.gpu
def test_bad_arguments_return_minus_one_with_acc_untouched(lib):
    n, m, layout = 257, 8, LAYOUTS[0]
    Cc, Ta, Tb = (draw(1900 + k, (n, m), False) for k in range(3))
    bc, ba, bb = Block(lib.torch, Cc, layout, OUT_GUARD), Block(lib.torch, Ta, layout, IN_GUARD), Block(lib.torch, Tb, layout, IN_GUARD)
    f = lib.g.gcge_hip_cheb_accum
    lib.torch.cuda.synchronize()
    assert f(n, bc.ptr, bc.ld, bc.ptr, bc.ld, 1.0, bb.ptr, bb.ld, 1.0, m, 0, lib.st) == -1          # acc == ta
    assert f(n, bc.ptr, bc.ld, ba.ptr, ba.ld, 1.0, bc.ptr, bc.ld, 1.0, m, 0, lib.st) == -1          # acc == tb
    assert f(n, None, bc.ld, ba.ptr, ba.ld, 1.0, bb.ptr, bb.ld, 1.0, m, 0, lib.st) == -1            # NULL acc
    assert f(n, bc.ptr, bc.ld, None, ba.ld, 1.0, bb.ptr, bb.ld, 1.0, m, 0, lib.st) == -1            # NULL ta
    assert f(-1, bc.ptr, bc.ld, ba.ptr, ba.ld, 1.0, bb.ptr, bb.ld, 1.0, m, 0, lib.st) == -1         # n < 0
    assert f(n, bc.ptr, bc.ld, ba.ptr, ba.ld, 1.0, bb.ptr, bb.ld, 1.0, -1, 0, lib.st) == -1         # m < 0
    assert f(0, bc.ptr, bc.ld, ba.ptr, ba.ld, 1.0, bb.ptr, bb.ld, 1.0, m, 0, lib.st) == 0           # nothing to do
    assert f(n, bc.ptr, bc.ld, ba.ptr, ba.ld, 1.0, bb.ptr, bb.ld, 1.0, 0, 0, lib.st) == 0
    lib.hip.sync()
    for b in (bc, ba, bb):
        b.unchanged("bad arguments")
