"""The three sweeps of GCGE_PCGSolve's step (csrc/hip/pcg_sweeps.hip) through their raw-pointer entry points, on EXACT data: the
blocks hold nonzero integers of magnitude <= 3 and alpha / beta are powers of two, so every product, every update and every sum is
exact in any order and the comparison with numpy is np.array_equal.

Every operand sits in a block larger than itself (helpers.Block: GR rows behind, columns on either side inside ld); what a sweep
writes carries a NaN with a payload of its own round it, which must come back bit for bit.  The four layouts put the operand on an
even or odd column of a block with an even or odd leading dimension: (even, even) with an even width takes the 16-byte lanes, the
three others and every odd width the scalar lanes — same results.  Rows: 1, 255 / 257 (round one workgroup's 256), 4099 (17
workgroups, the last one short)."""
import ctypes as C

import numpy as np
import pytest

from gcge_amd import abi
from helpers import IN_GUARD, LAYOUTS, OUT_GUARD, Block, bits, draw

ROWS = [1, 255, 257, 4099]
COLS = [1, 2, 7, 8, 64]
POW2 = np.array([0.5, -1.0, 2.0, -4.0, 1.0, -0.25])


class Lib:
    def __init__(self, hip):
        import torch
        self.torch, self.hip, self.g = torch, hip, hip.g
        self.st = hip.g.gcge_hip_stream()

    def call(self, name, *args):
        self.torch.cuda.synchronize()
        assert "gcge_hip_" + name in abi.HIP, name
        rc = getattr(self.g, "gcge_hip_" + name)(*args, self.st)
        self.hip.sync()
        assert rc == 0, (name, rc)


@pytest.fixture(scope="module")
def lib(hip):
    return Lib(hip)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def flags_for(m, seed, values):
    """a mix of the flag values, every one of them present when m allows"""
    f = np.random.default_rng(seed).integers(0, len(values), m)
    f[:min(m, len(values))] = np.arange(len(values))[::-1][:m]
    return np.asarray(values, dtype=np.int32)[f]


def coefs(m, seed):
    return POW2[np.random.default_rng(seed).integers(0, len(POW2), m)].copy()


def run_step(lib, n, m, layout, seed):
    P, W, X, R = (draw(seed + k, (n, m), False) for k in range(4))
    alpha, flag = coefs(m, seed + 4), flags_for(m, seed + 5, (0, 1))
    bp, bw = Block(lib.torch, P, layout, IN_GUARD), Block(lib.torch, W, layout, IN_GUARD)
    bx, br = Block(lib.torch, X, layout, OUT_GUARD), Block(lib.torch, R, layout, OUT_GUARD)
    rr = np.full(m, -1.0)
    lib.call("pcg_step", n, bp.ptr, bp.ld, bw.ptr, bw.ld, bx.ptr, bx.ld, br.ptr, br.ld, m, ptr(alpha), ptr(flag), ptr(rr))
    on = flag != 0
    xr, rn = np.where(on, X + alpha * P, X), np.where(on, R - alpha * W, R)
    what = ("pcg_step", n, m, layout)
    bx.check(xr, what); br.check(rn, what)          # (flagged columns updated, the others and the guards bit for bit what they were)
    bp.unchanged(what); bw.unchanged(what)
    assert np.array_equal(rr, np.where(on, (rn * rn).sum(axis=0), 0.0)), what
    return rr


def run_dots(lib, n, m, layout, seed):
    Z, R, W = (draw(seed + k, (n, m), False) for k in range(3))
    bz, br, bw = (Block(lib.torch, a, layout, IN_GUARD) for a in (Z, R, W))
    zr, zw = np.full(m, -1.0), np.full(m, -1.0)
    lib.call("pcg_dots", n, bz.ptr, bz.ld, br.ptr, br.ld, bw.ptr, bw.ld, m, ptr(zr), ptr(zw))
    what = ("pcg_dots", n, m, layout)
    assert np.array_equal(zr, (Z * R).sum(axis=0)) and np.array_equal(zw, (Z * W).sum(axis=0)), what
    for b in (bz, br, bw):
        b.unchanged(what)
    return np.concatenate([zr, zw])


def run_direction(lib, n, m, layout, seed):
    Z, P = draw(seed, (n, m), False), draw(seed + 1, (n, m), False)
    beta, flag = coefs(m, seed + 2), flags_for(m, seed + 3, (0, 1, 2))
    Pin = P.copy()
    Pin[:, flag == 2] = np.nan                      # p = z does not use p
    bz, bp = Block(lib.torch, Z, layout, IN_GUARD), Block(lib.torch, Pin, layout, OUT_GUARD)
    lib.call("pcg_direction", n, bz.ptr, bz.ld, bp.ptr, bp.ld, m, ptr(beta), ptr(flag))
    what = ("pcg_direction", n, m, layout)
    bp.check(np.where(flag == 1, Z + beta * P, np.where(flag == 2, Z, P)), what)
    bz.unchanged(what)


def test_the_data_is_exact():
    """the premise: the largest sum, 4099 rows of (3 + 4 * 3)^2, is an integer multiple of 2^-4 far below 2^53"""
    assert 4099 * (3 + 4 * 3) ** 2 * 16 < 2 ** 53
    for a in POW2:
        assert np.frexp(a)[0] in (0.5, -0.5)


@pytest.mark.gpu
@pytest.mark.parametrize("n", ROWS)
def test_pcg_step_rows(lib, n):
    for m in COLS:
        for li, layout in enumerate(LAYOUTS):
            a = run_step(lib, n, m, layout, 100 * m + li)
            b = run_step(lib, n, m, layout, 100 * m + li)
            assert np.array_equal(bits(a), bits(b))                 # the sums of two runs: the same bits


@pytest.mark.gpu
@pytest.mark.parametrize("n", ROWS)
def test_pcg_dots_rows(lib, n):
    for m in COLS:
        for li, layout in enumerate(LAYOUTS):
            a = run_dots(lib, n, m, layout, 200 * m + li)
            b = run_dots(lib, n, m, layout, 200 * m + li)
            assert np.array_equal(bits(a), bits(b))


@pytest.mark.gpu
@pytest.mark.parametrize("n", ROWS)
def test_pcg_direction_rows(lib, n):
    for m in COLS:
        for li, layout in enumerate(LAYOUTS):
            run_direction(lib, n, m, layout, 300 * m + li)


@pytest.mark.gpu
def test_sums_of_inexact_data_are_the_same_bits_on_every_run(lib):
    """uniform data, where the order of summation shows: the partial sums are added in a fixed order"""
    n, m = 4099, 8
    Z, R, W = (draw(400 + k, (n, m), True) for k in range(3))
    out = []
    for _ in range(2):
        bz, br, bw = (Block(lib.torch, a, LAYOUTS[0], IN_GUARD) for a in (Z, R, W))
        zr, zw = np.zeros(m), np.zeros(m)
        lib.call("pcg_dots", n, bz.ptr, bz.ld, br.ptr, br.ld, bw.ptr, bw.ld, m, ptr(zr), ptr(zw))
        alpha, flag, rr = coefs(m, 7), np.ones(m, dtype=np.int32), np.zeros(m)
        bx, bq = Block(lib.torch, Z, LAYOUTS[0], OUT_GUARD), Block(lib.torch, R, LAYOUTS[0], OUT_GUARD)
        lib.call("pcg_step", n, bz.ptr, bz.ld, bw.ptr, bw.ld, bx.ptr, bx.ld, bq.ptr, bq.ld, m, ptr(alpha), ptr(flag), ptr(rr))
        out.append(np.concatenate([zr, zw, rr]))
    assert np.array_equal(bits(out[0]), bits(out[1]))
    assert np.allclose(out[0][:m], (Z * R).sum(axis=0), rtol=0, atol=1e-11)
