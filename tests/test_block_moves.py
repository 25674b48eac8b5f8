"""The block moves of an outer iteration of GCG: right-hand sides packed from an even column of the eigenvector block
(GCGE_GcgRhsOrigin, csrc/host/gcg.c), X / W start vectors / b in one sweep (GCGE_BACKEND.block_moves, csrc/hip/vec_kernels.hip:
block_moves_kernel) and MultiVecAxpby on column ranges with odd ends in one launch (axpby_edge_rows_kernel).  Everything here is a
copy or one rounded product per element, so every comparison is bit for bit."""
import ctypes as C
import itertools

import numpy as np
import pytest

from gcge_amd.lib import hip_lib, host_lib, make_problem, run_gcg
from helpers import csr_from_scipy, uniform


# ---------------------------------------------------------------------------------------------- host: where b goes
def _origin(first, total, startN, endX):
    return host_lib().GCGE_GcgRhsOrigin(first, total, startN, endX)


def _host_stats():
    a, b, c = C.c_long(), C.c_long(), C.c_long()
    host_lib().GCGE_GcgBlockMoveStats(C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


def test_rhs_origin_is_even_whenever_a_placement_fits():
    """Every (startN, endX, first, total) of a small eigenvector block: b stays inside [startN, endX), moves by at most one column,
    is even whenever first, first + 1 (b still ends inside endX) or first - 1 (still inside startN) is an even placement, and
    stays at `first` in the corner where neither fits."""
    corners = 0
    for startN, endX in itertools.product(range(0, 6), range(6, 14)):
        for first in range(startN, endX):
            for total in range(1, endX - first + 1):
                b0 = _origin(first, total, startN, endX)
                assert startN <= b0 and b0 + total <= endX and abs(b0 - first) <= 1
                up, down = first + 1 + total <= endX, first - 1 >= startN
                if first % 2 == 0:
                    assert b0 == first
                elif up:
                    assert b0 == first + 1
                elif down:
                    assert b0 == first - 1
                else:
                    assert b0 == first
                    corners += 1
    assert corners > 0
    assert _origin(3, 5, 3, 8) == 3          # odd first column = startN and the runs fill the block: today's path
    assert _origin(3, 4, 3, 8) == 4 and _origin(5, 3, 3, 8) == 4 and _origin(4, 4, 3, 8) == 4


def test_gcg_on_the_oracle_moves_b_off_odd_columns(oracle):
    """Lap3D 16^3, nev 12 / block 8 / nevMax 24 on the CPU oracle: the first unconverged column is odd in many outer iterations, b
    moves to an even column in each of them, and the solve converges to the closed-form eigenvalues as before."""
    from helpers import lap3d_exact
    A, _ = make_problem("lap3d", 16)
    s0 = _host_stats()
    ev, res = run_gcg(oracle.ops_handle, oracle.matrix(A), None, ["-nevConv", 12, "-nevMax", 24, "-blockSize", 8])
    odd, realigned, fused = (v - w for v, w in zip(_host_stats(), s0))
    ex = lap3d_exact(16, 12)
    assert res.nevConv >= 12 and np.max(np.abs(ev[:12] - ex) / ex) < 1e-10
    assert odd >= 3 and realigned == odd and fused == 0


# ---------------------------------------------------------------------------------------------- HIP: the sweep
def _tridiag(hip, n):
    import scipy.sparse as sp
    S = sp.diags([-np.ones(n - 1), 2.0 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1]).tocsr()
    A, keep = csr_from_scipy(S)
    return hip.matrix(A), keep


def _fill(hip, mv, arr):
    a = np.asfortranarray(arr)
    hip.g.gcge_hip_mv_from_host(mv, 0, a.shape[1], a.ctypes.data_as(C.POINTER(C.c_double)), a.shape[0])


def _moves(hip, ritz, V, x0, x1, runs, w0, b, b0, scale):
    g = hip_lib()
    flat = [len(runs)] + [v for r in runs for v in r]
    sc = (C.c_double * max(1, len(scale)))(*scale)
    return g.gcge_hip_block_moves_mv(ritz, V, x0, x1, (C.c_int * len(flat))(*flat), w0, b, b0, sc)


def _expected(R, V, B, x0, x1, runs, w0, where, b0, scale):
    """(ritz, V, b) after the moves; where: None no b, "sep" a block of its own, "ritz" inside the eigenvector block."""
    R1, V1, B1 = R.copy(), V.copy(), B.copy()
    V1[:, x0:x1] = R[:, x0:x1]
    blk = 0
    for lo, hi in runs:
        V1[:, w0 + blk:w0 + blk + hi - lo] = R[:, lo:hi]
        q = R[:, lo:hi] * scale[blk:blk + hi - lo]
        if where == "sep":
            B1[:, b0 + blk:b0 + blk + hi - lo] = q
        elif where == "ritz":
            R1[:, b0 + blk:b0 + blk + hi - lo] = q
        blk += hi - lo
    return R1, V1, B1


RUNS = {"one": lambda x0: [(x0 + 2, x0 + 11)], "two_a": lambda x0: [(6, 11), (13, 18)], "two_b": lambda x0: [(7, 12), (14, 20)]}


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [37, 1025, 1500])
def test_block_moves_sweep_vs_numpy_bit_for_bit(hip, rows):
    """ritz of 40 columns, V of 72: every parity of x0 / x1, one run and two runs with odd and even ends, W at an even and an odd
    column, b absent / in a block of its own / inside ritz over the source columns (from lo - 1, lo and lo + 1) — the WHOLE blocks
    against numpy (sentinels everywhere else)."""
    mA, keep = _tridiag(hip, rows)
    R, V, B = uniform(11, (rows, 40)) - 0.5, uniform(12, (rows, 72)) + 7.0, uniform(13, (rows, 40)) - 9.0
    mr, mv, mb = hip.mv_from_numpy(mA, R), hip.mv_from_numpy(mA, V), hip.mv_from_numpy(mA, B)
    ncase = 0
    for x0, x1, tag in itertools.product((4, 5), (36, 37), RUNS):
        runs = RUNS[tag](x0)
        total, lo = sum(h - l for l, h in runs), runs[0][0]
        scale = list(1.0 + uniform(14 + x0 + x1, (total,)))
        w0 = 40 + (x1 & 1) + (1 if tag == "two_a" else 0)
        for where, b0 in [(None, 0), ("sep", 3), ("sep", 4), ("ritz", lo - 1), ("ritz", lo), ("ritz", lo + 1)]:
            _fill(hip, mr, R); _fill(hip, mv, V); _fill(hip, mb, B)
            took = _moves(hip, mr, mv, x0, x1, runs, w0, {None: None, "sep": mb, "ritz": mr}[where], b0, scale)
            assert took == 1, (x0, x1, tag, where, b0)
            e = _expected(R, V, B, x0, x1, runs, w0, where, b0, np.array(scale))
            got = (hip.mv_to_numpy(mr, rows, 0, 40), hip.mv_to_numpy(mv, rows, 0, 72), hip.mv_to_numpy(mb, rows, 0, 40))
            for name, a, b in zip(("ritz", "V", "b"), got, e):
                assert np.array_equal(a, b), (name, x0, x1, tag, where, b0)
            ncase += 1
    assert ncase == 72
    for h, w in ((mr, 40), (mv, 72), (mb, 40)):
        hip.ops.mv_destroy(h, w)
    hip.free_matrix(mA)


@pytest.mark.gpu
def test_block_moves_sweep_wide_rows_and_declines(hip):
    """300 columns: rows wider than one wave go through the workgroup form (loads, barrier, stores) with b over its own sources;
    shapes the hook does not take (V as the source, W inside X, a run outside [x0, x1)) are declined with nothing touched."""
    rows = 1100
    mA, keep = _tridiag(hip, rows)
    R, V = uniform(21, (rows, 300)) - 0.5, uniform(22, (rows, 560)) + 7.0
    mr, mv = hip.mv_from_numpy(mA, R), hip.mv_from_numpy(mA, V)
    runs = [(9, 40), (41, 120), (150, 283)]
    total = sum(h - l for l, h in runs)
    scale = 1.0 + uniform(23, (total,))
    for b0 in (8, 9, 10):
        _fill(hip, mr, R); _fill(hip, mv, V)
        assert _moves(hip, mr, mv, 3, 299, runs, 299, mr, b0, list(scale)) == 1
        e = _expected(R, V, R[:, :1], 3, 299, runs, 299, "ritz", b0, scale)
        assert np.array_equal(hip.mv_to_numpy(mr, rows, 0, 300), e[0]), b0
        assert np.array_equal(hip.mv_to_numpy(mv, rows, 0, 560), e[1]), b0
    _fill(hip, mr, R); _fill(hip, mv, V)
    assert _moves(hip, mv, mv, 3, 299, runs, 299, None, 0, [0.0]) == 0
    assert _moves(hip, mr, mv, 3, 299, runs, 200, None, 0, [0.0]) == 0
    assert _moves(hip, mr, mv, 10, 299, runs, 299, None, 0, [0.0]) == 0
    assert _moves(hip, mr, mv, 3, 299, runs, 299, mv, 8, list(scale)) == 0
    assert np.array_equal(hip.mv_to_numpy(mr, rows, 0, 300), R) and np.array_equal(hip.mv_to_numpy(mv, rows, 0, 560), V)
    hip.ops.mv_destroy(mr, 300)
    hip.ops.mv_destroy(mv, 560)
    hip.free_matrix(mA)


# ---------------------------------------------------------------------------------------------- HIP: axpby on odd ranges
@pytest.mark.gpu
@pytest.mark.parametrize("m", [9, 64])
@pytest.mark.parametrize("mode", ["copy", "scale", "axpby"])
def test_axpby_on_odd_ranges_equals_the_even_aligned_call(hip, m, mode):
    """gcge_hip_axpby with x and y starting on every combination of even / odd columns against the SAME numbers at column 0 of
    both blocks with an even width (the 16-byte row kernel): the m columns bit for bit, every other column of y untouched."""
    rows, me = 1500, m + (m & 1)
    mA, keep = _tridiag(hip, rows)
    g = hip_lib()
    alpha, beta = {"copy": (1.0, 0.0), "scale": (0.0, 0.375), "axpby": (1.7, -0.6)}[mode]
    X, Y = uniform(31, (rows, me)) - 0.5, uniform(32, (rows, me)) - 0.5

    def run(xo, yo, width):
        Xb, Yb = uniform(33, (rows, 80)) + 3.0, uniform(34, (rows, 80)) + 5.0
        Xb[:, xo:xo + me], Yb[:, yo:yo + me] = X, Y
        mx, my = hip.mv_from_numpy(mA, Xb), hip.mv_from_numpy(mA, Yb)
        ldx, ldy = C.c_long(), C.c_long()
        px, py = g.gcge_hip_mv_device_ptr(mx, C.byref(ldx)), g.gcge_hip_mv_device_ptr(my, C.byref(ldy))
        rc = g.gcge_hip_axpby(rows, alpha, None if mode == "scale" else px + 8 * xo, ldx.value, beta, py + 8 * yo, ldy.value, width, None)
        assert rc == 0
        out = hip.mv_to_numpy(my, rows, 0, 80)
        hip.ops.mv_destroy(mx, 80)
        hip.ops.mv_destroy(my, 80)
        return out, Yb

    ref, _ = run(0, 0, me)
    for xo, yo in itertools.product((2, 3), (4, 5)):
        out, Yb = run(xo, yo, m)
        assert np.array_equal(out[:, yo:yo + m], ref[:, :m]), (xo, yo)
        Yb[:, yo:yo + m] = ref[:, :m]
        assert np.array_equal(out, Yb), (xo, yo)
    hip.free_matrix(mA)


# ---------------------------------------------------------------------------------------------- HIP: GCG, one sweep against three moves
def _sweep_stats():
    out = (C.c_long * 4)()
    hip_lib().gcge_hip_sweep_stats(out)
    return tuple(out)


def _legacy_sums():
    g = hip_lib()
    return g.gcge_hip_bpcg_legacy_start_sums()


@pytest.mark.gpu
@pytest.mark.parametrize("size,nev,block,nevmax", [(20, 20, 16, 40), (16, 12, 8, 24)])
def test_gcg_block_amg_one_sweep_equals_the_three_moves(hip, monkeypatch, size, nev, block, nevmax):
    """Lap3D 20^3, nev 20 / block 16 / nevMax 40 (and 16^3, 12 / 8 / 24, whose level 0 takes the one-sweep CG starts), BlockAMG over
    3 levels, Cholesky-QR for X and W, host RNG, three runs in one process: the one-sweep moves ("sweep"), GCGE_NO_BLOCK_MOVES=1
    ("moves"), and the data flow before this change — b at the first unconverged column, three moves ("first":
    GCGE_RHS_FIRST_COLUMN=1 as well).  Eigenvalues, eigenvector block, numIter and nevConv are bit for bit the same in all three.
    With b on an even column at least three iterations start on an odd first unconverged column, b is realigned in each, and no CG
    start or fused residual is declined because of b's column; with b at the first column they are."""
    A, _ = make_problem("lap3d", size)
    n = A.nrows
    mA = hip.matrix(A)
    args = ["-nevConv", nev, "-nevMax", nevmax, "-blockSize", block, "-gcge_amg_levels", 3, "-gcge_initX_orth_method", "chol",
            "-gcge_compW_orth_method", "chol"]
    out = {}
    for tag in ("sweep", "moves", "first"):
        if tag != "sweep":
            monkeypatch.setenv("GCGE_NO_BLOCK_MOVES", "1")
        if tag == "first":
            monkeypatch.setenv("GCGE_RHS_FIRST_COLUMN", "1")
        hip.set_random_mode(0)
        C.CDLL(None).srand(0)
        h0, s0, l0 = _host_stats(), _sweep_stats(), _legacy_sums()
        ev, res, evec = run_gcg(hip.ops_handle, mA, None, args, keep_evec=True)
        out[tag] = (ev.copy(), hip.mv_to_numpy(evec, n, 0, nevmax), res.numIter, res.nevConv,
                    tuple(v - w for v, w in zip(_host_stats(), h0)), tuple(v - w for v, w in zip(_sweep_stats(), s0)), _legacy_sums() - l0)
        hip.ops.mv_destroy(evec, nevmax)
    monkeypatch.delenv("GCGE_NO_BLOCK_MOVES")
    monkeypatch.delenv("GCGE_RHS_FIRST_COLUMN")
    a, b, f = out["sweep"], out["moves"], out["first"]
    for t in ("sweep", "moves", "first"):
        print(t, "host (odd, realigned, fused)", out[t][4], "HIP (starts, declined for b, residuals, declined for b)", out[t][5],
              "starts with the column-dot sums", out[t][6])
    assert a[3] >= nev
    for other in (b, f):
        assert a[3] == other[3] and a[2] == other[2]
        assert np.array_equal(a[0], other[0])
        assert np.array_equal(a[1], other[1])
    for run in (a, b):
        odd, realigned, fused = run[4]
        assert odd >= 3 and realigned == odd
        assert run[5][2] > 0 and run[5][1] == 0 and run[5][3] == 0
    assert f[4][0] == a[4][0] and f[4][1] == 0 and f[5][3] > 0          # b at the first column: never realigned, residuals declined
    assert a[4][2] == a[2] and b[4][2] == 0 and f[4][2] == 0          # one sweep per outer iteration / none
    if size == 16:      # the plane is a multiple of 32 rows: the fused CG recomputes its product and starts in one sweep
        assert a[5][0] > 0 and a[6] > 0 and f[5][1] > 0 and f[6] == 0
    hip.free_matrix(mA)
