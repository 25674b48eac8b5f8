"""Ritz vectors written over X with P moved in behind them (GCGE_BACKEND.ritz_in_place: the panel update's row-copy epilogue,
csrc/hip/lincomb_mfma.hip), the block moves with V as their source, and the column norms summed by the panel update that wrote
the columns (GCGE_BACKEND.panel_norms_sq).  The new data flow moves where values are stored, not how they are computed: every
comparison of blocks is bit for bit; only the norms, summed in another order than the column-dot sweep's, have a tolerance."""
import ctypes as C
import itertools

import numpy as np
import pytest

from gcge_amd.lib import hip_lib, host_lib, make_problem, run_gcg
from helpers import uniform
from test_block_moves import RUNS, _fill, _host_stats, _moves, _tridiag


def _ritz_stats():
    a = C.c_long()
    host_lib().GCGE_GcgRitzInPlaceStats(C.byref(a))
    return a.value


def _kahan_stats():
    a, b, c = C.c_long(), C.c_long(), C.c_long()
    host_lib().GCGE_OrthKahanStats(C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


# ---------------------------------------------------------------------------------------------- CPU: the old flow stays
def test_gcg_on_the_oracle_keeps_the_three_steps(oracle):
    """The CPU oracle's table offers neither capability: the driver keeps ComputeRitzVec / ComputeP / ComputeX (no fused launch is
    counted, no norm comes from a panel update) and converges as before."""
    from helpers import lap3d_exact
    A, _ = make_problem("lap3d", 10)
    r0, k0 = _ritz_stats(), _kahan_stats()
    ev, res = run_gcg(oracle.ops_handle, oracle.matrix(A), None, ["-nevConv", 6, "-nevMax", 12, "-blockSize", 4,
                                                                  "-gcge_initX_orth_method", "chol", "-gcge_compW_orth_method", "chol"])
    ex = lap3d_exact(10, 6)
    assert res.nevConv >= 6 and np.max(np.abs(ev[:6] - ex) / ex) < 1e-10
    assert _ritz_stats() - r0 == 0
    assert _kahan_stats()[2] - k0[2] == 0


# ---------------------------------------------------------------------------------------------- HIP: the fused launch
def _ritz_in_place(V, n0, x1, w1, coef, S, p0, np_):
    g = hip_lib()
    return g.gcge_hip_ritz_in_place_mv(V, n0, x1, w1, coef.ctypes.data_as(C.POINTER(C.c_double)), coef.shape[0], S, p0, np_)


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [37, 1025, 1500])
def test_ritz_in_place_equals_the_staged_update_and_the_copy(hip, rows):
    """V[:, n0..x1) = V[:, n0..w1) C in place and V[:, p0..p0 + np) = S[:, 0..np) in one launch, against MultiVecLinearComb into
    another block + two MultiVecAxpby copies on the same numbers: the WHOLE block V bit for bit (so every column outside the two
    targets is untouched), and the panel against numpy's product.  k = 40 and 200; panels of 9, 64 and 128 columns (40 where k is
    40) from an even and an odd column; 1, 16 and 64 staged columns to an even and an odd target behind the panel — inside the input
    range at k = 200, as in the solver, and behind it at k = 40.  Rows that are no multiple of a block's 128.  Panels of 9 columns
    take the kernel that stages X through LDS, the wider ones the register form; at 1025 rows the register form is forced for the
    narrow panels too (gcge_hip_lincomb_tune(3)).  129 columns are declined with nothing touched."""
    mA, keep = _tridiag(hip, rows)
    W = 212
    V0, S0 = uniform(61, (rows, W)) - 0.5, uniform(62, (rows, 64)) + 3.0
    mv, mz, mref, ms = (hip.mv_from_numpy(mA, V0), hip.mv_from_numpy(mA, np.zeros((rows, W))), hip.mv_from_numpy(mA, V0),
                        hip.mv_from_numpy(mA, S0))
    ncase = 0
    try:
        for tune in ((0, 3) if rows == 1025 else (0,)):
            hip.g.gcge_hip_lincomb_tune(tune)
            for (k, m), n0 in itertools.product([(40, 9), (40, 40), (200, 9), (200, 64), (200, 128)], (2, 3)):
                x1, w1 = n0 + m, n0 + k
                coef = np.asfortranarray(uniform(63 + k + m + n0, (k, m)) - 0.5)
                _fill(hip, mv, V0)
                hip.ops.lincomb(mv, mz, (n0, n0), (w1, x1), coef, k, None, 0)          # staged: Z[:, n0..x1) = V[:, n0..w1) C
                Z = hip.mv_to_numpy(mz, rows, 0, W)
                ref = V0[:, n0:w1] @ coef
                assert np.max(np.abs(Z[:, n0:x1] - ref)) <= 1e-12 * max(1.0, np.max(np.abs(ref)))
                for np_, odd in itertools.product((1, 16, 64), (0, 1)):
                    p0 = x1 + ((x1 + odd) & 1)
                    _fill(hip, mv, V0); _fill(hip, mref, V0)
                    hip.ops.axpby(1.0, mz, 0.0, mref, (n0, n0), (x1, x1))
                    hip.ops.axpby(1.0, ms, 0.0, mref, (0, p0), (np_, p0 + np_))
                    assert _ritz_in_place(mv, n0, x1, w1, coef, ms, p0, np_) == 1, (tune, k, m, n0, np_, p0)
                    got, exp = hip.mv_to_numpy(mv, rows, 0, W), hip.mv_to_numpy(mref, rows, 0, W)
                    assert (p0 & 1) == odd and np.array_equal(exp[:, p0:p0 + np_], S0[:, :np_]) and np.array_equal(exp[:, n0:x1], Z[:, n0:x1])
                    untouched = np.ones(W, dtype=bool); untouched[n0:x1] = False; untouched[p0:p0 + np_] = False
                    assert np.array_equal(exp[:, untouched], V0[:, untouched])
                    assert np.array_equal(got, exp), (tune, k, m, n0, np_, p0)
                    ncase += 1
                # no staged columns: the in-place panel alone
                _fill(hip, mv, V0)
                assert _ritz_in_place(mv, n0, x1, w1, coef, None, 0, 0) == 1
                exp = V0.copy(); exp[:, n0:x1] = Z[:, n0:x1]
                assert np.array_equal(hip.mv_to_numpy(mv, rows, 0, W), exp), (tune, k, m, n0)
        assert ncase == (120 if rows == 1025 else 60)
        hip.g.gcge_hip_lincomb_tune(0)
        _fill(hip, mv, V0)
        coef = np.asfortranarray(uniform(64, (200, 129)) - 0.5)
        assert _ritz_in_place(mv, 2, 131, 202, coef, ms, 132, 16) == 0               # 129 output columns
        assert _ritz_in_place(mv, 2, 66, 202, coef, ms, 60, 16) == 0                 # the copy's target over the panel
        assert _ritz_in_place(mv, 2, 66, 202, coef, mv, 70, 16) == 0                 # V as its own staging block
        assert np.array_equal(hip.mv_to_numpy(mv, rows, 0, W), V0)
    finally:
        hip.g.gcge_hip_lincomb_tune(0)
        for h in (mv, mz, mref):
            hip.ops.mv_destroy(h, W)
        hip.ops.mv_destroy(ms, 64)
        hip.free_matrix(mA)


# ---------------------------------------------------------------------------------------------- HIP: block moves from V
@pytest.mark.gpu
@pytest.mark.parametrize("rows", [37, 1025, 1500])
def test_block_moves_from_v_equal_the_moves_from_the_eigenvector_block(hip, rows):
    """The runs, W targets and b placements of tests/test_block_moves.py that need no X move (b absent or in a block of its own),
    with V itself as the source (ritz == V, x0 == x1: the Ritz vectors already live in V's first 40 columns): V's W columns and b
    bit for bit what the call with the eigenvector block as source gives, every other column of V as it was.  V as source with an
    X move asked for, or with b inside V, is declined with nothing touched."""
    mA, keep = _tridiag(hip, rows)
    R, V, B = uniform(11, (rows, 40)) - 0.5, uniform(12, (rows, 72)) + 7.0, uniform(13, (rows, 40)) - 9.0
    V2 = V.copy(); V2[:, :40] = R
    mr, mv, mb, mv2, mb2 = (hip.mv_from_numpy(mA, R), hip.mv_from_numpy(mA, V), hip.mv_from_numpy(mA, B), hip.mv_from_numpy(mA, V2),
                            hip.mv_from_numpy(mA, B))
    ncase = 0
    for x0, x1, tag in itertools.product((4, 5), (36, 37), RUNS):
        runs = RUNS[tag](x0)
        total = sum(h - l for l, h in runs)
        scale = list(1.0 + uniform(14 + x0 + x1, (total,)))
        w0 = 40 + (x1 & 1) + (1 if tag == "two_a" else 0)
        for where, b0 in [(None, 0), ("sep", 3), ("sep", 4)]:
            _fill(hip, mr, R); _fill(hip, mv, V); _fill(hip, mb, B); _fill(hip, mv2, V2); _fill(hip, mb2, B)
            assert _moves(hip, mr, mv, x0, x1, runs, w0, mb if where else None, b0, scale) == 1
            assert _moves(hip, mv2, mv2, x1, x1, runs, w0, mb2 if where else None, b0, scale) == 1, (x0, x1, tag, where, b0)
            ref_v, got_v = hip.mv_to_numpy(mv, rows, 0, 72), hip.mv_to_numpy(mv2, rows, 0, 72)
            exp = V2.copy(); exp[:, w0:w0 + total] = ref_v[:, w0:w0 + total]
            assert np.array_equal(got_v, exp), (x0, x1, tag, where, b0)
            assert np.array_equal(hip.mv_to_numpy(mb2, rows, 0, 40), hip.mv_to_numpy(mb, rows, 0, 40)), (x0, x1, tag, where, b0)
            ncase += 1
    assert ncase == 36
    _fill(hip, mv2, V2)
    runs = RUNS["one"](4)
    assert _moves(hip, mv2, mv2, 4, 36, runs, 40, None, 0, [0.0]) == 0               # an X move from V to V
    assert _moves(hip, mv2, mv2, 36, 36, runs, 40, mv2, 50, [1.0] * 9) == 0          # b inside V
    assert _moves(hip, mv2, mv2, 36, 36, runs, 14, None, 0, [0.0]) == 0              # W over the runs
    assert np.array_equal(hip.mv_to_numpy(mv2, rows, 0, 72), V2)
    for h, w in ((mr, 40), (mv, 72), (mb, 40), (mv2, 72), (mb2, 40)):
        hip.ops.mv_destroy(h, w)
    hip.free_matrix(mA)


# ---------------------------------------------------------------------------------------------- HIP: norms from the update
def _panel_norms(y, start, end):
    g = hip_lib()
    out = np.full(end - start, -1.0)
    return g.gcge_hip_panel_norms_sq_mv(y, start, end, out.ctypes.data_as(C.POINTER(C.c_double))), out


@pytest.mark.gpu
@pytest.mark.parametrize("m", [64, 33])
def test_panel_norms_from_the_update_that_wrote_the_panel(hip, monkeypatch, m):
    """W += V C with k = 192, m = 64 and 33, 1025 rows, beta = 1 (the projection's update): the squared column norms the update
    summed from the values it stored are within 1e-13 relative of numpy's sums over the panel it wrote, two runs give the same
    bits, and the panel is bit for bit the one the kernel without the sums writes (GCGE_NO_PANEL_NORMS=1, which collects nothing).
    The sums are served once, for that panel only, and not after another call."""
    rows, k = 1025, 192
    mA, keep = _tridiag(hip, rows)
    Y0 = uniform(71, (rows, 256)) - 0.5
    coef = np.asfortranarray(uniform(72 + m, (k, m)) - 0.5)
    one = np.array([1.0])
    my = hip.mv_from_numpy(mA, Y0)
    runs = []
    for rep in range(2):
        _fill(hip, my, Y0)
        hip.ops.lincomb(my, my, (0, k), (k, k + m), coef, k, one, 0)
        took, sums = _panel_norms(my, k, k + m)
        assert took == 1
        assert _panel_norms(my, k, k + m)[0] == 0                                     # served once: a call came in between
        runs.append((sums, hip.mv_to_numpy(my, rows, 0, 256)))
    ref = np.array([float(np.sum(np.square(runs[0][1][:, k + j].astype(np.longdouble)))) for j in range(m)])
    rel = np.max(np.abs(runs[0][0] - ref) / ref)
    print("m = %d: largest relative deviation of the sums from numpy's %.3e" % (m, rel))
    assert rel <= 1e-13
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    _fill(hip, my, Y0)
    hip.ops.lincomb(my, my, (0, k), (k, k + m), coef, k, one, 0)
    assert _panel_norms(my, k, k + m - 1)[0] == 0                                     # another panel
    monkeypatch.setenv("GCGE_NO_PANEL_NORMS", "1")
    _fill(hip, my, Y0)
    hip.ops.lincomb(my, my, (0, k), (k, k + m), coef, k, one, 0)
    assert _panel_norms(my, k, k + m)[0] == 0
    plain = hip.mv_to_numpy(my, rows, 0, 256)
    monkeypatch.delenv("GCGE_NO_PANEL_NORMS")
    assert np.array_equal(plain, runs[0][1])
    keep_cols = np.ones(256, dtype=bool); keep_cols[k:k + m] = False
    assert np.array_equal(plain[:, keep_cols], Y0[:, keep_cols])
    assert np.max(np.abs(plain[:, k:k + m] - (Y0[:, k:k + m] + Y0[:, :k] @ coef))) <= 1e-12 * k
    hip.ops.mv_destroy(my, 256)
    hip.free_matrix(mA)


# ---------------------------------------------------------------------------------------------- HIP: GCG, the three data flows
@pytest.mark.gpu
@pytest.mark.parametrize("size,nev,block,nevmax", [(16, 12, 8, 24), (20, 20, 16, 40)])
def test_gcg_block_amg_ritz_in_place_equals_the_three_steps(hip, monkeypatch, size, nev, block, nevmax):
    """Lap3D 16^3 with 12 / 8 / 24 (nev / block / nevMax) and 20^3 with 20 / 16 / 40, BlockAMG over 3 levels, Cholesky-QR for X and W,
    host RNG, three runs in one process: the new flow (Ritz vectors in place, P through the work block, no ComputeX; norms from the
    panel updates), GCGE_NO_RITZ_IN_PLACE=1, and both opt-outs (GCGE_NO_PANEL_NORMS=1 as well).  Eigenvalues, the eigenvector block,
    numIter and nevConv are the same bit for bit in all three, and so is the number of "another pass" decisions of the projection.
    The new flow makes one fused launch per Rayleigh-Ritz step and still one sweep of block moves per outer iteration; the opt-out
    makes none."""
    A, _ = make_problem("lap3d", size)
    n = A.nrows
    mA = hip.matrix(A)
    args = ["-nevConv", nev, "-nevMax", nevmax, "-blockSize", block, "-gcge_amg_levels", 3, "-gcge_initX_orth_method", "chol",
            "-gcge_compW_orth_method", "chol"]
    out = {}
    for tag in ("in_place", "three_steps", "both_off"):
        if tag != "in_place":
            monkeypatch.setenv("GCGE_NO_RITZ_IN_PLACE", "1")
        if tag == "both_off":
            monkeypatch.setenv("GCGE_NO_PANEL_NORMS", "1")
        hip.set_random_mode(0)
        C.CDLL(None).srand(0)
        r0, k0, h0 = _ritz_stats(), _kahan_stats(), _host_stats()
        ev, res, evec = run_gcg(hip.ops_handle, mA, None, args, keep_evec=True)
        out[tag] = (ev.copy(), hip.mv_to_numpy(evec, n, 0, nevmax), res.numIter, res.nevConv, _ritz_stats() - r0,
                    tuple(v - w for v, w in zip(_kahan_stats(), k0)), _host_stats()[2] - h0[2])
        hip.ops.mv_destroy(evec, nevmax)
    monkeypatch.delenv("GCGE_NO_RITZ_IN_PLACE")
    monkeypatch.delenv("GCGE_NO_PANEL_NORMS")
    a = out["in_place"]
    for t in out:
        print(t, "numIter", out[t][2], "nevConv", out[t][3], "fused launches", out[t][4], "Kahan (tests, another pass, norms from the update)",
              out[t][5], "one-sweep moves", out[t][6])
    assert a[3] >= nev
    for other in (out["three_steps"], out["both_off"]):
        assert a[3] == other[3] and a[2] == other[2]
        assert np.array_equal(a[0], other[0])
        assert np.array_equal(a[1][:, :a[3]], other[1][:, :a[3]])
        assert np.array_equal(a[1], other[1])
        assert a[5][0] == other[5][0] and a[5][1] == other[5][1]
    assert a[4] == a[2] + 1 and out["three_steps"][4] == 0 and out["both_off"][4] == 0      # one per Rayleigh-Ritz step / none
    assert a[6] == a[2] and out["three_steps"][6] == a[2]                                     # one sweep of moves per outer iteration
    assert out["both_off"][5][2] == 0
    hip.free_matrix(mA)
