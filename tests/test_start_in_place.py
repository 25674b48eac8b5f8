"""BlockAMG's W solves started from the Ritz vectors where they lie (GCGE_LINSOL_ARGS.x_src, include/gcge_ops.h): the driver's run
and parity test (GCGE_GcgStartInPlaceRange, csrc/host/gcg.c), the start sweep that reads x from another block and stores the
right-hand sides it forms (kernel MODE 8, csrc/hip/spmm_pattern.hip), the x flush with a read operand of its own (cg_accum_x,
csrc/hip/block_pcg.hip), and GCG + BlockAMG with the new flow against GCGE_NO_START_IN_PLACE=1.  Every value is a copy, one
rounded product, one subtraction or the same chain of fused multiply-adds on the same operands in both flows, so every comparison
is bit for bit."""
import ctypes as C
import itertools

import numpy as np
import pytest

from gcge_amd.lib import hip_lib, host_lib, make_problem, run_gcg
from gcge_amd.ops_struct import LINSOL_ARGS
from helpers import csr_from_scipy, uniform


def _host_stats():
    a, b = C.c_long(), C.c_long()
    host_lib().GCGE_GcgStartInPlaceStats(C.byref(a), C.byref(b))
    return a.value, b.value


def _hip_stats():
    g = hip_lib()
    d = C.c_long()
    return g.gcge_hip_bpcg_start_in_place_stats(C.byref(d)), d.value


# ---------------------------------------------------------------------------------------------- host: runs and parity
def _range(runs, start_w):
    flat = [len(runs)] + [v for r in runs for v in r]
    lo, total = C.c_int(-1), C.c_int(-1)
    took = host_lib().GCGE_GcgStartInPlaceRange((C.c_int * len(flat))(*flat), start_w, C.byref(lo), C.byref(total))
    return (took, lo.value, total.value) if took else (0, None, None)


def test_start_range_takes_one_even_contiguous_range_only():
    """One run, adjacent runs (the unconverged tail plus the padding run) count as one range; a hole, an odd first column, an odd
    length, an odd W origin, an empty list: declined.  Every pair of runs in a small block against the rule itself."""
    assert _range([(4, 12)], 24) == (1, 4, 8)
    assert _range([(4, 10), (10, 12)], 24) == (1, 4, 8)
    assert _range([(4, 9), (9, 10), (10, 16)], 24) == (1, 4, 12)
    assert _range([(4, 8), (10, 14)], 24)[0] == 0
    assert _range([(5, 13)], 24)[0] == 0 and _range([(4, 11)], 24)[0] == 0 and _range([(4, 12)], 25)[0] == 0
    assert _range([], 24)[0] == 0 and _range([(4, 4)], 24)[0] == 0 and _range([(10, 14), (4, 8)], 24)[0] == 0
    for lo, hi, gap, n2, w in itertools.product(range(6), range(1, 9), range(3), range(1, 4), (12, 13)):
        if hi <= lo:
            continue
        length = hi + n2 - lo
        want = gap == 0 and not ((lo | length | w) & 1)
        assert _range([(lo, hi), (hi + gap, hi + gap + n2)], w) == ((1, lo, length) if want else (0, None, None))


def test_linsol_args_mirror_holds_x_src():
    names = [f[0] for f in LINSOL_ARGS._fields_]
    assert names[-3:] == ["x_src", "x_src_col", "final_residual_cols"]
    a = LINSOL_ARGS()
    assert a.x_src is None and a.x_src_col == 0


def test_gcg_on_the_oracle_never_starts_in_place(oracle):
    """The driver over the CPU oracle's table: its record offers no start_in_place, so ComputeW never publishes x_src and both
    counters stay where they were."""
    A, _ = make_problem("lap3d", 16)
    s0 = _host_stats()
    ev, res = run_gcg(oracle.ops_handle, oracle.matrix(A), None, ["-nevConv", 12, "-nevMax", 24, "-blockSize", 8])
    assert res.nevConv >= 12
    assert _host_stats() == s0


# ---------------------------------------------------------------------------------------------- HIP: the start sweep and the flush
def _lap_grid(nx, ny, nz):
    """7-point Laplacian on an nx x ny x nz grid, x fastest."""
    import scipy.sparse as sp
    def t(n):
        return sp.diags([-np.ones(n - 1), 2.0 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1])
    ex, ey, ez = sp.identity(nx), sp.identity(ny), sp.identity(nz)
    return (sp.kron(ez, sp.kron(ey, t(nx))) + sp.kron(ez, sp.kron(t(ny), ex)) + sp.kron(t(nz), sp.kron(ey, ex))).tocsr()


def _fill(hip, mv, arr):
    a = np.asfortranarray(arr)
    hip.g.gcge_hip_mv_from_host(mv, 0, a.shape[1], a.ctypes.data_as(C.POINTER(C.c_double)), a.shape[0])


@pytest.mark.gpu
@pytest.mark.parametrize("m", [16, 64])
@pytest.mark.parametrize("grid", [(16, 16, 16), (24, 16, 40)])
def test_start_sweep_from_x_elsewhere_equals_moves_then_start(hip, grid, m):
    """x at columns lo = 0, 2, 10 of a block V, W at lo + m of the same block, b at column 2 of a block of its own.  Reference:
    the block-move sweep (W = copy of x, b = x diag(s)), the MODE 5 start from those two copies, then a flush of three directions
    into W.  New: ONE start sweep (MODE 8) reading V[:, lo..) and storing r / p0 and b, then the flush reading V[:, lo..) and
    writing W.  r, p0, b, V (W after the flush and every other column) and rho are identical; b's block is untouched outside its
    m columns.  lo = 2 runs with r and p0 the same block (the start that stores p0 alone)."""
    g = hip_lib()
    vp, ci = C.c_void_p, C.c_int
    if grid[0] == grid[1] == grid[2]:
        A, _ = make_problem("lap3d", grid[0])
        keep = None
    else:
        A, keep = csr_from_scipy(_lap_grid(*grid))
    mat = hip.matrix(A)
    n = A.nrows
    if grid == (16, 16, 16):
        assert g.gcge_hip_mat_pattern_chain(mat) == 2          # chain + line exchange: the kernel BlockAMG's level 0 runs at the bench shape
    wv, wb, b0 = 2 * m + 12, m + 6, 2
    V0, B0 = uniform(71, (n, wv)) - 0.5, uniform(72, (n, wb)) + 3.0
    Q = [uniform(73 + q, (n, m)) - 0.5 for q in range(2)]
    s = uniform(76, (m,)) * 0.2 + 0.01
    coef = np.ascontiguousarray(uniform(77, (3 * m,)) - 0.5)
    mv, mb = hip.mv_from_numpy(mat, V0), hip.mv_from_numpy(mat, B0)
    r, p0 = hip.mv_from_numpy(mat, np.zeros((n, m))), hip.mv_from_numpy(mat, np.zeros((n, m)))
    q = [hip.mv_from_numpy(mat, a) for a in Q]
    sc = (C.c_double * m)(*s)

    def collect(rr):
        return (hip.mv_to_numpy(mv, n, 0, wv), hip.mv_to_numpy(mb, n, 0, wb), hip.mv_to_numpy(rr, n, 0, m), hip.mv_to_numpy(p0, n, 0, m))

    for lo in (0, 2, 10):
        w0 = lo + m
        rr = p0 if lo == 2 else r
        ring = (vp * 3)(p0, q[0], q[1])
        out = {}
        for flow in ("moves", "in_place"):
            _fill(hip, mv, V0); _fill(hip, mb, B0); _fill(hip, r, np.zeros((n, m))); _fill(hip, p0, np.zeros((n, m)))
            rho = np.zeros(m)
            if flow == "moves":
                runs = (ci * 3)(1, lo, lo + m)
                assert g.gcge_hip_block_moves_mv(mv, mv, w0, w0, runs, w0, mb, b0, sc) == 1
                assert g.gcge_hip_cg_start_mv(mat, mv, w0, mb, b0, rr, p0, 0, m, rho.ctypes.data) == 0
                assert g.gcge_hip_cg_accum_x_mv(mv, w0, mv, w0, m, ring, 3, coef.ctypes.data) == 0
            else:
                assert g.gcge_hip_cg_start_scaled_b_mv(mat, mv, lo, s.ctypes.data, rr, p0, 0, m, mb, b0, rho.ctypes.data) == 0
                started = collect(rr)
                assert np.array_equal(started[0], V0)                                   # the sweep writes nothing into V
                assert g.gcge_hip_cg_accum_x_mv(mv, lo, mv, w0, m, ring, 3, coef.ctypes.data) == 0
            out[flow] = collect(rr) + (rho,)
        a, e = out["in_place"], out["moves"]
        for name, x, y in zip(("V", "b", "r", "p0", "rho"), a, e):
            assert np.array_equal(x, y), (name, lo)
        assert np.array_equal(a[1][:, b0:b0 + m], V0[:, lo:lo + m] * s)                 # b: each product rounded once
        outside_b = [j for j in range(wb) if not b0 <= j < b0 + m]
        outside_w = [j for j in range(wv) if not w0 <= j < w0 + m]
        assert np.array_equal(a[1][:, outside_b], B0[:, outside_b]) and np.array_equal(a[0][:, outside_w], V0[:, outside_w])
        assert not np.array_equal(a[0][:, w0:w0 + m], V0[:, w0:w0 + m]) and np.all(a[4] > 0.0)
    # a flush with nothing pending is a plain copy; operands the sweep does not take are declined with nothing touched
    _fill(hip, mv, V0); _fill(hip, mb, B0)
    assert g.gcge_hip_cg_accum_x_mv(mv, 2, mv, 2 + m, m, None, 0, None) == 0
    got = hip.mv_to_numpy(mv, n, 0, wv)
    V1 = V0.copy(); V1[:, 2 + m:2 + 2 * m] = V0[:, 2:2 + m]
    assert np.array_equal(got, V1)
    _fill(hip, mv, V0)
    rho = np.zeros(m)
    assert g.gcge_hip_cg_start_scaled_b_mv(mat, mv, 3, s.ctypes.data, r, p0, 0, m, mb, b0, rho.ctypes.data) == -1      # odd source column
    assert g.gcge_hip_cg_start_scaled_b_mv(mat, mv, 2, s.ctypes.data, r, p0, 0, m, mb, 3, rho.ctypes.data) == -1       # odd b column
    assert g.gcge_hip_cg_start_scaled_b_mv(mat, mv, 2, s.ctypes.data, r, p0, 0, m, mv, 2 + m, rho.ctypes.data) == -1   # b inside x's block
    assert np.array_equal(hip.mv_to_numpy(mv, n, 0, wv), V0) and np.array_equal(hip.mv_to_numpy(mb, n, 0, wb), B0)
    for h, w in [(mv, wv), (mb, wb), (r, m), (p0, m), (q[0], m), (q[1], m)]:
        hip.ops.mv_destroy(h, w)
    hip.free_matrix(mat)


# ---------------------------------------------------------------------------------------------- HIP: the fused CG alone
@pytest.mark.gpu
@pytest.mark.parametrize("size", [16, 20])
def test_fused_cg_takes_the_initial_guess_from_elsewhere(hip, size):
    """HIP_BlockPCG with x_src / rhs_scale published (the guess in columns 4.. of a block X, the result to columns 2.. of another)
    against the same solve handed a copy of the guess and the formed b: x, b and the iteration count are identical, X is
    untouched.  16^3 starts in one sweep (also with no iteration at all: x is the plain copy), 20^3 — no chain + line-exchange
    form — makes the copy and b first.  Seven iterations at most, then (the direction ring exists by now) none."""
    for iters in (7, 0):
        _solve_from_elsewhere(hip, size, iters)


def _solve_from_elsewhere(hip, size, iters):
    A, _ = make_problem("lap3d", size)
    mat = hip.matrix(A)
    n, m = A.nrows, 16
    g, h = hip.g, hip.h
    X0, W0 = uniform(81, (n, m + 8)) - 0.5, uniform(82, (n, m + 4)) + 2.0
    s = uniform(83, (m,)) * 0.2 + 0.01
    sc = (C.c_double * m)(*s)
    out = {}
    g.gcge_hip_bpcg_setup(hip.ops_handle, iters, 1e-2, 1e-14, b"abs")
    try:
        for flow in ("elsewhere", "copied"):
            Wc = W0.copy()
            if flow == "copied":
                Wc[:, 2:2 + m] = X0[:, 4:4 + m]
            xs, w = hip.mv_from_numpy(mat, X0), hip.mv_from_numpy(mat, Wc)
            b = hip.mv_from_numpy(mat, np.full((n, m), 7.0) if flow == "elsewhere" else X0[:, 4:4 + m] * s)
            t0 = _hip_stats()
            if flow == "elsewhere":
                h.GCGE_SetLinearSolverArgs(C.byref(LINSOL_ARGS(rhs_scale=sc, x_src=xs, x_src_col=4)))
            try:
                hip.ops.multi_linear_solver(mat, b, w, (0, 2), (m, 2 + m))
            finally:
                h.GCGE_SetLinearSolverArgs(None)
            it = C.c_int(); g.gcge_hip_bpcg_stats(None, None, C.byref(it))
            out[flow] = (it.value, hip.mv_to_numpy(w, n, 0, m + 4), hip.mv_to_numpy(b, n, 0, m), hip.mv_to_numpy(xs, n, 0, m + 8),
                         tuple(v - u for v, u in zip(_hip_stats(), t0)))
            hip.ops.mv_destroy(xs, m + 8); hip.ops.mv_destroy(w, m + 4); hip.ops.mv_destroy(b, m)
    finally:
        g.gcge_hip_bpcg_setup(hip.ops_handle, 30, 1e-2, 1e-14, b"abs")
    a, e = out["elsewhere"], out["copied"]
    print(size, iters, "iterations", a[0], e[0], "(in place, materialised)", a[4], e[4])
    assert a[0] == e[0] <= iters
    assert np.array_equal(a[1], e[1]) and np.array_equal(a[2], X0[:, 4:4 + m] * s) and np.array_equal(a[3], X0)
    assert np.array_equal(a[1][:, :2], W0[:, :2]) and np.array_equal(a[1][:, 2 + m:], W0[:, 2 + m:])
    assert e[4] == (0, 0)
    assert a[4] == ((1, 0) if size == 16 else (0, 1))
    hip.free_matrix(mat)


# ---------------------------------------------------------------------------------------------- HIP: GCG + BlockAMG, both flows
@pytest.mark.gpu
@pytest.mark.parametrize("size,nev,block,nevmax", [(16, 12, 8, 24), (20, 20, 16, 40)])
def test_gcg_block_amg_start_in_place_equals_the_moves(hip, monkeypatch, size, nev, block, nevmax):
    """Lap3D 16^3 with 12 / 8 / 24 (nev / block / nevMax) and 20^3 with 20 / 16 / 40, BlockAMG over 3 levels, Cholesky-QR for X and
    W, host RNG, two runs in one process: the new flow and GCGE_NO_START_IN_PLACE=1.  Eigenvalues, the eigenvector block, numIter
    and nevConv are identical bit for bit.  The driver leaves the moves to the solver in some outer iterations and declines others
    (an odd first unconverged column, a hole between the runs); at 16^3 the solver starts those in one sweep, at 20^3 (no chain +
    line-exchange form on level 0) it makes the copy and b itself in every one of them."""
    A, _ = make_problem("lap3d", size)
    n = A.nrows
    mA = hip.matrix(A)
    args = ["-nevConv", nev, "-nevMax", nevmax, "-blockSize", block, "-gcge_amg_levels", 3, "-gcge_initX_orth_method", "chol",
            "-gcge_compW_orth_method", "chol"]
    out = {}
    for tag in ("in_place", "moves"):
        if tag == "moves":
            monkeypatch.setenv("GCGE_NO_START_IN_PLACE", "1")
        hip.set_random_mode(0)
        C.CDLL(None).srand(0)
        h0, d0 = _host_stats(), _hip_stats()
        ev, res, evec = run_gcg(hip.ops_handle, mA, None, args, keep_evec=True)
        out[tag] = (ev.copy(), hip.mv_to_numpy(evec, n, 0, nevmax), res.numIter, res.nevConv,
                    tuple(v - w for v, w in zip(_host_stats(), h0)), tuple(v - w for v, w in zip(_hip_stats(), d0)))
        hip.ops.mv_destroy(evec, nevmax)
    monkeypatch.delenv("GCGE_NO_START_IN_PLACE")
    a, b = out["in_place"], out["moves"]
    for t in out:
        print(t, "numIter", out[t][2], "nevConv", out[t][3], "driver (in place, declined)", out[t][4], "solver (one sweep, materialised)", out[t][5])
    assert a[3] >= nev and a[3] == b[3] and a[2] == b[2]
    assert np.array_equal(a[0], b[0])
    assert np.array_equal(a[1], b[1])
    assert a[4][0] > 0 and a[4][1] > 0 and a[4][0] + a[4][1] == a[2]
    assert b[4] == (0, 0) and b[5] == (0, 0)
    assert a[5] == ((a[4][0], 0) if size == 16 else (0, a[4][0]))
    hip.free_matrix(mA)
