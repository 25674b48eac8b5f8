"""Block streams of the BlockAMG V-cycle that nothing reads: the last iteration of a smoothing call runs no second CG pass (or one
over the 16 columns that hold column 0 in the cycle's last call) when BlockAMG says whose residual it reads
(GCGE_LINSOL_ARGS.final_residual_cols, include/gcge_ops.h).  x, the reported residual and every iteration count must stay bit for
bit what the whole last pass gives (GCGE_AMG_FULL_LAST_PASS=1)."""
import ctypes as C

import numpy as np
import pytest

from gcge_amd.lib import hip_lib, host_lib, make_problem
from gcge_amd.ops_struct import LINSOL_ARGS
from helpers import block_amg_solve, uniform
from test_multigrid import slot_multigrid


def _trimmed():
    g = hip_lib()
    return g.gcge_hip_bpcg_trimmed_iters()


def _column_stats():
    g = hip_lib()
    a, b = C.c_long(), C.c_long()
    g.gcge_hip_bpcg_column_stats(C.byref(a), C.byref(b))
    return a.value, b.value, g.gcge_hip_bpcg_surplus_iters()


def test_linsol_args_mirror_ends_with_final_residual_cols():
    """The ctypes mirror carries the new member last, so a record built by ctypes leaves it 0 (every column's residual)."""
    assert LINSOL_ARGS._fields_[-1][0] == "final_residual_cols"
    assert LINSOL_ARGS().final_residual_cols == 0


@pytest.mark.gpu
@pytest.mark.parametrize("kind,size,m", [("lap3d", 16, 16), ("lap3d", 16, 64), ("lap3d", 21, 66), ("fe3d", 12, 64), ("fe3d", 13, 16),
                                         ("sio2", 14, 64), ("sio2", 14, 66)])
@pytest.mark.parametrize("cycles", [1, 2])
@pytest.mark.parametrize("rates", ["bench", "fixed"])
def test_block_amg_last_pass_trim_is_bit_identical(hip, kind, size, m, cycles, rates, monkeypatch):
    """BlockAMG with the trimmed last passes against the whole last passes: the same x, niter and residual bit for bit (a second
    cycle reads the first one's residual), and the trim did happen where every call runs to its iteration limit."""
    A, _ = make_problem(kind, size)
    n = A.nrows
    mA = hip.matrix(A)
    Ah, Ph, done = slot_multigrid(hip, mA, None, 4)
    L = len(Ah)
    b = uniform(401, (n, m)) - 0.5
    x0 = uniform(402, (n, m)) - 0.5
    max_iter = [cycles, 3, 3] + [4, 4] * (L - 1)
    if rates == "bench":     # the bench's stopping rules (GCGE_AMGCreate): level 0 to 1e-2, the coarse levels to their limit
        rate, tol = [1e-2] + [1e-16] * (L - 1), [1e-14] + [1e-16] * (L - 1)
    else:
        rate, tol = [1e-30] * L, [1e-30] * L
    out = {}
    for tag in ("trim", "full"):
        if tag == "full":
            monkeypatch.setenv("GCGE_AMG_FULL_LAST_PASS", "1")
        t0, s0 = _trimmed(), _column_stats()
        out[tag] = block_amg_solve(hip, Ah, Ph, b, x0, max_iter, rate, tol)
        out[tag + "_trimmed"] = _trimmed() - t0
        out[tag + "_stats"] = tuple(v - w for v, w in zip(_column_stats(), s0))
    monkeypatch.delenv("GCGE_AMG_FULL_LAST_PASS")
    assert np.array_equal(out["trim"][0], out["full"][0])
    assert out["trim"][1] == out["full"][1]
    assert out["trim"][2] == out["full"][2]                  # (float equality: bit for bit)
    assert out["trim_stats"] == out["full_stats"]
    assert out["full_trimmed"] == 0
    if rates == "fixed":
        assert out["trim_trimmed"] > 0
    done()
    hip.free_matrix(mA)


@pytest.mark.gpu
@pytest.mark.parametrize("m", [16, 64])
def test_direct_fused_cg_keeps_its_last_pass(hip, m):
    """A direct call of the fused block CG (nothing published, as the GCG driver and the tests call it) runs its last pass whole;
    publishing final_residual_cols changes neither x, the iteration count, the column statistics nor, for column 0, the residual."""
    A, _ = make_problem("lap3d", 16)
    n = A.nrows
    mA = hip.matrix(A)
    g, h = hip_lib(), host_lib()
    b = uniform(501, (n, m)) - 0.5
    res = {}
    for cols in (0, 1, -1):
        g.gcge_hip_bpcg_setup(hip.ops_handle, 5, 1e-30, 1e-30, b"abs")
        args = LINSOL_ARGS()
        args.final_residual_cols = cols
        if cols != 0:
            h.GCGE_SetLinearSolverArgs(C.byref(args))
        mb = hip.mv_from_numpy(mA, b)
        mx = hip.mv_from_numpy(mA, np.zeros_like(b))
        t0, s0 = _trimmed(), _column_stats()
        hip.ops.multi_linear_solver(mA, mb, mx, (0, 0), (m, m))
        h.GCGE_SetLinearSolverArgs(None)
        it = C.c_int()
        g.gcge_hip_bpcg_stats(None, None, C.byref(it))
        res[cols] = (hip.mv_to_numpy(mx, n, 0, m), it.value, _trimmed() - t0, tuple(v - w for v, w in zip(_column_stats(), s0)),
                     g.gcge_hip_bpcg_last_residual())
        hip.ops.mv_destroy(mb, m)
        hip.ops.mv_destroy(mx, m)
    assert res[0][2] == 0                                    # nothing published: the whole last pass
    assert res[-1][2] == 1 and (res[1][2] == (1 if m > 16 else 0))
    for cols in (1, -1):
        assert np.array_equal(res[cols][0], res[0][0])
        assert res[cols][1] == res[0][1] == 5
        assert res[cols][3] == res[0][3]
    assert res[1][4] == res[0][4]
    hip.free_matrix(mA)

