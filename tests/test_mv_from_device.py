"""Blocks of vectors in from device memory (gcge_hip_mv_from_device, csrc/hip/mat_device.hip "blocks in"; HipBackend.mv_from_torch).

A copy has no rounding, so everything here is compared as bits: the written columns against the source, every other column of the
block (the padding columns up to ld cannot be read back through the public face; the columns beside the range can) against what was
there.  The sizes sit on the boundaries of the row tiling (one row, one wave less / exactly / one more, a few blocks), the column
ranges start on even and odd columns and the sources take each of the three kernel forms: rows contiguous with the two first
columns of equal parity (16-byte lanes with 8-byte edge lanes) and of different parity (8-byte lanes), columns contiguous (the LDS
transpose), and general strides (the element kernel).  A re-ordered handle adds the permutation, checked through a product as
well: two mutually inverse wrong permutations would pass a round trip."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from helpers import WARM_MODES, bits, csr_from_scipy, draw, load_golden, sine_start_block
from gcge_amd.lib import make_problem, run_gcg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM = load_golden("warm.json")


# ---- CPU: the public face -----------------------------------------------------------------------------------------------------------
def test_prototype_is_public_and_eigsh_imports_without_torch():
    text = open(os.path.join(ROOT, "include", "gcge_hip.h")).read()
    assert re.search(r"void gcge_hip_mv_from_device \(void \*\*mv, int c0, int c1, const double \*d_in, long row_stride, long col_stride\);", text)
    code = ("import sys; import gcge_amd; from gcge_amd import eigsh, EigshResult, NoConvergence; assert callable(eigsh); "
            "assert issubclass(NoConvergence, RuntimeError); assert 'torch' not in sys.modules; print('ok')")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr


# ---- sources ------------------------------------------------------------------------------------------------------------------------
class Foreign:
    """an object that has __cuda_array_interface__ and nothing else (it keeps its tensor alive)"""

    def __init__(self, t):
        self.t = t
        self.__cuda_array_interface__ = t.__cuda_array_interface__


def sources(torch, X, Xint):
    """(name, object to hand over, the (n, m) array it holds) for every way in; X real data, Xint small integers (exact in float32)"""
    n, m = X.shape
    x = torch.from_numpy(np.ascontiguousarray(X)).cuda()
    W = m + 4 + (m % 2)                                           # an even row stride: the parity of the first column decides the lanes
    wide = torch.zeros((n, W), dtype=torch.float64, device="cuda")
    out = [("contiguous", x, X)]
    for first in (2, 3):
        wide[:, first:first + m] = x
        out.append(("columns %d.. of a wider tensor" % first, wide.clone()[:, first:first + m], X))
    out.append(("columns contiguous", x.t().contiguous().t(), X))
    two = torch.zeros((2 * n, m), dtype=torch.float64, device="cuda")
    two[::2] = x
    out.append(("every second row", two[::2], X))
    out.append(("float32", torch.from_numpy(np.ascontiguousarray(Xint.astype(np.float32))).cuda(), Xint))
    out.append(("foreign", Foreign(x), X))
    return out


def diag_matrix(hip, n):
    import scipy.sparse as sp
    A, keep = csr_from_scipy(sp.diags(np.arange(1.0, n + 1.0)).tocsr())
    return hip.matrix(A), keep


# ---- exact round trip ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_written_columns_equal_the_source_and_the_rest_is_untouched(hip, n):
    import torch
    mat, keep = diag_matrix(hip, n)
    try:
        for ncols in (9, 64):
            base = draw(100 + ncols, (n, ncols), True)
            for c0, c1 in ((0, ncols), (2, 9), (3, 4), (1, 1)):
                m = c1 - c0
                X, Xint = draw(7 * n + c0, (n, m), True), draw(5 * n + c1, (n, m), False)
                for name, src, want in sources(torch, X, Xint):
                    mv = hip.mv_from_numpy(mat, base)
                    try:
                        assert hip.mv_from_torch(mat, src, mv=mv, c0=c0) is mv
                        got = hip.mv_to_numpy(mv, n, 0, ncols)
                    finally:
                        hip.ops.mv_destroy(mv, ncols)
                    ref = base.copy()
                    ref[:, c0:c1] = want
                    same = bits(np.ascontiguousarray(got)) == bits(np.ascontiguousarray(ref))
                    assert same.all(), (name, ncols, (c0, c1), np.argwhere(~same)[:4].tolist())
        # a new block: created with the tensor's columns
        X = draw(9 * n, (n, 9), True)
        mv = hip.mv_from_torch(mat, torch.from_numpy(X).cuda())
        try:
            assert hip.g.gcge_hip_mv_ncols(mv) == 9
            got = hip.mv_to_numpy(mv, n, 0, 9)
        finally:
            hip.ops.mv_destroy(mv, 9)
        assert np.array_equal(bits(np.ascontiguousarray(got)), bits(X))
    finally:
        hip.free_matrix(mat)


# ---- a re-ordered handle ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_block_into_a_reordered_handle(hip):
    import torch
    from test_mg_graph import geometric_graph
    g = hip.g
    S = geometric_graph(3000)
    n = S.shape[0]
    A, keep = csr_from_scipy(S)
    g.gcge_hip_spmm_reorder_mode(1)
    H = hip.matrix(A)
    try:
        order = g.gcge_hip_mat_row_order(H).decode()
        print("row order:", order)
        assert order != "as given"
        X = draw(3, (n, 9), True)
        x = torch.from_numpy(X).cuda()
        xn, yn = hip.mv_from_numpy(H, X), hip.mv_from_numpy(H, np.zeros((n, 9)))
        hip.ops.spmm(H, xn, yn, (0, 0), (9, 9))
        Yn = hip.mv_to_numpy(yn, n, 0, 9)
        for name, src in (("rows contiguous", x), ("columns contiguous", x.t().contiguous().t())):
            xt, yt = hip.mv_from_torch(H, src), hip.mv_from_numpy(H, np.zeros((n, 9)))
            try:
                assert np.array_equal(bits(np.ascontiguousarray(hip.mv_to_numpy(xt, n, 0, 9))), bits(X)), name
                assert np.array_equal(bits(np.ascontiguousarray(hip.mv_to_torch(xt, 0, 9).cpu().numpy())), bits(X)), name
                hip.ops.spmm(H, xt, yt, (0, 0), (9, 9))
                Yt = hip.mv_to_numpy(yt, n, 0, 9)
                assert np.array_equal(bits(np.ascontiguousarray(Yt)), bits(np.ascontiguousarray(Yn))), name
            finally:
                hip.ops.mv_destroy(xt, 9)
                hip.ops.mv_destroy(yt, 9)
        hip.ops.mv_destroy(xn, 9)
        hip.ops.mv_destroy(yn, 9)
    finally:
        g.gcge_hip_spmm_reorder_mode(0)
        hip.free_matrix(H)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
class OwnRange:
    """a (rows, cols) float64 view of device memory at ptr with a row stride of ld elements"""

    def __init__(self, ptr, rows, cols, ld):
        self.__cuda_array_interface__ = {"shape": (rows, cols), "typestr": "<f8", "data": (ptr, False), "version": 2, "strides": (8 * ld, 8)}


@pytest.mark.gpu
def test_refusals_raise_and_the_process_stays_usable(hip):
    import torch
    n = 65
    mat, keep = diag_matrix(hip, n)
    base = draw(1, (n, 9), True)
    X = draw(2, (n, 4), True)
    x = torch.from_numpy(X).cuda()
    mv = hip.mv_from_numpy(mat, base)

    def accepted():
        hip.mv_from_torch(mat, x, mv=mv, c0=5)
        ref = base.copy()
        ref[:, 5:9] = X
        assert np.array_equal(bits(np.ascontiguousarray(hip.mv_to_numpy(mv, n, 0, 9))), bits(ref))

    try:
        with pytest.raises(TypeError):
            hip.mv_from_torch(mat, torch.from_numpy(X), mv=mv, c0=5)                   # a host tensor
        accepted()
        with pytest.raises(ValueError):
            hip.mv_from_torch(mat, x[:n - 1], mv=mv, c0=5)                             # a wrong row count, into a block
        with pytest.raises(ValueError):
            hip.mv_from_torch(mat, x[:n - 1])                                          # ... and for a new one
        accepted()
        with pytest.raises(ValueError):
            hip.mv_from_torch(mat, x, mv=mv, c0=6)                                     # columns [6, 10) of 9
        with pytest.raises(ValueError):
            hip.mv_from_torch(mat, x, mv=mv, c0=-1)
        accepted()
        ld = C.c_long()
        ptr = hip.g.gcge_hip_mv_device_ptr(mv, C.byref(ld))
        with pytest.raises(ValueError):
            hip.mv_from_torch(mat, OwnRange(ptr, n, 4, ld.value), mv=mv, c0=5)         # the block's own columns [0, 4)
        with pytest.raises(ValueError):
            hip.mv_from_torch(mat, OwnRange(ptr + 8 * ld.value * (n - 1), n, 4, ld.value), mv=mv, c0=5)   # from its last row on
        accepted()
    finally:
        hip.ops.mv_destroy(mv, 9)
        hip.free_matrix(mat)


# ---- warm start ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("key", sorted(WARM))
def test_warm_start_fed_from_torch_equals_the_host_fed_run(hip, key):
    import torch
    from test_warm_start import _check
    c = WARM[key]
    A, B = make_problem(c["kind"], c["size"])
    mA = hip.matrix(A)
    mB = hip.matrix(B) if B is not None else None
    nev_max = 2 * c["nev"]
    X0 = np.zeros((A.nrows, nev_max))
    X0[:, :c["nevGiven"]] = sine_start_block(c["size"], WARM_MODES, c["eps"], c["seed"])
    got = {}
    try:
        for way in ("numpy", "torch"):
            hip.set_random_mode(0, 0)
            C.CDLL(None).srand(0)
            evec = hip.mv_from_numpy(mA, X0) if way == "numpy" else hip.mv_from_torch(mA, torch.from_numpy(X0).cuda())
            ev, res = run_gcg(hip.ops_handle, mA, mB, ["-nevConv", c["nev"]], given=(evec, c["nevGiven"]))
            V = hip.mv_to_numpy(evec, A.nrows, 0, res.nevConv)
            hip.ops.mv_destroy(evec, nev_max)
            got[way] = (ev.copy(), res, V)
    finally:
        hip.free_matrix(mA)
        if mB is not None:
            hip.free_matrix(mB)
    assert np.array_equal(bits(got["torch"][0]), bits(got["numpy"][0]))
    assert got["torch"][1].numIter == got["numpy"][1].numIter
    _check(c, A, B, got["torch"][0], got["torch"][1], got["torch"][2], 2)
