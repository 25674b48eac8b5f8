"""The Gram of a block with itself (csrc/hip/gram_mfma.hip, gram_tile_kernel<MS, 1, true>): gcge_hip_gram with d_q == d_p,
ldq == ldp and k == m <= 64 loads each row once and accumulates only the 16 x 16 fragments on and above the diagonal; the ones below
are mirrored in LDS.  A mirrored entry is the same products summed over the same rows in the same order as the entry the general
kernel accumulates, and chunking, the combine of the four waves and the reduction over the chunks are unchanged, so the symmetric
path and GCGE_GRAM_NO_SYM=1 are compared bit for bit — the kernel alone over row counts, widths and placements, and a GCG + BlockAMG
solve with Cholesky-QR.  Against numpy the tolerance is the one of tests/test_hip_parity.py::test_gram_and_dots_vs_oracle."""
import ctypes as C

import numpy as np
import pytest

from gcge_amd.lib import hip_lib, make_problem, run_gcg
from helpers import uniform
from slot_cases import _close

NMAX, LD = 4163, 192          # 4163 rows: 66 row chunks of 64 and a tail of 3 rows


@pytest.fixture(scope="module")
def blocks():
    """Host data, made once and never written: the operand block, and the operands of the k = 256, m = 64 Gram that dirties the
    shared partial workspace (values far from anything a Gram of the operand block holds)."""
    return {"B": np.ascontiguousarray(uniform(301, (NMAX, LD)) - 0.5),
            "DQ": np.ascontiguousarray(uniform(302, (NMAX, 256)) + 50.0),
            "DP": np.ascontiguousarray(uniform(303, (NMAX, 64)) + 70.0)}


def _gram(g, torch, x, ld, c0, k, y, ldy, c1, m, n):
    """gcge_hip_gram on columns [c0, c0 + k) of x and [c1, c1 + m) of y (device blocks, row-major); the k x m result as numpy.  The
    result buffer starts as NaN, so an entry the reduction does not write cannot pass for a value."""
    G = torch.full((k * m,), float("nan"), dtype=torch.float64, device="cuda")
    assert g.gcge_hip_gram(n, x.data_ptr() + 8 * c0, ld, k, y.data_ptr() + 8 * c1, ldy, m, G.data_ptr(), None) == 0
    torch.cuda.synchronize()
    return G.cpu().numpy().reshape(k, m)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 5, 64, 100, 4163])
def test_symmetric_gram_equals_the_general_kernel(hip, monkeypatch, blocks, n):
    """Row counts 1, 5, 64, 100, 4163 x widths k = m = 64, 50, 16, 8 x placements (columns [c0, c0 + k) of a block of 192 columns,
    c0 = 0, 2, 64, and a whole block of k columns).  In front of every call a k = 256, m = 64 Gram of other data runs, so the
    workspace the tile kernel fills holds foreign values wherever it does not write.  Both paths: identical k x k arrays, the lower
    triangle included, and within 1e-12 of numpy; the counter moves by one on the symmetric path only."""
    import torch
    g = hip.g
    B = blocks["B"]
    dB = torch.from_numpy(B[:n]).cuda()
    dQ, dP = torch.from_numpy(blocks["DQ"]).cuda(), torch.from_numpy(blocks["DP"]).cuda()

    def dirty():
        _gram(g, torch, dQ, 256, 0, 256, dP, 64, 0, 64, NMAX)

    for k in (64, 50, 16, 8):
        whole = torch.from_numpy(np.ascontiguousarray(B[:n, :k])).cuda()
        for x, ld, c0 in [(dB, LD, 0), (dB, LD, 2), (dB, LD, 64), (whole, k, 0)]:
            X = B[:n, c0:c0 + k]
            ref = X.T @ X
            dirty()
            c_before = g.gcge_hip_gram_sym_launches()
            sym = _gram(g, torch, x, ld, c0, k, x, ld, c0, k, n)
            assert g.gcge_hip_gram_sym_launches() == c_before + 1, (n, k, ld, c0)
            dirty()
            monkeypatch.setenv("GCGE_GRAM_NO_SYM", "1")
            gen = _gram(g, torch, x, ld, c0, k, x, ld, c0, k, n)
            monkeypatch.delenv("GCGE_GRAM_NO_SYM")
            assert g.gcge_hip_gram_sym_launches() == c_before + 1, (n, k, ld, c0)
            assert np.array_equal(sym, gen), (n, k, ld, c0, float(np.max(np.abs(sym - gen))))
            _close(sym, ref, tol=1e-12, what="symmetric gram n=%d k=%d ld=%d c0=%d" % (n, k, ld, c0))
            _close(gen, ref, tol=1e-12, what="general gram n=%d k=%d ld=%d c0=%d" % (n, k, ld, c0))


@pytest.mark.gpu
def test_other_operands_keep_the_general_kernel(hip, blocks):
    """The same block with different column origins, k != m on one origin, and k = m > 64 take the general kernel: the counter
    stands still and the result is numpy's."""
    import torch
    g = hip.g
    n = 100
    B = blocks["B"]
    dB = torch.from_numpy(B[:n]).cuda()
    c_before = g.gcge_hip_gram_sym_launches()
    for c0, k, c1, m in [(0, 64, 64, 64), (2, 16, 4, 16), (0, 64, 0, 32), (0, 16, 0, 64), (8, 8, 8, 50), (0, 65, 0, 65), (0, 128, 0, 128)]:
        got = _gram(g, torch, dB, LD, c0, k, dB, LD, c1, m, n)
        _close(got, B[:n, c0:c0 + k].T @ B[:n, c1:c1 + m], tol=1e-12, what="gram %d+%d x %d+%d" % (c0, k, c1, m))
    assert g.gcge_hip_gram_sym_launches() == c_before


@pytest.mark.gpu
def test_gcg_block_amg_symmetric_gram_equals_the_general_kernel(hip, monkeypatch):
    """Lap3D 16^3 with 12 / 8 / 24 (nev / block / nevMax), BlockAMG over 3 levels, Cholesky-QR for X and W, host RNG, two runs in one
    process: the symmetric Gram and GCGE_GRAM_NO_SYM=1.  Eigenvalues, the eigenvector block, numIter and nevConv are identical bit
    for bit; the symmetric kernel is launched on the new path and never with the switch."""
    g = hip_lib()
    A, _ = make_problem("lap3d", 16)
    n = A.nrows
    mA = hip.matrix(A)
    nev, block, nevmax = 12, 8, 24
    args = ["-nevConv", nev, "-nevMax", nevmax, "-blockSize", block, "-gcge_amg_levels", 3, "-gcge_initX_orth_method", "chol",
            "-gcge_compW_orth_method", "chol"]
    out = {}
    for tag in ("sym", "general"):
        if tag == "general":
            monkeypatch.setenv("GCGE_GRAM_NO_SYM", "1")
        hip.set_random_mode(0)
        C.CDLL(None).srand(0)
        c0 = g.gcge_hip_gram_sym_launches()
        ev, res, evec = run_gcg(hip.ops_handle, mA, None, args, keep_evec=True)
        out[tag] = (ev.copy(), hip.mv_to_numpy(evec, n, 0, nevmax), res.numIter, res.nevConv, g.gcge_hip_gram_sym_launches() - c0)
        hip.ops.mv_destroy(evec, nevmax)
    monkeypatch.delenv("GCGE_GRAM_NO_SYM")
    a, b = out["sym"], out["general"]
    for t in out:
        print(t, "numIter", out[t][2], "nevConv", out[t][3], "symmetric launches", out[t][4])
    assert a[3] >= nev and a[3] == b[3] and a[2] == b[2]
    assert np.array_equal(a[0], b[0])
    assert np.array_equal(a[1], b[1])
    assert a[4] > 0 and b[4] == 0
    hip.free_matrix(mA)
