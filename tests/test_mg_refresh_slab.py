"""A live multigrid hierarchy of ROW SLABS refreshed in place (gcge_hip_multigrid_refresh on the levels multigrid_create_slab built;
GCGE_AMGRefresh agreeing on the outcome over the communicator).  tests/test_mg_refresh.py covers whole matrices and stays as it is.

CPU: gcge_mg_slab_colagg (csrc/host/multigrid.c) — where every local column of a slab level lands among the local columns of the next
one — against what helpers.mg_hierarchy_slab's prolongations, the shared partition and the coarse slab's halo list imply, for every
rank, level and local column: the Laplacian on 8 x 8 x 16 in two slabs, on 8 x 8 x 24 in three, and on 8 x 8 x 16 cut on planes
[0, 7, 16] (an odd cut: the cells next to it are the ranks' own).

GPU (tests/slab_refresh_worker.py, 2 and 3 ranks sharing the one GPU over gloo): see its docstring."""
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from gcge_amd.lib import CSR, host_lib
from helpers import mg_hierarchy_slab

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ip_ = C.POINTER(C.c_int)

CUTS = [pytest.param((8, 8, 16), [0, 8, 16], id="8x8x16-two-slabs"), pytest.param((8, 8, 24), [0, 8, 16, 24], id="8x8x24-three-slabs"),
        pytest.param((8, 8, 16), [0, 7, 16], id="8x8x16-odd-cut")]


def ghosts_of(S, lo, hi):
    """ascending global columns of the slab's rows outside [lo, hi)"""
    cols = np.unique(S.tocsr().indices)
    return np.ascontiguousarray(cols[(cols < lo) | (cols >= hi)], dtype=np.int32)


@pytest.mark.parametrize("dims,planes", CUTS)
def test_colagg_names_the_coarse_local_column_of_every_local_column(dims, planes):
    h = host_lib()
    plane = dims[0] * dims[1]
    part = [p * plane for p in planes]
    world = len(part) - 1
    hier = []
    for r in range(world):
        A = CSR()
        assert h.gcge_problem_lap3d_box(dims[0], dims[1], dims[2], C.c_int64(part[r]), C.c_int64(part[r + 1]), C.byref(A)) == 0
        hier.append(mg_hierarchy_slab(A, dims, part, r, 4, scale=0.5))
    L = len(hier[0]["A"])
    assert L >= 3 and all(len(k["A"]) == L and k["part"] == hier[0]["part"] for k in hier)
    checked = 0
    for l in range(L - 1):
        pf, pc = hier[0]["part"][l], hier[0]["part"][l + 1]
        # global fine row -> global coarse row: every owner's prolongation, shifted by the owner's place in the two partitions
        to_coarse = np.concatenate([pc[q] + np.asarray(hier[q]["P"][l].tocsr().indices, dtype=np.int64) for q in range(world)])
        assert to_coarse.size == pf[-1]
        for r in range(world):
            nf, nc = pf[r + 1] - pf[r], pc[r + 1] - pc[r]
            gf = ghosts_of(hier[r]["A"][l], pf[r], pf[r + 1])
            gc = ghosts_of(hier[r]["A"][l + 1], pc[r], pc[r + 1])
            colagg = np.full(nf + gf.size, -7, dtype=np.int32)
            nlo = C.c_int(-1)
            d = (C.c_int * 3)(*hier[r]["dims"][l])
            parr = (C.c_long * (world + 1))(*pf)
            rc = h.gcge_mg_slab_colagg(d, parr, r, world, gf.ctypes.data_as(ip_), int(gf.size), gc.ctypes.data_as(ip_), int(gc.size),
                                       colagg.ctypes.data_as(ip_), C.byref(nlo))
            assert rc == 0, (l, r, rc)
            own = np.arange(pf[r], pf[r + 1])
            want_own = to_coarse[own] - pc[r]
            assert want_own.min() >= 0 and want_own.max() < nc                    # aggregates never cross a cut
            cg = to_coarse[gf.astype(np.int64)]                                   # the halo rows' global coarse rows: among the coarse halo rows
            pos = np.searchsorted(gc, cg)
            assert np.all(pos < gc.size) and np.array_equal(gc[pos], cg)
            want = np.concatenate([want_own, nc + pos]).astype(np.int32)
            assert np.array_equal(colagg, want), (l, r, np.flatnonzero(colagg != want)[:8])
            assert nlo.value == int(np.sum(gc < pc[r])), (l, r, nlo.value)
            checked += want.size
            if gf.size:                                                           # a halo row the coarse slab does not list is refused
                assert h.gcge_mg_slab_colagg(d, parr, r, world, gf.ctypes.data_as(ip_), int(gf.size), gc.ctypes.data_as(ip_), 0,
                                             colagg.ctypes.data_as(ip_), None) == -2
    assert checked > 0


# ---- GPU: ranks sharing the one GPU over gloo ---------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def _run(mode, spec, world, timeout=240):
    """every child under its own time limit; the first non-zero exit fails the test (a time-out is a failure to report, never retried)"""
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OMP_NUM_THREADS="1",
                   HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "slab_refresh_worker.py"), mode, spec], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    try:
        for p in procs:
            o, _ = p.communicate(timeout=timeout)
            outs.append(o)
    finally:
        for q in procs:
            if q.poll() is None:
                q.kill()
    for o in outs:
        print(o[-1500:])
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, "rank %d failed:\n%s" % (r, o[-3000:])
        assert "rank %d ok" % r in o, o[-2000:]


@pytest.mark.gpu
@pytest.mark.parametrize("world,spec", [(2, "lap:8,8,16"), (3, "lap:8,8,24"), (2, "lap:8,8,16:0,7,16"), (2, "sio2:16")])
def test_slab_hierarchy_refreshed_in_place_is_the_fresh_hierarchy_bit_for_bit(world, spec):
    _run("refresh", spec, world)


@pytest.mark.gpu
def test_ranks_agree_on_a_decline_and_nobody_hangs():
    _run("disagree", "sio2:16", 2)
