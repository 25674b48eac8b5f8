"""New values, in place, for ROW SLABS (gcge_hip_mat_update_values_device on a handle with halo columns and a halo plan;
hip_slab_matrix / NativeComm.slab_matrix / lap3d_slab(updatable=True)).  tests/test_mat_update.py, test_mat_update_forms.py and
test_mat_update_reordered.py cover whole matrices and stay as they are.

CPU: gcge_hip_value_maps_selfcheck_slab — the split and the block form of a slab built from val0 WITH their maps, the maps replayed on
val1 (new diagonal, new atom-block values, the same star coefficients: test_mat_update_forms.real_values), against the split and block
form built directly from val1: zero differing stored values.  Slabs 0, 1, 2 of the SiO2-like matrix on 24^3 cut on planes [0, 8, 16, 24]
and [0, 7, 16, 24] (an odd cut), and the lower slab of the ball in 24^3 cut between grid lines (a masked grid: the box index of every
local column named).  A changed star coefficient must report a pin violation.

GPU, one process (tests/slab_update_worker.py): the loop-back slab of tests/rccl_loopback_worker.py — the neighbour is the rank itself,
the halo travels over RCCL from C — created with updatable=True and updated; the products, with and without the interior swept while the
halo travels, must be bit-identical to those of a fresh slab handle created from the new values."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from gcge_amd import dist as gdist
from gcge_amd.lib import hip_lib
from slab_cases import G, dp_, ip_, plane_partitions, slab_of, values
from test_mat_update_forms import case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def selfcheck_slab(s, v0, v1, dense_mode=1):
    g = hip_lib()
    out = (C.c_long * 4)()
    box = s.box_local.ctypes.data_as(ip_) if s.box_local is not None else None
    d = s.dims if s.dims is not None else (0, 0, 0)
    bad = g.gcge_hip_value_maps_selfcheck_slab(s.n_loc, s.ncols, s.a, s.n_global, s.ghosts.ctypes.data_as(ip_), s.rp.ctypes.data_as(ip_),
                                               s.ci.ctypes.data_as(ip_), v0.ctypes.data_as(dp_), v1.ctypes.data_as(dp_), dense_mode,
                                               d[0], d[1], d[2], box, out)
    return bad, list(out)


def slabs():
    out = []
    for k, part in enumerate(plane_partitions()):
        for r in range(3):
            out.append(pytest.param("sio2", part[r], part[r + 1], id="sio2-%s-slab%d" % ("planes" if k == 0 else "oddcut", r)))
    return out


def ball_slab():
    c = case("ball")
    part = gdist.partition_lines(c.box, G, 2)
    return c, slab_of(c, part[0], part[1])


@pytest.mark.parametrize("name,a,b", slabs())
def test_slab_maps_replayed_on_the_host_store_what_a_creation_from_the_new_values_stores(name, a, b):
    c = case(name)
    s = slab_of(c, a, b)
    v0, v1 = values(c, s, 0), values(c, s, 2)
    assert s.ghosts.size >= 6 * G * G and np.any(v0[s.diag] != v1[s.diag]) and np.any(v0[s.free] != v1[s.free]) and np.array_equal(v0[s.pinned], v1[s.pinned])
    bad, out = selfcheck_slab(s, v0, v1)
    print(name, a, b, "differing stored values", bad, "forms", out[0], "layers", out[1], "pinned", out[2], "remainder entries in halo columns", out[3])
    assert bad == 0, (bad, out)
    assert out[0] == 3 and out[1] >= 1, out                   # the star and blocks under it
    assert out[2] == int(s.pinned.sum()), (out, int(s.pinned.sum()))
    if a == 0:                                                # (the cuts on planes 7 and 8 run through an atom, the cut on plane 16 does not)
        assert out[3] > 0, "no entry of the star's remainder sits in a halo column: the maps of halo columns are not exercised"
    assert selfcheck_slab(s, v0, v0)[0] == 0                  # the identity update


def test_slab_of_a_masked_grid_maps_replayed_on_the_host():
    c, s = ball_slab()
    v0, v1 = values(c, s, 0), values(c, s, 2)
    assert s.box_local is not None and s.ghosts.size > 0
    bad, out = selfcheck_slab(s, v0, v1)
    print("ball", s.a, s.b, "differing stored values", bad, "forms", out[0], "layers", out[1], "pinned", out[2], "remainder entries in halo columns", out[3])
    assert bad == 0 and out[0] == 3, (bad, out)
    assert out[2] == int(s.pinned.sum()), (out, int(s.pinned.sum()))
    assert selfcheck_slab(s, v0, v0)[0] == 0


@pytest.mark.parametrize("name", ["sio2", "ball"])
def test_a_changed_star_coefficient_on_a_slab_is_a_pin_violation(name):
    if name == "ball":
        c, s = ball_slab()
    else:
        c = case(name)
        part = plane_partitions()[1]
        s = slab_of(c, part[1], part[2])
    v0 = values(c, s, 0)
    pinned = np.flatnonzero(s.pinned)
    in_halo = pinned[s.ci[pinned] >= s.n_loc]                  # a pinned entry whose column is a halo row, and one inside the slab
    assert in_halo.size and pinned.size
    for q in (pinned[pinned.size // 2], in_halo[in_halo.size // 2]):
        v1 = values(c, s, 1)
        v1[q] = np.nextafter(v1[q], 0.0)
        assert selfcheck_slab(s, v0, v1)[0] == -2, q
    v1 = values(c, s, 1)
    v1[np.flatnonzero(s.diag)[5]] = np.nan
    assert selfcheck_slab(s, v0, v1)[0] == -2


# ---- GPU: the loop-back slab, one process -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("which", ["sio2", "ball", "lap", "lap_pad8"])
def test_loopback_slab_updated_in_place_is_a_fresh_slab_bit_for_bit(which):
    """tests/slab_update_worker.py: see its docstring.  The worker's time limit is the guard against a hang; a time-out is a failure."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "slab_update_worker.py"), which], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=240)
    print(p.stdout[-3000:])
    assert p.returncode == 0, p.stdout[-3000:]
    assert "slab update ok: %s" % which in p.stdout, p.stdout[-2000:]
