"""Matrices, case table and restated launch arithmetic for tests/test_star_rows.py and its worker tests/star_slab_worker.py: the plane
sweep of spmm_star.hip on EXACT data.

The matrix (build): a star of arm lengths (Rx, Ry, Rz) <= 6 on an nx x ny x nz grid, x fastest, truncated at the faces — or at the
rim of a convex set of grid points inside the box (a masked grid, rows in scan order).  Coefficients: nonzero integers of magnitude
<= 3, one set for all axes ("iso") or one per axis ("axis"); the diagonal of every row a nonzero integer of magnitude <= 3 of its
own, but for a few rows without a stored diagonal and a few with a stored 0.0.  Planted rows (symmetric pairs, every touched row
listed in `touched`, so that the clean count is exact):
  ("value", p, axis, k)     the star entry k steps up `axis` from point p, and its mirror, hold another value than the coefficient
  ("missing", p, axis, k)   that entry and its mirror are not stored
  ("off", p, q)             an entry between points p and q that is not on the star, and its mirror
  ("block", p0, (bx, by, bz))  every pair of the bx x by x bz points from p0 coupled: rows of >= 24 entries, a dense block of the remainder
X comes from helpers.draw(seed, shape, False): every product is an integer of magnitude <= (36 + 1 + 64) * 9, every column sum far
below 2^53 (test_exactness_premise_and_builder), so any order of summation gives the same doubles and the tests compare with
np.array_equal.  real=True: uniform - 0.5 in place of coefficients, diagonal and X, and a longdouble product formed term by term.
"""
import ctypes as C

import numpy as np

from helpers import draw

STAR_R = 6
ip_, dp_ = C.POINTER(C.c_int), C.POINTER(C.c_double)


def cdiv(a, b):
    return -(-a // b)


def other_value(c):
    """a nonzero integer of magnitude <= 3 that is not c"""
    return c - 1.0 if c in (3.0, -1.0) else c + 1.0


def ellipsoid(dims, shear=0.0):
    """the grid points of an ellipsoid that fills the box (shear: its centre moves by `shear` points in x from the first to the last
    plane — an affine image of a ball, hence convex): mask[z, y, x]"""
    nx, ny, nz = dims
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    cz, cy = (nz - 1) / 2.0, (ny - 1) / 2.0
    ax = nx / 2.0 - abs(shear) / 2.0
    cx = (nx - 1) / 2.0 + shear * (z - cz) / nz
    return ((x - cx) / ax) ** 2 + ((y - cy) / (ny / 2.0)) ** 2 + ((z - cz) / (nz / 2.0)) ** 2 <= 1.0


class Star:
    """One matrix: S (scipy CSR, sorted, explicit zeros kept), dims, arms, box (masked grids: box index of every row, else None),
    touched (rows that are not clean), nb[(axis, k, sign)] = row of that neighbour or -1."""

    def __init__(self, name, dims, arms, coef, seed, plant=(), mask=None, real=False, shear=0.0):
        import scipy.sparse as sp
        self.name, self.dims, self.arms, self.coef, self.seed, self.real = name, tuple(dims), tuple(arms), coef, seed, real
        nx, ny, nz = dims
        nbox = nx * ny * nz
        self.masked = bool(mask)
        inside = ellipsoid(dims, shear).ravel() if mask else np.ones(nbox, dtype=bool)
        box = np.flatnonzero(inside)
        n = self.n = int(box.size)
        self.box = np.ascontiguousarray(box, dtype=np.int32) if mask else None
        inv = np.full(nbox, -1, dtype=np.int64)
        inv[box] = np.arange(n)
        self.inv = inv
        co = [box % nx, (box // nx) % ny, box // (nx * ny)]
        self.co = co
        stride = [1, nx, nx * ny]
        c = draw(seed, (3, STAR_R), real)
        if coef == "iso":
            c[1], c[2] = c[0], c[0]
        else:
            assert not np.array_equal(c[0], c[1]) and not np.array_equal(c[0], c[2])
        self.c = c
        rows, cols, vals = [], [], []
        self.nb = {}
        for a in range(3):
            for k in range(1, arms[a] + 1):
                for sgn in (-1, 1):
                    t = co[a] + sgn * k
                    ok = (t >= 0) & (t < dims[a])
                    j = np.where(ok, inv[np.where(ok, box + sgn * k * stride[a], 0)], -1)
                    self.nb[(a, k, sgn)] = j
                    r = np.flatnonzero(j >= 0)
                    rows.append(r); cols.append(j[r]); vals.append(np.full(r.size, c[a, k - 1]))
        d = draw(seed + 1, (n,), real)
        self.nodiag = np.array([5, n // 2 + 1, n - 3])                  # rows without a stored diagonal
        self.zerodiag = np.array([7, n // 3])                           # rows with a stored 0.0
        d[self.zerodiag] = 0.0
        keep = np.ones(n, dtype=bool)
        keep[self.nodiag] = False
        d[self.nodiag] = 0.0
        self.diag = d
        r = np.flatnonzero(keep)
        rows.append(r); cols.append(r); vals.append(d[r])
        rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
        # planted rows: {(r, c): value or None}
        mods, touched = {}, set()

        def row_of(p):
            q = inv[p[0] + nx * (p[1] + ny * p[2])]
            assert q >= 0, (name, "a planted point outside the domain", p)
            return int(q)
        for op in plant:
            if op[0] in ("value", "missing"):
                _, p, a, k = op
                assert 1 <= k <= arms[a]
                q = list(p); q[a] += k
                r0, r1 = row_of(p), row_of(q)
                v = other_value(c[a, k - 1]) if op[0] == "value" else None
                mods[(r0, r1)] = mods[(r1, r0)] = v
                touched |= {r0, r1}
            elif op[0] == "off":
                r0, r1 = row_of(op[1]), row_of(op[2])
                d3 = [abs(op[1][i] - op[2][i]) for i in range(3)]
                assert sum(1 for v in d3 if v) >= 2 or max(d3) > STAR_R, (name, "not off the star", op)
                v = draw(seed + 3 + len(mods), (1,), False)[0]
                mods[(r0, r1)] = mods[(r1, r0)] = v
                touched |= {r0, r1}
            else:
                _, p0, (bx, by, bz) = op
                pts = [row_of((p0[0] + i, p0[1] + j, p0[2] + l)) for l in range(bz) for j in range(by) for i in range(bx)]
                w = draw(seed + 7, (len(pts), len(pts)), False)
                assert len(pts) >= 25 and min(bx, by, bz) >= 2             # >= 24 entries off the diagonal, some off the star in every row
                for i, ri in enumerate(pts):
                    for j, rj in enumerate(pts):
                        if i < j:
                            mods[(ri, rj)] = mods[(rj, ri)] = w[i, j]
                touched |= set(pts)
        self.block = [op for op in plant if op[0] == "block"]
        if mods:
            key = rows * n + cols
            order = np.argsort(key, kind="stable")
            rows, cols, vals, key = rows[order], cols[order], vals[order], key[order]
            drop = np.zeros(key.size, dtype=bool)
            add = []
            for (r0, r1), v in mods.items():
                i = int(np.searchsorted(key, r0 * n + r1))
                if i < key.size and key[i] == r0 * n + r1:
                    if v is None:
                        drop[i] = True
                    else:
                        vals[i] = v
                else:
                    assert v is not None
                    add.append((r0, r1, v))
            rows, cols, vals = rows[~drop], cols[~drop], vals[~drop]
            if add:
                rows = np.concatenate([rows, [t[0] for t in add]]); cols = np.concatenate([cols, [t[1] for t in add]])
                vals = np.concatenate([vals, [t[2] for t in add]])
        S = sp.coo_matrix((vals, (rows, cols)), shape=(n, n)).tocsr()
        S.sort_indices()
        assert S.nnz == rows.size                                           # (no entry twice; explicit zeros stay)
        self.S = S
        self.touched = np.array(sorted(touched), dtype=np.int64)
        self.nclean = n - len(touched)
        self._csr = None
        self._cache = {}

    def csr(self):
        """(CSR struct of gcge_amd.lib, keepalive)"""
        if self._csr is None:
            from helpers import csr_from_scipy
            self._csr = csr_from_scipy(self.S)
        return self._csr

    def detected_arms(self):
        """star_offsets: offset k of an axis counts when at least half of the rows carry it up or down — on a full box of edge n the
        rows with k <= c or c + k < n: n - max(0, 2 k - n) of n"""
        out = []
        for a in range(3):
            R = 0
            for k in range(1, self.arms[a] + 1):
                have = (self.nb[(a, k, -1)] >= 0) | (self.nb[(a, k, 1)] >= 0)
                if 2 * np.count_nonzero(have) >= self.n and R == k - 1:
                    R = k
            out.append(R)
        return tuple(out)

    def iso_on_device(self):
        """StarMat::iso: the three coefficient arrays equal as bits over all 6 arm positions — one set on axes of different arm lengths is not"""
        return self.coef == "iso" and len(set(self.arms)) == 1

    def X(self, width):
        return self._get(("X", width), lambda: draw(self.seed + 11, (self.n, width), self.real))

    def _get(self, key, make):
        if key not in self._cache:
            self._cache[key] = make()
        return self._cache[key]

    def product(self, X):
        """float64 from scipy (exact data)"""
        return np.ascontiguousarray(self.S @ X)

    def product_ld(self, X):
        """(A X, |A| |X|) in longdouble, term by term (no planted rows)"""
        assert self.touched.size == 0
        Xl = X.astype(np.longdouble)
        d = self.diag.astype(np.longdouble)[:, None]
        w, ab = d * Xl, np.abs(d) * np.abs(Xl)
        for (a, k, sgn), j in self.nb.items():
            ok = (j >= 0)[:, None]
            t = np.where(ok, Xl[np.maximum(j, 0)], np.longdouble(0.0))
            cc = np.longdouble(self.c[a, k - 1])
            w += cc * t
            ab += np.abs(cc) * np.abs(t)
        return w, ab


# ---- the slabs ---------------------------------------------------------------------------------------------------------------------
class Slab:
    pass


def slab_rows(st, a, b):
    """rows [a, b) of st with LOCAL columns: own columns c - a, halo columns n_loc + the rank among the ascending global halo rows
    (the renaming of gcge_dist_localize, as tests/slab_cases.slab_of does it)"""
    S = st.S
    s = Slab()
    q0, q1 = int(S.indptr[a]), int(S.indptr[b])
    s.a, s.b, s.n_loc, s.n_global = a, b, b - a, S.shape[0]
    s.rp = np.ascontiguousarray(S.indptr[a:b + 1] - q0, dtype=np.int32)
    gcol = S.indices[q0:q1].astype(np.int64)
    own = (gcol >= a) & (gcol < b)
    s.ghosts = np.ascontiguousarray(np.unique(gcol[~own]), dtype=np.int32)
    s.ci = np.ascontiguousarray(np.where(own, gcol - a, s.n_loc + np.searchsorted(s.ghosts, gcol)), dtype=np.int32)
    s.val = np.ascontiguousarray(S.data[q0:q1], dtype=np.float64)
    s.gcol, s.ncols = gcol, s.n_loc + int(s.ghosts.size)
    s.box_local = None
    if st.box is not None:
        s.box_local = np.ascontiguousarray(np.concatenate([st.box[a:b], st.box[s.ghosts]]), dtype=np.int32)
    # the loop-back operator: halo row g is served by own row (g - a) mod n_loc
    s.send_rows = np.ascontiguousarray((s.ghosts.astype(np.int64) - a) % s.n_loc, dtype=np.int32)
    s.nclean = s.n_loc - int(np.count_nonzero((st.touched >= a) & (st.touched < b)))
    return s


def loopback(s):
    """S[:, own] + S[:, halo] P with P the 0/1 matrix of the halo map"""
    import scipy.sparse as sp
    Sg = sp.csr_matrix((s.val, s.gcol, s.rp.astype(np.int64)), shape=(s.n_loc, s.n_global)).tocsc()
    ng = int(s.ghosts.size)
    P = sp.csr_matrix((np.ones(ng), (np.arange(ng), s.send_rows)), shape=(ng, s.n_loc))
    return (Sg[:, s.a:s.b] + Sg[:, s.ghosts] @ P).tocsr()


# ---- the launch arithmetic of spmm_star.hip restated --------------------------------------------------------------------------------
def launch(nx, ny, m, zlo, zhi, third):
    """star_launch over the output planes [zlo, zhi): dict of lpp, ntx, nty, npass, zchunks, zlen, the z ranges, the patches of a
    full grid and the workgroups (a masked grid in the third form launches only the patches that have rows: patches_masked)"""
    nzl = zhi - zlo
    if nzl <= 0:
        return None
    lpp = 8 if third else 4
    ty = 64 // lpp
    ntx, nty, npass = cdiv(nx, 16), cdiv(ny, ty), cdiv(m, 2 * lpp)
    P = ntx * nty * npass
    zchunks = max(1, min(nzl // 24, (2 * 256 + P - 1) // P))
    zlen = cdiv(nzl, zchunks)
    zchunks = cdiv(nzl, zlen)
    ranges = [(zlo + i * zlen, min(zhi, zlo + (i + 1) * zlen)) for i in range(zchunks)]
    return dict(lpp=lpp, ty=ty, ntx=ntx, nty=nty, npass=npass, zchunks=zchunks, zlen=zlen, ranges=ranges, npatch=ntx * nty,
                total=ntx * nty * zchunks * npass)


def pranges(st, ty):
    """first / last + 1 plane in which each 16 x ty patch of a masked grid has rows: {patch: (lo, hi)}, patches with rows only"""
    nx, ny, nz = st.dims
    ntx = cdiv(nx, 16)
    p = (st.co[1] // ty) * ntx + st.co[0] // 16
    out = {}
    for q in np.unique(p):
        z = st.co[2][p == q]
        out[int(q)] = (int(z.min()), int(z.max()) + 1)
    return out


def masked_spans(st, m, third):
    """the (z0, z1) of every (patch, range) workgroup of a masked grid: z0 >= z1 is the zero-fill branch"""
    nx, ny, nz = st.dims
    L = launch(nx, ny, m, 0, nz, third)
    pr = pranges(st, L["ty"])
    patches = sorted(pr) if third else range(L["npatch"])
    out = []
    for p in patches:
        lo, hi = pr.get(p, (nz, 0))
        for (r0, r1) in L["ranges"]:
            out.append((max(r0, lo), min(r1, hi)))
    return L, out


def interior(zs, ze, nz, R, masked_slab=False, shared_lo=0, shared_hi=0):
    """gcge_hip_star_interior: (has an interior, ilo, ihi) of a slab of planes [zs, ze) (zmin / zmax from the DETECTED arm length R; the
    sweep keeps STAR_R planes off either cut whatever R is)"""
    zmin, zmax = max(0, zs - R), min(nz, ze + R)
    if masked_slab:
        lo = zs + STAR_R + shared_lo if (zmin < zs or shared_lo) else zs
        hi = ze - STAR_R - shared_hi if (ze < zmax or shared_hi) else ze
        return hi > lo, lo, hi
    lo = zs + STAR_R if zmin < zs else zs
    hi = ze - STAR_R if ze < zmax else ze
    return (zmin < zs or ze < zmax) and hi > lo, lo, hi


def block_of(xcd, L, total):
    """star_block_of: the linear workgroup id the launch id L works as"""
    if not xcd:
        return L
    k = L & 7
    if xcd == 1:
        q, r = total >> 3, total & 7
        return k * q + min(k, r) + (L >> 3)
    G, s = xcd, L >> 3
    full = total // (8 * G) * (8 * G)
    return (s // G) * 8 * G + k * G + s % G if L < full else L


# ---- the case table -----------------------------------------------------------------------------------------------------------------
# (m, first column of X, first column of Y)
ALL_M = [(2, 0, 0), (14, 2, 4), (16, 0, 2), (18, 4, 0), (30, 4, 2), (32, 2, 2), (34, 0, 4), (66, 2, 0), (130, 0, 2)]
FEW_M = [(2, 2, 0), (18, 0, 4), (34, 4, 2)]
DOT_M = [(2, 0, 2), (30, 4, 2), (64, 2, 0)]
BASIC = lambda nx, ny, nz: [("value", (3, 4, nz // 2), 0, 1), ("missing", (nx - 2, ny - 1, 0), 2, 1), ("off", (0, 0, 0), (nx - 1, ny - 1, nz - 1)),
                            ("off", (min(15, nx - 2), 7, nz - 1), (min(16, nx - 1), 8, nz - 1))]
BLOCK = lambda z: [("block", (4, 3, z), (5, 3, 2))]

# name: (dims, arms, coef, plant, widths) — named for the branch of spmm_star.hip the case reaches
WHOLE = {
    "one_ragged_patch_all_clean": ((13, 13, 13), (6, 6, 6), "iso", [], FEW_M),
    "ragged_patch_14_planes": ((13, 13, 14), (6, 6, 6), "iso", BASIC(13, 13, 14), FEW_M),
    "exact_patches_15_planes": ((16, 16, 15), (5, 5, 5), "iso", BASIC(16, 16, 15), FEW_M),
    "exact_patches_16_planes": ((16, 16, 16), (4, 4, 4), "iso", BASIC(16, 16, 16) + BLOCK(9), ALL_M),
    "second_patch_column_14_planes": ((17, 24, 14), (3, 3, 3), "axis", BASIC(17, 24, 14) + [("off", (15, 15, 3), (16, 16, 3))], ALL_M),
    "ragged_both_ways_31_planes": ((33, 17, 31), (6, 6, 6), "iso", BASIC(33, 17, 31) + BLOCK(20) + [("value", (20, 9, 14), 2, 6)], ALL_M),
    "two_planes_arm_1": ((32, 32, 2), (1, 1, 1), "iso", [("block", (4, 3, 0), (5, 3, 2)), ("value", (17, 9, 0), 2, 1)], FEW_M),
    "two_planes_arms_661": ((32, 32, 2), (6, 6, 1), "iso", BASIC(32, 32, 2), FEW_M),
    "eight_planes": ((16, 16, 8), (6, 6, 6), "iso", BASIC(16, 16, 8), FEW_M),
    "nine_planes": ((16, 16, 9), (6, 6, 6), "iso", [], FEW_M),
    "planes_29_arm_2": ((13, 13, 29), (2, 2, 2), "iso", BASIC(13, 13, 29) + BLOCK(10), FEW_M),
    "planes_30_arm_3": ((13, 13, 30), (3, 3, 3), "iso", BASIC(13, 13, 30), FEW_M),
    "arms_456": ((13, 14, 13), (4, 5, 6), "axis", BASIC(13, 14, 13), FEW_M),
    # z ranges (13 x 13: two 16 x 8 patches or one 16 x 16 patch, so nz / 24 decides the ranges): 24 + 24, 25 + 24, 25 + 25 + 23
    "two_ranges_of_24": ((13, 13, 48), (2, 2, 2), "iso", BLOCK(30) + [("value", (3, 4, 23), 2, 1), ("off", (1, 2, 23), (2, 3, 24)), ("missing", (12, 12, 0), 2, 2)], FEW_M),
    "ranges_25_24": ((13, 13, 49), (6, 6, 6), "iso", [("value", (6, 6, 24), 2, 1), ("off", (0, 0, 0), (12, 12, 48))], FEW_M),
    "ranges_25_25_23": ((13, 13, 73), (3, 3, 3), "iso", [("missing", (5, 5, 24), 2, 1), ("value", (7, 2, 49), 2, 3)], FEW_M),
    "ranges_patches_passes": ((33, 17, 49), (6, 6, 6), "iso", BASIC(33, 17, 49) + [("value", (20, 9, 24), 2, 1)], [(34, 0, 2), (2, 2, 0)]),
    "single_patch_of_listed_rows": ((33, 17, 31), (6, 6, 6), "iso", [("off", (1, 1, 5), (2, 2, 5)), ("value", (3, 3, 7), 0, 2), ("missing", (5, 2, 9), 1, 1)], FEW_M),
}
XCD_BIG = ("xcd_270_workgroups", (40, 33, 48), (6, 6, 6), "iso", [("off", (0, 0, 0), (39, 32, 47)), ("value", (20, 20, 23), 2, 1)], 130)
MASKED = {
    "ellipsoid_20x27x33": ((20, 27, 33), 6, 0.0, [("value", (10, 13, 16), 2, 1), ("off", (9, 12, 10), (10, 13, 10)), ("block", (8, 12, 20), (5, 3, 2))]),
    "sheared_ellipsoid_20x20x50": ((20, 20, 50), 6, 8.0, [("value", (10, 10, 24), 2, 1), ("off", (9, 9, 30), (10, 10, 30)), ("block", (8, 8, 12), (5, 3, 2))]),
}
REAL = {
    "real_iso_arm_6": ((33, 17, 31), (6, 6, 6), "iso", None),
    "real_axis_arm_3": ((17, 24, 14), (3, 3, 3), "axis", None),
    "real_masked": ((20, 27, 33), (6, 6, 6), "iso", 0.0),
}
# slabs of planes [z0, z1) of a 16 x 16 x 40 grid: (arm, z0, z1, why)
SLAB_GRID = (16, 16, 40)
SLABS = {
    "lower": (6, 0, 14), "middle_empty_interior": (6, 14, 26), "middle_one_interior_plane": (6, 13, 26), "lower_halo_of_2_planes": (6, 2, 30),
    "upper": (6, 26, 40), "middle_arm_3": (3, 14, 26),
}
MASKED_SLABS = ["masked_lower", "masked_middle"]

_made = {}


def whole(name):
    if name not in _made:
        if name == XCD_BIG[0]:
            dims, arms, coef, plant = XCD_BIG[1:5]
        else:
            dims, arms, coef, plant, _ = WHOLE[name]
        _made[name] = Star(name, dims, arms, coef, 1000 + 37 * ([XCD_BIG[0]] + list(WHOLE)).index(name), plant)
    return _made[name]


def masked(name):
    if name not in _made:
        dims, R, shear, plant = MASKED[name]
        _made[name] = Star(name, dims, (R, R, R), "iso", 5000 + 37 * list(MASKED).index(name), plant, mask=True, shear=shear)
    return _made[name]


def real_case(name):
    if name not in _made:
        dims, arms, coef, shear = REAL[name]
        _made[name] = Star(name, dims, arms, coef, 7000 + 37 * list(REAL).index(name), (), mask=shear is not None, real=True, shear=shear or 0.0)
    return _made[name]


def slab_grid(R):
    key = ("slab_grid", R)
    if key not in _made:
        nx, ny, nz = SLAB_GRID
        plant = [("value", (3, 4, 13), 2, 1), ("off", (1, 2, 25), (2, 3, 26)), ("missing", (8, 8, 20), 0, 1), ("off", (0, 0, 2), (1, 1, 2)),
                 ("value", (5, 5, 29), 2, R), ("off", (15, 15, 39), (14, 14, 38)), ("off", (0, 0, 0), (1, 1, 1))]
        _made[key] = Star("slab_grid_R%d" % R, SLAB_GRID, (R, R, R), "iso", 9000 + R, plant)
    return _made[key]


def slab_case(name):
    """(Star, Slab, planes (zs, ze) or None on a masked grid)"""
    if name in SLABS:
        R, z0, z1 = SLABS[name]
        st = slab_grid(R)
        plane = SLAB_GRID[0] * SLAB_GRID[1]
        return st, slab_rows(st, z0 * plane, z1 * plane), (z0, z1)
    from gcge_amd import dist as gdist
    st = masked("sheared_ellipsoid_20x20x50")
    part = gdist.partition_lines(st.box, st.dims[0], 3)
    a, b = (part[0], part[1]) if name == "masked_lower" else (part[1], part[2])
    return st, slab_rows(st, a, b), None
