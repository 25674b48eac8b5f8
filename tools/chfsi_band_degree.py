"""The degree factor of GCGE_RunChFSIBand: degree = ceil(f (lmax - lmin) / (b - a)) for f in {2, 3, 4, 6} on the two CPU cases of
tests/test_chfsi_band_host.py (lap3d 12 with [1.0, 1.55], and the same matrix shifted by -1.3 with [-0.3, 0.25]), 48 columns, bounds =
the spectrum widened by 5 % of its width, 1e-8, over the CPU oracle's table.  Matrix products = columns x degree x filters (a run of k
outer iterations applies k + 1 filters) + the columns of each Rayleigh-Ritz and residual pass.

    python tools/chfsi_band_degree.py [--out profiles/chfsi_band]        (no GPU needed)"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chfsi_band"))
    a = ap.parse_args()
    from gcge_amd.lib import csr_to_scipy, make_problem, run_chfsi_band
    from helpers import OracleBackend
    oracle = OracleBackend()
    ncol, rows = 48, []
    for name, shift, lo, hi in (("lap3d 12, [1.0, 1.55]", 0.0, 1.0, 1.55), ("lap3d 12 - 1.3 I, [-0.3, 0.25]", 1.3, -0.3, 0.25)):
        A, _ = make_problem("lap3d", 12)
        val = np.ctypeslib.as_array(A.val, (int(A.nnz),))
        val[val == 6.0] -= shift
        lam = np.linalg.eigvalsh(csr_to_scipy(A).toarray())
        w = lam[-1] - lam[0]
        lmin, lmax = float(lam[0] - 0.05 * w), float(lam[-1] + 0.05 * w)
        inside = int(np.count_nonzero((lam >= lo) & (lam <= hi)))
        mA = oracle.matrix(A)
        for f in (2, 3, 4, 6):
            degree = min(1000, max(20, int(math.ceil(f * (lmax - lmin) / (hi - lo)))))
            evec = oracle.ops.mv_create(ncol, mA)
            try:
                ev, res, rc = run_chfsi_band(oracle.ops_handle, mA, ["-chfsi_band_lo", repr(lo), "-chfsi_band_hi", repr(hi), "-nevMax", ncol,
                                                                     "-chfsi_degree", degree, "-gcge_max_niter", 200, "-chfsi_lower_bound",
                                                                     repr(lmin), "-chfsi_upper_bound", repr(lmax)], evec)
            finally:
                oracle.ops.mv_destroy(evec, ncol)
            filters = res.numIter + 1
            products = ncol * degree * filters + 2 * ncol * filters
            rows.append(dict(case=name, f=f, degree=degree, rc=rc, converged=int(res.converged), pairs=int(res.nevConv), inside=inside,
                             outer_iterations=int(res.numIter), filters=filters, products=products))
            print(rows[-1], flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "degree_factor.json"), "w") as fh:
        json.dump(rows, fh, indent=1)
    lines = ["| case | f | degree | outer iterations | filters | pairs found / inside | matrix products |", "|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append("| %s | %d | %d | %d | %d | %d / %d | %d |" % (r["case"], r["f"], r["degree"], r["outer_iterations"], r["filters"], r["pairs"],
                                                                  r["inside"], r["products"]))
    total = {f: sum(r["products"] for r in rows if r["f"] == f) for f in (2, 3, 4, 6)}
    lines += ["", "Total products over both cases: " + ", ".join("f = %d: %d" % (f, total[f]) for f in sorted(total))]
    with open(os.path.join(a.out, "degree_factor.md"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
