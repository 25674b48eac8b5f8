"""A X = B on Lap3D N^3 with m random right-hand sides to the relative residual 1e-8, through HipBackend.linear_solver:
    plain     the fused block CG alone (amg=None): one call to "rel" tol
    V-cycle   flexible block CG preconditioned by one BlockAMG V-cycle per iteration: 6 levels, the bench's smoothing (1 cycle, 3 / 4
              CG steps on the finest / the coarser levels, level 0 to 1e-2)
For each: outer iterations (plain: CG iterations), V-cycles summed over the columns (a column that has converged takes none), seconds of the solve (the second of two runs; the
first creates the solver's blocks), the largest true relative residual; for the hierarchy its set-up seconds.
    python tools/linsolve_probe.py N m [--out FILE]"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from gcge_amd import HipBackend, NoConvergence, make_problem

argv = list(sys.argv[1:])
out_path = None
if "--out" in argv:
    i = argv.index("--out"); out_path = argv[i + 1]; del argv[i:i + 2]
N, m = int(argv[0]), int(argv[1])
TOL = 1e-8
hip = HipBackend()
t0 = time.perf_counter()
A = make_problem("lap3d", N)[0]
mat = hip.matrix(A)
hip.sync()
print("lap3d %d^3: n %d, m %d, matrix generated and uploaded in %.1f s" % (N, A.nrows, m, time.perf_counter() - t0), flush=True)
b = torch.rand((A.nrows, m), dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)) - 0.5
rows = []


def run(name, amg, maxiter, setup):
    with hip.linear_solver(mat, amg=amg, max_cols=m) as ls:
        for rep in range(2):
            try:
                r = ls.solve(b, tol=TOL, maxiter=maxiter)
            except NoConvergence as e:
                r = e.result
        vcycles = int(ls.column_iterations.sum()) if amg is not None else 0
    row = {"case": name, "N": N, "n": A.nrows, "m": m, "tol": TOL, "outer_iterations": int(r.iterations), "vcycles_all_columns": vcycles,
           "converged_columns": int(r.converged.sum()),
           "seconds": r.seconds, "setup_seconds": setup, "max_rel_res": float(r.residual_norms.max())}
    rows.append(row)
    print("%-8s outer iterations %4d  V-cycles (all columns) %4d  converged %d / %d  solve %8.3f s  set-up %s  max |b - A x| / |b| %.2e" % (
        name, row["outer_iterations"], vcycles, row["converged_columns"], m, r.seconds, "%.3f s" % setup if setup is not None else "-", row["max_rel_res"]), flush=True)
    return r


run("plain", None, 4000, None)
hip.sync()
t0 = time.perf_counter()
h = hip.multigrid(mat, levels=6, block_size=m, cycles=1, smooth0=3, smooth=4, rate=1e-2, refreshable=False)
hip.sync()
setup = time.perf_counter() - t0
print("hierarchy: %d levels, set-up %.3f s" % (h.num_levels, setup), flush=True)
r = run("V-cycle", h, 200, setup)
rows[-1]["levels"] = h.num_levels
h.close()
hip.free_matrix(mat)
if out_path:
    with open(out_path, "w") as f:
        json.dump(rows, f, indent=1)
