"""Times of the kernel polynomial method's pieces (gcge_hip_cheb_sweep_dots / gcge_hip_cheb_dots in csrc/hip/cheb_sweeps.hip,
gcge_hip_cheb_step_dots_mv, GCGE_ChebMoments, gcge_amd.eigenvalue_count).

    python tools/kpm_probe.py [--out DIR] [--runs R] [--only step|count]

  step    GCGE_ChebMoments on lap3d 256^3 with a block of 64 +-1 columns, degree 40 (20 steps), in four configurations:
          {fused step, GCGE_CHEB_NO_FUSE=1} x {cheb_step_dots slot, GCGE_NO_CHEB_STEP_DOTS=1}.  Without the slot every step is cheb_step
          followed by two MultiVecLocalInnerProd('D'): the route the table offered before the slot existed.  ms per step = the call's
          time / 20 (the first step, which has no z and takes the sweep in every configuration, and the product v . v are inside).
  count   lap3d 32^3: eigenvalue_count (32 probes, the driver's degree rule, given bounds) on an interval between two gaps of the lower
          spectrum chosen from the closed form, then the eigsh(interval=, nev_max=suggested) run it precedes; seconds of each, the
          count against the eigenvalues inside, the pairs found.
Each part is a child process of this file under its own `timeout`; a part that fails ends the run.  A part warms its paths up, then
times R >= 10 rounds, the configurations alternating inside a round, with the host clock round a call that ends in a stream
synchronise; median (min, max).  Writes DIR/results.json and DIR/README.md (default DIR: profiles/kpm)."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PARTS = [("step", 600), ("count", 600)]
SWITCHES = ("GCGE_CHEB_NO_FUSE", "GCGE_NO_CHEB_STEP_DOTS")


def timed(paths, runs, sync):
    import numpy as np
    for _, f in paths:
        f()
    sync()
    ts = {name: [] for name, _ in paths}
    for _ in range(runs):
        for name, f in paths:
            sync()
            t0 = time.perf_counter()
            f()
            sync()
            ts[name].append((time.perf_counter() - t0) * 1e3)
    return {name: [float(np.median(v)), float(min(v)), float(max(v))] for name, v in ts.items()}


def part_step(runs):
    import numpy as np
    import torch
    from gcge_amd import HipBackend
    from gcge_amd.lib import cheb_stats, cheb_step_dots_stats, make_problem
    hip = HipBackend()
    N, m, degree = 256, 64, 40
    steps = (degree + 1) // 2
    A, _ = make_problem("lap3d", N)
    mat = hip.matrix(A)
    n, nnz = A.nrows, int(A.nnz)
    gen = torch.Generator(device="cuda").manual_seed(3)
    V = torch.randint(0, 2, (n, m), generator=gen, device="cuda").to(torch.float64) * 2.0 - 1.0
    v = hip.mv_from_torch(mat, V)
    del V
    work = [hip.ops.mv_create(m, mat) for _ in range(3)]
    mom = np.zeros((degree + 1, m))
    got = {}

    def run(name, no_fuse, no_slot):
        def f():
            for key, on in zip(SWITCHES, (no_fuse, no_slot)):
                if on:
                    os.environ[key] = "1"
            try:
                rc = hip.h.GCGE_ChebMoments(mat, v, 0, m, degree, -0.5, 12.5, work[0], work[1], work[2], mom.ctypes.data_as(C.c_void_p), hip.ops_handle)
                assert rc == 0, rc
            finally:
                for key in SWITCHES:
                    os.environ.pop(key, None)
            got[name] = mom.copy()
        return name, f

    paths = [run("fused_slot", False, False), run("fused_noslot", False, True), run("sweep_slot", True, False), run("sweep_noslot", True, True)]
    d0, s0 = cheb_step_dots_stats(), cheb_stats()
    t = timed(paths, runs, hip.sync)
    d1, s1 = cheb_step_dots_stats(), cheb_stats()
    scale = float(n)
    row = dict(part="step", N=N, n=n, nnz=nnz, m=m, degree=degree, steps=steps, runs=runs, form=hip.g.gcge_hip_mat_spmm_form(mat).decode(),
               recompute_pays=int(hip.g.gcge_hip_cg_recompute_pays(mat)), slot_fused=d1[0] - d0[0], slot_swept=d1[1] - d0[1],
               plain_fused=s1[0] - s0[0], plain_swept=s1[1] - s0[1],
               max_moment_difference_over_n={k: float(np.abs(got[k] - got["fused_slot"]).max() / scale) for k in got},
               **{k + "_ms": v for k, v in t.items()})
    print(json.dumps(row), flush=True)
    return [row]


def lap3d_spectrum(N):
    import numpy as np
    c = 2.0 * np.cos(np.arange(1, N + 1) * np.pi / (N + 1))
    return np.sort((6.0 - c[:, None, None] - c[None, :, None] - c[None, None, :]).ravel())


def part_count(runs):
    import numpy as np
    import torch
    from gcge_amd import HipBackend, NoConvergence, eigenvalue_count, eigsh
    from gcge_amd.lib import csr_arrays, make_problem
    hip = HipBackend()
    hip.set_random_mode(1, 20240601)
    N = 32
    lam = lap3d_spectrum(N)
    gaps = np.diff(lam[:400])
    order = np.argsort(gaps)[::-1]
    i0 = int(min(i for i in order[:12] if i >= 20)) + 1                 # the first wide gap behind the 20 lowest eigenvalues
    i1 = int(min(i for i in order[:40] if i >= i0 + 30)) + 1            # the next wide gap at least 30 eigenvalues on
    a, b = float(0.5 * (lam[i0 - 1] + lam[i0])), float(0.5 * (lam[i1 - 1] + lam[i1]))
    inside = int(np.count_nonzero((lam >= a) & (lam <= b)))
    w = lam[-1] - lam[0]
    lmin, lmax = float(lam[0] - 0.05 * w), float(lam[-1] + 0.05 * w)
    A, _ = make_problem("lap3d", N)
    rp, ci, va = csr_arrays(A)
    mat = hip.matrix_from_device(torch.from_numpy(rp).cuda(), torch.from_numpy(ci).cuda(), torch.from_numpy(va).cuda())
    kw = dict(lower_bound=lmin, upper_bound=lmax, backend=hip)
    eigenvalue_count(mat, (a, b), probes=32, **kw)                       # warm-up
    tc = []
    for _ in range(runs):
        hip.sync()
        t0 = time.perf_counter()
        r = eigenvalue_count(mat, (a, b), probes=32, **kw)
        hip.sync()
        tc.append(time.perf_counter() - t0)
    hip.sync()
    t0 = time.perf_counter()
    try:
        e, done = eigsh(mat, interval=(a, b), nev_max=r.suggested_nev_max, method="chebyshev", maxiter=60, **kw), True
    except NoConvergence as ex:
        e, done = ex.result, False
    hip.sync()
    ts = time.perf_counter() - t0
    hip.free_matrix(mat)
    row = dict(part="count", N=N, n=int(A.nrows), interval=[a, b], gap_lo=float(lam[i0] - lam[i0 - 1]), gap_hi=float(lam[i1] - lam[i1 - 1]),
               inside=inside, probes=32, degree=r.degree, count=r.count, stderr=r.stderr, suggested_nev_max=r.suggested_nev_max, runs=runs,
               count_seconds=[float(np.median(tc)), float(min(tc)), float(max(tc))], solve_seconds=ts, solve_pairs=int(e.converged),
               solve_iterations=int(e.iterations), solve_converged=done)
    print(json.dumps(row), flush=True)
    return [row]


def readme(rows):
    f = lambda t: "%.3f (%.3f, %.3f)" % tuple(t)
    lines = ["# Kernel polynomial method: the step with its sums, the count before the solve", "",
             "Written by `tools/kpm_probe.py`: MI355X, host clock round calls that end in a stream synchronise, warm, the configurations",
             "alternating, median (min, max) of the rounds.  TB/s: block streams of 8 n m bytes plus 12 bytes per stored entry, over the",
             "median time per step.", ""]
    for r in rows:
        if r["part"] == "step":
            tb = lambda s, ms: (s * 8.0 * r["n"] * r["m"] + 12.0 * r["nnz"]) / (ms * 1e-3) / 1e12
            lines += ["`GCGE_ChebMoments`, lap3d %d^3 (%s), m = %d, degree %d: %d steps per call, %d rounds.  Steps through the slot: %d fused, %d swept;"
                      % (r["N"], r["form"], r["m"], r["degree"], r["steps"], r["runs"], r["slot_fused"], r["slot_swept"]),
                      "through `cheb_step` (slot switched off): %d fused, %d swept.  Largest difference between the configurations' moments: %.2e n."
                      % (r["plain_fused"], r["plain_swept"], max(r["max_moment_difference_over_n"].values())), "",
                      "| step | sums | call ms | ms per step | block streams per step | TB/s |", "|---|---|---|---|---|---|"]
            for key, step, sums, streams in (("fused_slot", "fused", "`cheb_step_dots` (the pass, then `cheb_dots`)", 5),
                                             ("fused_noslot", "fused", "two `MultiVecLocalInnerProd` (`GCGE_NO_CHEB_STEP_DOTS=1`)", 6),
                                             ("sweep_slot", "product + sweep (`GCGE_CHEB_NO_FUSE=1`)", "`cheb_step_dots` (inside the sweep)", 6),
                                             ("sweep_noslot", "product + sweep", "two `MultiVecLocalInnerProd`", 9)):
                t = r[key + "_ms"]
                lines.append("| %s | %s | %s | %.3f | %d | %.2f |" % (step, sums, f(t), t[0] / r["steps"], streams, tb(streams, t[0] / r["steps"])))
            lines += ["", "(block streams without the slot: the step's 3 or 6, then out once for out . out and out and y for out . y: 3 more from HBM — the",
                      "product of a block with itself asks for every entry twice, and the second request is served by the caches.)", ""]
        if r["part"] == "count":
            lines += ["`eigenvalue_count` before `eigsh(interval=)`, lap3d %d^3 (n = %d), interval (%.6f, %.6f) between gaps of %.4f and %.4f, %d eigenvalues inside:"
                      % (r["N"], r["n"], r["interval"][0], r["interval"][1], r["gap_lo"], r["gap_hi"], r["inside"]), "",
                      "| | seconds | result |", "|---|---|---|",
                      "| `eigenvalue_count`, %d probes, degree %d, %d rounds | %s | count %.2f, stderr %.2f, suggested nev_max %d |"
                      % (r["probes"], r["degree"], r["runs"], f(r["count_seconds"]), r["count"], r["stderr"], r["suggested_nev_max"]),
                      "| `eigsh(interval=, nev_max=%d)`, one run | %.3f | %d pairs in %d iterations%s |"
                      % (r["suggested_nev_max"], r["solve_seconds"], r["solve_pairs"], r["solve_iterations"], "" if r["solve_converged"] else " (NoConvergence)"), ""]
    return "\n".join(lines) + "\n"


def main():
    argv = list(sys.argv[1:])
    opt = {"--out": os.path.join(ROOT, "profiles", "kpm"), "--runs": "10", "--only": None, "--part": None, "--to": None}
    for name in list(opt):
        if name in argv:
            i = argv.index(name)
            opt[name] = argv[i + 1]
            del argv[i:i + 2]
    runs = max(10, int(opt["--runs"]))
    if opt["--part"] is not None:
        rows = {"step": part_step, "count": part_count}[opt["--part"]](runs)
        with open(opt["--to"], "w") as f:
            json.dump(rows, f)
        return 0
    os.makedirs(opt["--out"], exist_ok=True)
    rows = []
    if opt["--only"] is not None and os.path.exists(os.path.join(opt["--out"], "results.json")):      # one part again: the other's rows stay
        with open(os.path.join(opt["--out"], "results.json")) as f:
            rows = [r for r in json.load(f) if r["part"] != opt["--only"]]
    for name, limit in PARTS:
        if opt["--only"] not in (None, name):
            continue
        to = os.path.join(opt["--out"], "part_%s.json" % name)
        print("part %s (limit %d s)" % (name, limit), flush=True)
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--part", name, "--runs", str(runs), "--to", to])
        if r.returncode != 0:
            print("part %s ended with status %d: no further part is started" % (name, r.returncode), flush=True)
            return 1
        with open(to) as f:
            rows += json.load(f)
        os.remove(to)
        with open(os.path.join(opt["--out"], "results.json"), "w") as f:
            json.dump(rows, f, indent=1)
        with open(os.path.join(opt["--out"], "README.md"), "w") as f:
            f.write(readme(rows))
    return 0


if __name__ == "__main__":
    sys.exit(main())
