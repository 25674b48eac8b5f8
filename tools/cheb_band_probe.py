"""Times of the band-pass Chebyshev filter's pieces (gcge_hip_cheb_accum in csrc/hip/cheb_sweeps.hip, GCGE_ChebBandFilter,
eigsh(interval=...)).

    python tools/cheb_band_probe.py [--out DIR] [--runs R] [--only accum|filter|solve]

  accum   gcge_hip_cheb_accum in its three forms (two terms onto acc, init, one term) at n = 2^24 rows, m = 8 and 64, row-major blocks
          of leading dimension m, against gcge_hip_pcg_shift on the same blocks (both read three blocks and write one) and against
          the two gcge_hip_axpby calls the two-term form replaces (6 streams against 4: the count says 1.5).  The two-term median must
          be at most 1.10 x the shift's (the probe's exit status, the criterion tools/cheb_probe.py has for cheb_sweep); the ratio to
          the two Axpby calls is recorded.
  filter  one GCGE_ChebBandFilter of degree 60 on lap3d 256^3 x 64 columns, interval [1.0, 1.55] inside the bounds [-0.6, 12.6]:
          {fused step, GCGE_CHEB_NO_FUSE=1} x {cheb_accum slot, GCGE_NO_CHEB_ACCUM=1}; ms per step (the filter's time / 60: the first
          step is never fused and the last copy of acc into x is inside) and TB/s on 5 / 6 / 8 / 9 block streams per step plus the
          matrix (12 bytes per stored entry).  x is drawn again before every filter, outside the clock.
  solve   one eigsh(interval=(a, b)) on lap3d 128^3: a and b in the middle of the gaps round the eigenvalues 12 .. 48 of the closed
          form (37 inside, 11 below), nev_max = 74, the exact bounds [0, 12], the driver's own degree; seconds, outer iterations,
          filter steps.  No comparison with GCG: the two do not compute the same thing.
Each part is a child process of this file under its own `timeout`; a part that fails ends the run.  A part warms its paths up, then
times R >= 20 rounds (the solve: one run after a warm-up of one iteration), the paths alternating inside a round, each with the host
clock round a call that ends in a stream synchronise; median (min, max).  Writes DIR/results.json and DIR/results.md (default DIR:
profiles/chfsi_band; README.md there quotes them)."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PARTS = [("accum", 600), ("filter", 900), ("solve", 900)]
DEGREE = 60


def timed(paths, runs, sync, before=None):
    """median (min, max) in ms of every path over `runs` rounds, the paths alternating inside a round; `before` runs outside the clock"""
    import numpy as np
    for _, f in paths:
        if before is not None:
            before()
        f()
    sync()
    ts = {name: [] for name, _ in paths}
    for _ in range(runs):
        for name, f in paths:
            if before is not None:
                before()
            sync()
            t0 = time.perf_counter()
            f()
            sync()
            ts[name].append((time.perf_counter() - t0) * 1e3)
    return {name: [float(np.median(v)), float(min(v)), float(max(v))] for name, v in ts.items()}


def part_accum(runs):
    import numpy as np
    import torch
    from gcge_amd import HipBackend
    hip = HipBackend()
    g, sp, n, rows = hip.g, hip.g.gcge_hip_stream(), 1 << 24, []
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    for m in (8, 64):
        gen = torch.Generator(device="cuda").manual_seed(5)
        P, Q, W = (torch.rand((n, m), dtype=torch.float64, device="cuda", generator=gen) - 0.5 for _ in range(3))
        shift, flag, pw = np.linspace(0.25, 1.75, m) * 1e-3, np.ones(m, dtype=np.int32), np.zeros(m)
        torch.cuda.synchronize()

        def shift_sweep():
            assert g.gcge_hip_pcg_shift(n, P.data_ptr(), m, Q.data_ptr(), m, W.data_ptr(), m, m, ptr(shift), ptr(flag), ptr(pw), sp) == 0

        def accum(init, two):
            # (small coefficients: W stays of order one over all the rounds)
            assert g.gcge_hip_cheb_accum(n, W.data_ptr(), m, P.data_ptr(), m, 1e-3, Q.data_ptr() if two else None, m, -1e-3, m, init, sp) == 0

        def two_axpby():
            assert g.gcge_hip_axpby(n, 1e-3, P.data_ptr(), m, 1.0, W.data_ptr(), m, m, sp) == 0
            assert g.gcge_hip_axpby(n, -1e-3, Q.data_ptr(), m, 1.0, W.data_ptr(), m, m, sp) == 0

        t = timed([("pcg_shift", shift_sweep), ("accum_two", lambda: accum(0, True)), ("two_axpby", two_axpby), ("accum_init", lambda: accum(1, True)),
                   ("accum_one", lambda: accum(0, False))], runs, hip.sync)
        rows.append(dict(part="accum", n=n, m=m, runs=runs, **{k + "_ms": v for k, v in t.items()}))
        print(json.dumps(rows[-1]), flush=True)
        del P, Q, W
    return rows


def part_filter(runs):
    from gcge_amd import HipBackend
    from gcge_amd.lib import cheb_accum_stats, cheb_stats, make_problem
    hip = HipBackend()
    hip.set_random_mode(1, 20240601)          # device generator: x is drawn again before every filter
    N, m = 256, 64
    a, b, lmin, lmax = 1.0, 1.55, -0.6, 12.6
    A, _ = make_problem("lap3d", N)
    mat = hip.matrix(A)
    n, nnz = A.nrows, int(A.nnz)
    x, w1, w2, acc = (hip.ops.mv_create(m, mat) for _ in range(4))

    def draw():
        hip.ops.set_random(x, 0, m)

    def run(no_fuse, no_slot):
        def f():
            for name, on in (("GCGE_CHEB_NO_FUSE", no_fuse), ("GCGE_NO_CHEB_ACCUM", no_slot)):
                if on:
                    os.environ[name] = "1"
            try:
                assert hip.h.GCGE_ChebBandFilter(mat, x, 0, m, DEGREE, a, b, lmin, lmax, w1, w2, acc, hip.ops_handle) == 0
            finally:
                for name in ("GCGE_CHEB_NO_FUSE", "GCGE_NO_CHEB_ACCUM"):
                    os.environ.pop(name, None)
        return f

    s0, a0 = cheb_stats(), cheb_accum_stats()
    t = timed([("fused_slot", run(False, False)), ("fused_axpby", run(False, True)), ("sweep_slot", run(True, False)),
               ("sweep_axpby", run(True, True))], runs, hip.sync, before=draw)
    s1, a1 = cheb_stats(), cheb_accum_stats()
    row = dict(part="filter", N=N, n=n, nnz=nnz, m=m, degree=DEGREE, interval=[a, b], bounds=[lmin, lmax], runs=runs,
               form=hip.g.gcge_hip_mat_spmm_form(mat).decode(), steps_fused=s1[0] - s0[0], steps_swept=s1[1] - s0[1],
               sums_two=a1[0] - a0[0], sums_one=a1[1] - a0[1], **{k + "_ms": v for k, v in t.items()})
    print(json.dumps(row), flush=True)
    for v in (x, w1, w2, acc):
        hip.ops.mv_destroy(v, m)
    hip.free_matrix(mat)
    return [row]


def part_solve(runs):
    import numpy as np
    import torch
    from gcge_amd import HipBackend, NoConvergence, eigsh
    from gcge_amd.lib import cheb_accum_stats, cheb_stats, csr_arrays, make_problem
    hip = HipBackend()
    hip.set_random_mode(1, 20240601)          # device generator: the rand() calls of the default mode would dominate at this n
    N, first, count = 128, 11, 37
    c = 2.0 * np.cos(np.arange(1, N + 1) * np.pi / (N + 1))
    lam = np.sort((6.0 - c[:, None, None] - c[None, :, None] - c[None, None, :]).ravel())
    a, b = float(0.5 * (lam[first - 1] + lam[first])), float(0.5 * (lam[first + count - 1] + lam[first + count]))
    assert np.count_nonzero((lam >= a) & (lam <= b)) == count
    gaps = [float(lam[first] - lam[first - 1]), float(lam[first + count] - lam[first + count - 1])]
    A, _ = make_problem("lap3d", N)
    rp, ci, va = csr_arrays(A)
    mat = hip.matrix_from_device(torch.from_numpy(rp).cuda(), torch.from_numpy(ci).cuda(), torch.from_numpy(va).cuda())
    kw = dict(interval=(a, b), nev_max=2 * count, method="chebyshev", lower_bound=0.0, upper_bound=12.0, backend=hip)

    def solve(**more):
        hip.sync()
        t0, s0, a0 = time.perf_counter(), cheb_stats(), cheb_accum_stats()
        try:
            r, done = eigsh(mat, **kw, **more), True
        except NoConvergence as e:
            r, done = e.result, False
        hip.sync()
        return r, done, time.perf_counter() - t0, sum(cheb_stats()[:2]) - sum(s0[:2]), cheb_accum_stats()[0] - a0[0]

    solve(maxiter=1)                                                              # warm-up: first launches, pools
    r, done, t, steps, sums = solve(maxiter=40)
    got = r.eigenvalues.cpu().numpy()
    err = float(np.max(np.abs(got - lam[first:first + count]) / lam[first:first + count])) if r.converged == count else None
    row = dict(part="solve", N=N, n=int(A.nrows), interval=[a, b], gaps=gaps, inside=count, below=first, nev_max=2 * count, bounds=[0.0, 12.0],
               maxiter=40, finished=done, seconds=t, solver_seconds=r.seconds, iterations=r.iterations, converged=r.converged, filter_steps=steps,
               two_term_sums=sums, degree=steps // (r.iterations + 1), max_relative_eigenvalue_error=err,
               max_residual_norm=float(r.residual_norms.max()) if r.converged else None)
    print(json.dumps(row), flush=True)
    hip.free_matrix(mat)
    return [row]


def readme(rows):
    f = lambda t: "%.3f (%.3f, %.3f)" % tuple(t)
    lines = ["# Band-pass Chebyshev filter: sums, filter, solve", "",
             "Written by `tools/cheb_band_probe.py`: MI355X, host clock round calls that end in a stream synchronise, warm, the paths alternating,",
             "median (min, max) of the rounds.  TB/s: block streams of 8 n m bytes (plus 12 bytes per stored entry for a filter step) over the median.", ""]
    ac = [r for r in rows if r["part"] == "accum"]
    if ac:
        lines += ["| n | m | runs | pcg_shift ms | TB/s | cheb_accum (two terms) ms | TB/s | accum / shift | two axpby ms | TB/s | two axpby / accum | init ms | TB/s | one term ms | TB/s |",
                  "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
        for r in ac:
            tb = lambda s, ms: s * 8.0 * r["n"] * r["m"] / (ms * 1e-3) / 1e12
            s, a, x, i, o = r["pcg_shift_ms"], r["accum_two_ms"], r["two_axpby_ms"], r["accum_init_ms"], r["accum_one_ms"]
            lines.append("| %d | %d | %d | %s | %.2f | %s | %.2f | %.3f | %s | %.2f | %.3f | %s | %.2f | %s | %.2f |" % (
                r["n"], r["m"], r["runs"], f(s), tb(4, s[0]), f(a), tb(4, a[0]), a[0] / s[0], f(x), tb(6, x[0]), x[0] / a[0], f(i), tb(3, i[0]), f(o), tb(3, o[0])))
        lines.append("")
    for r in rows:
        if r["part"] == "filter":
            p = r["degree"]
            tb = lambda s, ms: (s * 8.0 * r["n"] * r["m"] + 12.0 * r["nnz"]) / (ms / p * 1e-3) / 1e12
            lines += ["lap3d %d^3 (%s), m = %d, degree %d, interval [%g, %g] in [%g, %g], %d rounds; steps fused / swept %d / %d, sums of two / one %d / %d:" % (
                          r["N"], r["form"], r["m"], p, r["interval"][0], r["interval"][1], r["bounds"][0], r["bounds"][1], r["runs"], r["steps_fused"],
                          r["steps_swept"], r["sums_two"], r["sums_one"]), "",
                      "| step | sums | filter ms | ms per step | block streams per step | TB/s |", "|---|---|---|---|---|---|"]
            for key, step, sums, streams in (("fused_slot", "fused", "cheb_accum", 5), ("fused_axpby", "fused", "two MultiVecAxpby", 6),
                                             ("sweep_slot", "product + sweep", "cheb_accum", 8), ("sweep_axpby", "product + sweep", "two MultiVecAxpby", 9)):
                t = r[key + "_ms"]
                lines.append("| %s | %s | %s | %.3f | %d | %.2f |" % (step, sums, f(t), t[0] / p, streams, tb(streams, t[0])))
            lines.append("")
        if r["part"] == "solve":
            lines += ["| lap3d %d^3 | interval | gaps at the ends | inside / below | nev_max | degree | seconds | outer iterations | filter steps | pairs | max eigenvalue error |" % r["N"],
                      "|---|---|---|---|---|---|---|---|---|---|---|",
                      "| eigsh(interval=) | [%.6f, %.6f] | %.2e, %.2e | %d / %d | %d | %d | %.3f | %d%s | %d | %d | %s |" % (
                          r["interval"][0], r["interval"][1], r["gaps"][0], r["gaps"][1], r["inside"], r["below"], r["nev_max"], r["degree"], r["seconds"],
                          r["iterations"], "" if r["finished"] else " (NOT converged at maxiter %d)" % r["maxiter"], r["filter_steps"], r["converged"],
                          "%.1e" % r["max_relative_eigenvalue_error"] if r["max_relative_eigenvalue_error"] is not None else "-"), ""]
    return "\n".join(lines) + "\n"


def main():
    argv = list(sys.argv[1:])
    opt = {"--out": os.path.join(ROOT, "profiles", "chfsi_band"), "--runs": "20", "--only": None, "--part": None, "--to": None}
    for name in list(opt):
        if name in argv:
            i = argv.index(name)
            opt[name] = argv[i + 1]
            del argv[i:i + 2]
    runs = max(20, int(opt["--runs"]))
    if opt["--part"] is not None:
        rows = {"accum": part_accum, "filter": part_filter, "solve": part_solve}[opt["--part"]](runs)
        with open(opt["--to"], "w") as f:
            json.dump(rows, f)
        return 0
    os.makedirs(opt["--out"], exist_ok=True)
    rows = []
    if opt["--only"] is not None and os.path.exists(os.path.join(opt["--out"], "results.json")):      # one part again: the others' rows stay
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
        with open(os.path.join(opt["--out"], "results.md"), "w") as f:
            f.write(readme(rows))
    slow = [r for r in rows if r["part"] == "accum" and r["accum_two_ms"][0] > 1.10 * r["pcg_shift_ms"][0]]
    for r in slow:
        print("cheb_accum at m = %d: median %.3f ms is above 1.10 x pcg_shift's %.3f ms" % (r["m"], r["accum_two_ms"][0], r["pcg_shift_ms"][0]), flush=True)
    return 2 if slow else 0


if __name__ == "__main__":
    sys.exit(main())
