"""Times of the Chebyshev filter's pieces (csrc/hip/cheb_sweeps.hip, gcge_hip_cheb_step_mv, eigsh(method="chebyshev")).

    python tools/cheb_probe.py [--out DIR] [--runs R] [--only sweep|step|solve]

  sweep   gcge_hip_cheb_sweep against gcge_hip_pcg_shift (q apart) at n = 2^24 rows, m = 8 and 64, row-major blocks of leading dimension
          m: both read three blocks and write one.  The sweep's median must be at most 1.10 x the shift's (the probe's exit status).
          Also the first step's sweep (beta = 0: 2 reads + 1 write).
  step    one step on lap3d 256^3, m = 64: the fused path and product + sweep (GCGE_CHEB_NO_FUSE=1), ms and TB/s on 3 and 6 block streams
          plus the matrix (12 bytes per stored entry).
  solve   lap3d 128^3, k = 50, nev_max = 128: eigsh(method="chebyshev", degree=20) against eigsh(method="gcg") with a kept hierarchy
          (levels 6, block 16), cold, and warm from the previous vectors after a 1 % perturbation of the diagonal through
          matrix_update_values (GCG: plus Hierarchy.refresh()).  Seconds, outer iterations, filter steps (= products per filtered column).
Each part is a child process of this file under its own `timeout`; a part that fails ends the run.  A part warms its paths up, then
times R >= 20 rounds, the paths alternating inside a round, each with the host clock round a call that ends in a stream synchronise;
median (min, max).  Writes DIR/results.json and DIR/results.md (default DIR: profiles/chfsi; README.md there quotes them)."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PARTS = [("sweep", 600), ("step", 600), ("solve", 900)]


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


def part_sweep(runs):
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

        def cheb(beta):
            # (alpha = 1, c and beta small: out stays of order one over all the rounds)
            assert g.gcge_hip_cheb_sweep(n, W.data_ptr(), m, P.data_ptr(), m, Q.data_ptr() if beta else None, m, m, 1.0, 1e-3, beta, sp) == 0

        t = timed([("pcg_shift", shift_sweep), ("cheb_sweep", lambda: cheb(1e-3)), ("cheb_sweep_first", lambda: cheb(0.0))], runs, hip.sync)
        rows.append(dict(part="sweep", n=n, m=m, runs=runs, **{k + "_ms": v for k, v in t.items()}))
        print(json.dumps(rows[-1]), flush=True)
        del P, Q, W
    return rows


def part_step(runs):
    import numpy as np
    from gcge_amd import HipBackend
    from gcge_amd.lib import cheb_stats, make_problem
    hip = HipBackend()
    N, m = 256, 64
    A, _ = make_problem("lap3d", N)
    mat = hip.matrix(A)
    n, nnz = A.nrows, int(A.nnz)
    blocks = [hip.ops.mv_create(m, mat) for _ in range(3)]
    for b in blocks:
        hip.ops.set_random(b, 0, m)

    def step():
        # alpha (A - c) with the spectrum of (A - 6) / 6 inside [-1, 1]: the iterates stay of order one as the blocks rotate
        assert hip.g.gcge_hip_cheb_step_mv(mat, blocks[1], 0, blocks[0], 0, blocks[2], 0, m, 1.0 / 6.0, 6.0, 0.5) == 0
        blocks.append(blocks.pop(0))

    def unfused():
        os.environ["GCGE_CHEB_NO_FUSE"] = "1"
        try:
            step()
        finally:
            del os.environ["GCGE_CHEB_NO_FUSE"]

    s0 = cheb_stats()
    t = timed([("fused", step), ("product_sweep", unfused)], runs, hip.sync)
    s1 = cheb_stats()
    row = dict(part="step", N=N, n=n, nnz=nnz, m=m, runs=runs, form=hip.g.gcge_hip_mat_spmm_form(mat).decode(),
               recompute_pays=int(hip.g.gcge_hip_cg_recompute_pays(mat)), steps_fused=s1[0] - s0[0], steps_swept=s1[1] - s0[1],
               **{k + "_ms": v for k, v in t.items()})
    print(json.dumps(row), flush=True)
    return [row]


def part_solve(runs):
    import numpy as np
    import torch
    from gcge_amd import HipBackend, NoConvergence, eigsh
    from gcge_amd.lib import cheb_stats, csr_arrays, make_problem
    hip = HipBackend()
    hip.set_random_mode(1, 20240601)          # device generator: the rand() calls of the default mode would dominate both methods at this n
    N, k, nev_max = 128, 50, 128
    A, _ = make_problem("lap3d", N)
    rp, ci, va = csr_arrays(A)
    crow, col = torch.from_numpy(rp).cuda(), torch.from_numpy(ci).cuda()
    diag = ci == np.repeat(np.arange(A.nrows), np.diff(rp))
    va1 = va.copy()
    va1[diag] *= 1.0 + 0.01 * (np.random.default_rng(7).random(int(diag.sum())) - 0.5)
    rows = []

    def solve(m, **kw):
        hip.sync()
        t0, s0 = time.perf_counter(), cheb_stats()
        try:
            r = eigsh(m, k, nev_max=nev_max, backend=hip, **kw)
        except NoConvergence as e:
            r = e.result
        hip.sync()
        return r, time.perf_counter() - t0, sum(cheb_stats()[:2]) - sum(s0[:2])

    for method in ("chebyshev", "gcg"):
        m = hip.matrix_from_device(crow, col, torch.from_numpy(va).cuda(), updatable=True)
        h = hip.multigrid(m, levels=6, block_size=16) if method == "gcg" else None
        kw = dict(method="chebyshev", degree=20) if method == "chebyshev" else dict(amg=h)
        solve(m, **kw)                                                            # warm-up: first launches, pools
        cold, tc, sc = solve(m, **kw)
        t0 = time.perf_counter()
        assert hip.matrix_update_values(m, torch.from_numpy(va1).cuda())
        if h is not None:
            assert h.refresh()
        hip.sync()
        tu = time.perf_counter() - t0
        warm, tw, sw = solve(m, X0=cold.eigenvectors, **kw)
        rows.append(dict(part="solve", method=method, N=N, k=k, nev_max=nev_max,
                         cold=dict(seconds=tc, solver_seconds=cold.seconds, iterations=cold.iterations, converged=cold.converged, filter_steps=sc),
                         update_and_refresh_seconds=tu,
                         warm=dict(seconds=tw, solver_seconds=warm.seconds, iterations=warm.iterations, converged=warm.converged, filter_steps=sw),
                         lambda_1=float(warm.eigenvalues[0]), lambda_k=float(warm.eigenvalues[-1])))
        print(json.dumps(rows[-1]), flush=True)
        if h is not None:
            h.close()
        hip.free_matrix(m)
    return rows


def readme(rows):
    f = lambda t: "%.3f (%.3f, %.3f)" % tuple(t)
    lines = ["# Chebyshev filter: sweep, step, solve", "",
             "Written by `tools/cheb_probe.py`: MI355X, host clock round calls that end in a stream synchronise, warm, the paths alternating,",
             "median (min, max) of the rounds.  TB/s: block streams of 8 n m bytes (plus 12 bytes per stored entry for a step) over the median.", ""]
    sw = [r for r in rows if r["part"] == "sweep"]
    if sw:
        lines += ["| n | m | runs | pcg_shift ms | TB/s | cheb_sweep ms | TB/s | cheb / shift | first step (beta = 0) ms | TB/s |", "|---|---|---|---|---|---|---|---|---|---|"]
        for r in sw:
            tb = lambda s, ms: s * 8.0 * r["n"] * r["m"] / (ms * 1e-3) / 1e12
            a, b, c = r["pcg_shift_ms"], r["cheb_sweep_ms"], r["cheb_sweep_first_ms"]
            lines.append("| %d | %d | %d | %s | %.2f | %s | %.2f | %.3f | %s | %.2f |" % (r["n"], r["m"], r["runs"], f(a), tb(4, a[0]), f(b), tb(4, b[0]),
                                                                                      b[0] / a[0], f(c), tb(3, c[0])))
        lines.append("")
    for r in rows:
        if r["part"] == "step":
            tb = lambda s, ms: (s * 8.0 * r["n"] * r["m"] + 12.0 * r["nnz"]) / (ms * 1e-3) / 1e12
            a, b = r["fused_ms"], r["product_sweep_ms"]
            lines += ["| matrix | form | m | fused ms | TB/s (3 streams) | product + sweep ms | TB/s (6 streams) | steps fused / swept |", "|---|---|---|---|---|---|---|---|",
                      "| lap3d %d^3 | %s | %d | %s | %.2f | %s | %.2f | %d / %d |" % (r["N"], r["form"], r["m"], f(a), tb(3, a[0]), f(b), tb(6, b[0]),
                                                                                 r["steps_fused"], r["steps_swept"]), ""]
    so = [r for r in rows if r["part"] == "solve"]
    if so:
        lines += ["| lap3d %d^3, k = %d, nev_max = %d | cold s | outer iterations | filter steps | update (+ refresh) s | warm s | outer iterations | filter steps |" %
                  (so[0]["N"], so[0]["k"], so[0]["nev_max"]), "|---|---|---|---|---|---|---|---|"]
        for r in so:
            c, w = r["cold"], r["warm"]
            lines.append("| %s | %.3f | %d (%d of %d) | %d | %.3f | %.3f | %d (%d of %d) | %d |" % (
                r["method"], c["seconds"], c["iterations"], c["converged"], r["k"], c["filter_steps"], r["update_and_refresh_seconds"], w["seconds"],
                w["iterations"], w["converged"], r["k"], w["filter_steps"]))
    return "\n".join(lines) + "\n"


def main():
    argv = list(sys.argv[1:])
    opt = {"--out": os.path.join(ROOT, "profiles", "chfsi"), "--runs": "20", "--only": None, "--part": None, "--to": None}
    for name in list(opt):
        if name in argv:
            i = argv.index(name)
            opt[name] = argv[i + 1]
            del argv[i:i + 2]
    runs = max(20, int(opt["--runs"]))
    if opt["--part"] is not None:
        rows = {"sweep": part_sweep, "step": part_step, "solve": part_solve}[opt["--part"]](runs)
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
    slow = [r for r in rows if r["part"] == "sweep" and r["cheb_sweep_ms"][0] > 1.10 * r["pcg_shift_ms"][0]]
    for r in slow:
        print("cheb_sweep at m = %d: median %.3f ms is above 1.10 x pcg_shift's %.3f ms" % (r["m"], r["cheb_sweep_ms"][0], r["pcg_shift_ms"][0]), flush=True)
    return 2 if slow else 0


if __name__ == "__main__":
    sys.exit(main())
