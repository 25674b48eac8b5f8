"""Time of gcge_hip_pcg_shift (csrc/hip/pcg_sweeps.hip) against the slot path it replaces in GCGE_PCGSolveDeflated.

    python tools/pcg_shift_probe.py [--out DIR] [--runs R] [--rows N]

On a window of m columns both compute  w -= q diag(shift) ;  pw_j = p_j . w_j  and end with the m sums on the host:
    sweep   one launch of the sweep, the fixed-order reduction, one copy to the host     3 reads + 1 write   (q == p: 2 + 1)
    slots   gcge_hip_axpby on one column, m times, then gcge_hip_coldots over the window   3 reads + 1 write + 2 reads, m + 1 launches
            and the copy of the sums (what MultiVecAxpby and MultiVecLocalInnerProd('D') of the HIP table do)
at n = 2^24 rows and m = 8, 64 — row-major blocks of leading dimension m, all columns flagged.  Each m is one step: a child process
of this file (--step M) under its own `timeout`; a step that fails ends the run.  A step warms both paths up, then times R >= 20
rounds, the two paths (and the sweep with q == p) alternating inside a round, each with the host clock round a call that ends in a
stream synchronise; medians are reported.  The two paths' w and sums are compared once on the same input before the timing.
Writes DIR/results.json and DIR/results.md (default DIR: profiles/pcg_shift; README.md there quotes them)."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = [(8, 300), (64, 600)]


def run_step(m, n, runs):
    import numpy as np
    import torch
    from gcge_amd import HipBackend
    hip = HipBackend()
    g, sp = hip.g, hip.g.gcge_hip_stream()
    gen = torch.Generator(device="cuda").manual_seed(5)
    P, Q, W0 = (torch.rand((n, m), dtype=torch.float64, device="cuda", generator=gen) - 0.5 for _ in range(3))
    W = W0.clone()
    sums = torch.empty(m, dtype=torch.float64, device="cuda")
    shift = np.linspace(0.25, 1.75, m) * 1e-3                          # (small: w stays of order one over all the rounds)
    flag, pw = np.ones(m, dtype=np.int32), np.zeros(m)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    torch.cuda.synchronize()

    def sweep(q):
        rc = g.gcge_hip_pcg_shift(n, P.data_ptr(), m, q.data_ptr(), m, W.data_ptr(), m, m, ptr(shift), ptr(flag), ptr(pw), sp)
        assert rc == 0, rc
        return pw.copy()

    def slots(q):
        for j in range(m):
            rc = g.gcge_hip_axpby(n, -float(shift[j]), q.data_ptr() + 8 * j, m, 1.0, W.data_ptr() + 8 * j, m, 1, sp)
            assert rc == 0, rc
        rc = g.gcge_hip_coldots(n, P.data_ptr(), m, W.data_ptr(), m, m, sums.data_ptr(), sp)
        assert rc == 0, rc
        hip.sync()
        return sums.cpu().numpy()

    # the same input through both paths: w bit for bit (one fused multiply-add per entry either way), the sums to summation order
    a = sweep(Q)
    wa = W.clone()
    W.copy_(W0)
    torch.cuda.synchronize()
    b = slots(Q)
    same_w = bool(torch.equal(wa, W))
    W.copy_(W0)
    torch.cuda.synchronize()
    del wa
    paths = [("sweep", lambda: sweep(Q)), ("slots", lambda: slots(Q)), ("sweep_q_is_p", lambda: sweep(P)), ("slots_q_is_p", lambda: slots(P))]
    for _, f in paths:
        f()
    hip.sync()
    ts = {name: [] for name, _ in paths}
    for _ in range(runs):
        for name, f in paths:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            hip.sync()
            ts[name].append((time.perf_counter() - t0) * 1e3)
    row = {"n": n, "m": m, "runs": runs, "w_bit_for_bit": same_w, "max_rel_difference_of_sums": float(np.max(np.abs(a - b) / np.abs(b)))}
    for name, _ in paths:
        row[name + "_ms"] = [float(np.median(ts[name])), float(min(ts[name])), float(max(ts[name]))]
    print(json.dumps(row), flush=True)
    return [row]


def readme(rows):
    tb = lambda streams, r, ms: streams * 8.0 * r["n"] * r["m"] / (ms * 1e-3) / 1e12
    lines = ["# gcge_hip_pcg_shift against the slot path it replaces", "",
             "Written by `tools/pcg_shift_probe.py`: MI355X, host clock round calls that end in a stream synchronise, warm, the paths",
             "alternating, median (min, max) of the rounds.  TB/s: the block streams the path needs (sweep 4, slots 6; q == p: 3 and 6, the",
             "slots read p twice there) of 8 n m bytes each over the median.", "",
             "| n | m | runs | sweep ms | TB/s | slots ms | TB/s | slots / sweep | sweep, q == p ms | TB/s | slots, q == p ms | w bit for bit | sums differ by |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    f = lambda t: "%.3f (%.3f, %.3f)" % tuple(t)
    for r in rows:
        s, o, sp, op = r["sweep_ms"], r["slots_ms"], r["sweep_q_is_p_ms"], r["slots_q_is_p_ms"]
        lines.append("| %d | %d | %d | %s | %.2f | %s | %.2f | %.2f | %s | %.2f | %s | %s | %.1e |" % (
            r["n"], r["m"], r["runs"], f(s), tb(4, r, s[0]), f(o), tb(6, r, o[0]), o[0] / s[0], f(sp), tb(3, r, sp[0]), f(op),
            "yes" if r["w_bit_for_bit"] else "NO", r["max_rel_difference_of_sums"]))
    return "\n".join(lines) + "\n"


def main():
    argv = list(sys.argv[1:])
    opt = {"--out": os.path.join(ROOT, "profiles", "pcg_shift"), "--runs": "20", "--rows": str(1 << 24), "--step": None, "--part": None}
    for name in list(opt):
        if name in argv:
            i = argv.index(name)
            opt[name] = argv[i + 1]
            del argv[i:i + 2]
    runs, n = max(20, int(opt["--runs"])), int(opt["--rows"])
    if opt["--step"] is not None:
        rows = run_step(int(opt["--step"]), n, runs)
        with open(opt["--part"], "w") as f:
            json.dump(rows, f)
        return 0
    os.makedirs(opt["--out"], exist_ok=True)
    rows = []
    for m, limit in STEPS:
        part = os.path.join(opt["--out"], "step_%d.json" % m)
        print("step m = %d (limit %d s)" % (m, limit), flush=True)
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", str(m), "--runs", str(runs),
                            "--rows", str(n), "--part", part])
        if r.returncode != 0:
            print("step m = %d ended with status %d: no further step is started" % (m, r.returncode), flush=True)
            return 1
        with open(part) as f:
            rows += json.load(f)
        os.remove(part)
        with open(os.path.join(opt["--out"], "results.json"), "w") as f:
            json.dump(rows, f, indent=1)
        with open(os.path.join(opt["--out"], "results.md"), "w") as f:
            f.write(readme(rows))
    return 0


if __name__ == "__main__":
    sys.exit(main())
