"""Time of gcge_hip_csr_sample_outer (csrc/hip/sample_outer.hip) against its byte model.

    python tools/sample_outer_bench.py [--out DIR] [--runs R]

Shapes: the 7-point Laplacian at 128^3 and 256^3 with k = 16, 64, 128; the SiO2-like matrix make_problem("sio2", 96, K=350, R0=2.0,
R1=5.0) (BASELINE config 5's atom density on a 96^3 grid) with k = 64.  U = V random, weights given, as the eigenvalue gradient
calls it.  Each matrix is one step: a child process of this file (--step NAME) under its own `timeout`, one after the other; a step
that fails ends the run (its rows come back through DIR/step_NAME.json).  A step warms every shape up, then times R >= 20 launches
one by one with events on the library's stream and reports the median.  At 128^3, k = 16 the torch expression (U[rows] * V[cols]).sum(1) is timed beside it the same way.

Bytes a launch has to move:  8 n k (U once) + V + 4 (n + 1 + nnz) (structure) + 8 nnz (output), with V counted
    per entry:  8 nnz k   what the kernel requests; on a banded pattern most of it is served by the caches
    per row:    8 n k     every row of V from memory once
and the rate of each against the read-plus-write stream rate of this chip, 5.5 TB/s (tools/seg_bench.hip, README round 4).
Writes DIR/results.json and DIR/results.md (default DIR: profiles/sample_outer; README.md there quotes them and says what the
numbers mean)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STREAM_TBPS = 5.5
STEPS = [("lap128", 600), ("lap256", 900), ("sio2_96", 900)]


def run_step(name, runs):
    import numpy as np
    import torch
    from gcge_amd import HipBackend, make_problem
    from gcge_amd.lib import csr_arrays
    if name.startswith("lap"):
        A = make_problem("lap3d", int(name[3:]))[0]
        ks, what = [16, 64, 128], "7-point Laplacian %s^3" % name[3:]
    else:
        A = make_problem("sio2", 96, K=350, R0=2.0, R1=5.0)[0]
        ks, what = [64], "SiO2-like, 96^3 grid, 350 atoms"
    hip = HipBackend()
    rp, ci, _ = csr_arrays(A)
    n, nnz = int(A.nrows), int(ci.size)
    crow, col = torch.from_numpy(np.ascontiguousarray(rp, dtype=np.int32)).cuda(), torch.from_numpy(np.ascontiguousarray(ci, dtype=np.int32)).cuda()
    sp = hip.g.gcge_hip_stream()
    stream = torch.cuda.ExternalStream(sp) if sp else torch.cuda.default_stream()
    out = torch.empty(nnz, dtype=torch.float64, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(5)

    def median_ms(launch, on):
        for _ in range(3):
            launch()
        torch.cuda.synchronize()
        ts = []
        for _ in range(runs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(on)
            launch()
            b.record(on)
            b.synchronize()
            ts.append(a.elapsed_time(b))
        return float(np.median(ts)), float(min(ts)), float(max(ts))

    rows = []
    for k in ks:
        U = torch.rand((n, k), dtype=torch.float64, device="cuda", generator=gen) - 0.5
        w = torch.rand(k, dtype=torch.float64, device="cuda", generator=gen) + 0.5
        torch.cuda.synchronize()

        def launch():
            rc = hip.g.gcge_hip_csr_sample_outer(n, crow.data_ptr(), col.data_ptr(), U.data_ptr(), k, U.data_ptr(), k, k, w.data_ptr(), 1.0,
                                                 out.data_ptr(), sp)
            if rc != 0:
                raise RuntimeError("gcge_hip_csr_sample_outer rc=%d" % rc)
        med, lo, hi = median_ms(launch, stream)
        fixed = 8.0 * n * k + 4.0 * (n + 1 + nnz) + 8.0 * nnz
        row = {"matrix": what, "n": n, "nnz": nnz, "k": k, "runs": runs, "median_ms": med, "min_ms": lo, "max_ms": hi,
               "bytes_v_per_entry": fixed + 8.0 * nnz * k, "bytes_v_per_row": fixed + 8.0 * n * k}
        if name == "lap128" and k == 16:
            r_of = torch.repeat_interleave(torch.arange(n, device="cuda"), (crow[1:] - crow[:-1]).long())
            cl = col.long()
            ref = hip.sample_outer(crow, col, U, U, weights=w)
            got = ((U * w)[r_of] * U[cl]).sum(1)
            row["max_abs_difference_from_torch"] = float((ref - got).abs().max())
            del ref, got
            row["torch_median_ms"] = median_ms(lambda: (U[r_of] * U[cl]).sum(1), torch.cuda.current_stream())[0]
            del r_of, cl
        rows.append(row)
        print(json.dumps(row), flush=True)
        del U
    return rows


def readme(rows):
    tb = lambda nbytes, ms: nbytes / (ms * 1e-3) / 1e12
    lines = ["# gcge_hip_csr_sample_outer against its byte model", "",
             "Written by `tools/sample_outer_bench.py`: MI355X, events on the library's stream, warm, median of the runs.",
             "V per entry: 8 n k + 8 nnz k + 4 (n + 1 + nnz) + 8 nnz bytes, what the kernel requests.  V per row: 8 nnz k replaced by",
             "8 n k, every row of V from memory once.  Share: of the %.1f TB/s read-plus-write stream rate (tools/seg_bench.hip)." % STREAM_TBPS, "",
             "| matrix | n | nnz | k | runs | median ms (min, max) | V per entry TB/s | V per row TB/s | share of stream rate, V per row |",
             "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        e, o = tb(r["bytes_v_per_entry"], r["median_ms"]), tb(r["bytes_v_per_row"], r["median_ms"])
        lines.append("| %s | %d | %d | %d | %d | %.3f (%.3f, %.3f) | %.2f | %.2f | %.2f |" % (r["matrix"], r["n"], r["nnz"], r["k"], r["runs"], r["median_ms"],
                                                                                     r["min_ms"], r["max_ms"], e, o, o / STREAM_TBPS))
    for r in rows:
        if "torch_median_ms" in r:
            lines += ["", "The torch expression `(U[rows] * V[cols]).sum(1)` on %s, k = %d: median %.3f ms, %.1f times the kernel's %.3f ms "
                      "(largest difference between the two results %.1e)." % (r["matrix"], r["k"], r["torch_median_ms"], r["torch_median_ms"] / r["median_ms"],
                                                                           r["median_ms"], r["max_abs_difference_from_torch"])]
    return "\n".join(lines) + "\n"


def main():
    argv = list(sys.argv[1:])
    opt = {"--out": os.path.join(ROOT, "profiles", "sample_outer"), "--runs": "20", "--step": None, "--rows": None}
    for name in list(opt):
        if name in argv:
            i = argv.index(name)
            opt[name] = argv[i + 1]
            del argv[i:i + 2]
    runs = max(20, int(opt["--runs"]))
    if opt["--step"] is not None:
        rows = run_step(opt["--step"], runs)
        with open(opt["--rows"], "w") as f:
            json.dump(rows, f)
        return 0
    os.makedirs(opt["--out"], exist_ok=True)
    rows = []
    for name, limit in STEPS:
        part = os.path.join(opt["--out"], "step_%s.json" % name)
        print("step %s (limit %d s)" % (name, limit), flush=True)
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name, "--runs", str(runs),
                            "--rows", part])
        if r.returncode != 0:
            print("step %s ended with status %d: no further step is started" % (name, r.returncode), flush=True)
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
