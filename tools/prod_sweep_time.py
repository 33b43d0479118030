"""Time per tape sweep of the prod row kernels (csrc/exec_hip.h sweep_prod_kernel / sweep_prod_long_kernel /
sweep_prod_hess_kernel) against two yardsticks measured in the same process, alternating sweep by sweep: the log_sum_exp
row kernels on a tape of the SAME (M, K), and the elementwise sweep (sweep_flat_kernel on a unary exp tape of the same
algorithmic byte volume as the prod sweep), per shape, with and without the Hessian.  Writes profiles/prod_sweep.jsonl,
one line per shape.

    python tools/prod_sweep_time.py            # on the MI355X; starts itself once more under rocprofv3 --kernel-trace

What is measured: the device's own begin / end timestamps of every kernel dispatch (rocprofv3 kernel trace only, the
program after `--`, a fresh child process), summed over the kernels of one sweep and averaged over REPS sweeps after WARM
warm-up sweeps.  The spread of the log_sum_exp yardstick is the largest relative distance between the means of its
BLOCKS consecutive blocks of sweeps in the same run: what a difference between prod and that yardstick has to exceed to
mean anything.  What is not measured: the host-to-device copy of x, the constant-map products behind eval_g / eval_h
(other kernels), launch gaps, and anything about a cold cache.

Algorithmic bytes of a row sweep: 8 + 4 read per entry (x and its index), 8 written per output, per d entry and, with the
Hessian on, per h entry (+ 8 read per row for its weight); prod has K (K - 1) / 2 Hessian entries per row, log_sum_exp
K (K + 1) / 2.  The exp tape has as many elements as give the prod volume at 8 read + 16 written (+ 8 + 8 with the
Hessian) per element."""
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

SHAPES = [(100000, 4), (100000, 10), (100000, 16), (5000, 64), (5000, 65), (500, 257), (2, 4097), (1, 8193)]
WARM, REPS, BLOCKS = 20, 200, 4
PROD_KERNELS = ("sweep_prod_kernel", "sweep_prod_long_kernel", "sweep_prod_hess_kernel")
LSE_KERNELS = ("sweep_rows_kernel", "sweep_rows_long_kernel", "sweep_rows_hess_kernel")
FLAT_KERNEL = "sweep_flat_kernel"


def row_bytes(M, K, with_h, strict):
    T = K * (K - 1) // 2 if strict else K * (K + 1) // 2
    return 12 * M * K + 8 * M + 8 * M * K + (8 * M * T + 8 * M if with_h else 0)


def exp_elements(nbytes, with_h):
    return max(2, int(nbytes // (40 if with_h else 24)) & ~1)


def child():
    import dnlp_amd as cp
    import lse_problems as lp
    import prod_problems as pp
    from dnlp_amd import _capi
    from dnlp_amd.tape import serialize
    for M, K in SHAPES:
        axis = 1 if M > 1 else None
        rng = np.random.default_rng(K)
        pa, px, plam, psigma = pp.rows_tape([rng.uniform(0.5, 1.5, (M, K))], axis=axis)
        la, lx, llam, lsigma = lp.rows_tape([rng.standard_normal((M, K))], axis=axis)
        pdev = _capi.DeviceProblem(serialize(pa), None, device=0)
        ldev = _capi.DeviceProblem(serialize(la), None, device=0)
        exps = {}
        for with_h in (False, True):
            n = exp_elements(row_bytes(M, K, with_h, True), with_h)
            v = cp.Variable(n)
            v.value = np.zeros(n)
            data = lp.lower(cp.Problem(cp.Minimize(0 * cp.sum(cp.Variable(1))), [cp.exp(v) <= 2]))
            exps[with_h] = (_capi.DeviceProblem(serialize(data["tape_arrays"]), None, device=0),
                            np.random.default_rng(1).standard_normal(int(data["tape_arrays"]["dims"][0])), np.ones(n))
        for with_h in (False, True):
            edev, ex, elam = exps[with_h]
            for _ in range(WARM + REPS):
                if with_h:
                    pdev.eval_h(px, plam, psigma)
                    ldev.eval_h(lx, llam, lsigma)
                    edev.eval_h(ex, elam, 1.0)
                else:
                    pdev.eval_g(px)
                    ldev.eval_g(lx)
                    edev.eval_g(ex)
        for d in (pdev, ldev, exps[False][0], exps[True][0]):
            d.close()
        print("ran", M, K, flush=True)


def parent():
    out_dir = tempfile.mkdtemp(prefix="prod_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", out_dir, "-o", "prod", "--",
           sys.executable, os.path.abspath(__file__), "--child"]
    subprocess.check_call(cmd, cwd=ROOT)
    files = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit("expected one kernel trace, found %r" % files)
    rows = []
    with open(files[0]) as fh:
        for rec in csv.DictReader(fh):
            name = next((k for k in PROD_KERNELS + LSE_KERNELS + (FLAT_KERNEL,) if k in rec["Kernel_Name"]), None)    # (mangled or not)
            if name is not None:
                rows.append((int(rec["Start_Timestamp"]), name, int(rec["End_Timestamp"]) - int(rec["Start_Timestamp"])))
    rows.sort()
    pos = 0
    lines = []
    for M, K in SHAPES:
        rec = {"M": M, "K": K, "form": "group" if K <= 64 else ("wavefront" if K <= 2048 else "workgroup"),
               "warm": WARM, "reps": REPS, "blocks": BLOCKS}
        for with_h in (False, True):
            per_row = 1 if K <= 64 else (2 if with_h else 1)
            t_prod, t_lse, t_flat = [], [], []
            for rep in range(WARM + REPS):
                got = rows[pos:pos + 2 * per_row + 1]
                pos += 2 * per_row + 1
                names = [g[1] for g in got]
                if (names[-1] != FLAT_KERNEL or any(n not in PROD_KERNELS for n in names[:per_row])
                        or any(n not in LSE_KERNELS for n in names[per_row:-1])):
                    raise SystemExit("unexpected kernel order at %d x %d: %r" % (M, K, names))
                if rep >= WARM:
                    t_prod.append(sum(g[2] for g in got[:per_row]))
                    t_lse.append(sum(g[2] for g in got[per_row:-1]))
                    t_flat.append(got[-1][2])
            pbytes, lbytes = row_bytes(M, K, with_h, True), row_bytes(M, K, with_h, False)
            ebytes = exp_elements(pbytes, with_h) * (40 if with_h else 24)
            tp, tl, tf = (float(np.mean(t)) * 1e-9 for t in (t_prod, t_lse, t_flat))
            blocks = [float(np.mean(b)) for b in np.array_split(np.asarray(t_lse, dtype=float), BLOCKS)]
            tag = "h" if with_h else "noh"
            rec.update({"bytes_" + tag: pbytes, "prod_us_" + tag: 1e6 * tp, "prod_us_min_" + tag: 1e-3 * float(np.min(t_prod)),
                        "prod_TBps_" + tag: pbytes / tp * 1e-12,
                        "lse_us_" + tag: 1e6 * tl, "lse_TBps_" + tag: lbytes / tl * 1e-12,
                        "lse_spread_" + tag: (max(blocks) - min(blocks)) / float(np.mean(blocks)),
                        "flat_us_" + tag: 1e6 * tf, "flat_TBps_" + tag: ebytes / tf * 1e-12,
                        "time_over_lse_" + tag: tp / tl, "byte_rate_over_flat_" + tag: (pbytes / tp) / (ebytes / tf)})
        lines.append(rec)
        print(json.dumps(rec), flush=True)
    if pos != len(rows):
        raise SystemExit("%d sweep kernels left over in the trace" % (len(rows) - pos))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "prod_sweep.jsonl"), "w") as fh:
        for rec in lines:
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    child() if "--child" in sys.argv else parent()
