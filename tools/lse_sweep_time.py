"""Time per tape sweep of the row-class kernels (csrc/exec_hip.h sweep_rows_kernel / sweep_rows_long_kernel /
sweep_rows_hess_kernel) against the elementwise yardstick (sweep_flat_kernel on a unary exp tape of the same algorithmic
byte volume), per shape, with and without the Hessian.  Writes profiles/log_sum_exp_sweep.jsonl, one line per shape.

    python tools/lse_sweep_time.py            # on the MI355X; starts itself once more under rocprofv3 --kernel-trace

What is measured: the device's own begin / end timestamps of every kernel dispatch (rocprofv3 kernel trace), summed over
the kernels of one sweep and averaged over REPS sweeps after WARM warm-up sweeps; the row tape and the exp tape alternate
sweep by sweep in one process.  What is not: the host-to-device copy of x and the constant-map products behind eval_g /
eval_h (other kernels), launch gaps, and anything about a cold cache (x and the tables are re-read every sweep: shapes
whose arrays fit the 256 MiB cache read from it).

Algorithmic bytes of a row sweep: 8 + 4 read per entry (x and its index), 8 written per output, per d entry and, with the
Hessian on, per h entry (+ 8 read per row for its weight).  The exp tape has as many elements as give the same volume at
8 read + 16 written (+ 8 + 8 with the Hessian) per element."""
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

# (rows, row length).  The issue's list at the sizes whose numpy lowering stays within seconds: the Hessian pattern of
# 2e4 x 64 is 4e7 entries and that of 16 x 4097 is 1.3e8; rows per shape are cut where they exceed ~3.4e7 entries.
SHAPES = [(100000, 4), (100000, 10), (100000, 16), (5000, 64), (5000, 65), (500, 257), (2, 4097), (1, 8193)]
WARM, REPS = 20, 200
ROW_KERNELS = ("sweep_rows_kernel", "sweep_rows_long_kernel", "sweep_rows_hess_kernel")
FLAT_KERNEL = "sweep_flat_kernel"


def row_bytes(M, K, with_h):
    T = K * (K + 1) // 2
    return 12 * M * K + 8 * M + 8 * M * K + (8 * M * T + 8 * M if with_h else 0)


def exp_elements(nbytes, with_h):
    return max(2, int(nbytes // (40 if with_h else 24)) & ~1)


def child():
    import dnlp_amd as cp
    import lse_problems as lp
    from dnlp_amd import _capi
    from dnlp_amd.tape import serialize
    for M, K in SHAPES:
        rows = np.random.default_rng(K).standard_normal((M, K))
        a, x, lam, sigma = lp.rows_tape([rows], axis=1 if M > 1 else None)
        dev = _capi.DeviceProblem(serialize(a), None, device=0)
        exps = {}
        for with_h in (False, True):
            n = exp_elements(row_bytes(M, K, with_h), with_h)
            v = cp.Variable(n)
            v.value = np.zeros(n)
            data = lp.lower(cp.Problem(cp.Minimize(0 * cp.sum(cp.Variable(1))), [cp.exp(v) <= 2]))
            exps[with_h] = (_capi.DeviceProblem(serialize(data["tape_arrays"]), None, device=0),
                            np.random.default_rng(1).standard_normal(int(data["tape_arrays"]["dims"][0])), np.ones(n))
        for with_h in (False, True):
            edev, ex, elam = exps[with_h]
            for _ in range(WARM + REPS):
                if with_h:
                    dev.eval_h(x, lam, sigma)
                    edev.eval_h(ex, elam, 1.0)
                else:
                    dev.eval_g(x)
                    edev.eval_g(ex)
        dev.close()
        for e in exps.values():
            e[0].close()
        print("ran", M, K, flush=True)


def parent():
    out_dir = tempfile.mkdtemp(prefix="lse_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", out_dir, "-o", "lse", "--",
           sys.executable, os.path.abspath(__file__), "--child"]
    subprocess.check_call(cmd, cwd=ROOT)
    files = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit("expected one kernel trace, found %r" % files)
    rows = []
    with open(files[0]) as fh:
        for rec in csv.DictReader(fh):
            name = next((k for k in ROW_KERNELS + (FLAT_KERNEL,) if k in rec["Kernel_Name"]), None)    # (mangled or not)
            if name is not None:
                rows.append((int(rec["Start_Timestamp"]), name, int(rec["End_Timestamp"]) - int(rec["Start_Timestamp"])))
    rows.sort()
    pos = 0
    lines = []
    for M, K in SHAPES:
        rec = {"M": M, "K": K, "form": "group" if K <= 64 else ("wavefront" if K <= 2048 else "workgroup"),
               "switch_group_to_wavefront": 64, "switch_wavefront_to_workgroup": 2048, "warm": WARM, "reps": REPS}
        for with_h in (False, True):
            per_row = 1 if K <= 64 else (2 if with_h else 1)
            t_row, t_flat = [], []
            for rep in range(WARM + REPS):
                got = rows[pos:pos + per_row + 1]
                pos += per_row + 1
                names = [g[1] for g in got]
                if names[-1] != FLAT_KERNEL or any(n not in ROW_KERNELS for n in names[:-1]):
                    raise SystemExit("unexpected kernel order at %d x %d: %r" % (M, K, names))
                if rep >= WARM:
                    t_row.append(sum(g[2] for g in got[:-1]))
                    t_flat.append(got[-1][2])
            nbytes = row_bytes(M, K, with_h)
            ebytes = exp_elements(nbytes, with_h) * (40 if with_h else 24)
            tr, tf = float(np.mean(t_row)) * 1e-9, float(np.mean(t_flat)) * 1e-9
            tag = "h" if with_h else "noh"
            rec.update({"bytes_" + tag: nbytes, "rows_us_" + tag: 1e6 * tr, "rows_us_min_" + tag: 1e-3 * float(np.min(t_row)),
                        "rows_GBps_" + tag: nbytes / tr * 1e-9, "flat_us_" + tag: 1e6 * tf, "flat_GBps_" + tag: ebytes / tf * 1e-9,
                        "ratio_" + tag: (nbytes / tr) / (ebytes / tf)})
        lines.append(rec)
        print(json.dumps(rec), flush=True)
    if pos != len(rows):
        raise SystemExit("%d sweep kernels left over in the trace" % (len(rows) - pos))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "log_sum_exp_sweep.jsonl"), "w") as fh:
        for rec in lines:
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    child() if "--child" in sys.argv else parent()
