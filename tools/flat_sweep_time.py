"""Time per tape sweep of sweep_flat_kernel (csrc/exec_hip.h) on ONE unary segment of 2^24 entries, per op, with and without
the Hessian, the ops alternating sweep by sweep in one process.

    python tools/flat_sweep_time.py --build NAME [--ops exp,logistic,...] [--fresh]        # on the MI355X

Appends one line per op to profiles/special_atoms_sweep.jsonl (--fresh: starts the file anew).  --build labels the library
that ran (DNLP_HIP_LIB chooses another build of it, whose ops may be fewer: name them with --ops).

What is measured: the device's own begin / end timestamps of every sweep_flat_kernel dispatch (rocprofv3 kernel trace only,
the program after `--`, a fresh child process with a time limit of its own; nothing further starts after a child that
fails), averaged over REPS sweeps after WARM warm-up sweeps.  `spread` is the largest relative distance between the means
of BLOCKS consecutive blocks of sweeps of that op in the same run: what a difference has to exceed to mean anything.  Not
measured: the copies of x and of the results, the constant-map products behind eval_g / eval_h, launch gaps.

One tape is lowered (exp over 2^24 entries) and its opcode replaced per op: the unary ops share their layout.  Arguments:
3 x standard normal for every op (both branches of the normal pair in every wavefront, |u| up to 15), its absolute value
plus 0.05 for loggamma (most of the recurrence's trip counts in every wavefront).  Algorithmic bytes per entry: 8 read + 16
written, + 8 + 8 with the Hessian."""
import argparse
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

N = 1 << 24
WARM, REPS, BLOCKS = 4, 40, 4
TRACE_LIMIT_S = 500
OPCODES = {"exp": 1, "logistic": 4, "log_normcdf": 14, "normcdf": 15, "loggamma": 16}
OUT = os.path.join(ROOT, "profiles", "special_atoms_sweep.jsonl")


def child(ops):
    import dnlp_amd as cp
    from dnlp_amd import _capi
    from dnlp_amd.dnlp2smooth import Dnlp2Smooth
    from dnlp_amd.nlp_solver import build_nlp_data
    from dnlp_amd.tape import serialize
    v = cp.Variable(N)
    v.value = np.zeros(N)
    pad = cp.Variable(2)
    smooth, _ = Dnlp2Smooth().apply(cp.Problem(cp.Minimize(0 * cp.sum(pad)), [cp.exp(v) <= 2]))
    a = dict(build_nlp_data(smooth)[0]["tape_arrays"])
    assert list(a["seg_op"]) == [1] and int(a["seg_n"][0]) == N and int(a["seg_a0_base"][0]) % 2 == 0
    x = np.zeros(int(a["dims"][0]))
    u = 3.0 * np.random.default_rng(1).standard_normal(N)
    lam = np.ones(int(a["dims"][1]))
    devs = []
    for op in ops:
        b = dict(a)
        b["seg_op"] = np.full_like(a["seg_op"], OPCODES[op])
        xo = x.copy()
        xo[int(a["seg_a0_base"][0]):int(a["seg_a0_base"][0]) + N] = np.abs(u) + 0.05 if op == "loggamma" else u
        devs.append((_capi.DeviceProblem(serialize(b), None, device=0), xo))
    for with_h in (False, True):
        for _ in range(WARM + REPS):
            for dev, xo in devs:
                dev.eval_h(xo, lam, 1.0) if with_h else dev.eval_g(xo)
    for dev, _ in devs:
        dev.close()
    print("ran", " ".join(ops), flush=True)


def spread(times):
    blocks = [float(np.mean(b)) for b in np.array_split(np.asarray(times, dtype=float), BLOCKS)]
    return (max(blocks) - min(blocks)) / float(np.mean(blocks))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--build", required=True, help="label of the library that runs")
    ap.add_argument("--ops", default=",".join(OPCODES))
    ap.add_argument("--fresh", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    ops = args.ops.split(",")
    if args.child:
        return child(ops)
    out_dir = tempfile.mkdtemp(prefix="flat_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", out_dir, "-o", "flat", "--",
           sys.executable, os.path.abspath(__file__), "--build", args.build, "--ops", args.ops, "--child"]
    out = subprocess.run(cmd, cwd=ROOT, check=True, stdout=subprocess.PIPE, text=True, timeout=TRACE_LIMIT_S).stdout
    if "ran " not in out:
        raise SystemExit("the child did not finish: %s" % out[-2000:])
    files = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit("expected one kernel trace, found %r" % files)
    rows = []
    with open(files[0]) as fh:
        for rec in csv.DictReader(fh):
            if "sweep_flat_kernel" in rec["Kernel_Name"]:
                rows.append((int(rec["Start_Timestamp"]), int(rec["End_Timestamp"]) - int(rec["Start_Timestamp"])))
    rows.sort()
    if len(rows) != 2 * (WARM + REPS) * len(ops):
        raise SystemExit("%d sweep_flat_kernel dispatches in the trace, %d expected" % (len(rows), 2 * (WARM + REPS) * len(ops)))
    ns = np.array([r[1] for r in rows], dtype=float).reshape(2, WARM + REPS, len(ops))[:, WARM:, :]
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w" if args.fresh else "a") as fh:
        for k, op in enumerate(ops):
            rec = {"build": args.build, "op": op, "opcode": OPCODES[op], "n": N, "warm": WARM, "reps": REPS, "blocks": BLOCKS,
                   "ops_alternating": ops}
            for h, tag, nbytes in ((0, "noh", 24 * N), (1, "h", 40 * N)):
                t = ns[h, :, k]
                rec.update({"us_" + tag: 1e-3 * float(t.mean()), "us_min_" + tag: 1e-3 * float(t.min()), "spread_" + tag: spread(t),
                            "bytes_" + tag: nbytes, "TBps_" + tag: nbytes / (float(t.mean()) * 1e-9) * 1e-12})
            fh.write(json.dumps(rec) + "\n")
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
