"""Time per flat tape sweep (sweep_flat_kernel, csrc/exec_hip.h) over 10^6 elements of atan, of asin and of atan2, with and
without the Hessian, each against an exp tape of the same algorithmic byte volume measured in the same process, alternating
sweep by sweep.

    python tools/trig_sweep_time.py [--tag NAME]      # on the MI355X

Writes one line per atom and mode to profiles/trig_sweep.jsonl (with --tag NAME to profiles/trig_sweep.<NAME>.jsonl).

The method is that of tools/row_sweep_time.py: the device's own begin / end timestamps of every kernel dispatch (rocprofv3
kernel trace only, the program after `--`, a fresh child process with a time limit of its own), averaged over REPS sweeps
after WARM warm-up sweeps.  The spread is the largest relative distance between the means of BLOCKS consecutive blocks of
sweeps of the exp yardstick in the same run: what a difference has to exceed to mean anything.  Not measured: the
host-to-device copy of x, the constant-map products behind eval_g / eval_h (other kernels), launch gaps, and anything about a
cold cache (x and the tables are re-read every sweep; 10^6 elements fit the 256 MiB cache).

Algorithmic bytes per element.  A unary op: 8 read and 16 written (z, d), with the Hessian 8 more read (w) and 8 more written:
24 / 40.  atan2: 16 read and 24 written (z, two d runs), with the Hessian 8 more read and 24 more written (three h runs):
40 / 72.  The unary ops move double2's (their arguments are contiguous and aligned); atan2 takes the scalar path."""
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

N = 1000000
ATOMS = ("atan", "asin", "atan2")
WARM, REPS, BLOCKS = 20, 200, 4
TRACE_LIMIT_S = 400
KERNEL = "sweep_flat_kernel"


def atom_bytes(atom, with_h):
    per = (72 if with_h else 40) if atom == "atan2" else (40 if with_h else 24)
    return per * N


def exp_elements(nbytes, with_h):
    return max(2, int(nbytes // (40 if with_h else 24)) & ~1)


def spread(times):
    blocks = [float(np.mean(b)) for b in np.array_split(np.asarray(times, dtype=float), BLOCKS)]
    return (max(blocks) - min(blocks)) / float(np.mean(blocks))


def _tape(atom, n):
    """-> (device problem, x, multipliers) of `atom(v) <= 2` over n elements, arguments inside the domain"""
    import dnlp_amd as cp
    from dnlp_amd import _capi
    from dnlp_amd.nlp_solver import build_nlp_data
    from dnlp_amd.tape import serialize
    vs = [cp.Variable(n) for _ in range(2 if atom == "atan2" else 1)]
    for v in vs:
        v.value = np.zeros(n)
    # (lowered as written: every argument is a bare variable, and asin's auxiliary variable would only add rows outside the sweep)
    a = build_nlp_data(cp.Problem(cp.Minimize(0 * cp.sum(cp.Variable(1))), [getattr(cp, atom)(*vs) <= 2]))[0]["tape_arrays"]
    assert list(a["seg_op"]) == [{"exp": 1, "atan": 18, "asin": 19, "atan2": 22}[atom]] and int(a["seg_n"][0]) == n
    x = np.random.default_rng(1).uniform(-0.95, 0.95, int(a["dims"][0]))
    return _capi.DeviceProblem(serialize(a), None, device=0), x, np.ones(n)


def child():
    for atom in ATOMS:
        for with_h in (False, True):
            dev, x, lam = _tape(atom, N)
            edev, ex, elam = _tape("exp", exp_elements(atom_bytes(atom, with_h), with_h))
            for _ in range(WARM + REPS):
                dev.eval_h(x, lam, 1.0) if with_h else dev.eval_g(x)
                edev.eval_h(ex, elam, 1.0) if with_h else edev.eval_g(ex)
            dev.close()
            edev.close()
            print("ran", atom, int(with_h), flush=True)


def trace():
    out_dir = tempfile.mkdtemp(prefix="trig_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", out_dir, "-o", "trig", "--",
           sys.executable, os.path.abspath(__file__), "--child"]
    subprocess.run(cmd, cwd=ROOT, check=True, stdout=subprocess.PIPE, text=True, timeout=TRACE_LIMIT_S)
    files = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit("expected one kernel trace, found %r" % files)
    rows = []
    with open(files[0]) as fh:
        for rec in csv.DictReader(fh):
            if KERNEL in rec["Kernel_Name"]:
                rows.append((int(rec["Start_Timestamp"]), int(rec["End_Timestamp"]) - int(rec["Start_Timestamp"])))
    rows.sort()
    return [r[1] for r in rows]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--tag", help="write profiles/trig_sweep.<TAG>.jsonl instead of profiles/trig_sweep.jsonl")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child()
    ns = trace()
    per_group = 2 * (WARM + REPS)
    if len(ns) != per_group * len(ATOMS) * 2:
        raise SystemExit("%d sweep kernels in the trace where %d were due" % (len(ns), per_group * len(ATOMS) * 2))
    lines, pos = [], 0
    for atom in ATOMS:
        for with_h in (False, True):
            part = ns[pos:pos + per_group]
            pos += per_group
            ta, te = part[2 * WARM::2], part[2 * WARM + 1::2]
            nbytes = atom_bytes(atom, with_h)
            en = exp_elements(nbytes, with_h)
            ebytes = en * (40 if with_h else 24)
            ma, me = float(np.mean(ta)) * 1e-9, float(np.mean(te)) * 1e-9
            rec = {"atom": atom, "n": N, "with_hessian": with_h, "path": "scalar" if atom == "atan2" else "double2", "warm": WARM,
                   "reps": REPS, "blocks": BLOCKS, "bytes": nbytes, "atom_us": 1e6 * ma, "atom_us_min": 1e-3 * float(np.min(ta)),
                   "atom_TBps": nbytes / ma * 1e-12, "atom_spread": spread(ta), "exp_n": en, "exp_bytes": ebytes, "exp_us": 1e6 * me,
                   "exp_us_min": 1e-3 * float(np.min(te)), "exp_TBps": ebytes / me * 1e-12, "exp_spread": spread(te),
                   "time_over_exp": ma / me, "byte_rate_over_exp": (nbytes / ma) / (ebytes / me)}
            lines.append(rec)
            print(json.dumps(rec), flush=True)
    name = "trig_sweep.jsonl" if not args.tag else "trig_sweep.%s.jsonl" % args.tag
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", name), "w") as fh:
        for rec in lines:
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
