"""Time per tape sweep of the quad_over_lin_rows row kernels (csrc/exec_hip.h sweep_qol_kernel / sweep_qol_long_kernel).
Writes profiles/quad_over_lin_rows_sweep.jsonl: one line per shape of (a), one per M of (b), one for (c).

    python tools/qol_rows_sweep_time.py        # on the MI355X; starts itself twice more under rocprofv3 --kernel-trace

(a) Against the HBM yardstick: the elementwise sweep (sweep_flat_kernel on a unary exp tape of the same algorithmic
byte volume), measured in the same process, alternating sweep by sweep, per shape, with and without the Hessian.  What
is measured: the device's own begin / end timestamps of every kernel dispatch (rocprofv3 kernel trace only, the program
after `--`, a fresh child process), summed over the kernels of one sweep and averaged over REPS sweeps after WARM warm-up
sweeps.  The spread is the largest relative distance between the means of BLOCKS consecutive blocks of sweeps of the
yardstick in the same run: what a difference has to exceed to mean anything.  Not measured: the host-to-device copy of
x, the constant-map products behind eval_g / eval_h (other kernels), launch gaps, anything about a cold cache.

Algorithmic bytes per row of K entries: read 8 K (+ 4 K index bytes where the row is gathered) + 8 (y), written
8 (K + 2) (z, g, g_y); with the Hessian 8 more read (w) and 8 (2 K + 1) more written: 8 K + 16 read, 8 (3 K + 3) written.
The exp tape has as many elements as give that volume at 8 read + 16 written (+ 8 + 8 with the Hessian) per element.

(b) Against the only statement there was before: a loop of M scalar quad_over_lin atoms (M reduction-class segments,
each a reduce launch, a stream synchronisation with a read-back and a map launch per sweep), K = 3, M = 100 and 1000
(200 and 400 between them locate a crossing, recorded in a summary line; the tool fails if the rows form is not faster
at M = 1000).  The cost of that
form is on the host, so this part is host wall-clock time per eval_h call (time.perf_counter, the two tapes alternating
call by call in this process, no profiler attached), beside the summed device time of the rows form from (a)'s method.

(c) Launches per sweep of a tape with many op-36 segments of both forms, counted from a kernel trace of its own
(rocprofv3 --kernel-trace --stats)."""
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

SHAPES = [(100000, 2), (100000, 3), (100000, 10), (100000, 16), (5000, 64), (5000, 65), (500, 257), (2, 4097)]
LOOP_M, LOOP_K = (100, 200, 400, 1000), 3      # (the ends are the two sizes to record; the others locate a crossing)
TRACE_LIMIT_S = 400                              # per rocprofv3 child
WARM, REPS, BLOCKS = 20, 200, 4
QOL_KERNELS = ("sweep_qol_kernel", "sweep_qol_long_kernel")
FLAT_KERNEL = "sweep_flat_kernel"
LAUNCH_SEGMENTS = [(300, 3), (40, 2), (7, 16), (1000, 3), (5, 64), (64, 7), (9, 65), (3, 300), (2, 2049), (1, 4097), (11, 129), (90, 5)]
LAUNCH_SWEEPS = 10


def row_bytes(M, K, with_h, gathered):
    return M * ((8 * K + (4 * K if gathered else 0) + 8 + 8 * (K + 2)) + (8 + 8 * (2 * K + 1) if with_h else 0))


def exp_elements(nbytes, with_h):
    return max(2, int(nbytes // (40 if with_h else 24)) & ~1)


def _rows_device(sets, axis=1):
    import qol_rows_problems as qp
    from dnlp_amd import _capi
    from dnlp_amd.tape import serialize
    a, x, lam, sigma = qp.rows_tape(sets, axis=axis)
    return _capi.DeviceProblem(serialize(a), None, device=0), a, x, lam, sigma


def _uniform_rows(M, K, seed):
    rng = np.random.default_rng([seed, M, K])
    return rng.uniform(0.5, 1.5, (M, K)), rng.uniform(0.5, 1.5, M)


def child():
    import dnlp_amd as cp
    import lse_problems as lp
    from dnlp_amd import _capi
    from dnlp_amd.tape import serialize
    for M, K in SHAPES:
        qdev, qa, qx, qlam, qsigma = _rows_device([_uniform_rows(M, K, 1)])
        gathered = int(qa["seg_a0_base"][0]) < 0
        exps = {}
        for with_h in (False, True):
            n = exp_elements(row_bytes(M, K, with_h, gathered), with_h)
            v = cp.Variable(n)
            v.value = np.zeros(n)
            data = lp.lower(cp.Problem(cp.Minimize(0 * cp.sum(cp.Variable(1))), [cp.exp(v) <= 2]))
            exps[with_h] = (_capi.DeviceProblem(serialize(data["tape_arrays"]), None, device=0),
                            np.random.default_rng(1).standard_normal(int(data["tape_arrays"]["dims"][0])), np.ones(n))
        for with_h in (False, True):
            edev, ex, elam = exps[with_h]
            for _ in range(WARM + REPS):
                if with_h:
                    qdev.eval_h(qx, qlam, qsigma)
                    edev.eval_h(ex, elam, 1.0)
                else:
                    qdev.eval_g(qx)
                    edev.eval_g(ex)
        for d in (qdev, exps[False][0], exps[True][0]):
            d.close()
        print("ran", M, K, int(gathered), flush=True)


def launches_child():
    qdev, qa, qx, qlam, qsigma = _rows_device([_uniform_rows(M, K, 2) for M, K in LAUNCH_SEGMENTS])
    for _ in range(LAUNCH_SWEEPS):
        qdev.eval_h(qx, qlam, qsigma)
    qdev.close()


def _trace(mode, extra=()):
    out_dir = tempfile.mkdtemp(prefix="qol_trace_")
    cmd = ["rocprofv3", "--kernel-trace", *extra, "--output-format", "csv", "-d", out_dir, "-o", "qol", "--",
           sys.executable, os.path.abspath(__file__), mode]
    out = subprocess.run(cmd, cwd=ROOT, check=True, stdout=subprocess.PIPE, text=True, timeout=TRACE_LIMIT_S).stdout
    files = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit("expected one kernel trace, found %r" % files)
    rows = []
    with open(files[0]) as fh:
        for rec in csv.DictReader(fh):
            name = next((k for k in QOL_KERNELS + (FLAT_KERNEL,) if k in rec["Kernel_Name"]), None)    # (mangled or not)
            if name is not None:
                rows.append((int(rec["Start_Timestamp"]), name, int(rec["End_Timestamp"]) - int(rec["Start_Timestamp"])))
    rows.sort()
    return rows, out


def part_a():
    rows, out = _trace("--child")
    gathered = {(int(t[1]), int(t[2])): bool(int(t[3])) for t in (ln.split() for ln in out.splitlines()) if t and t[0] == "ran"}
    pos = 0
    lines = []
    for M, K in SHAPES:
        rec = {"part": "a", "M": M, "K": K, "form": "group" if K <= 64 else ("wavefront" if K <= 2048 else "workgroup"),
               "gathered": gathered[(M, K)], "warm": WARM, "reps": REPS, "blocks": BLOCKS}
        for with_h in (False, True):
            t_qol, t_flat = [], []
            for rep in range(WARM + REPS):
                got = rows[pos:pos + 2]
                pos += 2
                if len(got) != 2 or got[0][1] not in QOL_KERNELS or got[1][1] != FLAT_KERNEL:
                    raise SystemExit("unexpected kernel order at %d x %d: %r" % (M, K, [g[1] for g in got]))
                if rep >= WARM:
                    t_qol.append(got[0][2])
                    t_flat.append(got[1][2])
            qbytes = row_bytes(M, K, with_h, gathered[(M, K)])
            ebytes = exp_elements(qbytes, with_h) * (40 if with_h else 24)
            tq, tf = (float(np.mean(t)) * 1e-9 for t in (t_qol, t_flat))
            blocks = [float(np.mean(b)) for b in np.array_split(np.asarray(t_flat, dtype=float), BLOCKS)]
            tag = "h" if with_h else "noh"
            rec.update({"bytes_" + tag: qbytes, "qol_us_" + tag: 1e6 * tq, "qol_us_min_" + tag: 1e-3 * float(np.min(t_qol)),
                        "qol_TBps_" + tag: qbytes / tq * 1e-12, "flat_us_" + tag: 1e6 * tf, "flat_TBps_" + tag: ebytes / tf * 1e-12,
                        "flat_spread_" + tag: (max(blocks) - min(blocks)) / float(np.mean(blocks)),
                        "byte_rate_over_flat_" + tag: (qbytes / tq) / (ebytes / tf)})
        lines.append(rec)
        print(json.dumps(rec), flush=True)
    if pos != len(rows):
        raise SystemExit("%d sweep kernels left over in the trace" % (len(rows) - pos))
    return lines


def part_b():
    import dnlp_amd as cp
    import lse_problems as lp
    from dnlp_amd import _capi
    from dnlp_amd.tape import serialize
    lines = []
    for M in LOOP_M:
        U, y = _uniform_rows(M, LOOP_K, 3)
        rdev, ra, rx, rlam, rsigma = _rows_device([(U, y)])
        cons = []
        for i in range(M):
            v, d = cp.Variable(LOOP_K), cp.Variable()
            v.value, d.value = U[i], y[i]
            cons.append(cp.quad_over_lin(v, d) <= 0)
        data = lp.lower(cp.Problem(cp.Minimize(0 * cp.sum(cp.Variable(1))), cons))
        la = data["tape_arrays"]
        assert list(la["seg_op"]) == [32] * M
        ldev = _capi.DeviceProblem(serialize(la), None, device=0)
        lx, llam = np.array(data["x0"], dtype=float), lp.multipliers(int(la["dims"][1]))
        t_rows, t_loop = [], []
        for rep in range(WARM + REPS):
            t0 = time.perf_counter()
            rdev.eval_h(rx, rlam, rsigma)
            t1 = time.perf_counter()
            ldev.eval_h(lx, llam, 0.5)
            t2 = time.perf_counter()
            if rep >= WARM:
                t_rows.append(t1 - t0)
                t_loop.append(t2 - t1)
        rdev.close()
        ldev.close()
        blocks = [float(np.mean(b)) for b in np.array_split(np.asarray(t_rows), BLOCKS)]
        rec = {"part": "b", "M": M, "K": LOOP_K, "warm": WARM, "reps": REPS, "what": "host wall-clock per eval_h call",
               "rows_us": 1e6 * float(np.mean(t_rows)), "rows_us_min": 1e6 * float(np.min(t_rows)),
               "loop_us": 1e6 * float(np.mean(t_loop)), "loop_us_min": 1e6 * float(np.min(t_loop)),
               "rows_spread": (max(blocks) - min(blocks)) / float(np.mean(blocks)),
               "loop_over_rows": float(np.mean(t_loop)) / float(np.mean(t_rows))}
        lines.append(rec)
        print(json.dumps(rec), flush=True)
    # where the two cross, if they do inside the measured range: log-linear between the neighbours on either side of 1
    ratios = [(r["M"], r["loop_over_rows"]) for r in lines]
    cross = None
    for (m0, q0), (m1, q1) in zip(ratios[:-1], ratios[1:]):
        if (q0 - 1.0) * (q1 - 1.0) <= 0 and q0 != q1:
            cross = float(np.exp(np.log(m0) + (np.log(m1) - np.log(m0)) * (1.0 - q0) / (q1 - q0)))
            break
    rec = {"part": "b", "summary": True, "K": LOOP_K, "loop_over_rows_by_M": dict(ratios), "crossing_M": cross,
           "crossing_note": None if cross is not None else ("rows faster over the whole range" if min(q for _, q in ratios) > 1 else "loop faster over the whole range")}
    lines.append(rec)
    print(json.dumps(rec), flush=True)
    return lines


def part_c():
    rows, _ = _trace("--launches-child", extra=("--stats",))
    names = [r[1] for r in rows if r[1] in QOL_KERNELS]
    per_sweep = len(names) / LAUNCH_SWEEPS
    rec = {"part": "c", "segments": len(LAUNCH_SEGMENTS), "short_segments": sum(K <= 64 for _, K in LAUNCH_SEGMENTS),
           "sweeps": LAUNCH_SWEEPS, "qol_launches": len(names), "launches_per_sweep": per_sweep,
           "by_kernel": {k: names.count(k) for k in QOL_KERNELS}}
    print(json.dumps(rec), flush=True)
    if per_sweep > 2:
        raise SystemExit("more than two launches per sweep: %r" % rec)
    return [rec]


def parent():
    lines = part_a() + part_c() + part_b()          # (b) last: this process opens the device only after the children are gone
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "quad_over_lin_rows_sweep.jsonl"), "w") as fh:
        for rec in lines:
            fh.write(json.dumps(rec) + "\n")
    # the loop form pays a stream synchronisation per segment and sweep: the rows form must be faster at the largest M
    last = [r for r in lines if r.get("part") == "b" and r.get("M") == LOOP_M[-1]][0]
    if not last["loop_over_rows"] > 1.0:
        raise SystemExit("rows form not faster than the loop of scalar atoms at M = %d: %r" % (LOOP_M[-1], last))


if __name__ == "__main__":
    if "--child" in sys.argv:
        child()
    elif "--launches-child" in sys.argv:
        launches_child()
    else:
        parent()
