"""Time per tape sweep of the row-class kernels (csrc/exec_hip_rows.h) of one atom, per shape, with and without the Hessian,
against yardsticks measured in the same process, alternating sweep by sweep.

    python tools/row_sweep_time.py --atom {log_sum_exp,prod,quad_over_lin_rows,log_det,matrix_frac} [--tag NAME]      # on the MI355X

Writes one line per shape to profiles/log_sum_exp_sweep.jsonl, prod_sweep.jsonl, quad_over_lin_rows_sweep.jsonl,
log_det_sweep.jsonl or matrix_frac_sweep.jsonl; with
--tag NAME to profiles/<file>.<NAME>.jsonl instead, so that a run of another build of the library (DNLP_HIP_LIB) does not
overwrite the current one.

What is measured: the device's own begin / end timestamps of every kernel dispatch (rocprofv3 kernel trace only, the
program after `--`, a fresh child process with a time limit of its own; nothing further starts after a child that fails),
summed over the kernels of one sweep and averaged over REPS sweeps after WARM warm-up sweeps.  A spread is the largest
relative distance between the means of BLOCKS consecutive blocks of sweeps of a yardstick in the same run: what a
difference has to exceed to mean anything.  Not measured: the host-to-device copy of x, the constant-map products behind
eval_g / eval_h (other kernels), launch gaps, and anything about a cold cache (x and the tables are re-read every sweep:
shapes whose arrays fit the 256 MiB cache read from it).

Yardsticks.  Every atom: the elementwise sweep (sweep_flat_kernel on a unary exp tape of the same algorithmic byte volume;
8 read + 16 written, + 8 + 8 with the Hessian, per element).  prod also: the log_sum_exp kernels on a tape of the SAME
(M, K).  log_det (M matrices of order n, one segment each) also: the log_sum_exp kernels on M rows of K = n^2 entries --
the same Hessian bytes and the same spread launch; its lines also give the time of one elimination step, the sweep without
the Hessian over n.  matrix_frac (M segments of P of order n and X of n x m, one segment each) also: the log_det kernels on M
matrices of order N = n + m -- the same elimination over N steps where matrix_frac walks n, so the lines give the time per
step of both -- and the log_sum_exp kernels on M rows of the same K = n N.

Algorithmic bytes of a row sweep.  log_sum_exp, prod: 8 + 4 read per entry (x and its index), 8 written per output, per d
entry and, with the Hessian on, per h entry (+ 8 read per row for its weight); K (K + 1) / 2 Hessian entries per row,
prod K (K - 1) / 2.  quad_over_lin_rows, per row of K entries: read 8 K (+ 4 K index bytes where the row is gathered)
+ 8 (y), written 8 (K + 2) (z, g, g_y); with the Hessian 8 more read (w) and 8 (2 K + 1) more written.

quad_over_lin_rows has two parts more.  (b) Against the only statement there was before: a loop of M scalar quad_over_lin
atoms (M reduction-class segments, each a reduce launch, a stream synchronisation with a read-back and a map launch per
sweep), K = 3, M = 100 and 1000 (200 and 400 between them locate a crossing, recorded in a summary line; the tool fails if
the rows form is not faster at M = 1000).  The cost of that form is on the host, so this part is host wall-clock time per
eval_h call (time.perf_counter, the two tapes alternating call by call in this process, no profiler attached).
(c) Launches per sweep of a tape with many op-36 segments of both forms, counted from a kernel trace of its own
(rocprofv3 --kernel-trace --stats)."""
import argparse
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

# (rows, row length).  Sizes whose numpy lowering stays within seconds: the Hessian pattern of 2e4 x 64 is 4e7 entries and
# that of 16 x 4097 is 1.3e8; rows per shape are cut where they exceed ~3.4e7 entries.
TRI_SHAPES = [(100000, 4), (100000, 10), (100000, 16), (5000, 64), (5000, 65), (500, 257), (2, 4097), (1, 8193)]
LOGDET_SHAPES = [(1024, 3), (256, 8), (64, 16), (16, 32), (4, 45)]      # (matrices, order)
MFRAC_SHAPES = [(1024, 3), (256, 7), (64, 15), (16, 31), (4, 44), (16, 16)]      # (segments, order n of P) ...
MFRAC_COLS = {(1024, 3): 1, (256, 7): 1, (64, 15): 1, (16, 31): 1, (4, 44): 1, (16, 16): 16}       # ... and the columns m of X
QOL_SHAPES = [(100000, 2), (100000, 3), (100000, 10), (100000, 16), (5000, 64), (5000, 65), (500, 257), (2, 4097)]
WARM, REPS, BLOCKS = 20, 200, 4
TRACE_LIMIT_S = 400                              # per rocprofv3 child
KERNELS = {"lse": ("sweep_rows_kernel", "sweep_rows_long_kernel", "sweep_rows_hess_kernel"),
           "prod": ("sweep_prod_kernel", "sweep_prod_long_kernel", "sweep_prod_hess_kernel"),
           "qol": ("sweep_qol_kernel", "sweep_qol_long_kernel"),
           "logdet": ("sweep_logdet_kernel", "sweep_logdet_long_kernel", "sweep_logdet_hess_kernel"),
           "mfrac": ("sweep_mfrac_kernel", "sweep_mfrac_long_kernel", "sweep_mfrac_hess_kernel"),
           "flat": ("sweep_flat_kernel",)}
# per atom: its output file, its shapes, and the tapes of one sweep round in the order they are evaluated (the first is
# the atom's own, the last the exp tape sized by the first one's bytes)
ATOMS = {"log_sum_exp": ("log_sum_exp_sweep.jsonl", TRI_SHAPES, ("lse", "flat")),
         "prod": ("prod_sweep.jsonl", TRI_SHAPES, ("prod", "lse", "flat")),
         "quad_over_lin_rows": ("quad_over_lin_rows_sweep.jsonl", QOL_SHAPES, ("qol", "flat")),
         "log_det": ("log_det_sweep.jsonl", LOGDET_SHAPES, ("logdet", "lse", "flat")),
         "matrix_frac": ("matrix_frac_sweep.jsonl", MFRAC_SHAPES, ("mfrac", "logdet", "lse", "flat"))}
LOOP_M, LOOP_K = (100, 200, 400, 1000), 3      # (the ends are the two sizes to record; the others locate a crossing)
LAUNCH_SEGMENTS = [(300, 3), (40, 2), (7, 16), (1000, 3), (5, 64), (64, 7), (9, 65), (3, 300), (2, 2049), (1, 4097), (11, 129), (90, 5)]
LAUNCH_SWEEPS = 10


def tri_bytes(M, K, with_h, strict):
    T = K * (K - 1) // 2 if strict else K * (K + 1) // 2
    return 12 * M * K + 8 * M + 8 * M * K + (8 * M * T + 8 * M if with_h else 0)


def qol_bytes(M, K, with_h, gathered):
    return M * ((8 * K + (4 * K if gathered else 0) + 8 + 8 * (K + 2)) + (8 + 8 * (2 * K + 1) if with_h else 0))


def exp_elements(nbytes, with_h):
    return max(2, int(nbytes // (40 if with_h else 24)) & ~1)


def launches(stream, K, with_h):
    return 2 if stream in ("lse", "prod", "logdet", "mfrac") and K > 64 and with_h else 1


def work(atom, stream, M, K):
    """What decides the kernel form of `stream` at shape (M, K) of `atom`: the row length, or the entries of the matrix."""
    if atom == "log_det":
        return K * K
    if atom == "matrix_frac":
        N = K + MFRAC_COLS[(M, K)]
        return K * N if stream == "lse" else N * N
    return K


def form(K):
    return "group" if K <= 64 else ("wavefront" if K <= 2048 else "workgroup")


def spread(times):
    blocks = [float(np.mean(b)) for b in np.array_split(np.asarray(times, dtype=float), BLOCKS)]
    return (max(blocks) - min(blocks)) / float(np.mean(blocks))


def _device(a):
    from dnlp_amd import _capi
    from dnlp_amd.tape import serialize
    return _capi.DeviceProblem(serialize(a), None, device=0)


def _exp_tape(n):
    """-> (device problem, x, multipliers) of `exp(v) <= 2` over n elements"""
    import dnlp_amd as cp
    import lse_problems as lp
    v = cp.Variable(n)
    v.value = np.zeros(n)
    a = lp.lower(cp.Problem(cp.Minimize(0 * cp.sum(cp.Variable(1))), [cp.exp(v) <= 2]))["tape_arrays"]
    return _device(a), np.random.default_rng(1).standard_normal(int(a["dims"][0])), np.ones(n)


def _qol_rows(M, K, seed):
    rng = np.random.default_rng([seed, M, K])
    return rng.uniform(0.5, 1.5, (M, K)), rng.uniform(0.5, 1.5, M)


def _row_tapes(atom, M, K):
    """-> ([(device problem, x, multipliers, sigma)] for the row streams of the atom, bytes(with_h) of its own sweep, note)"""
    import lse_problems as lp
    import prod_problems as pp
    import qol_rows_problems as qp
    if atom == "log_det":                                   # (M matrices of order K: the row length is K * K)
        import logdet_problems as lq
        import logdet_reference as lr
        mats = [lr.matrix(K, 100.0, False, seed=7000 + k) for k in range(M)]
        tapes = [lq.matrices_tape(mats), lp.rows_tape([np.random.default_rng(K).standard_normal((M, K * K))], axis=1)]
        return [(_device(t[0]),) + tuple(t[1:]) for t in tapes], (lambda with_h: tri_bytes(M, K * K, with_h, False)), 0
    if atom == "matrix_frac":                               # (M segments: P of order K, X of K x m)
        import logdet_problems as lq
        import logdet_reference as lr
        import matrix_frac_problems as mq
        import matrix_frac_reference as mr
        m = MFRAC_COLS[(M, K)]
        pairs = [mr.inputs_of(K, m, 100.0, False, seed=7000 + k) for k in range(M)]
        mats = [lr.matrix(K + m, 100.0, False, seed=7000 + k) for k in range(M)]
        tapes = [mq.segments_tape(pairs), lq.matrices_tape(mats),
                 lp.rows_tape([np.random.default_rng(K).standard_normal((M, K * (K + m)))], axis=1)]
        return [(_device(t[0]),) + tuple(t[1:]) for t in tapes], (lambda with_h: tri_bytes(M, K * (K + m), with_h, False)), 0
    axis = 1 if M > 1 else None
    rng = np.random.default_rng(K)
    if atom == "log_sum_exp":
        tapes = [lp.rows_tape([rng.standard_normal((M, K))], axis=axis)]
        nbytes = lambda with_h: tri_bytes(M, K, with_h, False)
    elif atom == "prod":
        tapes = [pp.rows_tape([rng.uniform(0.5, 1.5, (M, K))], axis=axis), lp.rows_tape([rng.standard_normal((M, K))], axis=axis)]
        nbytes = lambda with_h: tri_bytes(M, K, with_h, True)
    else:
        tapes = [qp.rows_tape([_qol_rows(M, K, 1)], axis=1)]
        gathered = int(tapes[0][0]["seg_a0_base"][0]) < 0
        return [(_device(t[0]),) + tuple(t[1:]) for t in tapes], (lambda with_h: qol_bytes(M, K, with_h, gathered)), int(gathered)
    return [(_device(t[0]),) + tuple(t[1:]) for t in tapes], nbytes, 0


def child(atom):
    for M, K in ATOMS[atom][1]:
        rows, nbytes, note = _row_tapes(atom, M, K)
        exps = {with_h: _exp_tape(exp_elements(nbytes(with_h), with_h)) for with_h in (False, True)}
        for with_h in (False, True):
            edev, ex, elam = exps[with_h]
            for _ in range(WARM + REPS):
                for dev, x, lam, sigma in rows:
                    dev.eval_h(x, lam, sigma) if with_h else dev.eval_g(x)
                edev.eval_h(ex, elam, 1.0) if with_h else edev.eval_g(ex)
        for d in [r[0] for r in rows] + [exps[False][0], exps[True][0]]:
            d.close()
        print("ran", M, K, note, flush=True)


def launches_child():
    import qol_rows_problems as qp
    a, x, lam, sigma = qp.rows_tape([_qol_rows(M, K, 2) for M, K in LAUNCH_SEGMENTS], axis=1)
    dev = _device(a)
    for _ in range(LAUNCH_SWEEPS):
        dev.eval_h(x, lam, sigma)
    dev.close()


def trace(atom, mode, extra=()):
    """The child `mode` under a kernel trace -> ([(start, kernel, ns)] of the sweep kernels in time order, the child's output)"""
    out_dir = tempfile.mkdtemp(prefix="row_trace_")
    cmd = ["rocprofv3", "--kernel-trace", *extra, "--output-format", "csv", "-d", out_dir, "-o", "rows", "--",
           sys.executable, os.path.abspath(__file__), "--atom", atom, mode]
    out = subprocess.run(cmd, cwd=ROOT, check=True, stdout=subprocess.PIPE, text=True, timeout=TRACE_LIMIT_S).stdout
    files = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit("expected one kernel trace, found %r" % files)
    names = [k for ks in KERNELS.values() for k in ks]
    rows = []
    with open(files[0]) as fh:
        for rec in csv.DictReader(fh):
            name = next((k for k in names if k in rec["Kernel_Name"]), None)    # (mangled or not)
            if name is not None:
                rows.append((int(rec["Start_Timestamp"]), name, int(rec["End_Timestamp"]) - int(rec["Start_Timestamp"])))
    rows.sort()
    return rows, out


def sweep_times(atom):
    """-> {(M, K, with_h): {stream: [ns per sweep, after the warm-up]}}, {(M, K): the child's note}"""
    shapes, streams = ATOMS[atom][1:]
    rows, out = trace(atom, "--child")
    notes = {(int(t[1]), int(t[2])): int(t[3]) for t in (ln.split() for ln in out.splitlines()) if t and t[0] == "ran"}
    pos, times = 0, {}
    for M, K in shapes:
        for with_h in (False, True):
            got = times[(M, K, with_h)] = {s: [] for s in streams}
            for rep in range(WARM + REPS):
                for s in streams:
                    L = work(atom, s, M, K)
                    part = rows[pos:pos + launches(s, L, with_h)]
                    pos += len(part)
                    if len(part) != launches(s, L, with_h) or any(p[1] not in KERNELS[s] for p in part):
                        raise SystemExit("unexpected kernel order at %d x %d: %r where %s was due" % (M, K, [p[1] for p in part], s))
                    if rep >= WARM:
                        got[s].append(sum(p[2] for p in part))
    if pos != len(rows):
        raise SystemExit("%d sweep kernels left over in the trace" % (len(rows) - pos))
    return times, notes


def shape_lines(atom):
    times, notes = sweep_times(atom)
    lines = []
    for M, K in ATOMS[atom][1]:
        if atom == "log_sum_exp":
            rec = {"M": M, "K": K, "form": form(K), "switch_group_to_wavefront": 64, "switch_wavefront_to_workgroup": 2048, "warm": WARM, "reps": REPS}
        elif atom == "prod":
            rec = {"M": M, "K": K, "form": form(K), "warm": WARM, "reps": REPS, "blocks": BLOCKS}
        elif atom == "log_det":
            rec = {"matrices": M, "n": K, "K": K * K, "form": form(K * K), "warm": WARM, "reps": REPS, "blocks": BLOCKS}
        elif atom == "matrix_frac":
            m = MFRAC_COLS[(M, K)]
            rec = {"segments": M, "n": K, "m": m, "N": K + m, "K": K * (K + m), "form": form((K + m) ** 2), "warm": WARM, "reps": REPS, "blocks": BLOCKS}
        else:
            rec = {"part": "a", "M": M, "K": K, "form": form(K), "gathered": bool(notes[(M, K)]), "warm": WARM, "reps": REPS, "blocks": BLOCKS}
        for with_h in (False, True):
            t = times[(M, K, with_h)]
            mean = {s: float(np.mean(v)) * 1e-9 for s, v in t.items()}
            tag = "h" if with_h else "noh"
            tf = mean["flat"]
            if atom == "log_sum_exp":
                nbytes, tr = tri_bytes(M, K, with_h, False), mean["lse"]
                ebytes = exp_elements(nbytes, with_h) * (40 if with_h else 24)
                rec.update({"bytes_" + tag: nbytes, "rows_us_" + tag: 1e6 * tr, "rows_us_min_" + tag: 1e-3 * float(np.min(t["lse"])),
                            "rows_GBps_" + tag: nbytes / tr * 1e-9, "flat_us_" + tag: 1e6 * tf, "flat_GBps_" + tag: ebytes / tf * 1e-9,
                            "ratio_" + tag: (nbytes / tr) / (ebytes / tf)})
            elif atom == "prod":
                nbytes, lbytes, tp, tl = tri_bytes(M, K, with_h, True), tri_bytes(M, K, with_h, False), mean["prod"], mean["lse"]
                ebytes = exp_elements(nbytes, with_h) * (40 if with_h else 24)
                rec.update({"bytes_" + tag: nbytes, "prod_us_" + tag: 1e6 * tp, "prod_us_min_" + tag: 1e-3 * float(np.min(t["prod"])),
                            "prod_TBps_" + tag: nbytes / tp * 1e-12,
                            "lse_us_" + tag: 1e6 * tl, "lse_TBps_" + tag: lbytes / tl * 1e-12, "lse_spread_" + tag: spread(t["lse"]),
                            "flat_us_" + tag: 1e6 * tf, "flat_TBps_" + tag: ebytes / tf * 1e-12,
                            "time_over_lse_" + tag: tp / tl, "byte_rate_over_flat_" + tag: (nbytes / tp) / (ebytes / tf)})
            elif atom == "log_det":
                nbytes, td, tl = tri_bytes(M, K * K, with_h, False), mean["logdet"], mean["lse"]
                ebytes = exp_elements(nbytes, with_h) * (40 if with_h else 24)
                rec.update({"bytes_" + tag: nbytes, "logdet_us_" + tag: 1e6 * td, "logdet_us_min_" + tag: 1e-3 * float(np.min(t["logdet"])),
                            "logdet_TBps_" + tag: nbytes / td * 1e-12,
                            "lse_us_" + tag: 1e6 * tl, "lse_spread_" + tag: spread(t["lse"]),
                            "flat_us_" + tag: 1e6 * tf, "time_over_lse_" + tag: td / tl})
                if not with_h:
                    rec["us_per_elimination_step"] = 1e6 * td / K
            elif atom == "matrix_frac":
                N = K + MFRAC_COLS[(M, K)]
                nbytes, tm, td, tl = tri_bytes(M, K * N, with_h, False), mean["mfrac"], mean["logdet"], mean["lse"]
                rec.update({"bytes_" + tag: nbytes, "mfrac_us_" + tag: 1e6 * tm, "mfrac_us_min_" + tag: 1e-3 * float(np.min(t["mfrac"])),
                            "mfrac_spread_" + tag: spread(t["mfrac"]),
                            "logdet_us_" + tag: 1e6 * td, "logdet_spread_" + tag: spread(t["logdet"]),
                            "lse_us_" + tag: 1e6 * tl, "lse_spread_" + tag: spread(t["lse"]), "flat_us_" + tag: 1e6 * tf,
                            "time_over_logdet_" + tag: tm / td, "time_over_lse_" + tag: tm / tl})
                if not with_h:       # (n steps on order N against log_det's N steps on order N)
                    rec.update({"us_per_elimination_step": 1e6 * tm / K, "logdet_us_per_elimination_step": 1e6 * td / N,
                                "step_over_logdet_step": (tm / K) / (td / N)})
            else:
                nbytes, tq = qol_bytes(M, K, with_h, bool(notes[(M, K)])), mean["qol"]
                ebytes = exp_elements(nbytes, with_h) * (40 if with_h else 24)
                rec.update({"bytes_" + tag: nbytes, "qol_us_" + tag: 1e6 * tq, "qol_us_min_" + tag: 1e-3 * float(np.min(t["qol"])),
                            "qol_TBps_" + tag: nbytes / tq * 1e-12, "flat_us_" + tag: 1e6 * tf, "flat_TBps_" + tag: ebytes / tf * 1e-12,
                            "flat_spread_" + tag: spread(t["flat"]), "byte_rate_over_flat_" + tag: (nbytes / tq) / (ebytes / tf)})
        lines.append(rec)
        print(json.dumps(rec), flush=True)
    return lines


def qol_loop_lines():
    """(b): the rows form against a loop of scalar atoms, host wall-clock per eval_h call"""
    import dnlp_amd as cp
    import lse_problems as lp
    import qol_rows_problems as qp
    lines = []
    for M in LOOP_M:
        U, y = _qol_rows(M, LOOP_K, 3)
        ra, rx, rlam, rsigma = qp.rows_tape([(U, y)], axis=1)
        rdev = _device(ra)
        cons = []
        for i in range(M):
            v, d = cp.Variable(LOOP_K), cp.Variable()
            v.value, d.value = U[i], y[i]
            cons.append(cp.quad_over_lin(v, d) <= 0)
        data = lp.lower(cp.Problem(cp.Minimize(0 * cp.sum(cp.Variable(1))), cons))
        la = data["tape_arrays"]
        assert list(la["seg_op"]) == [32] * M
        ldev = _device(la)
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
        rec = {"part": "b", "M": M, "K": LOOP_K, "warm": WARM, "reps": REPS, "what": "host wall-clock per eval_h call",
               "rows_us": 1e6 * float(np.mean(t_rows)), "rows_us_min": 1e6 * float(np.min(t_rows)),
               "loop_us": 1e6 * float(np.mean(t_loop)), "loop_us_min": 1e6 * float(np.min(t_loop)),
               "rows_spread": spread(t_rows), "loop_over_rows": float(np.mean(t_loop)) / float(np.mean(t_rows))}
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


def qol_launch_lines():
    """(c): launches per sweep of a tape with many segments of both forms"""
    rows, _ = trace("quad_over_lin_rows", "--launches-child", extra=("--stats",))
    names = [r[1] for r in rows if r[1] in KERNELS["qol"]]
    per_sweep = len(names) / LAUNCH_SWEEPS
    rec = {"part": "c", "segments": len(LAUNCH_SEGMENTS), "short_segments": sum(K <= 64 for _, K in LAUNCH_SEGMENTS),
           "sweeps": LAUNCH_SWEEPS, "qol_launches": len(names), "launches_per_sweep": per_sweep,
           "by_kernel": {k: names.count(k) for k in KERNELS["qol"]}}
    print(json.dumps(rec), flush=True)
    if per_sweep > 2:
        raise SystemExit("more than two launches per sweep: %r" % rec)
    return [rec]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--atom", required=True, choices=sorted(ATOMS))
    ap.add_argument("--tag", help="write profiles/<file>.<TAG>.jsonl instead of profiles/<file>.jsonl")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--launches-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.atom)
    if args.launches_child:
        return launches_child()
    lines = shape_lines(args.atom)
    if args.atom == "quad_over_lin_rows":
        lines += qol_launch_lines() + qol_loop_lines()      # (b) last: this process opens the device only after the children are gone
    name = ATOMS[args.atom][0]
    if args.tag:
        name = name[:-len("jsonl")] + args.tag + ".jsonl"
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", name), "w") as fh:
        for rec in lines:
            fh.write(json.dumps(rec) + "\n")
    if args.atom == "quad_over_lin_rows":
        # the loop form pays a stream synchronisation per segment and sweep: the rows form must be faster at the largest M
        last = [r for r in lines if r.get("part") == "b" and r.get("M") == LOOP_M[-1]][0]
        if not last["loop_over_rows"] > 1.0:
            raise SystemExit("rows form not faster than the loop of scalar atoms at M = %d: %r" % (LOOP_M[-1], last))


if __name__ == "__main__":
    main()
