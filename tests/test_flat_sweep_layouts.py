"""csrc/exec_hip.h sweep_flat_kernel (and the host loop of csrc/model.h over the same table) on every path, element by element
against mpmath (tests/atom_reference.py): the double2 path, the scalar path for a contiguous argument at an odd offset, gathered
arguments, lanes whose two units lie in different segments, blocks of nothing but segment starts, block boundaries inside
segments, a partial last block.

How the layouts are made.  Through the front-end every atom argument becomes a contiguous block of variables of its own, so
even and odd offsets come from the segment lengths.  The tape stores every argument's index list in gidx whether or not it is
contiguous, and every evaluator reads gidx when seg_a0_base / seg_a1_base is -1: a gathered argument is the front-end's segment
with its base set to -1 and its gidx entries permuted.  The Jacobian / Hessian maps (MJ, MH) were derived from the index lists at
lowering time and are NOT permuted with them: such a tape is no longer the derivative of one function, it is a table that says
"unit i reads x[gidx[perm i]] and its outputs go where MJ / MH send slot i", which is all the sweep knows about.  The expected
values follow the same statement, from the permuted indices.

Every evaluation at the test point is preceded by one at another point, so that a unit the sweep skipped holds a stale value of
the other point and not the right one from an earlier call."""
import numpy as np
import pytest

import atom_reference as ar
import dnlp_amd as cp
from dnlp_amd.dnlp2smooth import Dnlp2Smooth
from dnlp_amd.nlp_solver import build_nlp_data
from dnlp_amd.tape import serialize
from oracle.tape_eval import (OP_ASINH, OP_ATANH, OP_COS, OP_ENTR, OP_EXP, OP_LOG, OP_LOGISTIC, OP_MATMUL, OP_MUL,
                              OP_POWER, OP_REL_ENTR, OP_SIN, OP_SINH, OP_TAN, OP_TANH, OP_XEXP)
from test_atom_rules import _all_checks, _Callbacks, _multipliers

LENGTHS = [1, 2, 3, 63, 64, 65, 255, 257, 511, 512, 513, 1023, 1025, 4099]
UNARY = ["exp", "log", "entr", "logistic", "sin", "cos", "tan", "sinh", "tanh", "asinh", "atanh", "xexp", "power"]
OPCODE = {"exp": OP_EXP, "log": OP_LOG, "entr": OP_ENTR, "logistic": OP_LOGISTIC, "sin": OP_SIN, "cos": OP_COS, "tan": OP_TAN,
          "sinh": OP_SINH, "tanh": OP_TANH, "asinh": OP_ASINH, "atanh": OP_ATANH, "xexp": OP_XEXP, "power": OP_POWER,
          "mul": OP_MUL, "rel_entr": OP_REL_ENTR}
# planted at the first and the last element of a segment (an off-by-one hands them to the neighbour's op); 0 for log / entr
# and 1 for atanh are edges of the domain: the IEEE class is compared there
PLANTED = {OP_EXP: (650.0, -650.0), OP_LOG: (0.0, 1e300), OP_ENTR: (0.0, 1e-300), OP_LOGISTIC: (710.5, -800.0),
           OP_SIN: (1e22, np.pi / 2), OP_COS: (np.pi / 2, 1e22), OP_TAN: (np.pi / 2, 1e10), OP_SINH: (650.0, -650.0),
           OP_TANH: (19.1, -1e4), OP_ASINH: (1e100, -1e-100), OP_ATANH: (1.0 - 2.0 ** -53, 1.0), OP_XEXP: (650.0, -650.0),
           OP_POWER: (-2.0, 1e30)}


def _var(shape):
    v = cp.Variable(shape)
    v.value = np.full(shape, 0.5)
    return v


def _atom(kind, n):
    if kind == "power":
        return cp.power(_var(n), 3)
    if kind == "mul":
        return cp.multiply(_var(n), _var(n))
    if kind == "rel_entr":
        return cp.rel_entr(_var(n), _var(n))
    if isinstance(kind, tuple):                      # ("matmul", m, k, p)
        return _var((kind[1], kind[2])) @ _var((kind[2], kind[3]))
    return getattr(cp, kind)(_var(n))


def _units(kind, n):
    return kind[1] * kind[3] if isinstance(kind, tuple) else n


def _plan(name):
    """[(kind, n)] in tape order; the first two go into the objective."""
    if name == "long":
        # (two even lengths first: x, z, dvals and hvals offsets all start even, the double2 path)
        plan = [("sinh", 512), ("tanh", 66)]
        k = 0
        for rep, order in enumerate((LENGTHS, [513, 3, 1025, 2, 65, 1, 4099, 63, 257, 64, 511, 255, 1023, 512])):
            for n in order:
                plan.append((UNARY[k % len(UNARY)], n))
                k += 1
                if n in (3, 65, 513):
                    plan.append(("mul", n + 4))
                if n in (2, 257, 1023):
                    plan.append(("rel_entr", n + 1))
                if n == 64:
                    plan.append((("matmul", 3, 1 if rep == 0 else 65, 5), 0))
                if n == 255:
                    # (inner dimension 2 with an even number of outputs: the hvals offset keeps the parity of the z offset)
                    plan.append((("matmul", 6, 2, 9) if rep == 0 else ("matmul", 7, 7, 9), 0))
            if rep == 0:
                # 700 one-element segments, from just before a block boundary on: one whole block of nothing but segment starts
                pad = (-sum(_units(kind, n) for kind, n in plan) - 5) % 512 or 512
                plan += [("asinh", pad)] + [(UNARY[i % len(UNARY)], 1) for i in range(700)]
        return plan
    total = int(name)
    plan = [("tanh", 3), ("exp", 64), ("mul", 5), ("log", 65), ("sin", 1), ("rel_entr", 6), ("atanh", 2),
            (("matmul", 2, 7, 3), 0), ("xexp", 63), ("power", 100), ("cos", 1), ("entr", 1)]
    used = sum(_units(k, n) for k, n in plan)
    return plan + [("asinh", total - used - 33), ("logistic", 33)]


_built = {}


def _tape(name):
    """-> (tape arrays, x, another x, multipliers, sigma)."""
    if name in _built:
        return _built[name]
    plan = _plan(name)
    atoms = [_atom(k, n) for k, n in plan]
    cons = [(e == 0) if isinstance(k, tuple) or k == "mul" else (e <= 0) for (k, n), e in zip(plan[2:], atoms[2:])]
    prob = cp.Problem(cp.Minimize(cp.sum(atoms[0]) + cp.sum(atoms[1])), cons)
    smooth, _ = Dnlp2Smooth().apply(prob)
    data, _ = build_nlp_data(smooth)
    a = dict(data["tape_arrays"])
    want = [OP_MATMUL if isinstance(k, tuple) else OPCODE[k] for k, n in plan]
    assert list(a["seg_op"]) == want, "the lowering reordered or merged segments"
    rng = np.random.default_rng(31 + len(plan))
    for key in ("seg_a0_base", "seg_a1_base", "gidx"):
        a[key] = a[key].copy()
    N, m = int(a["dims"][0]), int(a["dims"][1])
    x, x_other = rng.uniform(0.1, 0.9, N), rng.uniform(0.1, 0.9, N)
    planted = set()
    for s, (kind, n) in enumerate(plan):
        op = int(a["seg_op"][s])
        o0, l0 = int(a["seg_a0_off"][s]), int(a["seg_a0_len"][s])
        if op < OP_MUL:
            # every third unary segment of two or more elements is gathered: base -1 and its index list permuted
            if l0 >= 2 and s % 3 == 1:
                a["seg_a0_base"][s] = -1
                a["gidx"][o0:o0 + l0] = a["gidx"][o0:o0 + l0][rng.permutation(l0)]
            if l0 >= 3 and op not in planted:
                planted.add(op)
                idx = a["gidx"][o0:o0 + l0]
                x[idx[0]], x[idx[-1]] = PLANTED[op]
        elif op in (OP_MUL, OP_REL_ENTR):
            # each argument contiguous or gathered: the four combinations in turn
            o1, l1 = int(a["seg_a1_off"][s]), int(a["seg_a1_len"][s])
            combo = s % 4
            if combo & 1:
                a["seg_a0_base"][s] = -1
                a["gidx"][o0:o0 + l0] = a["gidx"][o0:o0 + l0][rng.permutation(l0)]
            if combo & 2:
                a["seg_a1_base"][s] = -1
                a["gidx"][o1:o1 + l1] = a["gidx"][o1:o1 + l1][rng.permutation(l1)]
    _built[name] = (a, x, x_other, _multipliers(m), 0.5)
    return _built[name]


def _facts(a):
    """What the flat table of this tape (csrc/tape.h: one row per elementwise-class segment, one unit per output element,
    two consecutive units per lane, 512 per workgroup) puts in front of the kernel."""
    flat = [s for s in range(int(a["dims"][3])) if a["seg_op"][s] < 30 or a["seg_op"][s] == OP_MATMUL]
    units = [int(a["seg_d0"][s] * a["seg_d2"][s]) if a["seg_op"][s] == OP_MATMUL else int(a["seg_n"][s]) for s in flat]
    start = np.concatenate([[0], np.cumsum(units)])
    total = int(start[-1])
    f = dict(total=total, double2=0, contiguous_odd=0, gathered_unary=0, boundary_inside=0, straddle=0, blocks_of_starts=0,
             gathered_binary=set(), matmul_inner=set(), last_unit_alone=int(total % 2 == 1))
    for r, s in enumerate(flat):
        op, b0, b1 = int(a["seg_op"][s]), int(start[r]), int(start[r + 1])
        if op < OP_MUL:
            e0 = b0 + (b0 & 1)                                    # the first lane that starts inside the segment
            has_pair = e0 + 1 < b1
            i = e0 - b0
            offs = [int(a[k][s]) + i for k in ("seg_a0_base", "seg_zoff", "seg_doff", "seg_hoff")]
            if a["seg_a0_base"][s] < 0:
                f["gathered_unary"] += int(b1 - b0 >= 2)
            elif has_pair and all(o % 2 == 0 for o in offs):
                f["double2"] += 1
            elif has_pair:
                f["contiguous_odd"] += 1
        elif op in (OP_MUL, OP_REL_ENTR):
            f["gathered_binary"].add((op, bool(a["seg_a0_base"][s] < 0), bool(a["seg_a1_base"][s] < 0)))
        else:
            f["matmul_inner"].add(int(a["seg_d1"][s]))
        if (b0 // 512) != ((b1 - 1) // 512) and b1 - b0 >= 2:
            f["boundary_inside"] += 1
        if (b1 - 1) % 2 == 0 and b1 < total:                      # the lane of unit b1 - 1 takes unit b1 of the next segment
            f["straddle"] += 1
    for blk in range(total // 512):
        inside = (start[:-1] >= 512 * blk) & (start[:-1] < 512 * (blk + 1))
        f["blocks_of_starts"] += int(inside.sum() == 512)
    return f


def _assert_layout(name):
    a = _tape(name)[0]
    f = _facts(a)
    assert f["double2"] >= 1 and f["contiguous_odd"] >= 1 and f["gathered_unary"] >= 1 and f["straddle"] >= 1, f
    assert len(f["gathered_binary"]) >= 2, f
    if name == "long":
        assert f["total"] >= 20000 and f["total"] % 512 not in (0, 1), f
        assert f["double2"] >= 2 and f["contiguous_odd"] >= 4 and f["gathered_unary"] >= 4 and f["boundary_inside"] >= 8, f
        assert f["blocks_of_starts"] >= 1 and f["straddle"] >= 8, f
        assert len(f["gathered_binary"]) == 8 and f["matmul_inner"] == {1, 2, 7, 65}, f
    else:
        assert f["total"] == int(name), f
        assert f["last_unit_alone"] == int(name) % 2
        if int(name) == 513:
            assert f["boundary_inside"] >= 1, f
    return f


def _check(ev, name):
    a, x, x_other, lam, sigma = _tape(name)
    exp = ar.expected_oracles(a, x, lam, sigma)
    lam_other = lam[::-1].copy()

    def after_another_point(thunk, with_h):
        def run():
            ev.eval_h(x_other, lam_other, 2.0) if with_h else ev.eval_jac_g(x_other)
            return thunk()
        return run

    _all_checks([
        (exp["jac"], after_another_point(lambda: ev.eval_jac_g(x), True)),               # the sweep without the Hessian values
        (exp["hess"], after_another_point(lambda: ev.eval_h(x, lam, sigma), True)),      # with them: every element its own weight
        (exp["g"], after_another_point(lambda: ev.eval_g(x), False)),
        (exp["grad_f"], after_another_point(lambda: ev.eval_grad_f(x), False)),
    ])


NAMES = ["511", "512", "513", "long"]


@pytest.mark.parametrize("name", NAMES)
def test_the_tape_holds_the_layouts_it_was_built_for(name):
    _assert_layout(name)


@pytest.mark.parametrize("name", NAMES)
def test_numpy_evaluator_on_the_layouts(name):
    """The expectations (mpmath through the tape's maps, permuted gathers included) against the numpy tape evaluator."""
    _assert_layout(name)
    _check(_Callbacks(_tape(name)[0]), name)


@pytest.mark.parametrize("name", NAMES)
def test_host_loops_on_the_layouts(name):
    """csrc/model.h sweep_flat over host loops (one unit at a time, a binary search per unit) on the same tables: a failure of
    the device test alone then points at the kernel."""
    from oracle.oracle_capi import OracleProblem
    _assert_layout(name)
    _check(OracleProblem(serialize(_tape(name)[0])), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_sweep_flat_kernel_on_the_layouts(name, gpu_required):
    """sweep_flat_kernel: eval_jac_g (without Hessian values) and eval_h (with, multipliers differing from one element to the
    next), eval_g and eval_grad_f, each entry against mpmath."""
    from dnlp_amd import _capi
    _assert_layout(name)
    dev = _capi.DeviceProblem(serialize(_tape(name)[0]), None, device=0)
    try:
        _check(dev, name)
    finally:
        dev.close()
