"""The unrefined KKT path of the DEVICE build (DeviceProblem.kkt_probe) on the cases of kkt_problems.py, measured against
the host build's probe of the same case and the refined reference of kkt_reference.py (test_kkt_probe_cpu.py holds the
host build to that reference).

Per case: the path the case is meant for is the one the device handle takes (kkt_info / kkt_tail_nodes before, kkt_mode
after; for a sparse plan the device's numbers equal the host's, whose level statistics the path check reads); inertia
equal to the reference's; two probes on one handle return equal bits; and

    eta_dev <= M max(eta_host, n_row 2^-53)        fe_dev <= M max(fe_host, n_row 2^-53)

n_row is the largest number of terms summed into one entry: for a sparse plan the larger of kkt_info()'s max_struct and
the longest update group of a level, for a dense path the order of the matrix (a dot product of the factorisation runs
over a whole row).  Device and host run the same pivot sequence, so element growth is the same; only the order of the
sums differs (tree against serial), which is worth a small factor: M = 4, the starting value of a small power of two.
Bunch-Kaufman's device form (blocked, chip-wide) may choose other pivots than the host's where two candidates are within
rounding of each other; the bound is the same.

Every measured figure goes to profiles/kkt_probe.jsonl, one line per case, rewritten by each run of this file.

The level-kernel cases run with DNLP_LEVEL_FUSION and DNLP_LEVEL_GRAPHS on and off (set before the handle exists): the
four runs return identical bits — the level kernels gather every destination in a fixed order and hold no
floating-point atomics.  (Plans with a dense tail — panel gathers and the MFMA tail product in the level loop — are not in
that comparison.)
"""
import json
import os

import numpy as np
import pytest

import kkt_problems as kp

pytestmark = pytest.mark.gpu

M = 4.0
UNIT = 2.0 ** -53
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "kkt_probe.jsonl")
_written = []


def _record(row):
    first = not _written
    _written.append(row["case"])
    os.makedirs(os.path.dirname(PROFILE), exist_ok=True)
    with open(PROFILE, "w" if first else "a") as fh:
        if first:
            fh.write(json.dumps({"file": "written by tests/test_kkt_probe_gpu.py on an MI355X, one line per case",
                                 "bound": "eta_dev <= M max(eta_host, n_row 2^-53), fe_dev <= M max(fe_host, n_row 2^-53)",
                                 "M": M, "M_measured_on_device": "by the run that wrote this file: see the ratios"}) + "\n")
        fh.write(json.dumps(row) + "\n")


def _device_handle(case):
    from dnlp_amd import _capi
    data, blob = kp.lowered(case.name)
    h = _capi.DeviceProblem(blob, data["tape"], device=0)
    kp.apply_options(h, case)
    return h


def _n_row(hf):
    if hf["info"]["sparse"]:
        return max([hf["info"]["max_struct"], 1] + [v["max_group"] for v in hf["levels"]])
    return hf["order"]


def _check_path(case, dev, hf):
    info, tail = dev.kkt_info(), dev.kkt_tail_nodes()
    if info["sparse"]:
        assert info == hf["info"], (info, hf["info"])       # the host plan's level numbers describe the device's plan
    case.check_path(kp.host_handle(case), info, tail)


def _probe_and_check(case, dev, refd, hf):
    res = kp.probe(dev, refd["inputs"])
    assert dev.kkt_mode() == case.mode
    assert res["ok"]
    assert (res["nneg"], res["nzero"]) == refd["inertia"], (res["nneg"], res["nzero"], refd["inertia"])
    return res


def _bounds(case, refd, hf, res, extra=None):
    eta, fe = kp.figures(refd, res)
    floor = _n_row(hf) * UNIT
    row = dict(case=case.name, n_row=_n_row(hf), eta_host=hf["eta"], eta_dev=eta, fe_host=hf["fe"], fe_dev=fe,
               eta_ratio=eta / max(hf["eta"], floor), fe_ratio=fe / max(hf["fe"], floor), eta_ref=refd["eta_ref"])
    row.update(extra or {})
    print(json.dumps(row))
    _record(row)
    assert eta <= M * max(hf["eta"], floor), row
    assert fe <= M * max(hf["fe"], floor), row


@pytest.mark.parametrize("name", [c.name for c in kp.CASES if not c.grid])
def test_device_probe_against_the_host_build_and_the_reference(name, gpu_required):
    case = kp.CASES_BY_NAME[name]
    refd, hf = kp.reference(name), kp.host_figures(name)
    dev = _device_handle(case)
    assert dev.kkt_mode() is None
    _check_path(case, dev, hf)
    res = _probe_and_check(case, dev, refd, hf)
    if case.nzero:
        assert res["nzero"] == case.nzero
        _record(dict(case=name, nneg=res["nneg"], nzero=res["nzero"]))
        return
    res2 = kp.probe(dev, refd["inputs"])
    assert np.array_equal(res["sol"], res2["sol"]) and (res2["nneg"], res2["nzero"]) == (res["nneg"], res["nzero"])
    _bounds(case, refd, hf, res)


@pytest.mark.parametrize("name", [c.name for c in kp.CASES if c.grid])
def test_level_kernels_with_fusion_and_graph_replay_on_and_off(name, gpu_required, monkeypatch):
    case = kp.CASES_BY_NAME[name]
    refd, hf = kp.reference(name), kp.host_figures(name)
    sols = []
    for fusion, graphs in (("1", "1"), ("0", "1"), ("1", "0"), ("0", "0")):
        monkeypatch.setenv("DNLP_LEVEL_FUSION", fusion)
        monkeypatch.setenv("DNLP_LEVEL_GRAPHS", graphs)
        dev = _device_handle(case)
        if not sols:
            _check_path(case, dev, hf)
        res = _probe_and_check(case, dev, refd, hf)
        res2 = kp.probe(dev, refd["inputs"])                # (with graphs on: the captured level loops, replayed)
        assert np.array_equal(res["sol"], res2["sol"]), (fusion, graphs)
        sols.append(res["sol"])
    same = [bool(np.array_equal(sols[0], s)) for s in sols[1:]]
    _bounds(case, refd, hf, dict(sol=sols[0]), extra={"same_bits_fusion0_graphs1": same[0], "same_bits_fusion1_graphs0": same[1],
                                                      "same_bits_fusion0_graphs0": same[2]})
    assert all(same), same


@pytest.mark.parametrize("name", ["hs071-sparse", "hs071-dense", "sparse-recovery-paired", "phase-retrieval-tail"])
def test_probe_leaves_no_state_that_changes_a_later_solve(name, gpu_required):
    """solve -> probe -> solve on one handle against solve -> solve on another: identical bits."""
    from dnlp_amd.nlp_solver import HIPNLP
    case = kp.CASES_BY_NAME[name]
    data, _ = kp.lowered(name)
    runs = []
    for with_probe in (True, False):
        h = _device_handle(case)
        for k, v in HIPNLP.DEFAULT_OPTIONS.items():
            h.set_option(k, v)
        h.set_option("max_iter", 25)
        a = h.solve(data["x0"])
        if with_probe:
            assert kp.probe(h, kp.reference(name)["inputs"])["ok"]
        mode = h.kkt_mode()
        b = h.solve(data["x0"])
        runs.append((a, b, mode))
    (a1, b1, m1), (a2, b2, m2) = runs
    assert m1 == m2
    for u, v in ((a1, a2), (b1, b2)):
        assert u["status"] == v["status"] and u["iterations"] == v["iterations"]
        for key in ("x", "mult_g", "mult_x_L", "mult_x_U"):
            assert np.array_equal(u[key], v[key]), key
        assert u["obj_val"] == v["obj_val"]
