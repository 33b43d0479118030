"""The unrefined KKT path of the HOST build against an independent reference (kkt_reference.py), case by case
(kkt_problems.py): one assembly + factorisation and one plain solve per right-hand side through orc_kkt_probe — no
iterative refinement, no inertia loop, no retry, which in a whole solve repair what these tests measure.

Per case: the path the case is meant for is the one taken; the backward error of the host build's solution is at most
1e-12 (a condition on the INPUTS: a case whose reference run is already sloppy would hide failures — static pivots that
grow are a reason to change the case, not the bound); inertia against the reference's; and the two yardsticks a
device run of the same cases is measured against: the forward error against the refined reference, whose own
backward error has to be at least 100x below the host build's.

The one-lane policy of the host build takes none of the all-lanes branches of csrc/sparse_ldl.h and none of the level
kernels of csrc/exec_hip.h: those run only on the device; what is asserted here for them is that the plan's numbers
select them, so that a device run of these cases (DeviceProblem.kkt_probe) reaches them.
"""
import numpy as np
import pytest

import kkt_problems as kp
import kkt_reference as ref

ETA_INPUT = 1e-12
HOST_CASES = [c.name for c in kp.CASES if c.host]


@pytest.mark.parametrize("name", HOST_CASES)
def test_host_probe_against_the_reference(name):
    case = kp.CASES_BY_NAME[name]
    h = kp.host_handle(case)
    assert h.kkt_mode() is None
    case.check_path(h, h.kkt_info(), h.kkt_tail_nodes())
    refd = kp.reference(name)
    if case.check_inputs:
        case.check_inputs(h, refd)
    res = kp.probe(h, refd["inputs"])
    assert h.kkt_mode() == case.mode
    assert res["ok"]
    assert (res["nneg"], res["nzero"]) == refd["inertia"], (res["nneg"], res["nzero"], refd["inertia"])
    if case.nzero:
        # a structurally zero pivot: reported, nothing crashes; the solution of a singular system is not compared
        assert res["nzero"] == case.nzero
        return
    eta, fe = kp.figures(refd, res)
    print("%s: eta_host %.3e fe_host %.3e eta_ref %.3e" % (name, eta, fe, refd["eta_ref"]))
    assert eta <= ETA_INPUT, eta
    # forward error: at most 2 cond eta / (1 - cond eta) for a normwise backward error eta; cond is estimated from
    # below, in practice within a factor 3 (kkt_reference.cond_estimate), and the reference's own error is negligible
    cond = ref.cond_estimate(refd["K"])
    assert cond * eta < 1e-3 and fe <= 6.0 * cond * eta, (fe, cond, eta)
    # the reference has to be far better than what it judges
    assert refd["eta_ref"] <= eta / 100.0, (refd["eta_ref"], eta)
    # the same probe again on the same handle: same bits
    res2 = kp.probe(h, refd["inputs"])
    assert np.array_equal(res["sol"], res2["sol"]) and (res2["nneg"], res2["nzero"]) == (res["nneg"], res["nzero"])


@pytest.mark.parametrize("name", HOST_CASES)
def test_assembly_positions_are_unique(name):
    """The assemblies of csrc/kkt_dense.h add Hessian values with += and store Jacobian values with = inside parallel
    maps: no two entries of either pattern may share a position."""
    h = kp.host_handle(kp.CASES_BY_NAME[name])
    hr, hc = h.hess_structure()
    assert np.all(hr >= hc) and np.unique(hr.astype(np.int64) * h.n + hc).size == hr.size
    if h.m:
        jr, jc = h.jac_structure()
        assert np.unique(jr.astype(np.int64) * h.n + jc).size == jr.size


def test_overlap_case_overlaps():
    """... and in the overlap case at least three atoms feed one Hessian entry (merged by the tape's map MH)."""
    data, _ = kp.lowered("overlap-sparse")
    assert np.diff(data["tape_arrays"]["MH_ptr"]).max() >= 3


def test_indefinite_block_is_indefinite():
    """The case that checks the 2x2 pivots' inertia rule: static pairs with a < 0 and det > 0 (two negative eigenvalues
    from one block, kkt_problems._check_two_negative_pairs), pairs with det < 0, more negative eigenvalues than
    constraint rows, no regularisation."""
    refd = kp.reference("bilinear-sparse")
    h = kp.host_handle(kp.CASES_BY_NAME["bilinear-sparse"])
    kp.CASES_BY_NAME["bilinear-sparse"].check_inputs(h, refd)
    assert refd["inertia"][0] >= h.m + kp.CONCAVE_PAIRS and refd["inputs"]["delta_w"] == 0.0
    assert h.kkt_info()["pairs_2x2"] == h.m


def test_fixed_variables_cover_a_shared_one_and_an_equality():
    case = kp.CASES_BY_NAME["arrow-fixed-sparse"]
    h = kp.host_handle(case)
    fm = kp.reference(case.name)["inputs"]["fixmask"]
    jr, jc = h.jac_structure()
    assert fm.sum() >= h.n // 10 and fm[jc].any()


def test_probe_misuse_is_reported():
    case = kp.CASES_BY_NAME["hs071-sparse"]
    h = kp.host_handle(case)
    inp = kp.reference(case.name)["inputs"]
    nneg, nzero = kp.ctypes.c_int(), kp.ctypes.c_int()
    rc = h.api.kkt_probe(h.ptr, None, None, 1.0, None, None, None, 0.0, 0, None, None, kp.ctypes.byref(nneg), kp.ctypes.byref(nzero))
    assert rc == -199 and "kkt_probe" in h.api.error()
    with pytest.raises(ValueError):
        h.kkt_probe(inp["x"][:-1], inp["lam"], 1.0, inp["Sx"], inp["D"])
    # no right-hand side: the inertia alone
    res = h.kkt_probe(inp["x"], inp["lam"], 1.0, inp["Sx"], inp["D"])
    assert res["ok"] and res["sol"].shape == (0, h.n + h.m)


@pytest.mark.parametrize("name", ["hs071-sparse", "hs071-dense", "sparse-recovery-paired", "phase-retrieval-tail"])
def test_probe_leaves_no_state_that_changes_a_later_solve(name):
    """solve -> probe -> solve on one handle against solve -> solve on another: identical bits."""
    from dnlp_amd.nlp_solver import HIPNLP
    case = kp.CASES_BY_NAME[name]
    data, _ = kp.lowered(name)
    runs = []
    for with_probe in (True, False):
        h = kp.host_handle(case)
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
