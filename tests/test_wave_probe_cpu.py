"""The unrefined KKT path of the WAVEFRONT BATCH SOLVER's own restatement of the linear algebra (dnlp_amd/csrc/wave_ipm.h:
assemble_factor, ldl_factor, ldl_solve alone and for two systems, kkt_residual alone and for two systems, the dense tail;
wave_gen.h / wave_gen_rt.h: the generated phases) against the independent reference of kkt_reference.py, case by case
(wave_probe_problems.py), through WaveIpm::probe: one factorisation and plain solves — no refinement, no inertia loop, no
retry, which in a whole solve repair what these tests measure.

On the CPU the text runs on ONE host lane (its lane-strided loops are serial, its reductions plain sums): held to the
bounds test_kkt_probe_cpu.py holds the host build to, pinned bit for bit on the generic text (which = 1) and on the
generated text played for 64 and 256 lanes.  What only exists on the device (v_readlane, DPP sums, 16-bit tables, LDS
windows, address-space typing) is test_wave_probe_gpu.py's, which measures against the figures computed here."""
import numpy as np
import pytest

import kkt_reference as ref
import wave_probe_problems as wp

ETA_INPUT = 1e-12
KEYS = ("sol", "sol2", "res", "nneg", "nzero", "ok")


def _count(name):
    return 2 if name in wp.LARGE else wp.N_INST


def _same(a, b):
    return {k: bool(np.array_equal(a[k], b[k], equal_nan=True)) for k in KEYS}


@pytest.mark.parametrize("name", list(wp.TEMPLATES))
def test_case_selects_the_path_it_is_named_for(name):
    t = wp.template(name)
    t.check(t)


@pytest.mark.parametrize("name,pt", wp.CASES)
def test_host_lane_against_the_reference(name, pt):
    t, p, B = wp.template(name), wp.points(name)[pt], _count(name)
    res = wp.host_lane(name, pt, B)
    assert res["ok"].all()
    for i in range(B):
        r = wp.reference(name, pt, i)
        nneg_ref, nzero_ref = wp.inertia(name, pt, i)
        assert (int(res["nneg"][i]), int(res["nzero"][i])) == (nneg_ref, nzero_ref), (i, res["nneg"][i], res["nzero"][i], nneg_ref, nzero_ref)
        if pt == "indefinite":
            assert nneg_ref > t.m, (nneg_ref, t.m)           # the inertia count on something other than (N, m, 0)
        if pt == "fixed":
            assert wp.data_fixed(t, p.mat[i:i + 1])[0][p.fixmask != 0.0].all() and p.fixmask.sum() >= t.N // 7
        eta, fe = wp.figures(name, pt, i, res)
        assert eta <= ETA_INPUT, (i, eta)
        cond = ref.cond_estimate(r.K)
        assert cond * eta < 1e-3 and fe <= 6.0 * cond * eta, (i, fe, cond, eta)
        assert max(r.eta_ref) <= eta / 100.0, (i, r.eta_ref, eta)       # the reference is far better than what it judges
        # the kernel's own residual rhs - K v, single and two-system form, against the longdouble one: componentwise within the
        # forward bound of a dot product of n_row terms (n_row: the longest row of the merged matrix)
        assert wp.residual_excess(name, pt, i, res) <= 1.0, i
    # the joint solve returns the bits of the two single solves; the two-system residual's first system those of the single pass
    assert np.array_equal(res["sol2"], res["sol"][:, :2])
    assert np.array_equal(res["res"][:, 1], res["res"][:, 0])
    print("%s/%s: eta_host %.3e fe_host %.3e" % (name, pt, *np.max([wp.figures(name, pt, i, res) for i in range(B)], axis=0)))


@pytest.mark.parametrize("name,pt", wp.CASES)
def test_restatement_equals_the_generic_text_bit_for_bit(name, pt):
    """which = 0 (wave_ipm.h on one host lane) against which = 1 (Model / DenseKkt / Ipm over the host space with the template's
    plan): solutions, residuals, inertia — the pin that until now existed only through whole solves."""
    B = _count(name)
    w = wp.host_lane(name, pt, B)
    g = wp.host_probe(wp.template(name).hb, wp.inputs(name, pt, B), 1)
    assert all(_same(w, g).values()), _same(w, g)


@pytest.mark.parametrize("lanes", [64, 256])
@pytest.mark.parametrize("name", list(wp.TEMPLATES))
def test_generated_host_text_equals_the_interpreted_host_lane(name, lanes):
    """The per-template straight-line phases (wave_gen.h) played for 64 lanes, and for the 256 lanes of a workgroup of four
    wavefronts (staging and windows in the text), inside the same probe: the bits of the interpreted walk, joint solve included."""
    from wave_gen_host import GenHostBatch
    t = wp.template(name)
    g = GenHostBatch(t.pb, t.opts, lanes=lanes)
    assert ("#define WG_LANES %d" % lanes) in g.source or lanes == 64
    for pt in wp.POINTS_OF[name]:
        w = wp.host_lane(name, pt, 2)
        r = g.probe_gen(wp.inputs(name, pt, 2))
        assert all(_same(w, r).values()), (pt, _same(w, r))
        assert np.array_equal(r["sol2"], r["sol"][:, :2])


def test_which_templates_have_the_singular_point():
    assert [n for n in wp.TEMPLATES if wp.singular_row(wp.template(n)) is not None] == wp.SINGULAR


@pytest.mark.parametrize("name", wp.SINGULAR)
def test_an_exactly_zero_static_pivot_is_counted_alike_in_every_host_build(name):
    """The inertia-only point: D = 0 on the equality rows and on one first-level 1x1 inequality row, delta_w = 0.  nzero > 0
    and the ok flag, nneg too, equal between the host lane, the generic text and the generated text; solutions are not compared."""
    from wave_gen_host import GenHostBatch
    t = wp.template(name)
    assert wp.points(name)["singular"].D[wp.singular_row(t)] == 0.0 and wp.points(name)["singular"].dw == 0.0
    w = wp.host_lane(name, "singular", wp.N_INST)
    assert (w["nzero"] > 0).all()
    g = wp.host_probe(t.hb, wp.inputs(name, "singular", wp.N_INST), 1)
    r = GenHostBatch(t.pb, t.opts, lanes=64).probe_gen(wp.inputs(name, "singular", wp.N_INST))
    for other in (g, r):
        for k in ("nneg", "nzero", "ok"):
            assert np.array_equal(w[k], other[k]), k


@pytest.mark.parametrize("name", wp.TAILED)
def test_dense_tail_on_and_off_gives_equal_bits_on_the_host_lane(name, monkeypatch):
    """DNLP_WAVE_NO_TAIL=1: the level code for the same chain.  The tail's sums are those of the level code,
    so a host lane that owns every tail row returns the same bits — also for the width-32 tail and the truncated one."""
    from wave_oracle import HostBatch
    t = wp.template(name)
    for pt in wp.POINTS_OF[name]:
        w = wp.host_lane(name, pt, 2)
        monkeypatch.setenv("DNLP_WAVE_NO_TAIL", "1")
        hb = HostBatch(t.pb, t.opts)
        assert wp.wave_hdr(hb)["tail_T"] == 0 and t.hdr["tail_T"] > 0
        off = wp.host_probe(hb, wp.inputs(name, pt, 2), 0)
        monkeypatch.delenv("DNLP_WAVE_NO_TAIL")
        assert all(_same(w, off).values()), (pt, _same(w, off))


def test_probe_misuse_is_reported():
    t = wp.template("circle_packing4")
    inp = wp.inputs("circle_packing4", "interior", 2)
    h = t.hb.handle
    rc = h.api.batch_kkt_probe(h.ptr, 2, None, t.mat.shape[1], None, None, None, None, 0.0, 0, None, None, None, None, None, None, None, None)
    assert rc == -199 and "wave_probe" in h.api.error()
    with pytest.raises(RuntimeError, match="wave_probe.*stride"):
        h.batch_kkt_probe(inp["data"][:, :-1], inp["x"], inp["lagrange"], inp["Sx"], inp["D"])
    with pytest.raises(ValueError):
        h.batch_kkt_probe(inp["data"], inp["x"][:, :-1], inp["lagrange"], inp["Sx"], inp["D"])
    with pytest.raises(ValueError):
        h.batch_kkt_probe(inp["data"], inp["x"], inp["lagrange"], inp["Sx"], inp["D"], rhs=inp["rhs"][:, :, :-1])
    with pytest.raises(ValueError):
        h.batch_kkt_probe(inp["data"], inp["x"], inp["lagrange"], inp["Sx"], inp["D"], rhs=inp["rhs"][:, :1], v=inp["v"])
    # the handle's binding is the host lane; no right-hand side: the inertia alone
    res = h.batch_kkt_probe(inp["data"], inp["x"], inp["lagrange"], inp["Sx"], inp["D"])
    assert res["ok"].all() and res["sol"].shape == (2, 0, t.n) and res["sol2"] is None and res["res"] is None
    full = h.batch_kkt_probe(inp["data"], inp["x"], inp["lagrange"], inp["Sx"], inp["D"], inp["delta_w"], inp["rhs"], inp["v"])
    w = wp.host_lane("circle_packing4", "interior", 2)
    assert all(_same(w, full).values())


def test_a_template_the_wavefront_solver_refuses_gives_its_reason():
    """A dense quad_form block (problem_zoo) is not the wavefront solver's: a negative code and the reason, no result."""
    import problem_zoo as zoo
    from dnlp_amd.batch import instance_data, lower_arrays
    from dnlp_amd.tape import serialize
    from oracle.oracle_capi import OracleProblem
    import dnlp_amd as cp
    arrays = lower_arrays(zoo.portfolio_qp(cp))[0]
    h = OracleProblem(serialize(arrays))
    row = instance_data(arrays)[None, :]
    z = lambda w: np.zeros((1, max(w, 1)))
    with pytest.raises(RuntimeError, match="the wavefront solver does not take this launch"):
        h.batch_kkt_probe(row, z(h.n), z(h.m), z(h.n), z(h.m))
