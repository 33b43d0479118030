"""The unrefined KKT path of the wavefront batch solver ON THE DEVICE (dnlp_batch_kkt_probe -> WaveIpm::probe through the
probe entry points of wave_batch.h, wave_spec_kernel.h and wave_wg_kernel.h), form by form, on the cases of
wave_probe_problems.py, measured against the host lane's probe of the same case and the refined reference of
kkt_reference.py (test_wave_probe_cpu.py holds the host lane to that reference).

What the host lane cannot see runs here: the dense tail through v_readlane, the DPP sums of the wide forms and of the
all-lanes group sums, the 16-bit tables, the workgroup kernel's LDS ranges, staged phases, windows and right-hand sides typed
by address space, the TWO_PER_SIMD instantiation.  Each form is selected with the switches a solve obeys and asserted from
the launch record.  Per case, form and instance:

    eta_dev <= M max(eta_host, n_row 2^-53)        fe_dev <= M max(fe_host, n_row 2^-53)        M = 4

(test_kkt_probe_gpu.py's rule; n_row: the longest sum into one entry — the longest update group or forward gather of the plan,
T for the tail), the kernel's own residual within M times the componentwise bound of the CPU test, and
nneg / nzero equal to the reference inertia.  Every figure goes to profiles/wave_probe.jsonl, one line per case and form,
rewritten by each run of this file.  One device handle per template and form (a per-template kernel is compiled once)."""
import json
import os

import numpy as np
import pytest

import wave_probe_problems as wp

pytestmark = pytest.mark.gpu

M = 4.0
UNIT = 2.0 ** -53
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "wave_probe.jsonl")
SWITCHES = ("DNLP_BATCH_WAVE", "DNLP_WAVE_SPEC", "DNLP_WAVE_SPEC_TABLES", "DNLP_WAVE_FORM", "DNLP_WAVE_NO_TAIL", "DNLP_WAVE_WG_WAVES",
            "DNLP_WAVE_WG_SMALL", "DNLP_WAVE_WG_WINDOWS", "DNLP_WAVE_STAGE", "DNLP_WAVE_WG_LDS")
KEYS = ("sol", "sol2", "res", "nneg", "nzero", "ok")
_written = []
_handles = {}

# form label -> (switches, what the launch record must say)
LIB = {"DNLP_WAVE_SPEC": "0"}
FORMS = {
    "lib-x11": (LIB, lambda L: L["wave_form"] % 100 == 11 and not L["wave_spec"] and not L["wave_wg"]),
    "lib-110": (dict(LIB, DNLP_WAVE_FORM="110"), lambda L: L["wave_form"] == 110 and not L["wave_spec"] and not L["wave_wg"]),
    "lib-x10": (LIB, lambda L: L["wave_form"] % 100 == 10 and not L["wave_spec"] and not L["wave_wg"]),
    "lib-400": (dict(LIB, DNLP_BATCH_WAVE="2"), lambda L: L["wave_form"] == 400 and not L["wave_spec"] and not L["wave_wg"]),
    "lib-x10-notail": (dict(LIB, DNLP_WAVE_NO_TAIL="1"), lambda L: L["wave_form"] % 100 == 10 and not L["wave_spec"] and not L["wave_wg"]),
    "lib-400-notail": (dict(LIB, DNLP_BATCH_WAVE="2", DNLP_WAVE_NO_TAIL="1"), lambda L: L["wave_form"] == 400 and not L["wave_spec"] and not L["wave_wg"]),
    "lib-x11-notail": (dict(LIB, DNLP_WAVE_NO_TAIL="1"), lambda L: L["wave_form"] % 100 == 11 and not L["wave_spec"] and not L["wave_wg"]),
    "spec-lds": ({"DNLP_WAVE_SPEC": "1", "DNLP_WAVE_SPEC_TABLES": "0"}, lambda L: L["wave_spec"] and L["lds_mode"] & 1 == 1),
    "spec-global": ({"DNLP_WAVE_SPEC": "1", "DNLP_WAVE_SPEC_TABLES": "1"}, lambda L: L["wave_spec"] and L["lds_mode"] & 1 == 0),
    "wg-8": ({"DNLP_WAVE_SPEC": "1"}, lambda L: L["wave_wg"] and L["lanes"] == 512),
    "wg-4": ({"DNLP_WAVE_SPEC": "1", "DNLP_WAVE_WG_WAVES": "4"}, lambda L: L["wave_wg"] and L["lanes"] == 256),
    "wg-small": ({"DNLP_WAVE_SPEC": "1", "DNLP_WAVE_WG_SMALL": "1"}, lambda L: L["wave_wg"] and L["lanes"] == 128),
    "wg-8-nowindows": ({"DNLP_WAVE_SPEC": "1", "DNLP_WAVE_WG_WINDOWS": "0"}, lambda L: L["wave_wg"] and L["lanes"] == 512),
    "wg-8-nostage": ({"DNLP_WAVE_SPEC": "1", "DNLP_WAVE_STAGE": "0"}, lambda L: L["wave_wg"] and L["lanes"] == 512),
    "wg-8-nolds": ({"DNLP_WAVE_SPEC": "1", "DNLP_WAVE_WG_LDS": "0"}, lambda L: L["wave_wg"] and L["lanes"] == 512),
}


def _record(row):
    first = not _written
    _written.append(row.get("case"))
    os.makedirs(os.path.dirname(PROFILE), exist_ok=True)
    with open(PROFILE, "w" if first else "a") as fh:
        if first:
            fh.write(json.dumps({"file": "written by tests/test_wave_probe_gpu.py on an MI355X, one line per case and form",
                                 "bound": "eta_dev <= M max(eta_host, n_row 2^-53), fe_dev <= M max(fe_host, n_row 2^-53), per instance; "
                                          "res_excess: the kernel's residual in units of (n_row_K + 2) 2^-53 (|r| + |K||v|), <= M",
                                 "M": M, "ratios": "the largest over the instances, without M"}) + "\n")
        fh.write(json.dumps(row) + "\n")


def _run(monkeypatch, name, form, pt, count=wp.N_INST, tile=1):
    """One probe launch of the first `count` instances (tiled `tile` times) in the given form; the handle is kept per template and form."""
    from dnlp_amd.batch import _device_handle
    env, says = FORMS[form]
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    t = wp.template(name)
    if (name, form) not in _handles:
        _handles[(name, form)] = _device_handle(t.pb.arrays0, t.pb.data0["tape"], None, dict(t.opts))
    inp = wp.inputs(name, pt, count)
    if tile > 1:
        inp = {k: (np.ascontiguousarray(np.concatenate([v] * tile)) if isinstance(v, np.ndarray) else v) for k, v in inp.items()}
    res = _handles[(name, form)].batch_kkt_probe(**inp)
    assert says(res["launch"]), (form, res["launch"])
    return res


def _hold(name, pt, form, res, count=wp.N_INST, extra=None):
    """The bounds of the module docstring for the first `count` instances; one line of figures."""
    t = wp.template(name)
    host = wp.host_lane(name, pt, wp.N_INST)
    floor = wp.n_row_plan(t) * UNIT
    assert res["ok"][:count].all()
    worst = dict(eta_host=0.0, eta_dev=0.0, fe_host=0.0, fe_dev=0.0, eta_ratio=0.0, fe_ratio=0.0, res_excess=0.0, joint_eta_ratio=0.0)
    for i in range(count):
        assert (int(res["nneg"][i]), int(res["nzero"][i])) == wp.inertia(name, pt, i), (i, res["nneg"][i], res["nzero"][i])
        eh, fh = wp.figures(name, pt, i, host)
        ed, fd = wp.figures(name, pt, i, res)
        ej, fj = wp.figures(name, pt, i, {"sol": np.concatenate([res["sol2"], res["sol"][:, 2:]], axis=1)})
        rx = wp.residual_excess(name, pt, i, res)
        for k, v in (("eta_host", eh), ("eta_dev", ed), ("fe_host", fh), ("fe_dev", fd), ("eta_ratio", ed / max(eh, floor)),
                     ("fe_ratio", fd / max(fh, floor)), ("res_excess", rx), ("joint_eta_ratio", max(ej / max(eh, floor), fj / max(fh, floor)))):
            worst[k] = max(worst[k], float(v))
    row = dict(case="%s/%s" % (name, pt), form=form, launch=res["launch"], n_row=wp.n_row_plan(t),
               joint_equals_single=bool(np.array_equal(res["sol2"][:count], res["sol"][:count, :2])), **worst)
    row.update(extra or {})
    print(json.dumps(row))
    _record(row)
    assert worst["eta_ratio"] <= M and worst["fe_ratio"] <= M and worst["joint_eta_ratio"] <= M and worst["res_excess"] <= M, row
    return row


def _same(a, b, lo=0, hi=None):
    return {k: bool(np.array_equal(a[k][lo:hi], b[k][lo:hi], equal_nan=True)) for k in KEYS}


CASES = (
    [("localization", "lib-x11"), ("localization16", "lib-x11"), ("circle_packing4", "lib-x11"), ("circle_packing4", "lib-x11-notail"),
     ("circle_packing10", "lib-x11"), ("circle_packing10", "lib-110"), ("circle_packing10", "lib-x11-notail"), ("circle_packing12", "lib-x10"),
     ("circle_packing12", "lib-x10-notail"), ("circle_packing17", "lib-400"), ("circle_packing17", "lib-400-notail"), ("path_planning", "lib-400"), ("power_flow", "lib-400")] +
    [(n, f) for n in ("localization", "circle_packing4", "circle_packing10") for f in ("spec-lds", "spec-global")] +
    [("circle_packing12", "spec-global")] +         # (width-32 tail; its share leaves no room for the tables in LDS)
    [(n, f) for n in ("path_planning", "power_flow") for f in ("wg-8", "wg-4")] +
    [("circle_packing10", "wg-small")])


@pytest.mark.parametrize("name,form", CASES)
def test_device_probe_against_the_host_lane_and_the_reference(name, form, gpu_required, monkeypatch):
    t = wp.template(name)
    t.check(t)
    for pt in wp.POINTS_OF[name]:
        res = _run(monkeypatch, name, form, pt)
        again = _run(monkeypatch, name, form, pt)
        assert all(_same(res, again).values()), (pt, _same(res, again))          # launch to launch: the same bits
        _hold(name, pt, form, res)
    if name in wp.SINGULAR:
        # inertia only: one static pivot is exactly zero in every build — the counts and the ok flag of the host lane
        res, host = _run(monkeypatch, name, form, "singular"), wp.host_lane(name, "singular", wp.N_INST)
        row = dict(case="%s/singular" % name, form=form, launch=res["launch"], nneg=res["nneg"].tolist(), nzero=res["nzero"].tolist(),
                   ok=res["ok"].tolist(), nneg_host=host["nneg"].tolist(), nzero_host=host["nzero"].tolist())
        print(json.dumps(row))
        _record(row)
        assert (res["nzero"] > 0).all() and np.array_equal(res["nzero"], host["nzero"]) and np.array_equal(res["ok"], host["ok"])
        assert np.array_equal(res["nneg"], host["nneg"])


def test_width_32_case_has_no_room_for_its_tables_in_lds(gpu_required, monkeypatch):
    """circle packing 12 (105 KB of state per instance): with DNLP_WAVE_SPEC_TABLES=0 the per-template kernel does not fit and the
    launch is the library's — which is why that case runs the per-template kernel with its tables in global memory only."""
    env, _ = FORMS["spec-lds"]
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    from dnlp_amd.batch import _device_handle
    t = wp.template("circle_packing12")
    h = _device_handle(t.pb.arrays0, t.pb.data0["tape"], None, dict(t.opts))
    L = h.batch_kkt_probe(**wp.inputs("circle_packing12", "interior", 2))["launch"]
    assert not L["wave_spec"] and not L["wave_wg"] and L["wave_form"] % 100 == 10, L


def test_two_per_simd_instantiation(gpu_required, monkeypatch):
    """More than four wavefronts per workgroup is another compilation of the same text (wave_batch.h TWO_PER_SIMD: 256 registers,
    spills to scratch): 2048 localization instances — the 8 data rows tiled — give a launch of at least five per compute unit.
    All copies of a row return identical bits; the errors are held to the bound; whether the bits equal the four-wavefront
    form's is recorded, not asserted (two compilations may contract differently)."""
    name, pt = "localization", "interior"
    res = _run(monkeypatch, name, "lib-x11", pt, tile=256)
    assert res["launch"]["wave_form"] // 100 > 4, res["launch"]
    for k in KEYS:
        a = res[k].reshape((256, wp.N_INST) + res[k].shape[1:])
        assert np.array_equal(a, np.broadcast_to(a[0], a.shape), equal_nan=True), k
    few = _run(monkeypatch, name, "lib-x11", pt)
    assert few["launch"]["wave_form"] // 100 <= 4
    _hold(name, pt, "lib-x11-two-per-simd", res, extra={"same_bits_as_the_8_instance_launch": _same(res, few, 0, wp.N_INST)})


@pytest.mark.parametrize("name,on,off", [("localization", "spec-lds", "spec-global"), ("path_planning", "wg-8", "wg-8-nowindows"),
                                         ("path_planning", "wg-8", "wg-8-nostage"), ("path_planning", "wg-8", "wg-8-nolds")])
def test_placement_switches_change_no_bit(name, on, off, gpu_required, monkeypatch):
    """DNLP_WAVE_SPEC_TABLES, DNLP_WAVE_WG_WINDOWS, DNLP_WAVE_STAGE, DNLP_WAVE_WG_LDS change where operands live, not the order of
    any sum: equal bits with each switch on and off."""
    pt = "interior"
    a = _run(monkeypatch, name, on, pt)
    b = _run(monkeypatch, name, off, pt)
    same = _same(a, b)
    _hold(name, pt, off, b, extra={"same_bits_as": on, "same_bits": same})
    assert all(same.values()), same


@pytest.mark.parametrize("name,form", [("circle_packing4", "lib-x11"), ("localization", "spec-lds")])
def test_ragged_probe_launches_repeat_the_instances_of_the_full_one(name, form, gpu_required, monkeypatch):
    pt = "indefinite"
    full = _run(monkeypatch, name, form, pt)
    for count in (1, 3):
        part = _run(monkeypatch, name, form, pt, count=count)
        assert all(_same(part, full, 0, count).values()), (count, _same(part, full, 0, count))


def test_a_refused_launch_says_why(gpu_required, monkeypatch):
    """DNLP_BATCH_WAVE=0: the launch would run the generic kernel — a negative code and the reason, no generic-kernel result."""
    from dnlp_amd.batch import _device_handle
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("DNLP_BATCH_WAVE", "0")
    t = wp.template("circle_packing4")
    h = _device_handle(t.pb.arrays0, t.pb.data0["tape"], None, {})
    with pytest.raises(RuntimeError, match="dnlp_batch_kkt_probe: the wavefront solver does not take this launch"):
        h.batch_kkt_probe(**wp.inputs("circle_packing4", "interior", 2))
