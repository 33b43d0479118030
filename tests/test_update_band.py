"""The banded tile order of the lower-triangle Schur update (csrc/lower_tile_map.h, lower_tile_map_banded; bit 2 of
DNLP_LDLT_UPDATE_FORM, band height DNLP_LDLT_UPDATE_BAND): the same tiles as lower_tile_map, visited in bands of tile
rows so that a band's W rows are read again while they are still in the Infinity Cache.  Every tile adds the same
products in the same order, so the factor is equal bit for bit to the one of form 0.

The index map is checked on the host against a plain enumeration.  On the device, n = 777 (7 tile rows: several bands, a
partial last band, edge and diagonal masks, the rectangular next-panel launches) and n = 1500 (a 12-row triangle over
several panels) with bands of 1, 2 and 3 tile rows are the smallest shapes at which a wrong or duplicated tile index
or a band boundary that crosses the diagonal shows."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ENV = ("DNLP_LDLT_SMALL_TILES", "DNLP_LDLT_NB", "DNLP_LDLT_UPDATE_FORM", "DNLP_LDLT_UPDATE_BAND")


def _factor(A, b, form, band=None):
    """dnlp_ldlt_host with the 128 x 128 update kernel forced on (256-column outer panels); `band` None leaves the
    default band height."""
    from dnlp_amd import _capi
    api = _capi.require_device(0)
    env = {"DNLP_LDLT_SMALL_TILES": "0", "DNLP_LDLT_NB": "256", "DNLP_LDLT_UPDATE_FORM": str(form)}
    if band is not None:
        env["DNLP_LDLT_UPDATE_BAND"] = str(band)
    saved = {k: os.environ.pop(k, None) for k in _ENV}
    os.environ.update(env)
    try:
        n = A.shape[0]
        Af = np.asfortranarray(A.copy())
        ipiv = np.zeros(n, np.int32)
        nneg, nzero, sec = C.c_int(), C.c_int(), C.c_double()
        sol = np.zeros(n)
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
        rc = api.lib.dnlp_ldlt_host(0, dp(Af), n, n, ipiv.ctypes.data_as(C.POINTER(C.c_int32)), 0, C.byref(nneg),
                                    C.byref(nzero), dp(np.ascontiguousarray(b)), dp(sol), C.byref(sec))
        assert rc == 0, api.error()
    finally:
        for k in _ENV:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]
    return np.tril(Af), nneg.value, nzero.value, sol


_CASES = {}


def _case(n, form=None):
    """The quasi-definite matrix of tests/test_update_forms.py with its numpy solution and condition number, and the
    factorisation of one form without a band height (each computed once per order and left unchanged)."""
    if n not in _CASES:
        rng = np.random.default_rng(n)
        n1 = (3 * n) // 4
        G = rng.standard_normal((n1, n1))
        H = G @ G.T / n1 + np.eye(n1)
        J = rng.standard_normal((n - n1, n1))
        A = np.block([[H, J.T], [J, -1e-2 * np.eye(n - n1)]])
        b = rng.standard_normal(n)
        _CASES[n] = {"A": A, "b": b, "n2": n - n1, "ref": np.linalg.solve(A, b), "cond": np.linalg.cond(A)}
    c = _CASES[n]
    if form is not None and form not in c:
        c[form] = _factor(c["A"], c["b"], form)
    return c


@pytest.mark.gpu
@pytest.mark.parametrize("band", [1, 2, 3])
@pytest.mark.parametrize("n", [777, 1500])
def test_banded_order_gives_the_factor_of_form_0(n, band, gpu_required):
    c = _case(n, 0)
    F0, neg0, zero0, _ = c[0]
    F, neg, zero, x = _factor(c["A"], c["b"], 7, band)
    assert (neg, zero) == (neg0, zero0) == (c["n2"], 0)
    assert np.array_equal(F, F0), np.abs(F - F0).max()
    assert np.linalg.norm(x - c["ref"]) <= 1e-9 * np.linalg.norm(c["ref"]) * c["cond"]


@pytest.mark.gpu
def test_default_band_is_taller_than_a_small_order_and_gives_form_3(gpu_required):
    """n = 777 has 7 tile rows, fewer than the default band: the launches keep the order of form 3."""
    c = _case(777, 3)
    F3, neg3, zero3, x3 = c[3]
    F, neg, zero, x = _factor(c["A"], c["b"], 7)
    assert (neg, zero) == (neg3, zero3) == (c["n2"], 0)
    assert np.array_equal(F, F3), np.abs(F - F3).max()
    assert np.array_equal(x, x3)
    assert np.linalg.norm(x - c["ref"]) <= 1e-9 * np.linalg.norm(c["ref"]) * c["cond"]


_MAP_MAIN = r"""
#include "lower_tile_map.h"
#include <cstdio>
#include <cstdlib>
// argv: triples "ntm ntn band" up to a "--", then indices (none: every index of each launch).
// Per triple a line "# ntm ntn band count", then one "idx tm tn tm0 tn0" line per index: the banded map, then the
// column-by-column map of the same index.
int main(int argc, char** argv) {
  int split = 1;
  while (split < argc && argv[split][0] != '-') ++split;
  for (int p = 1; p + 2 < split; p += 3) {
    const int ntm = atoi(argv[p]), ntn = atoi(argv[p + 1]), band = atoi(argv[p + 2]);
    const long long count = dnlp::lower_tile_count(ntm, ntn);
    printf("# %d %d %d %lld\n", ntm, ntn, band, count);
    const long long nidx = split + 1 < argc ? argc - split - 1 : count;
    for (long long q = 0; q < nidx; ++q) {
      const long long idx = split + 1 < argc ? atoll(argv[split + 1 + q]) : q;
      int tm, tn, tm0, tn0;
      dnlp::lower_tile_map_banded(idx, ntm, ntn, band, &tm, &tn);
      dnlp::lower_tile_map(idx, ntm, ntn, &tm0, &tn0);
      printf("%lld %d %d %d %d\n", idx, tm, tn, tm0, tn0);
    }
  }
  return 0;
}
"""


def _expected(ntm, ntn, band):
    return [(tm, tn) for b in range(-(-ntm // band)) for tn in range(min(ntn, ntm, (b + 1) * band))
            for tm in range(max(tn, b * band), min(ntm, (b + 1) * band))]


@pytest.fixture(scope="module")
def map_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("band_map")
    src = d / "map_main.cpp"
    src.write_text(_MAP_MAIN)
    exe = str(d / "map_main")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-I", os.path.join(ROOT, "dnlp_amd", "csrc"),
                           str(src), "-o", exe])

    def run(triples, idx=()):
        """{(ntm, ntn, band): (count, [(idx, tm, tn, tm0, tn0), ...])}, a few hundred launches per process"""
        got = {}
        for at in range(0, len(triples), 200):
            args = [str(v) for tr in triples[at:at + 200] for v in tr] + ["--"] + [str(i) for i in idx]
            out = subprocess.run([exe] + args, capture_output=True, text=True, check=True)
            for ln in out.stdout.split("\n"):
                if ln.startswith("#"):
                    _, ntm, ntn, band, count = ln.split()
                    rows = got[(int(ntm), int(ntn), int(band))] = (int(count), [])
                elif ln:
                    rows[1].append(tuple(int(v) for v in ln.split()))
        return got

    return run


def test_banded_map_enumerates_every_lower_tile_once_band_by_band(map_exe):
    triples = [(ntm, ntn, band) for ntm in range(1, 65) for ntn in sorted({ntm, min(1, ntm), min(2, ntm), min(8, ntm)})
               for band in (1, 2, 3, 8, 64)]
    got = map_exe(triples)
    assert sorted(got) == sorted(triples)
    for ntm, ntn, band in triples:
        want = _expected(ntm, ntn, band)
        lower = {(tm, tn) for tn in range(ntn) for tm in range(tn, ntm)}
        count, rows = got[(ntm, ntn, band)]
        key = (ntm, ntn, band)
        assert count == len(want) == len(lower), key                 # lower_tile_count: the grid size is unchanged
        assert [r[0] for r in rows] == list(range(count)), key
        tiles = [(r[1], r[2]) for r in rows]
        assert tiles == want, key
        assert len(set(tiles)) == count and set(tiles) == lower, key      # every lower tile exactly once
        if band >= ntm:
            assert tiles == [(r[3], r[4]) for r in rows], key         # one band: the column-by-column order


def test_banded_map_at_order_131072(map_exe):
    for ntn in (1024, 8):
        want = _expected(1024, ntn, 128)
        rng = np.random.default_rng(1024 + ntn)
        idx = [0, len(want) - 1] + [int(i) for i in rng.integers(0, len(want), 1000)]
        count, rows = map_exe([(1024, ntn, 128)], idx)[(1024, ntn, 128)]
        assert count == len(want)
        assert [(r[1], r[2]) for r in rows] == [want[i] for i in idx], ntn
    # a band as tall as the launch, or taller: lower_tile_map for every sampled index
    for band in (1024, 4096):
        count, rows = map_exe([(1024, 1024, band)], idx)[(1024, 1024, band)]
        assert [(r[1], r[2]) for r in rows] == [(r[3], r[4]) for r in rows], band
