"""The forms of the 128 x 128 Schur update kernel (csrc/ldlt_blocked.h, gemm_nt_update_fast*; DNLP_LDLT_UPDATE_FORM):
the software-pipelined operand reads on the lower-triangle grid (default) against the single-register-set loop on the
full grid (form 0).  Both add the same products in the same order, so the factors are equal bit for bit.

The small-tile router would send every launch of these orders to the 64 x 64 kernel; DNLP_LDLT_SMALL_TILES=0 and a
256-column outer panel put them on the 128 x 128 kernel: n = 300 a single partial diagonal tile, 512 exactly 2 x 2 tiles,
777 edge and diagonal masks together plus the rectangular next-panel launches, 1500 a 78-tile triangle over several
panels.  The tile index map of the triangular grid (csrc/lower_tile_map.h) is checked on the host."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDERS = [300, 512, 777, 1500]


def _factor(A, b, form):
    """dnlp_ldlt_host with the 128 x 128 update kernel forced on; `form` None leaves the default form."""
    from dnlp_amd import _capi
    api = _capi.require_device(0)
    env = {"DNLP_LDLT_SMALL_TILES": "0", "DNLP_LDLT_NB": "256"}
    if form is not None:
        env["DNLP_LDLT_UPDATE_FORM"] = str(form)
    saved = {k: os.environ.get(k) for k in list(env) + ["DNLP_LDLT_UPDATE_FORM"]}
    os.environ.pop("DNLP_LDLT_UPDATE_FORM", None)
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
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return np.tril(Af), nneg.value, nzero.value, sol


_CASES = {}


def _case(n):
    """The quasi-definite matrix of test_blocked_mfma_ldlt_quasidefinite with its numpy solution and condition number
    (computed once per order)."""
    if n not in _CASES:
        rng = np.random.default_rng(n)
        n1 = (3 * n) // 4
        G = rng.standard_normal((n1, n1))
        H = G @ G.T / n1 + np.eye(n1)
        J = rng.standard_normal((n - n1, n1))
        A = np.block([[H, J.T], [J, -1e-2 * np.eye(n - n1)]])
        b = rng.standard_normal(n)
        _CASES[n] = (A, b, n - n1, np.linalg.solve(A, b), np.linalg.cond(A))
    return _CASES[n]


@pytest.mark.gpu
@pytest.mark.parametrize("n", ORDERS)
def test_update_forms_give_the_same_factor(n, gpu_required):
    A, b, n2, ref, cond = _case(n)
    F1, neg1, zero1, x1 = _factor(A, b, None)
    F0, neg0, zero0, x0 = _factor(A, b, 0)
    assert (neg1, zero1) == (neg0, zero0) == (n2, 0)
    assert np.array_equal(F1, F0), np.abs(F1 - F0).max()
    for x in (x1, x0):
        assert np.linalg.norm(x - ref) <= 1e-9 * np.linalg.norm(ref) * cond


@pytest.mark.gpu
@pytest.mark.parametrize("form", [1, 2])
def test_each_lever_alone_gives_the_same_factor(form, gpu_required):
    """Form 1 = pipelined reads on the full grid, form 2 = the parent loop on the triangular grid (n = 777: every mask)."""
    A, b, n2, ref, cond = _case(777)
    F0, neg0, zero0, _ = _factor(A, b, 0)
    F, neg, zero, x = _factor(A, b, form)
    assert (neg, zero) == (neg0, zero0) == (n2, 0)
    assert np.array_equal(F, F0), np.abs(F - F0).max()
    assert np.linalg.norm(x - ref) <= 1e-9 * np.linalg.norm(ref) * cond


_MAP_MAIN = r"""
#include "lower_tile_map.h"
#include <cstdio>
#include <cstdlib>
// argv: pairs "ntm ntn" up to a "--", then indices (none: every index of each launch).
// Per pair a line "# ntm ntn count", then one "idx tm tn" line per index.
int main(int argc, char** argv) {
  int split = 1;
  while (split < argc && argv[split][0] != '-') ++split;
  for (int p = 1; p + 1 < split; p += 2) {
    const int ntm = atoi(argv[p]), ntn = atoi(argv[p + 1]);
    const long long count = dnlp::lower_tile_count(ntm, ntn);
    printf("# %d %d %lld\n", ntm, ntn, count);
    const long long nidx = split + 1 < argc ? argc - split - 1 : count;
    for (long long q = 0; q < nidx; ++q) {
      const long long idx = split + 1 < argc ? atoll(argv[split + 1 + q]) : q;
      int tm, tn;
      dnlp::lower_tile_map(idx, ntm, ntn, &tm, &tn);
      printf("%lld %d %d\n", idx, tm, tn);
    }
  }
  return 0;
}
"""


def _expected(ntm, ntn):
    """Today's order: the full grid column by column, tm ascending, keeping the tiles with tm*128 + 127 >= tn*128."""
    return [(tm, tn) for tn in range(ntn) for tm in range(ntm) if tm * 128 + 127 >= tn * 128]


def test_lower_tile_map_enumerates_the_lower_tiles_in_grid_order(tmp_path):
    src = tmp_path / "map_main.cpp"
    src.write_text(_MAP_MAIN)
    exe = str(tmp_path / "map_main")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-I", os.path.join(ROOT, "dnlp_amd", "csrc"),
                           str(src), "-o", exe])

    def run(pairs, idx=()):
        args = [str(v) for pr in pairs for v in pr] + ["--"] + [str(i) for i in idx]
        out = subprocess.run([exe] + args, capture_output=True, text=True, check=True)
        got = {}
        for ln in out.stdout.split("\n"):
            if ln.startswith("#"):
                _, ntm, ntn, count = ln.split()
                rows = got[(int(ntm), int(ntn))] = (int(count), [])
            elif ln:
                rows[1].append(tuple(int(v) for v in ln.split()))
        return got

    pairs = [(ntm, ntn) for ntm in range(1, 65) for ntn in sorted({ntm, min(1, ntm), min(2, ntm), min(8, ntm)})]
    got = run(pairs)
    assert sorted(got) == sorted(pairs)
    for ntm, ntn in pairs:
        want = _expected(ntm, ntn)
        count, rows = got[(ntm, ntn)]
        assert count == len(want), (ntm, ntn)
        assert [r[0] for r in rows] == list(range(count)), (ntm, ntn)
        assert [(r[1], r[2]) for r in rows] == want, (ntm, ntn)
    for ntn in (1024, 1, 2, 8):
        want = _expected(1024, ntn)
        rng = np.random.default_rng(1024 + ntn)
        idx = [0, len(want) - 1] + [int(i) for i in rng.integers(0, len(want), 1000)]
        count, rows = run([(1024, ntn)], idx)[(1024, ntn)]
        assert count == len(want)
        assert [(r[1], r[2]) for r in rows] == [want[i] for i in idx], ntn
