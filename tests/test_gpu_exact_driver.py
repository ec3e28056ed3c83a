"""The exact-fit kernel's structured driver (socp_small.hpp run_exact: one loop,
a trip per factorisation, in place of the micro-phase switch) against the
generic pure-slot kernel, which keeps the switch: the same bits.

The scheme is test_gpu_exact_fit.py's: every case (tests/exact_driver_cases.py)
is at n = 64, m = 16, k = 96, POC32 + SOC32 + SOC32 and is solved with
SOCP_EXACT_FIT unset and =0, each setting in a fresh child process, one child
per setting for all the cases.  Unset and =0 must agree bitwise on x, y, z, s,
iters, status (and res where asked for), and the host rule must have named the
exact-fit kernel in the first child and the generic one in the second.

The cases are the driver's paths that exact_fit_cases.py leaves open:
maxit = 0 without and with `res` (the exits before and after the residuals);
maxit = 1; tol = 1e-5 on 96 problems with `res` (problems of one batch leave at
different iterations); `sing` absent with a healthy batch, with one problem
whose G has a zero column (the probe finds G'G singular, the initial point is
rebuilt with A'A) and with that problem's A column zero too (the probe, the
rebuilt initial point and its chol(H) failure in one launch); a warm start
with maxit = 0 and `res` (enters at an iteration trip, forms the residual
norms, leaves); 1,100 problems under the reference rule at maxit = 3 (waves
take further problems; nothing converges that early, so the same batch is also
run at maxit = 40, where problems leave at different iterations).

Oracle gate (maxit = 0 and maxit = 1, both settings): that of
test_gpu_parity.py::test_trajectory_parity -- the oracle in the reference
order, same status and rel <= 1e-8 on x, z, s per problem.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from exact_driver_cases import CASES, MANY_RULE, MANY_RULE40, ORACLE_CASES
from exact_fit_cases import BAD_P, CONES, K, KEYS, M, N, NGEN, SEED

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
MAXIT_STATUS, CHOL_H_FAILED = 1, 2
BY_NAME = {c.name: c for c in CASES}


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


@pytest.fixture(scope="module")
def runs(oracle, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("exact_driver")
    d = oracle.generate(CONES, NGEN, N, M, K, SEED)
    want = {}
    for name in ORACLE_CASES:
        c = BY_NAME[name]
        B = c.batch
        want[name] = oracle.batch_solve(CONES, N, M, K, d["c"][:B * N], d["A"][:B * M * N], d["b"][:B * M],
                                        d["G"][:B * K * N], d["h"][:B * K], sing=np.zeros(B, np.uint8),
                                        params=oracle.Params(maxit=c.maxit, tol=0.0))
    inp = str(tmp / "in.npz")
    np.savez(inp, **{key: d[key] for key in ("c", "A", "b", "G", "h")})
    got = {}
    for sw in ("unset", "0"):
        outp = str(tmp / f"out_{sw}.npz")
        env = dict(os.environ)
        for name in ("SOCP_EXACT_FIT", "SOCP_FUSE_U", "SOCP_SLOT_SPECIALISE", "SOCP_INIT_OVERLAP"):
            env.pop(name, None)
        if sw == "0":
            env["SOCP_EXACT_FIT"] = "0"
        p = subprocess.run([sys.executable, os.path.join(HERE, "exact_driver_cases.py"), inp, outp], env=env,
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        got[sw] = dict(np.load(outp))
    return got, want


def assert_bitwise(on, off, name, keys=KEYS):
    for key in keys:
        a, b = on[f"{name}/{key}"], off[f"{name}/{key}"]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (name, key)


def assert_kernels(on, off, name):
    assert bool(on[f"{name}/exact"]) and not bool(off[f"{name}/exact"]), name
    assert "socp_small_kernel<4,24,1>" in str(on[f"{name}/kernel"])
    assert str(on[f"{name}/kernel"]) == str(off[f"{name}/kernel"])


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_switch_unset_and_off_bitwise(runs, case):
    got, _ = runs
    on, off = got["unset"], got["0"]
    name, B = case.name, case.batch
    assert_kernels(on, off, name)
    assert_bitwise(on, off, name, KEYS + (("res",) if case.res else ()))
    st, it = on[f"{name}/status"], on[f"{name}/iters"]
    print(f"{name}: status counts {np.bincount(st, minlength=5).tolist()}, iters {it.tolist()}")
    if case.res:
        assert np.isfinite(on[f"{name}/res"]).all()
    if case.healthy:
        # the defective problem's neighbours are bitwise the healthy batch's
        others = np.arange(B) != BAD_P
        for g in (on, off):
            for key, L in (("x", N), ("y", M), ("z", K), ("s", K), ("iters", 1), ("status", 1)):
                a = g[f"{name}/{key}"].reshape(B, L)[others]
                b = g[f"{case.healthy}/{key}"].reshape(B, L)[others]
                assert a.tobytes() == b.tobytes(), (name, key)


def test_maxit0_is_the_initial_point_with_and_without_res(runs):
    got, _ = runs
    for g in got.values():
        assert (g["maxit0/iters"] == 0).all() and (g["maxit0/status"] == MAXIT_STATUS).all()
        # forming the residual norms changes nothing else
        for key in KEYS:
            assert g[f"maxit0_res/{key}"].tobytes() == g[f"maxit0/{key}"].tobytes(), key
        assert (g["maxit1/iters"] == 1).all()


def test_tol_problems_leave_at_different_iterations(runs):
    got, _ = runs
    on = got["unset"]
    it, st = on["tol_res/iters"], on["tol_res/status"]
    print(f"tol_res: iterations {it.min()}..{it.max()}, status counts {np.bincount(st, minlength=5).tolist()}")
    conv = st == 0
    assert conv.any() and it[conv].min() < it[conv].max()
    # a converged problem's residual norms are those of its exit test
    res = on["tol_res/res"].reshape(-1, 3)
    assert (res[conv, 0] + res[conv, 1] + res[conv, 2] < BY_NAME["tol_res"].tol).all()


def test_probe_then_rebuilt_initial_point(runs):
    got, _ = runs
    for g in got.values():
        # a zero column of G alone: the probe reports it, A'A makes H definite, the problem is solved on
        assert not (g["probe_sing/status"][BAD_P] == CHOL_H_FAILED and g["probe_sing/iters"][BAD_P] == 0)
        # with A's column zero too, chol(H) fails at the initial point
        assert g["probe_fail/status"][BAD_P] == CHOL_H_FAILED and g["probe_fail/iters"][BAD_P] == 0


def test_warm_start_that_only_forms_res(runs):
    got, _ = runs
    for g in got.values():
        assert (g["warm_res_only/iters"] == 0).all()
        for key in "xyzs":  # the iterate goes through unchanged
            assert g[f"warm_res_only/{key}"].tobytes() == g[f"maxit1/{key}"].tobytes(), key
        assert np.isfinite(g["warm_res_only/res"]).all()


def test_more_problems_than_waves_under_the_rule(runs):
    got, _ = runs
    on, off = got["unset"], got["0"]
    assert_kernels(on, off, "many_rule")
    assert_bitwise(on, off, "many_rule")
    assert MANY_RULE["batch"] > 4 * 256  # more problems than one-wave-per-SIMD workgroups on the device
    it = on["many_rule/iters"]
    print(f"many_rule: iterations {it.min()}..{it.max()}, "
          f"status counts {np.bincount(on['many_rule/status'], minlength=5).tolist()}")
    assert it.max() <= MANY_RULE["maxit"]
    # the same batch at maxit = 40: problems leave at different iterations and their waves go on
    assert_kernels(on, off, "many_rule40")
    assert_bitwise(on, off, "many_rule40")
    it, st = on["many_rule40/iters"], on["many_rule40/status"]
    print(f"many_rule40: iterations {it.min()}..{it.max()}, status counts {np.bincount(st, minlength=5).tolist()}")
    assert it.max() <= MANY_RULE40["maxit"] and it[st == 0].min() < it[st == 0].max()


@pytest.mark.parametrize("name", ORACLE_CASES)
def test_against_the_oracle(runs, name):
    got, want = runs
    c, r = BY_NAME[name], want[name]
    for sw, g in got.items():
        assert (g[f"{name}/status"] == r["status"]).all(), sw
        for p in range(c.batch):
            for key, L in (("x", N), ("z", K), ("s", K)):
                e = rel(g[f"{name}/{key}"][p * L:(p + 1) * L], r[key][p * L:(p + 1) * L])
                print(f"{name} SOCP_EXACT_FIT {sw} p={p} {key} rel={e:.3e}")
                assert e <= 1e-8, (sw, p, key, e)
