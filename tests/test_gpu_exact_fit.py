"""The exact-fit solver kernel (socp_small.hpp ExactFit: the SOC+POC pure-slot
solver of <4,24,1> with n, m, k, the cone table, al_rows, slot_rot and fuse_u as
compile-time constants) against the generic pure-slot kernel it replaces: the
same bits.

Every case (tests/exact_fit_cases.py) is at the one geometry the kernel exists
for -- n = 64, m = 16, k = 96, POC32 + SOC32 + SOC32 -- and is solved twice,
with SOCP_EXACT_FIT unset and =0, each setting in a fresh child process (the
switch is read at launch); one child per setting solves all the cases.  Unset
and =0 must agree bitwise on x, y, z, s, iters, status (and res where asked
for), and the host rule must have named the exact-fit kernel in the first
child and the generic one in the second.

Batches of 1, 7 and 96 problems at K = 8; `sing` with ones and zeros in one
batch (A'A added) and `sing` absent (the kernel's own G'G probe); the final
residual norms; a warm start (no forming load);
one problem with a zero column in G and one with a NaN in h among healthy ones
(the same failure on both kernels, the neighbours bitwise those of the healthy
batch); a shared-matrices batch; 1,100 problems at K = 2 (more problems than
waves: the persistent loop takes a second problem); 256 problems under the
reference rule (tol 1e-5, maxit 40), which leave at different iterations.

Oracle gate (the K = 2 case, both settings): that of
test_gpu_parity.py::test_trajectory_parity -- the oracle in the reference
order, same status and rel <= 1e-8 on x, z, s per problem -- so that a bug both
kernels share does not pass.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from exact_fit_cases import BAD_P, CASES, CONES, K, KEYS, M, MANY, N, NGEN, RULE, SEED

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CHOL_H_FAILED = 2
ORACLE_CASE = "b7_k2"


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


@pytest.fixture(scope="module")
def runs(oracle, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("exact_fit")
    d = oracle.generate(CONES, NGEN, N, M, K, SEED)
    c = next(c for c in CASES if c.name == ORACLE_CASE)
    B = c.batch
    want = oracle.batch_solve(CONES, N, M, K, d["c"][:B * N], d["A"][:B * M * N], d["b"][:B * M], d["G"][:B * K * N],
                              d["h"][:B * K], sing=np.zeros(B, np.uint8),
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
        p = subprocess.run([sys.executable, os.path.join(HERE, "exact_fit_cases.py"), inp, outp], env=env,
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        got[sw] = dict(np.load(outp))
    return got, want


def assert_bitwise(on, off, name, keys=KEYS):
    for key in keys:
        a, b = on[f"{name}/{key}"], off[f"{name}/{key}"]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (name, key)


def assert_kernels(on, off, name):
    # the rule named the exact-fit kernel with the switch unset and the generic one with =0;
    # the reported name is the plain solver's either way
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
        # the defective problem fails the same way on both kernels (bitwise above); the
        # others are bitwise the healthy batch's (the same data, the same parameters)
        if case.zero_col:
            assert st[BAD_P] == CHOL_H_FAILED and it[BAD_P] == 0
        others = np.arange(B) != BAD_P
        for g in (on, off):
            for key, L in (("x", N), ("y", M), ("z", K), ("s", K), ("iters", 1), ("status", 1)):
                a = g[f"{name}/{key}"].reshape(B, L)[others]
                b = g[f"{case.healthy}/{key}"].reshape(B, L)[others]
                assert a.tobytes() == b.tobytes(), (name, key)


def test_batches_are_prefixes_of_each_other(runs):
    # per-problem determinism across batch sizes: problem p of 1, 7 and 96
    got, _ = runs
    for g in got.values():
        for key, L in (("x", N), ("y", M), ("z", K), ("s", K), ("iters", 1), ("status", 1)):
            big = g[f"b96/{key}"]
            for small in ("b1", "b7"):
                v = g[f"{small}/{key}"]
                assert v.tobytes() == big[:v.size].tobytes(), (small, key)


def test_k2_against_the_oracle(runs):
    got, r = runs
    c = next(c for c in CASES if c.name == ORACLE_CASE)
    for sw, g in got.items():
        assert (g[f"{c.name}/status"] == r["status"]).all(), sw
        for p in range(c.batch):
            for key, L in (("x", N), ("z", K), ("s", K)):
                e = rel(g[f"{c.name}/{key}"][p * L:(p + 1) * L], r[key][p * L:(p + 1) * L])
                print(f"{c.name} SOCP_EXACT_FIT {sw} p={p} {key} rel={e:.3e}")
                assert e <= 1e-8, (sw, p, key, e)


def test_second_problem_on_a_wave(runs):
    got, _ = runs
    on, off = got["unset"], got["0"]
    assert_kernels(on, off, "many")
    assert_bitwise(on, off, "many")
    assert MANY["batch"] > 4 * 256  # more problems than one-wave-per-SIMD workgroups on the device
    assert (on["many/iters"] == MANY["maxit"]).all()


def test_reference_rule_problems_leave_at_different_iterations(runs):
    got, _ = runs
    on, off = got["unset"], got["0"]
    assert_kernels(on, off, "rule")
    assert_bitwise(on, off, "rule")
    it = on["rule/iters"]
    print(f"rule: {RULE['batch']} problems, iterations {it.min()}..{it.max()}, "
          f"status counts {np.bincount(on['rule/status'], minlength=5).tolist()}")
    assert it.min() < it.max()
