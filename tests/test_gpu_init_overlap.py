"""G'G of the initial point formed inside load_problem, under G's load
(SmallArgs::init_overlap, FAC_IDENT_H), against form_H's own row loop
(FAC_IDENT): the same bits, and both match the CPU oracle.

Every case is solved twice, with SOCP_INIT_OVERLAP=1 and =0, each in a fresh
child process (the switch is read at launch): one child per setting solves all
the cases (tests/init_overlap_cases.py).  Batches of 16 problems, m = 16,
tol = 0.  On and off must agree bitwise on x, y, z, s, iters and status.

Oracle gate (the maxit = 0 and K = 2 cases): that of test_gpu_fuse_u.py /
test_gpu_slot_kinds.py as it stands -- the oracle in the kernels' operation
order (oracle.F_STRUCTURED | F_CHOLSOLVE): same status and rel <= 1e-8 on x, z,
s per problem; the distance to the reference order is held to 1e-8 plus twice
the distance between the oracle's own two orders on the same vector.

The cases: C2's shape at the initial point alone and at K = 2; the mixed kernel
on C2's table; n = 50 (padded columns, the padded diagonal of H); k = 90 (a
partial last row step, and a row step of padding only); `sing` with ones and
zeros in one batch (A'A added to a pre-formed G'G); sing=None (the probe takes
the pre-formed G'G and the initial point rebuilds H); a warm start from the
oracle's iterate (no initial factorisation: the tiles the load left must
disturb nothing); one problem with a zero column in G among healthy ones
(CHOL_H_FAILED at the initial factorisation, its neighbours bitwise those of
the healthy batch); a shared-matrices batch with more problems than waves (a
resident-G problem, whose load returns nothing and forms no H, follows a
loading one on the same wave); and one batch of 4,096 problems under the
reference rule (tol 1e-5, maxit 40), so that every persistent wave loads
several problems.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from init_overlap_cases import BATCH, CASES, KEYS, LIFE, SEED, SHARED, WARM_AT, ZERO_COL_J, ZERO_COL_P, sing_of

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CHOL_H_FAILED = 2


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


@pytest.fixture(scope="module")
def runs(oracle, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("init_overlap")
    inputs, want = {}, {}
    KERNEL_ORDER = oracle.F_STRUCTURED | oracle.F_CHOLSOLVE
    for c in CASES:
        d = oracle.generate(c.cones, BATCH, c.n, c.m, c.k, SEED)
        if c.zero_col:
            o = ZERO_COL_P * c.k * c.n + ZERO_COL_J * c.k  # column-major k x n per problem
            d["G"][o:o + c.k] = 0.0
        args = (c.cones, c.n, c.m, c.k, d["c"], d["A"], d["b"], d["G"], d["h"])
        if c.warm:
            w = oracle.batch_solve(*args, sing=sing_of(c), params=oracle.Params(maxit=WARM_AT, tol=0.0))
            for q in "xyzs":
                d[f"w{q}"] = w[q]
        if c.oracle:
            want[c.name] = [oracle.batch_solve(*args, sing=sing_of(c),
                                               params=oracle.Params(maxit=c.maxit, tol=0.0, flags=fl))
                            for fl in (KERNEL_ORDER, 0)]
        for key, v in d.items():
            inputs[f"{c.name}/{key}"] = v
    inp = str(tmp / "in.npz")
    np.savez(inp, **inputs)
    got = {}
    for sw in ("1", "0"):
        outp = str(tmp / f"out{sw}.npz")
        env = dict(os.environ, SOCP_INIT_OVERLAP=sw)
        p = subprocess.run([sys.executable, os.path.join(HERE, "init_overlap_cases.py"), inp, outp], env=env,
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        got[sw] = dict(np.load(outp))
    return got, want


def assert_bitwise(on, off, name, keys=KEYS):
    for key in keys:
        a, b = on[f"{name}/{key}"], off[f"{name}/{key}"]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (name, key)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_switch_on_off_bitwise(runs, case):
    got, want = runs
    on, off = got["1"], got["0"]
    name = case.name
    assert case.variant in str(on[f"{name}/kernel"]) and str(on[f"{name}/kernel"]) == str(off[f"{name}/kernel"])
    assert_bitwise(on, off, name)
    st = on[f"{name}/status"]
    print(f"{name}: status counts {np.bincount(st, minlength=5).tolist()}, iters {on[f'{name}/iters'].tolist()}")
    if case.zero_col:
        # the defective problem fails at the initial factorisation; the others are
        # bitwise the healthy batch's (c2_k2: the same data, the same parameters)
        assert st[ZERO_COL_P] == CHOL_H_FAILED and on[f"{name}/iters"][ZERO_COL_P] == 0
        others = np.arange(BATCH) != ZERO_COL_P
        assert (st[others] != CHOL_H_FAILED).all()
        for g in (on, off):
            for key, L in (("x", case.n), ("y", case.m), ("z", case.k), ("s", case.k), ("iters", 1), ("status", 1)):
                a = g[f"{name}/{key}"].reshape(BATCH, L)[others]
                b = g[f"c2_k2/{key}"].reshape(BATCH, L)[others]
                assert a.tobytes() == b.tobytes(), (name, key)
    elif case.sing != "none":
        assert (st != CHOL_H_FAILED).all()
    if not case.oracle:
        return
    r, r_ref = want[name]  # the oracle in the kernels' order, and in the reference's
    for sw, g in (("on", on), ("off", off)):
        assert (g[f"{name}/status"] == r["status"]).all(), (name, sw)
        for p in range(BATCH):
            for key, L in (("x", case.n), ("z", case.k), ("s", case.k)):
                vec = g[f"{name}/{key}"][p * L:(p + 1) * L]
                e, e_ref = rel(vec, r[key][p * L:(p + 1) * L]), rel(vec, r_ref[key][p * L:(p + 1) * L])
                floor = rel(r[key][p * L:(p + 1) * L], r_ref[key][p * L:(p + 1) * L])  # the oracle's two orders
                print(f"{name} {sw} p={p} {key} rel={e:.3e} (reference order {e_ref:.3e}, oracle orders {floor:.3e})")
                assert e <= 1e-8, (name, sw, p, key, e)
                assert e_ref <= 1e-8 + 2.0 * floor, (name, sw, p, key, e_ref, floor)


def test_resident_g_problem_after_a_loading_one(runs):
    got, _ = runs
    on, off = got["1"], got["0"]
    assert_bitwise(on, off, "shared")
    assert SHARED["batch"] > 4 * 256  # more problems than one-wave-per-SIMD workgroups on the device
    assert (on["shared/status"] != CHOL_H_FAILED).all() and (on["shared/iters"] == SHARED["maxit"]).all()


def test_tiles_do_not_outlive_their_problem(runs):
    got, _ = runs
    on, off = got["1"], got["0"]
    assert_bitwise(on, off, "life")
    it = on["life/iters"]
    print(f"life: {LIFE['batch']} problems, iterations {it.min()}..{it.max()}, "
          f"status counts {np.bincount(on['life/status'], minlength=5).tolist()}")
    # the case is about problems leaving at different iterations
    assert it.min() < it.max()
