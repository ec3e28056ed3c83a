"""U formed inside the residuals' G x pass (SmallArgs::fuse_u) against
compute_U() in factor(): the same bits, and both match the CPU oracle.

Every case is solved twice, with SOCP_FUSE_U=1 and =0, each in a fresh child
process (the switch is read at launch): one child per setting solves all the
cases (tests/fuse_u_cases.py).  Batches of 16 problems, m = 16, fixed K = 4,
tol = 0.  Oracle gate: that of test_gpu_slot_kinds.py, in the kernels'
operation order (oracle.F_STRUCTURED | F_CHOLSOLVE): same status and rel <=
1e-8 on x, z, s per problem; the distance to the reference order is held to
1e-8 plus twice the distance between the oracle's own two orders on the same
vector (CPU against CPU: the floor below which no kernel-order implementation
can come).  The warm-started case continues the oracle's iterate after 2
iterations for 2 more, so its first factorisation already takes a fused U.

The fusion applies where every cone is 32 or 64 rows (a G x chunk of 8 row
steps then lies in one cone).  The cases place a cone on exactly one chunk
(C2's own variant, the SOC+POC kernel) and across two chunks (k = 128); run the
mixed kernel on a fused table; an LP (nothing flushed).  Tables that do not
take the fusion run compute_U() under either setting: cones of 16 rows (half a
chunk, and the one-slot shape with chunks of 8 then 4 row steps), unaligned
cones, unequal dims.

Lifetime of "U is formed": one batch of 4,096 problems under the reference
rule (tol 1e-5, maxit 40), so every persistent wave takes several problems
that leave MP_ITER at different iterations -- a wave that carried "U is
formed" from one problem to the next would factor with a stale U.  On and
off must agree bitwise, with and without the residuals after the last
iteration (res=True, which forms a U that no factorisation takes).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from fuse_u_cases import BATCH, CASES, FIXED_K, KEYS, LIFE, SEED, WARM_AT

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


@pytest.fixture(scope="module")
def runs(oracle, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("fuse_u")
    inputs, want = {}, {}
    KERNEL_ORDER = oracle.F_STRUCTURED | oracle.F_CHOLSOLVE
    for c in CASES:
        d = oracle.generate(c.cones, BATCH, c.n, c.m, c.k, SEED)
        sing = np.zeros(BATCH, np.uint8)
        args = (c.cones, c.n, c.m, c.k, d["c"], d["A"], d["b"], d["G"], d["h"])
        if c.warm:
            w = oracle.batch_solve(*args, sing=sing, params=oracle.Params(maxit=WARM_AT, tol=0.0))
            warm = (w["x"], w["y"], w["z"], w["s"])
            for q, v in zip("xyzs", warm):
                d[f"w{q}"] = v
            want[c.name] = [oracle.batch_solve(*args, sing=sing, warm=warm,
                                               params=oracle.Params(maxit=FIXED_K - WARM_AT, tol=0.0, flags=fl))
                            for fl in (KERNEL_ORDER, 0)]
        else:
            want[c.name] = [oracle.batch_solve(*args, sing=sing, params=oracle.Params(maxit=FIXED_K, tol=0.0, flags=fl))
                            for fl in (KERNEL_ORDER, 0)]
        for key, v in d.items():
            inputs[f"{c.name}/{key}"] = v
    inp = str(tmp / "in.npz")
    np.savez(inp, **inputs)
    got = {}
    for sw in ("1", "0"):
        outp = str(tmp / f"out{sw}.npz")
        env = dict(os.environ, SOCP_FUSE_U=sw)
        p = subprocess.run([sys.executable, os.path.join(HERE, "fuse_u_cases.py"), inp, outp], env=env,
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        got[sw] = dict(np.load(outp))
    return got, want


def assert_bitwise(on, off, name, keys):
    for key in keys:
        a, b = on[f"{name}/{key}"], off[f"{name}/{key}"]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (name, key)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_switch_on_off_bitwise_and_oracle(runs, case):
    got, want = runs
    on, off = got["1"], got["0"]
    name = case.name
    assert case.variant in str(on[f"{name}/kernel"]) and case.variant in str(off[f"{name}/kernel"])
    assert str(on[f"{name}/kernel"]) == str(off[f"{name}/kernel"])
    assert_bitwise(on, off, name, KEYS)
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


@pytest.mark.parametrize("name", ["life", "life_res"])
def test_flag_does_not_outlive_its_problem(runs, name):
    got, _ = runs
    on, off = got["1"], got["0"]
    assert_bitwise(on, off, name, KEYS + (("res",) if name == "life_res" else ()))
    it = on[f"{name}/iters"]
    print(f"{name}: {LIFE['batch']} problems, iterations {it.min()}..{it.max()}, "
          f"status counts {np.bincount(on[f'{name}/status'], minlength=5).tolist()}")
    # the case is about problems leaving at different iterations
    assert it.min() < it.max()
