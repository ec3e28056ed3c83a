"""Every compiled instantiation of the register-resident kernel against the
oracle: the cases of variant_cases.py (two shapes per variant, the pure-slot
tables of the two-slot variants), one test function per mode, the variant in
the test id.  tests/test_variant_table_cpu.py holds the preconditions: the
shapes select their variants, the cases reach all 220 (variant, KM) kernels,
the oracle runs each to maxit and its one-rounding floor is at most 1e-9.

Every case first checks socp_last_kernel_name: the mode's entry name and
<NQ,NP,MQ>, which pins variant_cases.pick_variant to the library's.  Gates,
all of them the project's own:
  plain solver   K = 1..3 against the oracle in the kernels' order within
                 10 floor + 1e-13 per vector (problems.trajectory_at_floor);
  detecting      on these feasible batches bitwise the plain call (which took
                 a pure-slot kernel where the table has one: also a check of
                 the slot kernels against the mixed kernel's bits);
  QP             P = 0 bitwise the plain call; P = R'R/n at the full shapes
                 against qp_cases.qp_reference at K = 2, rel <= 1e-8;
  plugin         batch_kkt_solve at the oracle's first iterate: block-row
                 backward error <= max(1e-12, 10 x the oracle's); setup_iter +
                 solve_kkt bitwise the fused call;
  explicit inv.  MQ = 1: the same two comparisons with the flag, against
                 F_STRUCTURED | F_INV_YTY; MQ > 1: the flag selects the
                 default kernel and its bits.
<4,8,1> holds no solvable problem (variant_cases.EXEMPT): its kernels are
launched, their names checked, and no problem may report convergence.

Measured on MI355X: 468 cases in 7.8 s; worst error / gate: plain solver 0.75,
explicit-inverse solver 0.39, plugin entries 0.40 and 0.54 (explicit inverse),
QP against the restatement 3.2e-4.  Before the z's sum of the residual passes
became an explicit fma (socp_small.hpp), the QP solver's res[2] at P = 0 was 1
to 64 ulps from the plain call's on 9 cases with k > 64.
"""
import functools

import numpy as np
import pytest

import oracle as O
import problems
import qp_cases as Q
import socp_amd as S
import variant_cases as V

pytestmark = pytest.mark.gpu

OUT = ("x", "y", "z", "s", "iters", "status")
MIXED = [c for c in V.CASES if V.plugin_case(c)]
# worst error / gate per mode, printed by every case (-s shows them)
WORST = {}


def note(mode, case, ratio):
    WORST[mode] = max(WORST.get(mode, 0.0), ratio)
    print(f"{mode} {case.id}: error / gate {ratio:.3g} (worst so far {WORST[mode]:.3g})")


def kernel_is(case, km):
    name = S.default_context().last_kernel_name()
    assert name == V.kernel_name(case.variant, km), (name, case.id, km)
    return name


def solve(case, K=V.K, P=None, **kw):
    d = V.data(case)
    return S.batch_solve(list(case.cones), case.n, case.m, case.k, d["c"], d["A"], d["b"], d["G"], d["h"],
                         V.sing_bytes(case), maxit=K, tol=0.0, P=P, **kw)


@functools.lru_cache(maxsize=None)
def plain(case, K=V.K):
    """The plain call's outputs (with res), launched once per case and K."""
    out = solve(case, K, res=True)
    kernel_is(case, V.solver_km(case))
    return out


def same(a, b, keys=OUT):
    for key in keys:
        u, v = np.asarray(a[key]), np.asarray(b[key])
        assert u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes(), key


def rel(u, v):
    return float(np.linalg.norm(u - v) / np.linalg.norm(v)) if len(v) else 0.0


def exempt(case):
    return case.variant in V.EXEMPT


def no_convergence(out):
    assert (out["status"] != S.CONVERGED).all(), out["status"]


def trajectory(case, explicit_inverse):
    km = 2 if explicit_inverse else V.solver_km(case)

    def run(K):
        g = solve(case, K, explicit_inverse=explicit_inverse)
        kernel_is(case, km)
        return g

    rows = problems.trajectory_at_floor(O, case, V.data(case), V.B, V.K, V.kernel_order(O, case, explicit_inverse),
                                        run, ref=V.reference(case, explicit_inverse))
    note("xi" if explicit_inverse else "plain", case, rows[0][0])
    assert rows[0][0] <= 1.0, rows[:6]


# --------------------------------------------- KM 0, 16, 32, 64: plain solver
@pytest.mark.parametrize("case", V.CASES, ids=V.case_id)
def test_plain_solver(case):
    if exempt(case):
        no_convergence(plain(case))
        return
    trajectory(case, False)
    ref = V.reference(case)
    out = plain(case)  # the K = 3 run once more, with res: the same bits
    assert (out["status"] == S.MAXIT).all() and (out["iters"] == V.K).all()
    for p in range(V.B):
        assert np.isfinite(out["res"][3 * p:3 * p + 3]).all()
        assert rel(out["x"][p * case.n:(p + 1) * case.n], ref[p][0][V.K][0]) <= 1e-8


# -------------------------------------------------- KM 4: detecting solver
@pytest.mark.parametrize("case", V.CASES, ids=V.case_id)
def test_detecting_solver(case):
    on = solve(case, detect_infeasible=True, res=True)
    kernel_is(case, 4)
    if exempt(case):
        no_convergence(on)
        return
    same(on, plain(case))


# ----------------------------------------------------------- KM 8: QP solver
@pytest.mark.parametrize("case", V.CASES, ids=V.case_id)
def test_qp_solver(case):
    zero = np.zeros(V.B * case.n * case.n)
    got = solve(case, P=zero, res=True)
    kernel_is(case, 8)
    if exempt(case):
        no_convergence(got)
        return
    same(got, plain(case), OUT + ("res",))
    if case.shape != "full" or case.table != "mixed":
        return
    Ps = V.qp_matrices(case)
    K = 2
    got = solve(case, K, P=np.concatenate([Pm.ravel(order="F") for Pm in Ps]))
    kernel_is(case, 8)
    n, m, k = case.n, case.m, case.k
    worst = 0.0
    for p in range(V.B):
        c, A, b, G, h = V.problem(case, p)
        r = Q.qp_reference(list(case.cones), (Ps[p], c, A, b, G, h), V.sing_bool(case), maxit=K, tol=0.0)
        assert got["status"][p] == r["status"] == S.MAXIT and got["iters"][p] == K, (p, r["status"])
        for key, L in (("x", n), ("y", m), ("z", k), ("s", k)):
            e = rel(got[key][p * L:(p + 1) * L], r[key])
            worst = max(worst, e / 1e-8)
            assert e <= 1e-8, (p, key, e)
    note("qp", case, worst)


# ------------------------------------------ KM 1, 3: plugin entries
def kkt_inputs(case):
    """The oracle's iterate at t = 1 of every problem and seeded right-hand sides."""
    flags = V.kernel_order(O, case)
    s, z = [], []
    for p in range(V.B):
        c, A, b, G, h = V.problem(case, p)
        tr = O.solve_trace(list(case.cones), c, A, b, G, h, sing=V.sing_bool(case),
                           params=O.Params(maxit=2, tol=0.0, flags=flags), max_trace=3)
        s.append(tr["trace"][1][3])
        z.append(tr["trace"][1][2])
    rng = np.random.default_rng(case.seed + 1)
    rhs = [rng.standard_normal(V.B * q) for q in (case.n, case.m, case.k, case.k)]
    return np.concatenate(s), np.concatenate(z), rhs


def backward_error(case, p, s, z, rhs, sol):
    """test_gpu_parity.py::test_kkt_backward_error's: the largest block-row residual relative to the data."""
    c, A, b, G, h = V.problem(case, p)
    sc = O.compute_scaling(list(case.cones), s, z)
    W, lam = sc["W"], sc["l"]
    cx, cy, cz, cs = sol
    r1 = A.T @ cy + G.T @ cz - rhs[0]
    r2 = A @ cx - rhs[1]
    r3 = G @ cx + cs - rhs[2]
    r4 = O.vprod(list(case.cones), lam, W @ cz + np.linalg.solve(W.T, cs)) - rhs[3]
    scale = max(np.abs(np.concatenate(rhs)).max(), np.abs(np.concatenate([cx, cy, cz, cs])).max())
    return max(np.abs(rr).max() for rr in (r1, r2, r3, r4)) / scale


def plugin_entries(case, explicit_inverse):
    d = V.data(case)
    n, m, k = case.n, case.m, case.k
    mode = "xi_kkt" if explicit_inverse else "kkt"
    if exempt(case):  # no iterate to stand at: the cones' identity; the factorisation fails or not by rounding
        e = np.tile(O.make_e(list(case.cones), k), V.B)
        rng = np.random.default_rng(case.seed + 1)
        rhs = [rng.standard_normal(V.B * q) for q in (n, m, k, k)]
        S.batch_kkt_solve(list(case.cones), n, m, k, d["A"], d["G"], V.sing_bytes(case), e, e, *rhs,
                          explicit_inverse=explicit_inverse)
        kernel_is(case, 3 if explicit_inverse else 1)
        return
    s, z, rhs = kkt_inputs(case)
    fused = S.batch_kkt_solve(list(case.cones), n, m, k, d["A"], d["G"], V.sing_bytes(case), s, z, *rhs,
                              explicit_inverse=explicit_inverse)
    name = kernel_is(case, 3 if explicit_inverse else 1)
    assert (fused["status"] == 0).all(), fused["status"]
    worst = 0.0
    for p in range(V.B):
        sl = lambda v, q: v[p * q:(p + 1) * q]  # noqa: E731
        rp = [sl(v, q) for v, q in zip(rhs, (n, m, k, k))]
        sp, zp = sl(s, k), sl(z, k)
        c, A, b, G, h = V.problem(case, p)
        o = O.kkt_single(list(case.cones), A, G, V.sing_bool(case), sp, zp, *rp)
        ref_err = backward_error(case, p, sp, zp, rp, (o["cx"], o["cy"], o["cz"], o["cs"]))
        err = backward_error(case, p, sp, zp, rp, (sl(fused["cx"], n), sl(fused["cy"], m), sl(fused["cz"], k),
                                                   sl(fused["cs"], k)))
        gate = max(1e-12, 10 * ref_err)
        worst = max(worst, err / gate)
        assert err <= gate, (p, err, ref_err)
    note(mode, case, worst)
    hd = S.DenseHandle(list(case.cones), n, m, k, d["A"], d["G"], V.sing_bytes(case), explicit_inverse=explicit_inverse)
    try:
        assert (hd.setup_iter(s, z) == 0).all()
        assert S.default_context().last_kernel_name() == name
        split = hd.solve_kkt(*rhs)
        assert S.default_context().last_kernel_name() == name
    finally:
        hd.close()
    same(split, fused, ("cx", "cy", "cz", "cs", "status"))


@pytest.mark.parametrize("case", MIXED, ids=V.case_id)
def test_plugin_entries(case):
    plugin_entries(case, False)


# ------------------------------------------------ KM 2, 3: explicit inverse
@pytest.mark.parametrize("case", MIXED, ids=V.case_id)
def test_explicit_inverse(case):
    if case.variant[2] > 1:
        # m > 16 forms H^-1 anyway: the flag selects the default kernels and their bits
        on = solve(case, explicit_inverse=True, res=True)
        name = kernel_is(case, 0)
        assert "xi" not in name
        same(on, solve(case, res=True), OUT + ("res",))
        d = V.data(case)
        s, z, rhs = kkt_inputs(case)
        args = (list(case.cones), case.n, case.m, case.k, d["A"], d["G"], V.sing_bytes(case), s, z) + tuple(rhs)
        on = S.batch_kkt_solve(*args, explicit_inverse=True)
        assert "xi" not in kernel_is(case, 1)
        same(on, S.batch_kkt_solve(*args), ("cx", "cy", "cz", "cs", "status"))
        return
    if exempt(case):
        no_convergence(solve(case, explicit_inverse=True))
        kernel_is(case, 2)
        plugin_entries(case, True)
        return
    trajectory(case, True)
    plugin_entries(case, True)
