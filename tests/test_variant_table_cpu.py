"""Preconditions of test_gpu_variants.py, checked on the CPU: the cases of
variant_cases.py reach every compiled (variant, KM) kernel of gen_inst.py,
the oracle runs every one of them to maxit, their one-rounding floors keep the
floor gate inside gate P4, and the gate is sensitive to a dropped row of G.
"""
import functools

import numpy as np
import pytest

import problems
import socp_amd as S
import variant_cases as V

MAXIT_ST = 1
MIXED = [c for c in V.NUMERIC if V.plugin_case(c)]


def orders(c):
    """Whether the case runs in the default order only, or in the explicit-inverse order too."""
    return (False, True) if V.plugin_case(c) and c.variant[2] == 1 else (False,)


# ------------------------------------------------------------ 1. the picker
@pytest.mark.parametrize("case", V.CASES, ids=V.case_id)
def test_shape_selects_its_variant(case):
    assert V.pick_variant(case.n, case.m, case.k) == case.variant
    assert sum(c[2] for c in case.cones) == case.k and len(case.cones) <= 8
    assert [c[1] for c in case.cones] == list(np.cumsum([0] + [c[2] for c in case.cones[:-1]]))
    kinds = [c[0] for c in case.cones]
    assert kinds == sorted(kinds)  # POC (0) before SOC (1)
    if case.sing:
        assert case.k < case.n and case.variant in V.UNREACHED_BY_FULL_RANK
    else:
        assert case.k > case.n
    assert case.m <= case.n


def test_picker_restates_the_cost_rule():
    # the first minimum in table order; nothing above the table's edges
    assert V.pick_variant(64, 16, 96) == (4, 24, 1) and V.pick_variant(32, 8, 48) == (2, 12, 1)
    assert V.pick_variant(49, 16, 97) is None and V.pick_variant(48, 16, 128) == (3, 32, 1)
    assert V.pick_variant(65, 1, 66) is None and V.pick_variant(16, 17, 32) == (2, 8, 2)
    assert V.pick_variant(10, 0, 12) == V.pick_variant(10, 1, 12) == (1, 4, 1)
    assert V.VARIANTS == sorted(V.VARIANTS)  # the table's order, for the first minimum


def test_full_and_sparse_shapes_sit_at_the_tile_edges():
    for c in V.CASES:
        NQ, NP, MQ = c.variant
        if c.shape == "full" and not c.sing:
            assert c.k == 4 * NP - 1 and c.k % 4 and c.n % 16 and c.m % 16
            if (c.variant, "full") not in V.SHAPE:
                assert c.n == min(16 * NQ - 1, c.k - 1) and c.m == (c.n // 2 if NQ == 1 else min(16 * MQ - 1, c.n - 1))
        if c.shape == "sparse" and not c.sing and (c.variant, "sparse") not in V.SHAPE and c.variant[2] == 1:
            # one less in any dimension selects a smaller variant, or breaks m <= n < k
            # (n is one past the next smaller compiled NQ also where no variant of that NQ holds m:
            # MQ = 4 is compiled for NQ = 4 alone)
            for n, m, k in ((c.n - 1, c.m, c.k), (c.n, c.m - 1, c.k), (c.n, c.m, c.k - 1)):
                if n < c.n and not any(u[0] < NQ and u[2] >= MQ for u in V.VARIANTS):
                    continue
                assert min(n, m) < 1 or not m <= n < k or V.pick_variant(n, m, k) != c.variant, (c.id, n, m, k)
        if c.shape == "sp":
            assert c.k % 16 == 0 and c.k in ((80, 96) if NP == 24 else (112,))


# ----------------------------------------------------- 2., 3. the coverage
def test_every_compiled_kernel_is_launched():
    compiled = {(v, km) for v in V.VARIANTS for km in V.kms(v)}
    assert len(V.VARIANTS) == 36 and len(compiled) == 220
    got = set()
    for c in V.CASES:
        got |= V.launched(c)
    assert got == compiled
    # every variant has a full and a sparse shape, every two-slot variant its three pure-slot tables
    for v in V.VARIANTS:
        mine = [c for c in V.CASES if c.variant == v]
        assert {c.shape for c in mine} >= {"full", "sparse"}
        assert {c.table for c in mine} == ({"mixed", "ps", "pp", "sp"} if v[1] > 16 else {"mixed"})
    assert len({c.id for c in V.CASES}) == len(V.CASES)
    # one sparse case per NQ leaves sing to the device probe
    assert sorted(c.variant[0] for c in V.CASES if c.sing is None) == [1, 2, 3, 4]


def test_the_exemption_is_one_variant():
    assert V.EXEMPT == {(4, 8, 1)}
    assert {c.variant for c in V.EXEMPT_CASES} == V.EXEMPT
    assert sorted(V.SING_SHAPES) == sorted(V.UNREACHED_BY_FULL_RANK) and len(V.UNREACHED_BY_FULL_RANK) == 7
    # every numeric comparison of the GPU module runs on all the other kernels
    numeric = set()
    for c in V.NUMERIC:
        numeric |= V.launched(c)
    assert numeric == {(v, km) for v in V.VARIANTS for km in V.kms(v) if v not in V.EXEMPT}
    # rank(H) <= k + m < n at every shape that selects the exempt variant
    for n in range(49, 65):
        for m in range(0, 17):
            for k in range(1, 33):
                if V.pick_variant(n, m, k) == (4, 8, 1):
                    assert k + m < n


def test_exempt_variant_holds_no_solvable_problem(oracle):
    for c in V.EXEMPT_CASES:
        d = V.data(c)
        for flags in (0, V.kernel_order(oracle, c), V.kernel_order(oracle, c, True)):
            r = oracle.batch_solve(list(c.cones), c.n, c.m, c.k, d["c"], d["A"], d["b"], d["G"], d["h"],
                                   sing=np.ones(V.B, np.uint8), params=oracle.Params(maxit=V.K, tol=0.0, flags=flags))
            assert (r["status"] == 2).all() and (r["iters"] == 0).all(), (c.id, flags, r["status"])


def test_slot_tables_take_their_kernels():
    """The kernel name does not tell the slot kernels apart: the host's plan does."""
    for c in V.CASES:
        if c.k > 64:
            assert S.slot_plan(list(c.cones), c.k) == V.TABLE_PLAN[c.table], c.id
            if c.table == "mixed":  # both kinds in slot 0
                assert c.cones[0][0] == V.P_ and c.cones[0][2] < 64 and c.cones[1][0] == V.Q_
        else:
            assert c.table == "mixed" and S.slot_plan(list(c.cones), c.k) == (0, 0, 0)


# ------------------------------------------------ 4., 5. the oracle's runs
@pytest.mark.parametrize("case", V.NUMERIC, ids=V.case_id)
def test_oracle_runs_to_maxit_in_the_kernels_order(oracle, case):
    d = V.data(case)
    for xi in orders(case):
        for K in range(1, V.K + 1):
            r = oracle.batch_solve(list(case.cones), case.n, case.m, case.k, d["c"], d["A"], d["b"], d["G"], d["h"],
                                   sing=np.full(V.B, V.sing_bool(case), np.uint8),
                                   params=oracle.Params(maxit=K, tol=0.0, flags=V.kernel_order(oracle, case, xi)))
            assert (r["status"] == MAXIT_ST).all() and (r["iters"] == K).all(), (xi, K, r["status"])


@pytest.mark.parametrize("case", V.NUMERIC, ids=V.case_id)
def test_floor_is_inside_the_trajectory_gate(case):
    for xi in orders(case):
        ref = V.reference(case, xi)
        assert len(ref) == V.B
        worst = max(fl[key] for _, floors in ref for fl in floors for key in "xzs")
        print(f"{case.id} explicit_inverse={xi} worst floor {worst:.2e}")
        assert worst <= V.FLOOR_CAP, (xi, worst)
        assert problems.FLOOR_FACTOR * worst + problems.FLOOR_ABS <= 1.0001e-8


@pytest.mark.parametrize("case", [c for c in MIXED if c.shape == "full"], ids=V.case_id)
def test_qp_restatement_runs_its_two_iterations(case):
    """The nonzero-P comparison of test_gpu_variants.py: qp_cases.qp_reference reaches maxit at K = 2
    on every problem, at a conditioning where rel <= 1e-8 is the gate of tests/test_gpu_qp.py
    (kappa_2(H) <= 1e6: 1e-16 kappa is two orders inside it)."""
    import qp_cases as Q
    worst = 0.0
    for p, Pm in enumerate(V.qp_matrices(case)):
        c, A, b, G, h = V.problem(case, p)
        r = Q.qp_reference(list(case.cones), (Pm, c, A, b, G, h), V.sing_bool(case), maxit=2, tol=0.0)
        assert r["status"] == MAXIT_ST and r["iters"] == 2, (p, r["status"])
        worst = max(worst, max(r["kappa"]))
    print(f"{case.id}: worst kappa_2(H) {worst:.2e}")
    assert worst <= 1e6, worst


@pytest.mark.parametrize("case", MIXED, ids=V.case_id)
def test_conditioning_is_inside_the_window_of_the_tight_gates(case):
    kappa = V.conditioning(case)
    print(f"{case.id}: kappa {kappa:.2e}")
    if case.id in V.KAPPA_ABOVE:  # the sing shapes that stand as given
        assert case.sing and V.KAPPA_CAP < kappa <= 4e6, kappa  # measured 8.0e5 .. 3.8e6
    else:
        assert kappa <= V.KAPPA_CAP, kappa


def test_probe_cases_are_not_sing(oracle):
    # sing = None runs the device probe; these G have full column rank, so the probe says 0 as the oracle's rule does
    for c in V.CASES:
        if c.sing is None:
            for p in range(V.B):
                assert not oracle.sing_flag(V.problem(c, p)[3]), (c.id, p)


# ------------------------------------------------------- 6. the gate bites
@functools.lru_cache(maxsize=None)
def _dropped_row(case):
    """Worst error / gate of the oracle on G with its last row zeroed -- what a
    kernel that dropped its ragged last row step would solve -- against the
    oracle on the case's own data."""
    import oracle
    d = dict(V.data(case))
    G = d["G"].copy().reshape(V.B, case.n, case.k)  # [problem, column, row]
    G[:, :, case.k - 1] = 0.0
    d["G"] = G.reshape(-1)
    flags = V.kernel_order(oracle, case)
    sing = np.full(V.B, V.sing_bool(case), np.uint8)

    def solve(K):
        r = oracle.batch_solve(list(case.cones), case.n, case.m, case.k, d["c"], d["A"], d["b"], d["G"], d["h"],
                               sing=sing, params=oracle.Params(maxit=K, tol=0.0, flags=flags))
        r["status"] = np.ones_like(r["status"])  # only the distance is asked for here
        return r

    return problems.trajectory_at_floor(oracle, case, V.data(case), V.B, V.K, flags, solve,
                                        ref=V.reference(case))[0]


@pytest.mark.parametrize("case", [c for c in V.NUMERIC if c.shape == "full"], ids=V.case_id)
def test_gate_sees_a_dropped_last_row(case):
    row = _dropped_row(case)
    print(f"{case.id}: dropped last row of G, worst error / gate {row[0]:.3g} (K={row[1]}, {row[3]})")
    assert row[0] >= 100.0, row
