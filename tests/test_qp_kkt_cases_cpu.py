"""The preconditions of test_gpu_qp_kkt.py, without a device: the table of
qp_kkt_cases.py names the kernel each case must select, the numpy restatement
(qp_cases._Factor) is pinned to the CPU oracle at P = 0, every case's block
system is nonsingular and its refinement converges, and the restatement's own
error e_rs -- ten times which is the GPU tests' gate -- is printed per case.
The MOI adapter's quadratic objective (parsing, P, sense, objective_value) and
the Python entries' host-side checks are here too.
"""
import numpy as np
import pytest

import kkt_cases as KC
import qp_kkt_cases as QK
import socp_amd as S
from socp_amd import _lib, moi


# ------------------------------------------------------------------ the table
@pytest.mark.parametrize("case", QK.CASES, ids=QK.case_id)
def test_case_selects_its_kernel(case):
    assert QK.kernel_name(case) == case.kernel
    assert sum(d for _, _, d in case.cones) == case.k
    if case.sing:
        assert case.m >= 1 and case.n - case.m <= case.k


def test_every_variant_has_the_qp_plugin_kernel():
    import gen_inst
    for v in gen_inst.VARIANTS:
        assert gen_inst.qp_kkt_kms(v) == (9,) and 9 in gen_inst.all_kms(v), v
    assert gen_inst.SUFFIX[9] == "_qpkkt"


def test_exports():
    import ctypes
    L = ctypes.CDLL(_lib.LIB_PATH)
    header = open(_lib.HEADER).read()
    for name in ("socp_batch_kkt_solve_qp", "socp_dense_create_qp", "socp_ingest_submit_qp",
                 "socp_ingest_set_matrices_qp", "socp_ingest_next_P"):
        assert name in _lib.EXPORTED + _lib.EXPORTED_MIXED_CASE
        assert name + "(" in header and hasattr(L, name), name


# ------------------------------------------------- the restatement at P = 0
@pytest.mark.parametrize("case", QK.CASES, ids=QK.case_id)
def test_restatement_equals_oracle_at_zero_P(oracle, case):
    """qp_cases._Factor(...).solve with P = 0 against oracle.kkt_single in the
    kernels' order (structured=True, chol=True): rel <= 1e-11, the figure
    test_qp_cpu.py holds the same pair to."""
    d = QK.inputs(case)
    n = case.n
    worst = 0.0
    for p in range(QK.B):
        rhs = KC.problem_rhs(d, p)
        rs = QK.restatement_of(case.cones, np.zeros((n, n)), d["A"][p], d["G"][p], case.sing, d["s"][p], d["z"][p], rhs)
        orc = KC.oracle_of(case.cones, d["A"][p], d["G"][p], bool(case.sing), d["s"][p], d["z"][p], rhs, False)
        for r, o in zip(rs, orc):
            assert o["status"] == 0
            for u, key in zip(r, KC.KEYS):
                if len(u):
                    worst = max(worst, np.linalg.norm(u - o[key]) / np.linalg.norm(o[key]))
    print(f"{case.id}: worst rel {worst:.2e}")
    assert worst <= 1e-11


# ------------------------------------------------------------ the reference
@pytest.mark.parametrize("case", QK.CASES, ids=QK.case_id)
def test_reference_converges_and_restatement_error(oracle, case):
    """K is nonsingular (kappa_2 (n + m + 2k) 2^-53 < 1e-6), refined_solve's last
    correction is below the floor (n + m + 2k) 2^-53, and P is what the module
    says: symmetric, positive semidefinite, singular."""
    d = QK.inputs(case)
    n, m, k = case.n, case.m, case.k
    for p in range(QK.B):
        P = d["P"][p]
        assert np.array_equal(P, P.T)
        w = np.linalg.eigvalsh(P)
        assert w[0] > -1e-12 * w[-1] and np.linalg.matrix_rank(P) <= n // 2 < n
        if case.sing:
            z = QK.zeroed(case)
            assert not d["G"][p][:, z].any() and not P[z, :].any() and not P[:, z].any()
            assert not any(r[1][p].any() for r in d["rhs"])
        kap = QK.kappa(case, p)
        assert np.isfinite(kap) and kap * KC.floor(n, m, k) < 1e-6, kap  # the refinement contracts
        ref = QK.reference(case, p)
        assert (ref.corr <= KC.floor(n, m, k)).all(), (ref.corr, ref.steps)
        for j in range(QK.NRHS):
            e = QK.restatement_errors(case, p)[j]
            g = QK.gates(case, p, j)
            print(f"{case.id} p={p} rhs {j}: kappa(K) {kap:.2e}, e_rs "
                  + " ".join("-" if v is None else f"{v:.2e}" for v in e)
                  + " gate " + " ".join("-" if v is None else f"{v:.2e}" for v in g))
            for v in e:  # the restatement solves the block system: within kappa(K) roundings of a sum
                assert v is None or v <= kap * KC.floor(n, m, k)


def test_P_moves_the_solution(oracle):
    """At (32, 8, 48) the reference with P differs from the one without by
    more than 100 gates in every vector: a build that ignores P cannot pass."""
    case = QK.BY_ID["c1"]
    d = QK.inputs(case)
    for p in range(QK.B):
        with_P = QK.reference(case, p)
        no_P = QK.reference_of(case.cones, np.zeros((case.n, case.n)), d["A"][p], d["G"][p], d["s"][p], d["z"][p],
                               KC.problem_rhs(d, p))
        for j in range(QK.NRHS):
            e = KC.rel_errors(no_P.sol[j], with_P.sol[j])
            for ev, gv in zip(e, QK.gates(case, p, j)):
                assert ev > 100.0 * gv


# ---------------------------------------------------------- host-side checks
def test_python_entries_check_P():
    c = QK.BY_ID["s8"]
    d = QK.inputs(c)
    Af, Gf = KC.flat(d)
    args = (list(c.cones), c.n, c.m, c.k, Af, Gf, QK.sing_bytes(c), d["s"].ravel(), d["z"].ravel(),
            *KC.flat_rhs(d, 0, c.m))
    bad = QK.flat_P(d).copy()
    bad[1] += 1.0
    with pytest.raises(ValueError, match="symmetric"):
        S.batch_kkt_solve(*args, P=bad)
    with pytest.raises(ValueError, match="P:"):
        S.batch_kkt_solve(*args, P=bad[:-1])
    with pytest.raises(ValueError, match="symmetric"):
        S.DenseHandle(*args[:7], P=bad)
    with pytest.raises(ValueError, match="P:"):
        S.DenseHandle(*args[:7], P=bad[:-1])


def test_sparse_solver_refuses_P():
    c = QK.BY_ID["s8"]
    d = QK.inputs(c)
    cones = [S.SOC(0, 16)]
    prob = S.Problem(np.zeros(c.n), d["A"][0], np.zeros(c.m), d["G"][0], np.zeros(c.k), cones, P=d["P"][0])
    with pytest.raises(ValueError, match="linear objectives only"):
        S.SparseSolver(prob)


# ------------------------------------------------------------------------ MOI
def _model(sense=moi.MIN_SENSE, flip=1.0):
    o = moi.Optimizer()
    x = o.add_variables(3)
    o.add_constraint(moi.vaf([(1, x[0], 1.0), (2, x[1], 1.0), (3, x[2], 1.0)], [0.0, 0.0, 0.0]), moi.Nonnegatives(3))
    # x'Qx/2 + a'x + 7 with Q = [[4, 1, 0], [1, 2, -3], [0, -3, 6]]: the (2, 3) entry given in two terms
    f = moi.sqf([(x[0], x[0], flip * 4.0), (x[0], x[1], flip * 1.0), (x[1], x[1], flip * 2.0),
                 (x[1], x[2], flip * -1.0), (x[2], x[1], flip * -2.0), (x[2], x[2], flip * 6.0)],
                [(x[0], flip * 1.0), (x[2], flip * -2.0)], flip * 7.0)
    o.set_objective_sense(sense)
    o.set_objective_function(f)
    return o, x


Q_EXPECT = np.array([[4.0, 1.0, 0.0], [1.0, 2.0, -3.0], [0.0, -3.0, 6.0]])


def test_moi_quadratic_function_assembles_P():
    o, _ = _model()
    d = o.build()
    assert np.array_equal(d.P, Q_EXPECT) and np.array_equal(d.P, d.P.T)
    assert np.array_equal(d.c, [1.0, 0.0, -2.0]) and d.objconstant == 7.0
    lin, _ = _model()
    lin.set_objective_function(moi.saf([], 0.0))
    assert lin.build().P is None


def test_moi_max_sense_negates_P_with_c():
    o, _ = _model(moi.MAX_SENSE, -1.0)  # maximise -(x'Qx/2 + a'x + 7)
    d = o.build()
    assert np.array_equal(d.P, Q_EXPECT) and np.array_equal(d.c, [1.0, 0.0, -2.0])


def test_moi_objective_value_adds_the_quadratic_term():
    xv = np.array([0.5, -1.0, 2.0])
    want = 0.5 * xv @ Q_EXPECT @ xv + np.array([1.0, 0.0, -2.0]) @ xv + 7.0
    o, x = _model()
    o.build()
    o._set_solution(xv, np.zeros(0), np.zeros(3), np.zeros(3), 1, 0)
    assert o.objective_value() == pytest.approx(want, rel=1e-15)
    o, x = _model(moi.MAX_SENSE, -1.0)
    o.build()
    o._set_solution(xv, np.zeros(0), np.zeros(3), np.zeros(3), 1, 0)
    assert o.objective_value() == pytest.approx(-want, rel=1e-15)


def test_moi_objective_checks():
    o = moi.Optimizer()
    x = o.add_variables(2)
    with pytest.raises(ValueError, match="unknown variable"):
        o.set_objective_function(moi.sqf([(x[0], moi.VariableIndex(3), 1.0)]))
    with pytest.raises(TypeError):
        o.set_objective_function(moi.vaf([], []))
