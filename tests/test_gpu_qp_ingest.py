"""Quadratic objectives through the pipelined ingest (socp_ingest_submit_qp,
socp_ingest_set_matrices_qp, socp_ingest_next_P) and the MOI adapter
(ScalarQuadraticFunction): every result is bitwise ``batch_solve(P=...)`` on
the same inputs, a submit without P between QP submits is bitwise the linear
solve, and the two refused flags leave the slot free.
"""
import numpy as np
import pytest

import qp_cases as Q
import socp_amd as S
from socp_amd import _lib, moi

pytestmark = pytest.mark.gpu

KEYS = ("x", "y", "z", "s", "iters", "status")
NB = 8  # problems per batch


def same(a, b):
    for key in KEYS:
        u, v = np.asarray(a[key]), np.asarray(b[key])
        assert u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes(), key


def part(d, i):
    """Batch i (NB problems) of the flat arrays of a qp_cases batch."""
    n, m, k = d.shape.n, d.shape.m, d.shape.k
    sl = lambda v, q: v[i * NB * q:(i + 1) * NB * q]  # noqa: E731
    return dict(P=sl(d.P, n * n), c=sl(d.c, n), A=sl(d.A, m * n) if m else None, b=sl(d.b, m) if m else None,
                G=sl(d.G, k * n), h=sl(d.h, k), sing=sl(d.sing, 1))


def solve(d, q, P=True):
    sh = d.shape
    return S.batch_solve(list(sh.cones), sh.n, sh.m, sh.k, q["c"], q["A"], q["b"], q["G"], q["h"], q["sing"],
                         P=q["P"] if P else None)


@pytest.mark.parametrize("name", ["c1", "blk"])  # (32, 8, 48): the register kernel; (80, 20, 120): the blocked one
def test_three_qp_batches_and_a_linear_one_through_two_slots(name):
    d = Q.batch(name, 3 * NB)
    sh = d.shape
    n, m, k = sh.n, sh.m, sh.k
    q = [part(d, i) for i in range(3)]
    want = [solve(d, q[i]) for i in range(3)]
    qp_name = S.default_context().last_kernel_name()
    assert "_qp_" in qp_name, qp_name
    want_lin = solve(d, q[1], P=False)
    assert "_qp_" not in S.default_context().last_kernel_name()
    assert not np.array_equal(want_lin["x"], want[1]["x"])
    ing = S.Ingest(list(sh.cones), n, m, k, NB)
    try:
        sub = lambda v, **kw: ing.submit(v["c"], v["A"], v["b"], v["G"], v["h"], v["sing"], **kw)  # noqa: E731
        t0 = sub(q[0], P=q[0]["P"])
        # batch 1 written in place into the other slot's pinned blocks
        pin = ing.next_inputs(P=True)
        for key, v in q[1].items():
            if v is not None:
                pin[key][:np.size(v)] = v
        cut = {key: (pin[key][:np.size(v)] if v is not None else None) for key, v in q[1].items()}
        t1 = sub(cut, P=cut["P"])
        assert (t0, t1) == (0, 1)
        same(ing.wait(t0), want[0])
        t2 = sub(q[1])  # the linear solve between two QP batches, through slot 0 (which has carried a P)
        same(ing.wait(t1), want[1])
        t3 = sub(q[2], P=q[2]["P"])
        same(ing.wait(t2), want_lin)
        same(ing.wait(t3), want[2])
        assert S.default_context().last_kernel_name() == qp_name
    finally:
        ing.close()


def test_refused_flags_leave_the_slot_free():
    d = Q.batch("c1", 3 * NB)
    sh = d.shape
    q = part(d, 0)
    ing = S.Ingest(list(sh.cones), sh.n, sh.m, sh.k, NB)
    try:
        for flag in ("explicit_inverse", "detect_infeasible"):
            with pytest.raises(S.SocpError) as ei:
                ing.submit(q["c"], q["A"], q["b"], q["G"], q["h"], q["sing"], P=q["P"], **{flag: True})
            assert ei.value.code == _lib.SOCP_E_UNSUPPORTED and "socp_ingest_submit_qp" in str(ei.value)
        t = ing.submit(q["c"], q["A"], q["b"], q["G"], q["h"], q["sing"], P=q["P"])
        assert t == 0  # no ticket was spent on the refusals
        same(ing.wait(t), solve(d, q))
        # without a P both flags keep their meaning
        t = ing.submit(q["c"], q["A"], q["b"], q["G"], q["h"], q["sing"], detect_infeasible=True)
        assert t == 1
        ing.wait(t)
    finally:
        ing.close()


@pytest.mark.parametrize("name", ["c1", "blk"])
def test_shared_P_through_set_matrices(name):
    d = Q.shared_batch(name, NB)
    sh = d.shape
    n, m, k = sh.n, sh.m, sh.k
    sing = np.zeros(1, np.uint8)
    bs = lambda P: S.batch_solve(list(sh.cones), n, m, k, d.c, d.A, d.b, d.G, d.h, sing,  # noqa: E731
                                 shared_matrices=True, P=P)
    want, want_lin = bs(d.P), bs(None)
    assert not np.array_equal(want["x"], want_lin["x"])
    ing = S.Ingest(list(sh.cones), n, m, k, NB, shared_matrices=True)
    try:
        ing.set_matrices(d.A, d.G, sing)
        with pytest.raises(S.SocpError):  # no P yet
            ing.submit(d.c, None, d.b, None, d.h, qp=True)
        ing.set_matrices(d.A, d.G, sing, P=d.P)
        with pytest.raises(S.SocpError):  # the slots of a shared ingest stage no P
            ing.next_inputs(P=True)
        t0 = ing.submit(d.c, None, d.b, None, d.h, qp=True)
        t1 = ing.submit(d.c, None, d.b, None, d.h)  # the plain submit stays the linear solve
        assert (t0, t1) == (0, 1)
        same(ing.wait(t0), want)
        same(ing.wait(t1), want_lin)
        ing.set_matrices(d.A, d.G, sing)  # clears the P
        with pytest.raises(S.SocpError) as ei:
            ing.submit(d.c, None, d.b, None, d.h, qp=True)
        assert ei.value.code == _lib.SOCP_E_INVALID
        t2 = ing.submit(d.c, None, d.b, None, d.h)
        assert t2 == 2
        same(ing.wait(t2), want_lin)
    finally:
        ing.close()


# ------------------------------------------------------------------------ MOI
def _model(prob, sense, const):
    """The model of one qp_cases problem (P, c, A, b, G, h) with s16's cones:
    the objective given as MOI gives it (upper triangle, one term per pair).
    sense = MAX_SENSE: the twin that maximises minus the objective."""
    Pm, c, A, b, G, h = prob
    n = len(c)
    f = -1.0 if sense == moi.MAX_SENSE else 1.0
    o = moi.Optimizer()
    x = o.add_variables(n)
    rows = lambda M, r0, r1: [(i - r0 + 1, x[j], -M[i, j]) for i in range(r0, r1) for j in range(n)]  # noqa: E731
    o.add_constraint(moi.vaf(rows(A, 0, len(b)), b), moi.Zeros(len(b)))
    o.add_constraint(moi.vaf(rows(G, 0, 8), h[:8]), moi.Nonnegatives(8))
    o.add_constraint(moi.vaf(rows(G, 8, 24), h[8:]), moi.SecondOrderCone(16))
    o.set_objective_sense(sense)
    o.set_objective_function(moi.sqf([(x[i], x[j], f * Pm[i, j]) for i in range(n) for j in range(i, n)],
                                     [(x[j], f * c[j]) for j in range(n)], f * const))
    return o, x


def test_moi_quadratic_objective():
    d = Q.batch("s16", 4)
    sh = d.shape
    n, m, k = sh.n, sh.m, sh.k
    const = 3.5
    mins = [_model(p, moi.MIN_SENSE, const) for p in d.probs]
    maxs = [_model(p, moi.MAX_SENSE, const) for p in d.probs]
    moi.optimize_batched([o for o, _ in mins])
    assert "_qp_" in S.default_context().last_kernel_name()
    moi.optimize_batched([o for o, _ in maxs])
    # the models' own data: P symmetrised from the upper triangle, everything else the batch's bits
    Ps = []
    for (o, _), prob in zip(mins, d.probs):
        Pm = np.triu(prob[0]) + np.triu(prob[0], 1).T
        assert np.array_equal(o.data.P, Pm) and np.array_equal(o.data.c, prob[1])
        assert np.array_equal(o.data.A, prob[2]) and np.array_equal(o.data.G, prob[4])
        Ps.append(Pm)
    sing = np.array([moi._sing(p[4]) for p in d.probs], np.uint8)
    want = S.batch_solve(list(sh.cones), n, m, k, d.c, d.A, d.b, d.G, d.h, sing,
                         P=np.concatenate([P.ravel(order="F") for P in Ps]))
    assert (want["status"] == S.CONVERGED).all()
    for i, ((o, x), (omax, xmax)) in enumerate(zip(mins, maxs)):
        xs = o.variable_primal(x)
        assert xs.tobytes() == want["x"][i * n:(i + 1) * n].tobytes()
        assert o.termination_status() == "OPTIMAL"
        c = d.probs[i][1]
        val = float(c @ xs + const) + 0.5 * float(xs @ (Ps[i] @ xs))
        assert o.objective_value() == val
        assert omax.variable_primal(xmax).tobytes() == xs.tobytes()
        assert omax.objective_value() == -val
