"""Quadratic objectives without a device: the numpy restatement the GPU tests
compare against (tests/qp_cases.py) is pinned to the CPU oracle at P = 0, it
converges on the GPU tests' batches, and the entry's host-side checks fire."""
import ctypes as C

import numpy as np
import pytest

import qp_cases as Q
import socp_amd as S
from socp_amd import _lib


# (8,2,16), (10,4,8) with sing = 1, (32,8,48), (64,16,96)
@pytest.mark.parametrize("name", ["s8", "sing", "c1", "c2"])
def test_restatement_equals_oracle_at_zero_P(oracle, name):
    """Iterates 0..2 against oracle.solve_trace in the kernels' order: rel <=
    1e-11, 30 x the 3.1e-13 measured when the restatement was written."""
    d = Q.batch(name, 4, True)
    cones = d.shape.cones
    worst = 0.0
    for prob in d.probs:
        Pm, c, A, b, G, h = prob
        assert not Pm.any()
        r = Q.qp_reference(cones, prob, bool(d.shape.sing), maxit=3, tol=0.0)
        o = oracle.solve_trace(cones, c, A, b, G, h, sing=bool(d.shape.sing),
                               params=oracle.Params(maxit=3, tol=0.0, flags=oracle.F_STRUCTURED | oracle.F_CHOLSOLVE))
        assert r["status"] == o["status"] == 1
        for t in range(3):
            for u, v in zip(r["trace"][t], o["trace"][t]):
                if len(v):
                    worst = max(worst, np.linalg.norm(u - v) / np.linalg.norm(v))
    print(f"{name}: worst rel {worst:.2e}")
    assert worst <= 1e-11


@pytest.mark.parametrize("name", Q.RULE_SHAPES)
def test_restatement_converges_on_the_gpu_batches(oracle, name):
    """Status 0 on every problem of the batches the GPU tests run under the
    reference rule; at least 3/4 of each batch exits at an iteration that
    rounding does not decide."""
    rs = Q.reference(name)
    st = np.array([r["status"] for r in rs])
    it = np.array([r["iters"] for r in rs])
    ncl = sum(Q.clear(r) for r in rs)
    print(f"{name}: iterations {it.min()}..{it.max()}, clear {ncl}/{len(rs)}")
    assert (st == 0).all(), st
    assert 4 * ncl >= 3 * len(rs)
    d = Q.batch(name)
    for r, prob in zip(rs, d.probs):
        Pm, c, A, b, G, h = prob
        assert np.linalg.norm(G @ r["x"] + r["s"] - h) / (1.0 + np.linalg.norm(h)) <= 1e-7


@pytest.mark.parametrize("name", [nm for nm in Q.SHAPES if nm != "gv"])  # (gv: checked where it runs, on 8 problems)
def test_trajectory_batches_are_well_conditioned(oracle, name):
    """kappa_2(H) <= 1e5 at every factorisation through iteration 2 (the
    initial point's and three iterations'): what the GPU trajectory gate of
    1e-8 assumes (gate P4 of DESIGN section 7).  The singular shape (k < n: H
    leans on P and A'A) reaches 2e5 - 9e6 at iteration 2 on every seed tried;
    it is held to 1e7, where kappa 2^-53 is still a decade under the gate."""
    rs = Q.reference(name, 3, 0.0)
    assert all(r["status"] == 1 and r["iters"] == 3 for r in rs)
    kap = max(max(r["kappa"]) for r in rs)
    print(f"{name}: kappa_2(H) <= {kap:.2e}")
    assert kap <= (1e7 if name.startswith("sing") else 1e5)


def test_symbol_and_null_ctx():
    L = _lib.load()
    assert "socp_batch_solve_qp" in _lib.EXPORTED
    fn = L.socp_batch_solve_qp
    dims = _lib.Dims(1, 2, 0, 2, 1)
    rc = fn(None, dims, *([None] * 18))
    assert rc == _lib.SOCP_E_INVALID
    assert b"ctx" in L.socp_last_error()


def test_wrapper_checks_P():
    cones, n, k = [S.POC(0, 2)], 2, 2
    c, G, h = np.zeros(n), np.eye(2).ravel(), np.ones(k)
    with pytest.raises(ValueError, match="P"):
        S.batch_solve(cones, n, 0, k, c, None, None, G, h, P=np.zeros(3))
    with pytest.raises(ValueError, match="P.*symmetric"):
        S.batch_solve(cones, n, 0, k, c, None, None, G, h, P=np.array([1.0, 0.5, 0.0, 1.0]))
    with pytest.raises(ValueError, match="P"):  # shared: ONE matrix
        S.batch_solve(cones, n, 0, k, np.zeros(2 * n), None, None, G, np.ones(2 * k), P=np.zeros(2 * n * n),
                      shared_matrices=True)


def test_wrapper_wants_P_on_the_side_of_G():
    import torch
    cones, n, k = [S.POC(0, 2)], 2, 2
    c, G, h = np.zeros(n), np.eye(2).ravel(), np.ones(k)
    with pytest.raises(ValueError, match="P must be on the same side as G"):
        S.batch_solve(cones, n, 0, k, c, None, None, G, h, P=torch.eye(2, dtype=torch.float64).reshape(-1))
    with pytest.raises(ValueError, match="P must be on the same side as G"):  # wrong dtype beside a tensor G
        S.batch_solve(cones, n, 0, k, torch.from_numpy(c), None, None, torch.from_numpy(G), torch.from_numpy(h),
                      P=torch.eye(2, dtype=torch.float32).reshape(-1))


def test_problem_asserts_P_shape():
    args = (np.zeros(2), np.zeros((0, 2)), np.zeros(0), np.eye(2), np.ones(2), [S.POC(0, 2)])
    assert S.Problem(*args).P is None
    assert S.Problem(*args, P=np.eye(2)).P.shape == (2, 2)
    with pytest.raises(AssertionError):
        S.Problem(*args, P=np.eye(3))
