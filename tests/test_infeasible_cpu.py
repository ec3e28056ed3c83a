"""Infeasibility detection without a GPU: the ABI surface, the host tables, the
problem builder and the restated rule on the CPU oracle's traces."""
import ctypes as C
import re

import numpy as np
import pytest

import socp_amd as S
from socp_amd import _lib
from socp_amd import moi as M
import infeasible as I

CONES = [(0, 0, 6), (1, 6, 5), (1, 11, 5)]


def _header_defines():
    txt = open(_lib.HEADER).read()
    return {k: int(v) for k, v in re.findall(r"#define (SOCP_[A-Z_]+) \(?(-?\d+)\)?", txt)}


def test_constants_match_the_header():
    d = _header_defines()
    assert d["SOCP_F_DETECT_INFEASIBLE"] == 256 == _lib.F_DETECT_INFEASIBLE
    assert d["SOCP_PRIMAL_INFEASIBLE"] == 5 == S.PRIMAL_INFEASIBLE == I.ST_PRIMAL_INF
    assert d["SOCP_DUAL_INFEASIBLE"] == 6 == S.DUAL_INFEASIBLE == I.ST_DUAL_INF
    # the oracle's own flags keep bits 16..128
    import oracle as O
    for f in (O.F_STRUCTURED, O.F_SQR, O.F_CHOLSOLVE, O.F_INV_YTY):
        assert not f & _lib.F_DETECT_INFEASIBLE


def test_status_names_and_moi_tables():
    assert S.STATUS_NAMES[S.PRIMAL_INFEASIBLE] == "primal infeasible"
    assert S.STATUS_NAMES[S.DUAL_INFEASIBLE] == "dual infeasible"
    assert sorted(S.STATUS_NAMES) == list(range(7))
    assert M.TERMINATION[S.PRIMAL_INFEASIBLE] == "INFEASIBLE"
    assert M.TERMINATION[S.DUAL_INFEASIBLE] == "DUAL_INFEASIBLE"
    assert (M.PRIMAL_STATUS[S.PRIMAL_INFEASIBLE], M.DUAL_STATUS[S.PRIMAL_INFEASIBLE]) == (
        "NO_SOLUTION", "INFEASIBILITY_CERTIFICATE")
    assert (M.PRIMAL_STATUS[S.DUAL_INFEASIBLE], M.DUAL_STATUS[S.DUAL_INFEASIBLE]) == (
        "INFEASIBILITY_CERTIFICATE", "NO_SOLUTION")
    assert (M.PRIMAL_STATUS[S.CONVERGED], M.DUAL_STATUS[S.CONVERGED]) == ("FEASIBLE_POINT", "FEASIBLE_POINT")
    assert set(M.PRIMAL_STATUS) == set(M.DUAL_STATUS) == set(M.TERMINATION) == set(S.STATUS_NAMES)
    o = M.Optimizer()
    assert o.primal_status() == o.dual_status() == "NO_SOLUTION"


def test_setter_is_exported():
    L = C.CDLL(_lib.LIB_PATH)
    assert hasattr(L, "socp_ctx_set_infeasibility_tol")
    assert "socp_ctx_set_infeasibility_tol" in _lib.EXPORTED
    # a NULL context is an API error, not a crash
    L.socp_ctx_set_infeasibility_tol.argtypes = [C.c_void_p, C.c_double]
    assert L.socp_ctx_set_infeasibility_tol(None, 1e-7) == _lib.SOCP_E_INVALID


def test_keywords_exist():
    import inspect
    for fn in (S.batch_solve, S.SqrHandle.solve_socp, S.Ingest.submit, S.Ingest.submit_csc, S.solve_socp_batched):
        assert inspect.signature(fn).parameters["detect_infeasible"].default is False, fn
    assert callable(S.Context.set_infeasibility_tol)


@pytest.mark.parametrize("n,m,k", [(8, 2, 16), (8, 0, 16)])
def test_builder_certificates_are_exact(n, m, k):
    flat, kinds, probs, certs = I.make_batch(CONES, n, m, k, per_kind=4, seed=3)
    assert list(kinds) == [0, 1, 2] * 4
    assert flat["G"].size == 12 * k * n and flat["A"].size == 12 * m * n
    for kind, (c, A, b, G, h), cert in zip(kinds, probs, certs):
        scale = np.linalg.norm(G)
        if kind == I.PRIMAL_INF:
            y, z = cert
            assert np.linalg.norm(A.T @ y + G.T @ z) < 1e-12 * scale and abs(b @ y + h @ z + 1) < 1e-12 * scale
            assert I.in_cone(CONES, z)
            assert I.certificate_ratios((c, A, b, G, h), np.zeros(n), y, z, np.zeros(k))[0] < 1e-12 * scale
        elif kind == I.DUAL_INF:
            xd, s = cert
            assert np.linalg.norm(A @ xd) < 1e-12 * scale and np.linalg.norm(G @ xd + s) < 1e-12 * scale
            assert abs(c @ xd + 1) < 1e-12 * scale and I.in_cone(CONES, s)
        else:
            assert cert is None


@pytest.mark.parametrize("order", ["kernel", "sqr"])
@pytest.mark.parametrize("n,m,k", [(8, 2, 16), (8, 0, 16)])
def test_restated_rule_on_oracle_traces(oracle, order, n, m, k):
    """The rule fires, with the right kind, on every infeasible problem of the
    builder and never on a feasible one (which converges first)."""
    O = oracle
    flags = (O.F_STRUCTURED | O.F_CHOLSOLVE) if order == "kernel" else O.F_SQR
    flat, kinds, probs, _ = I.make_batch(CONES, n, m, k, per_kind=8, seed=11)
    for kind, prob in zip(kinds, probs):
        c, A, b, G, h = prob
        r = O.solve_trace(CONES, c, A, b, G, h, sing=False, params=O.Params(flags=flags))
        st, it, ratios = I.rule_fire(prob, r)
        if kind == I.FEASIBLE:
            assert st is None and r["status"] == 0
            assert min(min(q) for q in ratios) > 1e3 * I.TAU
        else:
            assert st == (I.ST_PRIMAL_INF if kind == I.PRIMAL_INF else I.ST_DUAL_INF), (kind, r["status"], r["iters"])
            assert 0 < it <= r["iters"]
            x, y, z, s = r["trace"][it]
            assert I.in_cone(CONES, z) and I.in_cone(CONES, s)
