"""SOCP_F_SHARED_MATRICES without a GPU: the flag's value, the host-side size
checks of a shared call, the equality check of solve_socp_batched, and the
C ABI's argument checking with the flag set."""
import ctypes as C
import re

import numpy as np
import pytest

import socp_amd as S
from socp_amd import _lib
from socp_amd.configs import C1
from shared_cases import SHAPES, make


def test_flag_value_matches_header():
    assert _lib.F_SHARED_MATRICES == 512 and S.F_SHARED_MATRICES == 512
    txt = open(_lib.HEADER).read()
    m = re.search(r"^#define\s+SOCP_F_SHARED_MATRICES\s+(\d+)\s*$", txt, flags=re.M)
    assert m and int(m.group(1)) == _lib.F_SHARED_MATRICES
    assert "socp_ingest_set_matrices" in _lib.EXPORTED
    assert hasattr(C.CDLL(_lib.LIB_PATH), "socp_ingest_set_matrices")


def test_shared_host_arrays_are_size_checked():
    cfg = C1
    B, n, m, k = 3, cfg.n, cfg.m, cfg.k
    c, b, h = np.zeros(B * n), np.zeros(B * m), np.zeros(B * k)
    A, G = np.zeros(m * n), np.zeros(k * n)
    call = lambda A_, G_, sing=None: S.batch_solve(cfg.cones, n, m, k, c, A_, b, G_, h, sing,  # noqa: E731
                                                  shared_matrices=True)
    with pytest.raises(ValueError, match="A"):
        call(np.zeros(B * m * n), G)  # the replicated form under the flag
    for d in (-1, 1):
        with pytest.raises(ValueError, match="G"):
            call(A, np.zeros(k * n + d))
    with pytest.raises(ValueError, match="sing"):
        call(A, G, np.zeros(B, np.uint8))
    # the same checks guard the plugin entries, the handles and the ingest's matrices
    z = np.zeros(B * k)
    with pytest.raises(ValueError, match="G"):
        S.batch_kkt_solve(cfg.cones, n, m, k, A, np.zeros(B * k * n), None, z, z, np.zeros(B * n), np.zeros(B * m),
                          z, z, shared_matrices=True)
    with pytest.raises(ValueError, match="A"):
        S.DenseHandle(cfg.cones, n, m, k, np.zeros(B * m * n), G, shared_matrices=True, batch=B)
    with pytest.raises(ValueError, match="sing"):
        S.SqrHandle(cfg.cones, n, m, k, A, G, np.zeros(B, np.uint8), shared_matrices=True, batch=B)
    with pytest.raises(ValueError, match="batch"):
        S.DenseHandle(cfg.cones, n, m, k, A, G, shared_matrices=True)


def problems_of(d):
    cones, n, m, k = d.shape
    cl = [S.POC(o, q) if kind == 0 else S.SOC(o, q) for kind, o, q in cones]
    A = d.A.reshape(n, m).T
    G = d.G.reshape(n, k).T
    return [S.Problem(d.c[p * n:(p + 1) * n], A.copy(), d.b[p * m:(p + 1) * m], G.copy(), d.h[p * k:(p + 1) * k], cl)
            for p in range(d.B)]


def test_solve_socp_batched_rejects_unequal_matrices():
    probs = problems_of(make("c1", 3, 1))
    probs[1].G[5, 7] += 1e-9  # one entry of the second problem's G
    with pytest.raises(ValueError, match="problem 1's G"):
        S.solve_socp_batched(probs, shared_matrices=True)
    probs = problems_of(make("c1", 3, 1))
    probs[2].A[0, 0] = np.nextafter(probs[2].A[0, 0], 1.0)
    with pytest.raises(ValueError, match="problem 2's A"):
        S.solve_socp_batched(probs, solver="sqr", shared_matrices=True)


def test_null_context_with_the_flag_is_an_api_error():
    L = _lib.load()
    d = _lib.Dims(4, 3, 0, 4, 2)
    P = _lib.default_params(flags=_lib.F_SHARED_MATRICES)
    rc = L.socp_batch_solve(None, C.byref(d), None, None, None, None, None, None, None, None, None, P,
                            None, None, None, None, None, None)
    assert rc == _lib.SOCP_E_INVALID
    assert b"ctx" in L.socp_last_error()
    rc = L.socp_batch_kkt_solve(None, C.byref(d), *[None] * 17,_lib.F_SHARED_MATRICES)
    assert rc == _lib.SOCP_E_INVALID
    out = C.c_void_p()
    for create in (L.socp_dense_create, L.socp_sqr_create):
        assert create(None, C.byref(d), None, None, None, None, None, None, _lib.F_SHARED_MATRICES,
                      C.byref(out)) == _lib.SOCP_E_INVALID
    assert L.socp_ingest_create(None, C.byref(d), None, None, None, _lib.F_SHARED_MATRICES,
                                C.byref(out)) == _lib.SOCP_E_INVALID
    assert L.socp_ingest_set_matrices(None, None, None, None) == _lib.SOCP_E_INVALID


def test_shared_cases_are_strictly_feasible():
    d = make("c2", 4, 3)
    cones, n, m, k = d.shape
    assert d.A.size == m * n and d.G.size == k * n and d.c.size == 4 * n
    assert not np.array_equal(d.c[:n], d.c[n:2 * n])
    assert set(SHAPES) >= {"c1", "c2", "mq2", "m0", "sing", "wide"}
