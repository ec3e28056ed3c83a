"""Differentiable solves without a GPU: the formulas of socp_batch_vjp against
finite differences, the centring table of DESIGN.md §24, and the argument
checks of the two entries and their Python calls.  References: vjp_cases.py.

Measured here (the numpy / oracle restatement, fp64 with np.longdouble
residuals): the formulas' worst relative distance from central differences
2.2e-8; the table's j = 4 column at most 1.1e-4, its j = 0 column at least
0.39 per shape.
"""
import ctypes as C

import numpy as np
import pytest

import qp_cases as QC
import socp_amd as S
import vjp_cases as V
from socp_amd import _lib

EPS = 1e-6
FD_GATE = 1e-6


def _perturbed(prob, i, D, t):
    q = list(prob)
    q[i] = q[i] + t * D
    return tuple(q)


@pytest.mark.parametrize("name", ["s8", "m0", "s16"])
def test_formulas_match_central_differences(name):
    """vjp_reference at exact_centre(mu = 1e-3) against central differences of
    that centre, eps = 1e-6, in a random direction of each of c, b, h, P
    (symmetrised), A and G, with all of gx, gy, gz, gs nonzero.  Gate: relative
    1e-6 (the difference quotient's own rounding is about 1e-7 at this eps)."""
    d = QC.batch(name, 4)
    cones, n, m, k, sing = d.shape
    g = V.upstream(name, 4)
    rng = np.random.default_rng([n, m, k, 3])
    for p in range(2):
        prob = d.probs[p]
        r = QC.qp_reference(cones, prob, bool(sing), tol=1e-5)
        assert r["status"] == 0
        base, res = V.exact_centre(cones, prob, r["x"], r["y"], r["z"], r["s"], 1e-3)
        assert res <= 1e-13
        gp = [v[p] for v in g]
        assert all(np.linalg.norm(v) > 0 for v in gp if v.size)
        ref = V.vjp_reference(cones, prob, *base, *gp)
        loss = lambda pt: sum(float(a @ b) for a, b in zip(gp, pt))  # noqa: E731
        # prob = (P, c, A, b, G, h)
        for i, key in ((1, "dc"), (3, "db"), (5, "dh"), (0, "dP"), (2, "dA"), (4, "dG")):
            if prob[i].size == 0:
                continue
            D = rng.standard_normal(prob[i].shape)
            if key == "dP":
                D = (D + D.T) / 2.0
            pts = []
            for t in (EPS, -EPS):
                pt, res = V.exact_centre(cones, _perturbed(prob, i, D, t), *base, 1e-3)
                assert res <= 1e-13
                pts.append(pt)
            fd = (loss(pts[0]) - loss(pts[1])) / (2.0 * EPS)
            an = float(np.sum(ref[key] * D))
            rel = abs(fd - an) / abs(an)
            print(f"{name} p{p} {key}: fd {fd:.12e} formula {an:.12e} rel {rel:.2e}")
            assert rel <= FD_GATE, (name, p, key, rel)


@pytest.mark.parametrize("name", V.TABLE_SHAPES)
def test_centring_table(name):
    """The gradient error against true_gradient after j = 0 .. 4 reference
    centring steps from qp_reference(tol = 1e-5)'s iterate, 8 problems with P
    (DESIGN.md §24's table; tools/vjp_table.py records it).  What the choice of
    inputs guarantees: every problem converges, the uncentred iterate is wrong
    by more than 1e-1 on the worst problem of the shape, and after four steps
    every problem is below 1e-3."""
    rows = V.table(name)
    assert all(r["status"] == 0 for r in rows)
    assert all(r["path_res"] <= 1e-13 for r in rows)
    assert all(len(r["pts"]) == V.STEPS + 1 for r in rows)
    worst = [max(r["err"][j] for r in rows) for j in range(V.STEPS + 1)]
    print(name, "worst gradient error by centring steps:", " ".join(f"{w:.1e}" for w in worst))
    print(name, "worst off-centre measure:", " ".join(f"{max(r['off'][j] for r in rows):.1e}"
                                                      for j in range(V.STEPS + 1)))
    assert worst[0] > 1e-1
    assert all(r["err"][V.STEPS] < 1e-3 for r in rows), [r["err"][V.STEPS] for r in rows]
    # the centring keeps the complementarity level: z's moves by the residuals' share only
    for r in rows:
        g0 = float(r["pts"][0][2] @ r["pts"][0][3])
        g4 = float(r["pts"][-1][2] @ r["pts"][-1][3])
        assert g0 / 2.0 <= g4 <= 2.0 * g0


# ------------------------------------------------------------------ the ABI
def _dims_and_cones():
    d = _lib.Dims(2, 3, 0, 4, 2)
    kind = np.array([0, 1], np.int32)
    offs = np.array([0, 1], np.int32)
    dim = np.array([1, 3], np.int32)
    return d, kind, offs, dim


def _centre(ctx, steps, flags):
    L = _lib.load()
    d, kind, offs, dim = _dims_and_cones()
    return L.socp_batch_centre(ctx, C.byref(d), kind.ctypes.data, offs.ctypes.data, dim.ctypes.data,
                               *[None] * 7, steps, flags, *[None] * 6)


def _vjp(ctx, flags, dG=None):
    L = _lib.load()
    d, kind, offs, dim = _dims_and_cones()
    outs = [None] * 9
    outs[5] = dG
    return L.socp_batch_vjp(ctx, C.byref(d), kind.ctypes.data, offs.ctypes.data, dim.ctypes.data,
                            *[None] * 13, flags, *outs, None)


@pytest.fixture()
def blank_ctx():
    """Zeroed memory in a context's place: both entries check steps and flags
    before they touch the context, so these checks run without a device."""
    buf = C.create_string_buffer(1 << 16)
    return C.cast(buf, C.c_void_p)


def test_null_context():
    L = _lib.load()
    assert _centre(None, 4, 0) == _lib.SOCP_E_INVALID and b"ctx" in L.socp_last_error()
    assert _vjp(None, 0) == _lib.SOCP_E_INVALID and b"ctx" in L.socp_last_error()


def test_steps_out_of_range(blank_ctx):
    L = _lib.load()
    for steps in (-1, 17):
        assert _centre(blank_ctx, steps, 0) == _lib.SOCP_E_INVALID
        assert b"steps" in L.socp_last_error()


def test_flags(blank_ctx):
    L = _lib.load()
    assert _centre(blank_ctx, 4, _lib.F_EXPLICIT_INVERSE) == _lib.SOCP_E_UNSUPPORTED
    assert b"socp_batch_centre" in L.socp_last_error()
    assert _vjp(blank_ctx, _lib.F_EXPLICIT_INVERSE) == _lib.SOCP_E_UNSUPPORTED
    assert b"socp_batch_vjp" in L.socp_last_error()
    for bad in (_lib.F_WARM_START, _lib.F_DETECT_INFEASIBLE, _lib.F_EQUILIBRATE, 1 << 20):
        assert _centre(blank_ctx, 4, bad) == _lib.SOCP_E_INVALID
        assert _vjp(blank_ctx, bad) == _lib.SOCP_E_INVALID


def test_shared_matrix_gradients_are_unsupported(blank_ctx):
    L = _lib.load()
    dG = np.zeros(2 * 4 * 3)
    assert _vjp(blank_ctx, _lib.F_SHARED_MATRICES, dG=dG.ctypes.data) == _lib.SOCP_E_UNSUPPORTED
    assert b"SOCP_F_SHARED_MATRICES" in L.socp_last_error()


def test_python_size_checks():
    d = QC.batch("s8", 2)
    cones, n, m, k, _ = d.shape
    x, y, z, s = np.zeros(2 * n), np.zeros(2 * m), np.ones(2 * k), np.ones(2 * k)
    with pytest.raises(ValueError, match="multiple of n"):
        S.batch_centre(cones, n, m, k, d.c, d.A, d.b, d.G, d.h, d.sing, x[:-1], y, z, s)
    with pytest.raises(ValueError, match="h: "):
        S.batch_centre(cones, n, m, k, d.c, d.A, d.b, d.G, d.h[:-1], d.sing, x, y, z, s)
    with pytest.raises(ValueError, match="z: "):
        S.batch_centre(cones, n, m, k, d.c, d.A, d.b, d.G, d.h, d.sing, x, y, z[:-1], s)
    with pytest.raises(ValueError, match="gs: "):
        S.batch_vjp(cones, n, m, k, d.A, d.G, d.sing, x, y, z, s, gs=np.zeros(3))
    with pytest.raises(ValueError, match="G: "):
        S.batch_vjp(cones, n, m, k, d.A, d.G[:-1], d.sing, x, y, z, s)
    with pytest.raises(ValueError, match="skip: "):
        S.batch_vjp(cones, n, m, k, d.A, d.G, d.sing, x, y, z, s, skip=np.zeros(3, np.int32))
    with pytest.raises(ValueError, match="unknown output"):
        S.batch_vjp(cones, n, m, k, d.A, d.G, d.sing, x, y, z, s, want=["dQ"])
    with pytest.raises(ValueError, match="needs c, b and h"):
        S.batch_vjp(cones, n, m, k, d.A, d.G, d.sing, x, y, z, s, centre_steps=2)
    with pytest.raises(ValueError, match="symmetric"):
        S.batch_vjp(cones, n, m, k, d.A, d.G, d.sing, x, y, z, s, P=np.arange(2.0 * n * n))


def test_torch_layer_imports_without_a_gpu():
    import socp_amd.torch_layer as T
    layer = T.SocpLayer(QC.SHAPES["s8"].cones, 8, 2, 16, centre_steps=3, maxit=30)
    assert layer.cfg.centre_steps == 3 and layer.cfg.solve_options == dict(maxit=30)
    assert issubclass(T.SocpFunction, __import__("torch").autograd.Function)
