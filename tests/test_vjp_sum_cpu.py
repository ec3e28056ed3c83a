"""socp_batch_vjp_sum without a GPU: the ABI, the flag checks on a blank
context, the slab rule, the Python size checks, and that vjp_sum_cases' gate is
not vacuous -- a float64 sum passes it and three plausible mistakes do not.
"""
import ctypes as C
import re

import numpy as np
import pytest

import qp_cases as QC
import socp_amd as S
import vjp_sum_cases as VS
from socp_amd import _lib

NEW = ("socp_batch_vjp_sum", "socp_debug_vjp_sum_plan")


def test_declared_and_exported():
    txt = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    L = _lib.load()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert name in _lib.EXPORTED
        assert hasattr(L, name), name


# ------------------------------------------------------------------ flags
def _sum(ctx, flags):
    L = _lib.load()
    d = _lib.Dims(2, 3, 0, 4, 2)
    kind, offs, dim = np.array([0, 1], np.int32), np.array([0, 1], np.int32), np.array([1, 3], np.int32)
    return L.socp_batch_vjp_sum(ctx, C.byref(d), kind.ctypes.data, offs.ctypes.data, dim.ctypes.data,
                                *[None] * 13, flags, *[None] * 9, None)


@pytest.fixture()
def blank_ctx():
    """Zeroed memory in a context's place: the entry checks its flags before it
    touches the context, so these checks run without a device."""
    buf = C.create_string_buffer(1 << 16)
    return C.cast(buf, C.c_void_p)


def test_null_context():
    assert _sum(None, _lib.F_SHARED_MATRICES) == _lib.SOCP_E_INVALID
    assert b"ctx" in _lib.load().socp_last_error()


def test_flags(blank_ctx):
    L = _lib.load()
    sh = _lib.F_SHARED_MATRICES
    for flags in (0, _lib.F_DEVICE_PTRS, _lib.F_FORCE_LARGE):
        assert _sum(blank_ctx, flags) == _lib.SOCP_E_INVALID
        msg = L.socp_last_error()
        assert b"socp_batch_vjp_sum" in msg and b"SOCP_F_SHARED_MATRICES" in msg
    for flags in (_lib.F_EXPLICIT_INVERSE, sh | _lib.F_EXPLICIT_INVERSE):
        assert _sum(blank_ctx, flags) == _lib.SOCP_E_UNSUPPORTED
        assert b"socp_batch_vjp_sum" in L.socp_last_error()
    for bad in (_lib.F_WARM_START, _lib.F_DETECT_INFEASIBLE, _lib.F_EQUILIBRATE, 1 << 20):
        assert _sum(blank_ctx, sh | bad) == _lib.SOCP_E_INVALID
        assert b"socp_batch_vjp_sum" in L.socp_last_error()


# --------------------------------------------------------------- the slab rule
@pytest.mark.parametrize("shape", [(8, 2, 16), (64, 16, 96), (16, 4, 1200)], ids=["s8", "c2", "gv"])
def test_plan(shape):
    for B in (1, 3, 4, 5, 1000, 65536):
        slabs, slab = S.vjp_sum_plan(B, *shape)
        assert slabs * slab >= B and (slabs - 1) * slab < B and slab >= 4, (B, slabs, slab)
        assert S.vjp_sum_plan(B, *shape) == (slabs, slab)
    # the partial sums stay below the cap by growing the slab, and only then
    slabs, slab = S.vjp_sum_plan(10 ** 7, *shape)
    n, m, k = shape
    assert slabs == 1 or slabs * (k + m + n) * n * 8 <= 64 << 20
    assert slab == 512 or 2 * slabs * (k + m + n) * n * 8 > 64 << 20


def test_plan_rejects_bad_dims():
    L = _lib.load()
    a, b = C.c_int64(), C.c_int64()
    for d in (_lib.Dims(0, 8, 2, 16, 0), _lib.Dims(4, 0, 2, 16, 0), _lib.Dims(4, 8, -1, 16, 0)):
        assert L.socp_debug_vjp_sum_plan(C.byref(d), C.byref(a), C.byref(b)) == _lib.SOCP_E_INVALID
    assert L.socp_debug_vjp_sum_plan(None, C.byref(a), C.byref(b)) == _lib.SOCP_E_INVALID


# ---------------------------------------------------------- the gate has teeth
@pytest.mark.parametrize("name", ["s8", "m0", "c1", "blk", "gv"])
def test_gate_is_not_vacuous(name):
    """Synthetic standard-normal ux .. x of the GPU tests' shapes, B = 8.  The
    float64 numpy sums pass the gate; the sums without the last problem, dA
    with i and j swapped, and dG with uz in w's place do not."""
    cones, n, m, k, _ = QC.SHAPES[name]
    B = 8
    rng = np.random.default_rng([n, m, k, 9])
    v = {key: rng.standard_normal((B, q)) for key, q in
         (("x", n), ("y", m), ("z", k), ("gs", k), ("ux", n), ("uy", m), ("uz", k))}
    status = np.zeros(B, np.int32)
    ref = VS.sum_reference(v["x"], v["y"], v["z"], v["gs"], v["ux"], v["uy"], v["uz"], status)
    assert set(ref) == ({"dG", "dP"} | ({"dA"} if m else set()))

    def f64(upto=B, w_is_uz=False, swap_dA=False):
        x, y, z, ux, uy, uz = [v[key][:upto] for key in ("x", "y", "z", "ux", "uy", "uz")]
        w = uz if w_is_uz else uz + v["gs"][:upto]
        M = ux.T @ x
        out = dict(dG=VS.col(-(z.T @ ux + w.T @ x)), dP=VS.col(-(M + M.T) / 2))
        if m:
            dA = -(y.T @ ux + uy.T @ x)
            out["dA"] = np.ascontiguousarray(dA.ravel()) if swap_dA else VS.col(dA)
        return out

    def ratios(got):
        return {key: VS.worst(got[key], *ref[key], B) for key in ref}

    good = ratios(f64())
    print(name, "float64 sums, worst |err| / gate:", good)
    assert max(good.values()) <= 1.0
    short = ratios(f64(upto=B - 1))
    assert min(short.values()) > 1.0, short
    assert ratios(f64(w_is_uz=True))["dG"] > 1.0
    if m:
        assert ratios(f64(swap_dA=True))["dA"] > 1.0


# ------------------------------------------------------------- Python checks
def test_python_size_checks():
    sh = QC.shared_batch("s8", 2)
    cones, n, m, k, _ = sh.shape
    x, y, z, s = np.zeros(2 * n), np.zeros(2 * m), np.ones(2 * k), np.ones(2 * k)
    call = lambda **kw: S.batch_vjp(list(cones), n, m, k, sh.A, sh.G, None, x, y, z, s, P=sh.P,  # noqa: E731
                                    shared_matrices=True, **kw)
    with pytest.raises(ValueError, match="dG: "):
        call(want=["dG"], out=dict(dG=np.zeros(2 * k * n)))
    with pytest.raises(ValueError, match="dA: "):
        call(want=["dA"], out=dict(dA=np.zeros(2 * m * n)))
    with pytest.raises(ValueError, match="dP: "):
        call(want=["dP"], out=dict(dP=np.zeros(n * n + 1)))
    with pytest.raises(ValueError, match="G: "):
        S.batch_vjp(list(cones), n, m, k, sh.A, np.tile(sh.G, 2), None, x, y, z, s, shared_matrices=True,
                    want=["dG"])
