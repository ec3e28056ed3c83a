"""The QP plugin entries -- socp_batch_kkt_solve_qp (MODE_KKT) and
socp_dense_create_qp + socp_dense_setup_iter / socp_dense_solve_kkt
(MODE_SETUP, MODE_SOLVEKKT) -- on the register kernel's KM = 9 instantiations
and the blocked QP kernels, against the refined block system with P of
qp_kkt_cases.py.  tests/test_qp_kkt_cases_cpu.py holds the preconditions: the
table, the kernel each case must select, the restatement pinned to the oracle
at P = 0, the refinement's convergence.

The gate, per vector cx, cy, cz, cs (empty ones skipped), with
e = ||got - ref||_2 / ||ref||_2:

    e <= max(10 e_rs, (n + m + 2k) 2^-53)

e_rs the same error of the numpy restatement (qp_cases._Factor) on the same
inputs.  No measurement of a kernel enters it.

  gate      fused entry and handle (setup once, a solve per right-hand side)
            at every shape, status 0, the QP kernel's name;
  bits      the handle equals the fused entry bitwise, and a second solve_kkt
            the first;
  null      P == NULL through both new entries: the linear entries' bytes and
            kernel name; an all-zero P: the linear entries' values;
  used      at (32, 8, 48) the result with P is more than 100 gates from the
            result without;
  shared    SOCP_F_SHARED_MATRICES with one P: the replicated call's bits, on a
            register and a blocked shape;
  isolated  P = -10 I on one problem of four: SOCP_CHOL_H_FAILED and NaN for it
            alone, the neighbours' bits unchanged;
  refused   SOCP_F_EXPLICIT_INVERSE with a P: -2, the entry named;
  plugin    DenseSolver(Problem(..., P=P)) through compute_scaling /
            setup_iter / solve_kkt equals batch_kkt_solve(P=P) bitwise.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import kkt_cases as KC
import qp_kkt_cases as QK
import socp_amd as S
from socp_amd import _lib

pytestmark = pytest.mark.gpu

OUT = KC.KEYS + ("status",)


def kernel_is(name, ctx=None):
    got = (ctx or S.default_context()).last_kernel_name()
    assert got == name, (got, name)


def same(a, b, keys=OUT):
    for key in keys:
        u, v = np.asarray(a[key]), np.asarray(b[key])
        assert u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes(), key


def vectors(out, p, n, m, k):
    return [out[key][p * q:(p + 1) * q] for key, q in zip(KC.KEYS, (n, m, k, k))]


def check_gate(tag, case, out, j):
    n, m, k = case.n, case.m, case.k
    assert (out["status"] == 0).all(), out["status"]
    worst = 0.0
    for p in range(QK.B):
        e = KC.rel_errors(vectors(out, p, n, m, k), QK.reference(case, p).sol[j])
        for key, ev, gv in zip(KC.KEYS, e, QK.gates(case, p, j)):
            if ev is None:
                continue
            print(f"  {tag} {case.id} p={p} rhs {j} {key}: e = {ev:.3g}, gate {gv:.3g}")
            worst = max(worst, ev / gv)
    print(f"{tag} {case.id} on {case.kernel}: worst error / gate {worst:.3g}")
    assert worst <= 1.0, (case.id, j, worst)


def fused(case, d, j, P="case", nb=None, **kw):
    nb = len(d["G"]) if nb is None else nb
    Af, Gf = KC.flat(d, nb)
    kw.setdefault("sing", QK.sing_bytes(case, nb))
    sl = slice(0, nb)
    dx, dy, dz, ds = d["rhs"][j]
    return S.batch_kkt_solve(list(case.cones), case.n, case.m, case.k, Af, Gf, kw.pop("sing"),
                             d["s"][sl].ravel(), d["z"][sl].ravel(), dx[sl].ravel(),
                             dy[sl].ravel() if case.m else None, dz[sl].ravel(), ds[sl].ravel(),
                             force_large=case.force_large, P=QK.flat_P(d, nb) if isinstance(P, str) else P, **kw)


def handle(case, d, P="case", **kw):
    Af, Gf = KC.flat(d)
    kw.setdefault("sing", QK.sing_bytes(case, len(d["G"])))
    return S.DenseHandle(list(case.cones), case.n, case.m, case.k, Af, Gf, kw.pop("sing"),
                         force_large=case.force_large, P=QK.flat_P(d) if isinstance(P, str) else P, **kw)


@functools.lru_cache(maxsize=None)
def fused_once(case, j):
    out = fused(case, QK.inputs(case), j)
    kernel_is(case.kernel)
    return out


# ------------------------------------------------------- 1. the gate, 2. bits
@pytest.mark.parametrize("case", QK.CASES, ids=QK.case_id)
def test_fused(case):
    check_gate("fused", case, fused_once(case, 0), 0)


@pytest.mark.parametrize("case", QK.CASES, ids=QK.case_id)
def test_handle(case):
    n, m, k = case.n, case.m, case.k
    d = QK.inputs(case)
    h = handle(case, d)
    try:
        # A, G, sing and P move once, at create
        assert h.h2d_bytes == QK.B * ((m * n + k * n + n * n) * 8 + 1)
        st = h.setup_iter(d["s"].ravel(), d["z"].ravel())
        kernel_is(case.kernel)
        assert (st == 0).all(), st
        assert h.h2d_bytes == QK.B * 2 * k * 8
        first = None
        for j in range(QK.NRHS):
            got = h.solve_kkt(*KC.flat_rhs(d, j, m))
            kernel_is(case.kernel)
            assert h.h2d_bytes == QK.B * (n + m + 2 * k) * 8
            check_gate("handle", case, got, j)
            same(got, fused_once(case, j))
            first = first or got
        same(h.solve_kkt(*KC.flat_rhs(d, 0, m)), first)  # the record is read, not consumed
    finally:
        h.close()


# ---------------------------------------------------- 3. P == NULL and zero P
class RawQpHandle(S.DenseHandle):
    """socp_dense_create_qp called directly, so that P may be NULL."""

    def __init__(self, case, d, P):
        self.cones, self.n, self.m, self.k = list(case.cones), case.n, case.m, case.k
        self.kind, self.offs, self.dim = S.cone_arrays(self.cones)
        self.B, self.dev, self.shared_matrices, self.ctx = len(d["G"]), False, False, S.default_context()
        Af, Gf = KC.flat(d)
        p = _lib.ptr
        h = C.c_void_p()
        _lib.check(_lib.load().socp_dense_create_qp(
            self.ctx.handle, _lib.Dims(self.B, case.n, case.m, case.k, len(self.kind)), p(self.kind), p(self.offs),
            p(self.dim), p(P), p(Af), p(Gf), p(QK.sing_bytes(case, self.B)),
            S.F_FORCE_LARGE if case.force_large else 0, C.byref(h)))
        self.handle = h


def raw_fused(case, d, j, P):
    """socp_batch_kkt_solve_qp called directly, so that P may be NULL."""
    n, m, k, nb = case.n, case.m, case.k, len(d["G"])
    Af, Gf = KC.flat(d)
    kind, offs, dim = S.cone_arrays(list(case.cones))
    out = dict(cx=np.zeros(nb * n), cy=np.zeros(nb * m), cz=np.zeros(nb * k), cs=np.zeros(nb * k),
               status=np.zeros(nb, np.int32))
    dx, dy, dz, ds = KC.flat_rhs(d, j, m)
    p = _lib.ptr
    keep = [np.ascontiguousarray(v) for v in (d["s"].ravel(), d["z"].ravel(), dx, dz, ds)]
    dyc = np.ascontiguousarray(dy) if m else None
    _lib.check(_lib.load().socp_batch_kkt_solve_qp(
        S.default_context().handle, _lib.Dims(nb, n, m, k, len(kind)), p(kind), p(offs), p(dim), p(P), p(Af), p(Gf),
        p(QK.sing_bytes(case, nb)), p(keep[0]), p(keep[1]), p(keep[2]), p(dyc), p(keep[3]), p(keep[4]),
        p(out["cx"]), p(out["cy"] if m else None), p(out["cz"]), p(out["cs"]), p(out["status"]),
        S.F_FORCE_LARGE if case.force_large else 0))
    return out


NULL_CASES = [QK.BY_ID[i] for i in ("c1", "mq2", "sing", "edge65", "gv")]


@pytest.mark.parametrize("case", NULL_CASES, ids=QK.case_id)
def test_null_P_is_the_linear_entry(case):
    d = QK.inputs(case)
    lin_name = QK.linear_kernel_name(case)
    lin = fused(case, d, 0, P=None)
    kernel_is(lin_name)
    assert (lin["status"] == 0).all()
    got = raw_fused(case, d, 0, None)
    kernel_is(lin_name)
    same(got, lin)
    hl, hq = handle(case, d, P=None), RawQpHandle(case, d, None)
    try:
        for h in (hl, hq):
            st = h.setup_iter(d["s"].ravel(), d["z"].ravel())
            kernel_is(lin_name)
            assert (st == 0).all()
        a, b = hl.solve_kkt(*KC.flat_rhs(d, 0, case.m)), hq.solve_kkt(*KC.flat_rhs(d, 0, case.m))
        kernel_is(lin_name)
        same(b, a)
        same(a, lin)
    finally:
        hl.close()
        hq.close()


@pytest.mark.parametrize("case", NULL_CASES, ids=QK.case_id)
def test_zero_P_equals_the_linear_entry(case):
    d = QK.inputs(case)
    lin = fused(case, d, 0, P=None)
    zero = np.zeros(QK.B * case.n * case.n)
    got = fused(case, d, 0, P=zero)
    kernel_is(case.kernel)
    h = handle(case, d, P=zero)
    try:
        assert (h.setup_iter(d["s"].ravel(), d["z"].ravel()) == 0).all()
        split = h.solve_kkt(*KC.flat_rhs(d, 0, case.m))
    finally:
        h.close()
    for key in OUT:
        assert np.array_equal(got[key], lin[key]), key
        assert np.array_equal(split[key], lin[key]), key


# ----------------------------------------------------------- 4. P is used
@pytest.mark.parametrize("cid", ["c1", "c1_large"])
def test_P_is_used(cid):
    case = QK.BY_ID[cid]
    d = QK.inputs(case)
    n, m, k = case.n, case.m, case.k
    with_P, no_P = fused_once(case, 0), fused(case, d, 0, P=None)
    for p in range(QK.B):
        e = KC.rel_errors(vectors(no_P, p, n, m, k), vectors(with_P, p, n, m, k))
        for key, ev, gv in zip(KC.KEYS, e, QK.gates(case, p, 0)):
            print(f"  {cid} p={p} {key}: with P against without {ev:.3g}, gate {gv:.3g}")
            assert ev > 100.0 * gv, (key, ev, gv)


# ----------------------------------------------------------- 5. shared P
@pytest.mark.parametrize("cid", ["c1", "edge65"])
def test_shared_P(cid):
    case = QK.BY_ID[cid]
    d = dict(QK.inputs(case))
    nb = QK.B
    for key in ("A", "G", "P"):  # problem 0's matrices for both problems; s, z and the right-hand sides stay per problem
        d[key] = np.stack([d[key][0]] * nb)
    rep = fused(case, d, 0)
    kernel_is(case.kernel)
    assert (rep["status"] == 0).all()
    Af, Gf = KC.flat(d, 1)
    P1 = QK.flat_P(d, 1)
    dx, dy, dz, ds = KC.flat_rhs(d, 0, case.m)
    one = S.batch_kkt_solve(list(case.cones), case.n, case.m, case.k, Af, Gf, QK.sing_bytes(case, 1), d["s"].ravel(),
                            d["z"].ravel(), dx, dy, dz, ds, force_large=case.force_large, shared_matrices=True, P=P1)
    kernel_is(case.kernel)
    same(one, rep)
    h = S.DenseHandle(list(case.cones), case.n, case.m, case.k, Af, Gf, QK.sing_bytes(case, 1),
                      force_large=case.force_large, shared_matrices=True, batch=nb, P=P1)
    try:
        assert h.h2d_bytes == (case.m * case.n + case.k * case.n + case.n * case.n) * 8 + 1
        assert (h.setup_iter(d["s"].ravel(), d["z"].ravel()) == 0).all()
        same(h.solve_kkt(dx, dy, dz, ds), rep)
    finally:
        h.close()


# ------------------------------------------------------ 6. failure isolation
@pytest.mark.parametrize("cid", ["c1", "c1_large"])
def test_indefinite_P_fails_alone(cid):
    case = QK.BY_ID[cid]
    n, m, k, nb, bad = case.n, case.m, case.k, 4, 2
    d = KC.make_inputs(n, m, k, case.cones, (False,) * nb, nb)
    rng = np.random.default_rng([n, m, k, 2])
    R = rng.standard_normal((nb, n // 2, n))
    d["P"] = np.einsum("pij,pik->pjk", R, R) / n
    good = fused(case, d, 0)
    assert (good["status"] == 0).all()
    d2 = dict(d, P=d["P"].copy())
    d2["P"][bad] = -10.0 * np.eye(n)
    import oracle
    import qp_cases as QC
    sc = oracle.compute_scaling(list(case.cones), d["s"][bad], d["z"][bad])
    assert QC._Factor(list(case.cones), d2["P"][bad], d["A"][bad], d["G"][bad], False, sc).status == S.CHOL_H_FAILED
    got = fused(case, d2, 0)
    kernel_is(case.kernel)
    h = handle(case, d2)
    try:
        st = h.setup_iter(d["s"].ravel(), d["z"].ravel())
        split = h.solve_kkt(*KC.flat_rhs(d, 0, m))
    finally:
        h.close()
    want = np.zeros(nb, np.int32)
    want[bad] = S.CHOL_H_FAILED
    assert np.array_equal(st, want)
    for out in (got, split):
        assert np.array_equal(out["status"], want)
        for key, q in zip(KC.KEYS, (n, m, k, k)):
            v = out[key].reshape(nb, q)
            assert np.isnan(v[bad]).all(), key
            others = [p for p in range(nb) if p != bad]
            assert v[others].tobytes() == good[key].reshape(nb, q)[others].tobytes(), key


# ------------------------------------------------------------- 7. refusal
def test_explicit_inverse_with_P_is_refused():
    case = QK.BY_ID["c1"]
    d = QK.inputs(case)
    with pytest.raises(S.SocpError) as ei:
        fused(case, d, 0, explicit_inverse=True)
    assert ei.value.code == _lib.SOCP_E_UNSUPPORTED and "socp_batch_kkt_solve_qp" in str(ei.value)
    with pytest.raises(S.SocpError) as ei:
        handle(case, d, explicit_inverse=True)
    assert ei.value.code == _lib.SOCP_E_UNSUPPORTED and "socp_dense_create_qp" in str(ei.value)
    # without a P the flag stays what it was
    out = fused(case, d, 0, P=None, explicit_inverse=True)
    assert (out["status"] == 0).all()
    kernel_is("socp_small_xi_kkt_kernel<2,12,1>")


# ------------------------------------------------- 8. the plugin loop on a QP
def test_plugin_loop_solves_the_QP_system():
    case = QK.BY_ID["c1"]
    d = QK.inputs(case)
    n, m, k = case.n, case.m, case.k
    cones = [S.SOC(0, 48)]
    prob = S.Problem(np.zeros(n), d["A"][0], np.zeros(m), d["G"][0], np.zeros(k), cones, P=d["P"][0])
    assert not prob.sing
    solver = S.DenseSolver(prob)
    ss = S.SolverState(prob, solver)
    state = S.State(prob, np.zeros(n), np.zeros(m), d["z"][0], d["s"][0])
    S.compute_scaling(prob.cones, ss.scaling, state.s, state.z)
    S.setup_iter(solver, prob, state, ss.scaling)
    kernel_is(case.kernel)
    dx, dy, dz, ds = (v[0] for v in d["rhs"][0])
    cx, cy, cz, cs = np.zeros(n), np.zeros(m), np.zeros(k), np.zeros(k)
    S.solve_kkt(solver, prob, state, ss.scaling, dx, dy, dz, ds, cx, cy, cz, cs)
    want = fused(case, d, 0, nb=1)
    for got, key in zip((cx, cy, cz, cs), KC.KEYS):
        assert got.tobytes() == want[key].tobytes(), key
    # and it is the QP's system: not the linear one
    lin = fused(case, d, 0, P=None, nb=1)
    assert not np.array_equal(cx, lin["cx"])
