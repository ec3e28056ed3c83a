"""Quadratic objectives on the device: socp_batch_solve_qp (batch_solve's P) on
the register kernel's QP instantiations and the blocked kernel's.

The reference is tests/qp_cases.py's numpy restatement of the method in the
kernels' operation order, which tests/test_qp_cpu.py pins to the CPU oracle at
P = 0.  Gates: np.array_equal / tobytes where two device runs must agree;
rel <= 1e-8 on x, y, z, s per problem against the restatement over the first
iterations (gate P4 of DESIGN section 7; kappa_2(H) of those factorisations is
bounded in test_qp_cpu.py), and max(1e-8, 1e-12 kappa) for the longer
trajectories, the fixtures' gate.
"""
import functools

import numpy as np
import pytest

import qp_cases as Q
import socp_amd as S
from infeasible import in_cone

pytestmark = pytest.mark.gpu

KEYS = ("x", "y", "z", "s", "res", "iters", "status")
# (id, shape, force_large, kernel family)
CASES = [("c1", "c1", False, "small"), ("c2", "c2", False, "small"), ("mq2", "mq2", False, "small"),
         ("m0", "m0", False, "small"), ("sing", "sing", False, "small"), ("c1_large", "c1", True, "large"),
         ("blk", "blk", False, "large")]
CASE_IDS = [c[0] for c in CASES]


def solve(d, P, sing="batch", **kw):
    cones, n, m, k = d.shape[:4]
    sg = d.sing if isinstance(sing, str) else sing
    out = S.batch_solve(list(cones), n, m, k, d.c, d.A if m else None, d.b if m else None, d.G, d.h, sg,
                        res=True, P=P, **kw)
    return out, S.default_context().last_kernel_name()


def check_kernel(name, family, qp=True):
    assert family in name, name
    assert ("qp" in name) == qp, name


def same(a, b, keys=KEYS):
    for key in keys:
        u, v = np.asarray(a[key]), np.asarray(b[key])
        assert u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes(), key


def rel(u, v):
    return float(np.linalg.norm(u - v) / np.linalg.norm(v)) if len(v) else 0.0


def rows(out, d, p):
    cones, n, m, k = d.shape[:4]
    return (out["x"][p * n:(p + 1) * n], out["y"][p * m:(p + 1) * m], out["z"][p * k:(p + 1) * k],
            out["s"][p * k:(p + 1) * k])


def qp_entry_null_P(d, force_large=False, maxit=40, tol=1e-5):
    """socp_batch_solve_qp called directly with P == NULL (the wrapper routes
    P=None to socp_batch_solve_ex, so it never makes this call)."""
    from socp_amd import _lib
    cones, n, m, k = d.shape[:4]
    kind, offs, dim = S.cone_arrays(list(cones))
    B = d.B
    out = dict(x=np.zeros(B * n), y=np.zeros(max(B * m, 1)), z=np.zeros(B * k), s=np.zeros(B * k),
               iters=np.zeros(B, np.int32), status=np.zeros(B, np.int32), res=np.zeros(3 * B))
    pr = _lib.default_params(maxit=maxit, tol=tol, flags=_lib.F_FORCE_LARGE if force_large else 0)
    p, ctx = _lib.ptr, S.default_context()
    rc = _lib.load().socp_batch_solve_qp(
        ctx.handle, _lib.Dims(B, n, m, k, len(kind)), p(kind), p(offs), p(dim), None, p(d.c), p(d.A) if m else None,
        p(d.b) if m else None, p(d.G), p(d.h), p(d.sing), pr, p(out["x"]), p(out["y"]) if m else None, p(out["z"]),
        p(out["s"]), p(out["iters"]), p(out["status"]), p(out["res"]))
    _lib.check(rc)
    if m == 0:
        out["y"] = out["y"][:0]
    return out, ctx.last_kernel_name()


# ------------------------------------------------------------------ 1. P = 0
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_zero_P_equals_the_linear_solve(case):
    _, name, large, family = case
    d = Q.batch(name)
    zero = np.zeros_like(d.P)
    for kw in (dict(), dict(maxit=4, tol=0.0)):
        plain, kn = solve(d, None, force_large=large, **kw)
        check_kernel(kn, family, qp=False)
        none, kn2 = solve(d, None, force_large=large, **kw)
        assert kn2 == kn
        same(none, plain)  # P=None: the plain call's kernel and bytes
        null, kn3 = qp_entry_null_P(d, force_large=large, **kw)
        assert kn3 == kn
        same(null, plain)  # socp_batch_solve_qp itself with P == NULL
        got, kq = solve(d, zero, force_large=large, **kw)
        check_kernel(kq, family)
        for key in KEYS:
            assert np.array_equal(got[key], plain[key], equal_nan=True), (key, kw)


@pytest.mark.parametrize("case", [CASES[0], ("singz", "singz", False, "small"), ("singz_large", "singz", True, "large"),
                                  CASES[5]], ids=["c1", "singz", "singz_large", "c1_large"])
def test_sing_probe_never_sees_P(case):
    """sing = None: the device factors G'G alone, so the probe's verdict -- and
    with it every output bit -- is that of the byte passed explicitly: 0 at c1;
    1 at the shape whose G has a zero column, where cholesky(G'G) meets an
    exactly zero pivot although P + G'G is positive definite."""
    _, name, large, family = case
    d = Q.batch(name)
    for kw in (dict(), dict(maxit=4, tol=0.0)):
        want, _ = solve(d, d.P, force_large=large, **kw)
        got, kn = solve(d, d.P, sing=None, force_large=large, **kw)
        check_kernel(kn, family)
        same(got, want)


def term_scales(prob, x, y, z, s):
    """The magnitudes of what the three exit quantities are summed from:
    | |P||x| + |c| + |A'||y| + |G'||z| |, | |A||x| + |b| |, |z|'|s|."""
    Pm, c, A, b, G, h = prob
    ab = np.abs
    return (np.linalg.norm(ab(Pm) @ ab(x) + ab(c) + ab(A).T @ ab(y) + ab(G).T @ ab(z)),
            np.linalg.norm(ab(A) @ ab(x) + ab(b)), ab(z) @ ab(s))


def check_res(res, prob, x, y, z, s, first=False):
    """res at an iterate well before convergence against |rd|, |rp|, z's formed
    in numpy from the outputs.  A sum of N = n + m + k + 2 terms is off by at
    most u = N 2^-53 of the magnitude of its terms in either order (N <= 1222:
    u <= 1.4e-13; measured 2e-16).  Each quantity is held to 1e-13 of that
    magnitude, and to 1e-9 of the quantity itself wherever that is attainable:
    where the quantity is at least u / 1e-9 of the magnitude (3e-6 .. 1.4e-4).
    After the first iteration |rd| and z's must be (first=True);
    |rp| never is: the initial point solves Ax = b and Newton steps keep it,
    so |rp| is rounding (1e-14) from the first iterate on.  Returns the worst
    error relative to a quantity."""
    terms = Q.exit_terms(prob, x, y, z, s)
    worst = 0.0
    thr = (len(x) + len(y) + len(z) + 2) * 2.0 ** -53 / 1e-9
    for q, scale in enumerate(term_scales(prob, x, y, z, s)):
        err = abs(res[q] - terms[q])
        assert err <= 1e-13 * scale, (q, res[q], terms[q], scale)
        if first and q != 1:
            assert terms[q] >= thr * scale, (q, terms[q], scale)
        if terms[q] > 0.0 and terms[q] >= thr * scale:
            worst = max(worst, err / terms[q])
            assert err <= 1e-9 * terms[q], (q, res[q], terms[q])
    return worst


# ------------------------------------------------------------ 2. trajectory
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_trajectory_against_the_restatement(case):
    """x, y, z, s against the restatement; and, for K <= 3, res against the
    three exit quantities formed in numpy from the outputs (check_res): after
    one to three iterations |rd| and z's are far above the rounding of their
    terms, so the bound relative to the quantity itself holds there and a
    wrong Px term or norm cannot pass."""
    _, name, large, family = case
    d = Q.batch(name)
    for K in (1, 2, 3) + ((6,) if name in ("c2", "blk") else ()):
        ref = Q.reference(name, K, 0.0)
        got, kn = solve(d, d.P, force_large=large, maxit=K, tol=0.0)
        check_kernel(kn, family)
        worst, worst_res = 0.0, 0.0
        for p, r in enumerate(ref):
            assert got["status"][p] == r["status"], (K, p)
            gate = 1e-8 if K <= 3 else max(1e-8, 1e-12 * max(r["kappa"]))
            for u, v in zip(rows(got, d, p), (r["x"], r["y"], r["z"], r["s"])):
                e = rel(u, v)
                worst = max(worst, e / gate)
                assert e <= gate, (K, p, e, gate)
            if K <= 3:
                worst_res = max(worst_res, check_res(got["res"][3 * p:3 * p + 3], d.probs[p], *rows(got, d, p),
                                                      first=K == 1))
        print(f"{case[0]} K={K}: worst error / gate {worst:.2e}, res vs numpy worst rel {worst_res:.2e} on {kn}")


def test_global_vector_blocked_kernel():
    """k = 1200: the problem's vectors exceed a CU's LDS, so the blocked
    kernel's global-vector QP instantiation runs.  (The restatement's dense
    k x k scaling matrices cost minutes at this k, so the outputs are checked
    on their own.)  Under the reference rule every problem converges and its
    outputs satisfy the optimality conditions of the QP in numpy -- |Px + c +
    A'y + G'z| + |Ax - b| + z's < tol, s and z in K, |Gx + s - h| <= 1e-7 (1 +
    |h|) -- and at K = 1, tol 0, res equals the three quantities formed from
    the outputs (check_res)."""
    d = Q.batch("gv", 8)
    cones = d.shape.cones
    got, kn = solve(d, d.P)
    assert kn == "socp_large_qp_gv_kernel", kn
    assert (got["status"] == S.CONVERGED).all(), got["status"]
    for p, prob in enumerate(d.probs):
        x, y, z, s = rows(got, d, p)
        assert sum(Q.exit_terms(prob, x, y, z, s)) < Q.TOL, p
        assert in_cone(cones, s) and in_cone(cones, z), p
        assert np.linalg.norm(prob[4] @ x + s - prob[5]) <= 1e-7 * (1.0 + np.linalg.norm(prob[5])), p
    its = got["iters"]
    got, kn = solve(d, d.P, maxit=1, tol=0.0)
    assert kn == "socp_large_qp_gv_kernel", kn
    worst = max(check_res(got["res"][3 * p:3 * p + 3], prob, *rows(got, d, p), first=True)
                for p, prob in enumerate(d.probs))
    print(f"gv: iterations {its.min()}..{its.max()}, K = 1 res vs numpy worst rel {worst:.2e}")


# --------------------------------------------------------- 3. reference rule
@pytest.mark.parametrize("name", Q.RULE_SHAPES)
def test_reference_rule(name):
    """res against the same three quantities formed in numpy from the outputs,
    to 1e-13 of the magnitude of the terms each is summed from (term_scales):
    a sum of n + m + k + 2 <= 180 terms is off by at most 180 x 2^-53 = 2e-14
    of that magnitude in either order, measured 1.8e-16.  At a converged
    iterate |rd| and |rp| are what is left of O(1) terms after cancellation
    (1e-7 .. 1e-10 here), so relative to the residual itself the kernel and
    numpy differ by up to 4.1e-7 on c1 (printed below), as two numpy orders
    do; the bound relative to the quantity itself, 1e-9, is asserted where it
    is attainable, at the fixed-K iterates of
    test_trajectory_against_the_restatement."""
    d = Q.batch(name)
    cones, n, m, k = d.shape[:4]
    ref = Q.reference(name)
    got, kn = solve(d, d.P)
    check_kernel(kn, "small")
    assert (got["status"] == S.CONVERGED).all(), got["status"]
    nclear, worst, worst_self = 0, 0.0, 0.0
    for p, (r, prob) in enumerate(zip(ref, d.probs)):
        x, y, z, s = rows(got, d, p)
        terms = Q.exit_terms(prob, x, y, z, s)
        assert sum(terms) < Q.TOL, (p, terms)
        assert in_cone(cones, s) and in_cone(cones, z), p
        for q, scale in enumerate(term_scales(prob, x, y, z, s)):
            err = abs(got["res"][3 * p + q] - terms[q])
            if scale:
                worst = max(worst, err / scale)
            if terms[q]:
                worst_self = max(worst_self, err / terms[q])
        if Q.clear(r):
            nclear += 1
            assert got["iters"][p] == r["iters"], (p, got["iters"][p], r["iters"])
    print(f"{name}: {nclear} clear problems, iterations {got['iters'].min()}..{got['iters'].max()}, "
          f"res vs numpy worst rel {worst:.2e} of the terms' magnitude, {worst_self:.2e} of the residual itself")
    assert worst <= 1e-13
    assert nclear >= 24


# ------------------------------------------------------ 4. a known answer
def test_projection_onto_a_second_order_cone():
    """x* = the projection of a onto K.  With (x, z, s) the outputs, rd = x - a
    - z, rz = s - x: a = (x - rd) - z with z's = gap, so by Moreau's
    decomposition and the 1-Lipschitz projection |x - Pi_K(a)| <= sqrt(gap) +
    |rd| + 2 |Gx + s - h|."""
    cones, a, P, c, G, h = Q.projection_batch()
    nb, n = a.shape
    got = S.batch_solve(list(cones), n, 0, n, c, None, None, G, h, np.zeros(nb, np.uint8), res=True, P=P)
    check_kernel(S.default_context().last_kernel_name(), "small")
    assert (got["status"] == S.CONVERGED).all(), got["status"]
    worst = 0.0
    for p in range(nb):
        x, z, s = (got[key][p * n:(p + 1) * n] for key in "xzs")
        gap = max(float(z @ s), 0.0)
        bound = np.sqrt(gap) + np.linalg.norm(x - a[p] - z) + 2.0 * np.linalg.norm(s - x)
        err = np.linalg.norm(x - Q.soc_projection(a[p]))
        worst = max(worst, err / bound)
        assert bound < 2.0 * np.sqrt(Q.TOL), (p, bound)
        assert err <= bound, (p, err, bound)
    print(f"projection: iterations {got['iters'].min()}..{got['iters'].max()}, worst error / bound {worst:.3f}")


# ----------------------------------------------------------------- 5. shared
@functools.lru_cache(maxsize=None)
def num_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("name,large", [("c1", False), ("c2", False), ("mq2", False), ("c1", True)],
                         ids=["c1", "c2", "mq2", "c1_large"])
def test_shared_P_equals_replicated(name, large):
    # 16 problems per CU on the register kernel: every wave takes several problems
    nb = 64 if large else 16 * num_cu()
    d = Q.shared_batch(name, nb)
    cones, n, m, k = d.shape[:4]
    for kw in (dict(), dict(maxit=4, tol=0.0)):
        sh = S.batch_solve(list(cones), n, m, k, d.c, d.A, d.b, d.G, d.h, np.zeros(1, np.uint8), res=True,
                           shared_matrices=True, P=d.P, force_large=large, **kw)
        kn = S.default_context().last_kernel_name()
        check_kernel(kn, "large" if large else "small")
        rp = S.batch_solve(list(cones), n, m, k, d.c, np.tile(d.A, nb), d.b, np.tile(d.G, nb), d.h,
                           np.zeros(nb, np.uint8), res=True, P=np.tile(d.P, nb), force_large=large, **kw)
        assert S.default_context().last_kernel_name() == kn
        same(sh, rp)
    assert (sh["status"] == 1).all()


# ---------------------------------------------------------------- 6. bitwise
@pytest.mark.parametrize("case", [CASES[0], CASES[1], CASES[5]], ids=["c1", "c2", "c1_large"])
def test_warm_start_single_problem_and_device_tensors(case):
    import torch
    _, name, large, family = case
    d = Q.batch(name)
    cones, n, m, k = d.shape[:4]
    full, _ = solve(d, d.P, force_large=large, maxit=3, tol=0.0)
    a2, _ = solve(d, d.P, force_large=large, maxit=2, tol=0.0)
    a3, kn = solve(d, d.P, force_large=large, maxit=1, tol=0.0, warm=(a2["x"], a2["y"], a2["z"], a2["s"]))
    check_kernel(kn, family)
    same(a3, full, ("x", "y", "z", "s", "res", "status"))
    # problem p alone
    p = 5
    one = S.batch_solve(list(cones), n, m, k, d.c[p * n:(p + 1) * n], d.A[p * m * n:(p + 1) * m * n],
                        d.b[p * m:(p + 1) * m], d.G[p * k * n:(p + 1) * k * n], d.h[p * k:(p + 1) * k],
                        d.sing[p:p + 1], res=True, P=d.P[p * n * n:(p + 1) * n * n], force_large=large, maxit=3, tol=0.0)
    for u, v in zip(rows(full, d, p), (one["x"], one["y"], one["z"], one["s"])):
        assert u.tobytes() == v.tobytes()
    assert one["res"].tobytes() == full["res"][3 * p:3 * p + 3].tobytes()
    # torch device tensors, used in place
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()  # noqa: E731
    dev = S.batch_solve(list(cones), n, m, k, t(d.c), t(d.A), t(d.b), t(d.G), t(d.h), t(d.sing), res=True,
                        P=t(d.P), force_large=large, maxit=3, tol=0.0)
    S.default_context().sync()
    assert "qp" in S.default_context().last_kernel_name()
    same({key: v.cpu().numpy()[:full[key].size] for key, v in dev.items()}, full)


# -------------------------------------------------------------- 7. isolation
@pytest.mark.parametrize("case", [CASES[0], CASES[1], CASES[5]], ids=["c1", "c2", "c1_large"])
def test_indefinite_P_fails_its_problem_alone(case):
    _, name, large, family = case
    d = Q.batch(name)
    n = d.shape.n
    base, _ = solve(d, d.P, force_large=large)
    bad = 7
    P = d.P.copy()
    P[bad * n * n:(bad + 1) * n * n] = (-1e6 * np.eye(n)).ravel()
    got, kn = solve(d, P, force_large=large)
    check_kernel(kn, family)
    assert got["status"][bad] == S.CHOL_H_FAILED
    keep = np.arange(d.B) != bad
    for key in KEYS:
        per = np.asarray(got[key]).reshape(d.B, -1), np.asarray(base[key]).reshape(d.B, -1)
        assert per[0][keep].tobytes() == per[1][keep].tobytes(), key


# --------------------------------------------------------------- 8. refusals
@pytest.mark.parametrize("flag", ["explicit_inverse", "detect_infeasible"])
def test_refused_flags(flag):
    d = Q.batch("c1")
    with pytest.raises(S.SocpError) as e:
        solve(d, d.P, **{flag: True})
    assert e.value.code == -2  # SOCP_E_UNSUPPORTED
    assert "socp_batch_solve_qp" in str(e.value)
    plain, _ = solve(d, None, **{flag: True})  # the linear solve still takes the flag
    assert plain["status"].size == d.B
