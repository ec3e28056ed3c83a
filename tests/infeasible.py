"""Problems without a solution, and the detection rule restated in numpy.

``make_batch`` builds strictly feasible random problems and, from the same
draws, primal-infeasible and dual-infeasible ones whose certificates are known
in closed form.  ``rule_ratios`` / ``rule_fire`` restate the rule of
include/socp.h (SOCP_F_DETECT_INFEASIBLE) on the iterates of an
``oracle.solve_trace`` trace.
"""
import numpy as np

FEASIBLE, PRIMAL_INF, DUAL_INF = 0, 1, 2
ST_PRIMAL_INF, ST_DUAL_INF = 5, 6
TAU = 1e-7  # the library's default tolerance


def interior_point(rng, cones, k):
    """A point strictly inside the product cone."""
    v = np.zeros(k)
    for kind, o, d in cones:
        if kind == 0:
            v[o:o + d] = np.abs(rng.standard_normal(d)) + 0.5
        else:
            t = rng.standard_normal(d - 1)
            v[o + 1:o + d] = t
            v[o] = np.linalg.norm(t) + abs(rng.standard_normal()) + 0.5
    return v


def in_cone(cones, v):
    """v in K (closed): every POC element >= 0, every SOC head >= |tail|."""
    for kind, o, d in cones:
        if kind == 0:
            if not (v[o:o + d] >= 0).all():
                return False
        elif not v[o] >= np.linalg.norm(v[o + 1:o + d]):
            return False
    return True


def feasible_problem(rng, cones, n, m, k):
    """(c, A, b, G, h) with a strictly feasible primal-dual pair (x, s), (y, z),
    and those points."""
    A, G = rng.standard_normal((m, n)), rng.standard_normal((k, n))
    s, z = interior_point(rng, cones, k), interior_point(rng, cones, k)
    x, y = rng.standard_normal(n), rng.standard_normal(m)
    h, b = G @ x + s, A @ x
    c = -(A.T @ y + G.T @ z)
    return (c, A, b, G, h), (x, y, z, s)


def primal_infeasible(prob, pts):
    """Rank-one corrections of G and h after which (y, z) is an exact
    certificate: A'y + G'z = 0, b'y + h'z = -1, z interior."""
    c, A, b, G, h = prob
    x, y, z, s = pts
    r = A.T @ y + G.T @ z
    G = G - np.outer(z, r) / (z @ z)
    h = h - z * (h @ z + b @ y + 1.0) / (z @ z)
    return c, A, b, G, h


def dual_infeasible(rng, prob, pts):
    """Rank-one corrections of G and c after which (xd, s) is an exact ray:
    A xd = 0, G xd + s = 0, c'xd = -1, s interior."""
    c, A, b, G, h = prob
    x, y, z, s = pts
    n, m = len(c), len(b)
    xd = rng.standard_normal(n)
    if m:
        Q = np.linalg.svd(A)[2][m:].T  # an orthonormal basis of null(A)
        xd = Q @ rng.standard_normal(n - m)
    G = G - np.outer(G @ xd + s, xd) / (xd @ xd)
    c = c - xd * (c @ xd + 1.0) / (xd @ xd)
    return (c, A, b, G, h), xd


def make_batch(cones, n, m, k, per_kind=16, seed=0):
    """3 * per_kind problems, interleaved feasible / primal-infeasible /
    dual-infeasible, in the flat layout of include/socp.h.  Returns
    (flat dict(c, A, b, G, h), kinds[B], problems[B] = (c, A, b, G, h),
    certs[B] = None, (y, z) or (xd, s): the builder's exact certificate)."""
    rng = np.random.default_rng(seed)
    probs, kinds, certs = [], [], []
    for _ in range(per_kind):
        base, pts = feasible_problem(rng, cones, n, m, k)
        dual, xd = dual_infeasible(rng, base, pts)
        probs += [base, primal_infeasible(base, pts), dual]
        kinds += [FEASIBLE, PRIMAL_INF, DUAL_INF]
        certs += [None, (pts[1], pts[2]), (xd, pts[3])]
    flat = dict(c=np.concatenate([p[0] for p in probs]),
                A=np.concatenate([p[1].ravel(order="F") for p in probs]) if m else np.zeros(0),
                b=np.concatenate([p[2] for p in probs]) if m else np.zeros(0),
                G=np.concatenate([p[3].ravel(order="F") for p in probs]),
                h=np.concatenate([p[4] for p in probs]))
    return flat, np.array(kinds), probs, certs


def certificate_ratios(prob, x, y, z, s):
    """(primal ratio, dual ratio) of the rule at one iterate: the certificate's
    residual over its normalisation, inf where the sign test fails."""
    c, A, b, G, h = prob
    hz = h @ z + b @ y
    cx = c @ x
    with np.errstate(all="ignore"):
        rp = np.linalg.norm(A.T @ y + G.T @ z) / -hz if hz < 0 else np.inf
        rd = max(np.linalg.norm(A @ x), np.linalg.norm(G @ x + s)) / -cx if cx < 0 else np.inf
    return float(rp), float(rd)


def rule_ratios(prob, trace):
    """certificate_ratios at every iterate of an oracle.solve_trace trace."""
    return [certificate_ratios(prob, *it) for it in trace]


def rule_fire(prob, result, tau=TAU, maxit=40, tol=1e-5):
    """The rule on an oracle.solve_trace result: (status, iteration, ratios), with
    status 5 / 6 and the iteration at whose start it fires, or (None, None,
    ratios) when it never does.  Evaluated where the kernels evaluate it:
    iteration t < maxit, after the domain check and the exit test."""
    c, A, b, G, h = prob
    trace = result["trace"]
    ratios = rule_ratios(prob, trace)
    for t, (x, y, z, s) in enumerate(trace):
        if t >= maxit:
            break
        if t == result["iters"] and result["status"] == 4:  # compute_scaling's DomainError comes first
            break
        ex = np.linalg.norm(A.T @ y + G.T @ z + c) + np.linalg.norm(A @ x - b) + z @ s
        if ex < tol:
            break
        rp, rd = ratios[t]
        if rp < tau:
            return ST_PRIMAL_INF, t, ratios
        if rd < tau:
            return ST_DUAL_INF, t, ratios
    return None, None, ratios


def clear_firing(status, it, ratios, tau=TAU, margin=1.1):
    """Whether the firing iteration is decided by more than rounding: the fired
    kind's ratio below tau / margin at iterate `it` and above margin * tau at
    the one before."""
    q = 0 if status == ST_PRIMAL_INF else 1
    if not ratios[it][q] < tau / margin:
        return False
    return it == 0 or ratios[it - 1][q] > margin * tau
