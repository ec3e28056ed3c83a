"""References of the differentiable solves (test_vjp_cpu.py, test_gpu_vjp.py):
socp_batch_centre and socp_batch_vjp.  Helpers only, no tests.

Problem: minimise x'Px/2 + c'x  s.t.  Ax = b, Gx + s = h, s in K; prob is
qp_cases' tuple (P, c, A, b, G, h) of matrices, cones ((kind, offs, dim), ...).

vjp_reference   the definition of socp_batch_vjp (include/socp.h) on the block
                system itself: qp_kkt_cases.kkt_matrix at (s, z), solved by
                kkt_cases.refined_solve for the right-hand side
                (gx - G'gs, gy, gz, 0) formed in np.longdouble, then the six
                formulas.  It knows nothing of H, S or any operation order.
centre_reference  socp_batch_centre's rule restated: mu = s'z/deg, lam from
                oracle.compute_scaling, the right-hand side with the residuals,
                the step from refined_solve on the block system, t = 1 halved
                while z + t dz or s + t ds is not interior (down to 2^-30).
                (A `sing` problem's step is the block system's here and the
                sing formula's on the device; kkt_cases.py's header says why
                the two differ by the size of rp only.)
exact_centre    the point of the central path at a given mu: damped Newton on
                (rd, rp, Gx + s - h, s o z - mu e) with kkt_cases.arrow, the
                iterate and the residual in np.longdouble, to 1e-13.
true_gradient   the derivative of the exact solution: vjp_reference at
                exact_centre, continued down mu = 1e-3, 1e-5, 1e-7, 1e-9, 1e-10.
"""
import functools

import numpy as np

import kkt_cases as KC
import oracle as O
import qp_cases as QC
import qp_kkt_cases as QK

P_, Q_ = KC.P_, KC.Q_
LD = np.longdouble
GRADS = ("dc", "db", "dh", "dP", "dA", "dG")
MU_PATH = (1e-3, 1e-5, 1e-7, 1e-9, 1e-10)
TABLE_SHAPES = ("s8", "m0", "s16", "c1")
TABLE_B = 8
STEPS = 4


def is_interior(cones, v):
    """POC entries > 0, SOC v0 > sqrt(sum_{i>=1} v_i^2) (socp_batch_centre's test)."""
    for kind, o, d in cones:
        if kind == P_:
            if not (v[o:o + d] > 0).all():
                return False
        elif not v[o] > np.sqrt(np.sum(v[o + 1:o + d] * v[o + 1:o + d])):
            return False
    return True


def jordan(cones, u, v):
    """u o v = Arw(u) v in the arguments' own precision (kkt_cases.arrow is float64)."""
    out = u * v
    for kind, o, d in cones:
        if kind == Q_:
            out[o] = u[o:o + d] @ v[o:o + d]
            out[o + 1:o + d] = u[o] * v[o + 1:o + d] + v[o] * u[o + 1:o + d]
    return out


def residuals(prob, x, y, z, s, dtype=np.float64):
    """(rd, rp, rz) = (Px + c + A'y + G'z, Ax - b, Gx + s - h)."""
    Pm, c, A, b, G, h = [np.asarray(v, dtype) for v in prob]
    rd = Pm @ x + c + G.T @ z + (A.T @ y if len(b) else 0)
    rp = A @ x - b if len(b) else np.zeros(0, dtype)
    return rd, rp, G @ x + s - h


def off_centre(cones, s, z, gap=None):
    """|lam o lam - mu e|_2 / mu with lam from oracle.compute_scaling, mu = s'z/deg
    (gap: s'z as the caller has it; near a solution s'z cancels, and two orders
    of summation differ by as much as a centred point's measure)."""
    cl = list(cones)
    sc = O.compute_scaling(cl, s, z, iwiw=False)
    assert sc["status"] == 0
    mu = float(s @ z if gap is None else gap) / O.deg(cl)
    return float(np.linalg.norm(O.vprod(cl, sc["l"], sc["l"]) - mu * O.make_e(cl, len(s))) / mu)


# -------------------------------------------------------------- the adjoint
def vjp_reference(cones, prob, x, y, z, s, gx, gy, gz, gs):
    """dict(dc, db, dh, dP, dA, dG, ux, uy, uz, w) of one problem, matrices as matrices."""
    Pm, c, A, b, G, h = prob
    k, n = G.shape
    m = A.shape[0]
    K = QK.kkt_matrix(cones, Pm, A, G, s, z)
    rx = gx.astype(LD) - G.T.astype(LD) @ gs.astype(LD)
    R = np.concatenate([rx, gy.astype(LD), gz.astype(LD), np.zeros(k, LD)])[:, None]
    u, _, _ = KC.refined_solve(K, R)
    ux, uy, uz, _ = KC.split(u[:, 0], n, m, k)
    w = uz + gs
    return dict(dc=-ux, db=uy, dh=w, dP=-(np.outer(ux, x) + np.outer(x, ux)) / 2.0,
                dA=-(np.outer(y, ux) + np.outer(uy, x)), dG=-(np.outer(z, ux) + np.outer(w, x)),
                ux=ux, uy=uy, uz=uz, w=w)


def grad_error(got, ref):
    """The largest, over the six gradients, of |got - ref|_2 / |ref|_2 (empty ones skipped)."""
    worst = 0.0
    for key in GRADS:
        r = np.asarray(ref[key]).ravel()
        if r.size == 0:
            continue
        worst = max(worst, float(np.linalg.norm(np.asarray(got[key]).ravel() - r) / np.linalg.norm(r)))
    return worst


# -------------------------------------------------------------- the centring
def centre_step(cones, prob, x, y, z, s):
    """One pass of socp_batch_centre's rule; None where (s, z) is not interior or no step length is found."""
    Pm, c, A, b, G, h = prob
    k, n = G.shape
    m = A.shape[0]
    cl = list(cones)
    mu = float(s @ z) / O.deg(cl)
    sc = O.compute_scaling(cl, s, z, iwiw=False)
    if sc["status"]:
        return None
    rd, rp, rz = residuals(prob, x, y, z, s)
    ds = mu * O.make_e(cl, k) - O.vprod(cl, sc["l"], sc["l"])
    K = QK.kkt_matrix(cones, Pm, A, G, s, z)
    u, _, _ = KC.refined_solve(K, np.concatenate([-rd, -rp, -rz, ds])[:, None])
    cx, cy, cz, cs = KC.split(u[:, 0], n, m, k)
    t = 1.0
    while not (is_interior(cones, z + t * cz) and is_interior(cones, s + t * cs)):
        t *= 0.5
        if t < 2.0 ** -30:
            return None
    return x + t * cx, y + t * cy, z + t * cz, s + t * cs


def centre_reference(cones, prob, x, y, z, s, steps=STEPS):
    """[(x, y, z, s) after j passes, j = 0 .. steps] (shorter where a pass finds no step)."""
    pts = [(x, y, z, s)]
    for _ in range(steps):
        nxt = centre_step(cones, prob, *pts[-1])
        if nxt is None:
            break
        pts.append(nxt)
    return pts


def exact_centre(cones, prob, x, y, z, s, mu, tol=1e-13, maxit=200):
    """The central-path point at mu from the interior start (x, y, z, s):
    ((x, y, z, s) in float64, the residual norm reached)."""
    Pm, c, A, b, G, h = prob
    k, n = G.shape
    m = A.shape[0]
    cl = list(cones)
    e = O.make_e(cl, k).astype(LD)
    x, y, z, s = [np.asarray(v, LD).copy() for v in (x, y, z, s)]

    def F(x, y, z, s):
        rd, rp, rz = residuals(prob, x, y, z, s, LD)
        return np.concatenate([rd, rp, rz, jordan(cones, s, z) - mu * e])

    f = F(x, y, z, s)
    N = n + m + 2 * k
    for _ in range(maxit):
        nf = float(np.linalg.norm(f))
        if nf <= tol:
            break
        J = np.zeros((N, N))
        J[:n, :n] = Pm
        J[:n, n:n + m] = A.T
        J[:n, n + m:n + m + k] = G.T
        J[n:n + m, :n] = A
        J[n + m:n + m + k, :n] = G
        J[n + m:n + m + k, n + m + k:] = np.eye(k)
        J[n + m + k:, n + m:n + m + k] = KC.arrow(cones, s.astype(np.float64))
        J[n + m + k:, n + m + k:] = KC.arrow(cones, z.astype(np.float64))
        d = np.linalg.solve(J, -f.astype(np.float64)).astype(LD)
        dx, dy, dz, ds = KC.split(d, n, m, k)
        t = LD(1.0)
        while t > 2.0 ** -40:
            cand = (x + t * dx, y + t * dy, z + t * dz, s + t * ds)
            if is_interior(cones, cand[2]) and is_interior(cones, cand[3]):
                fc = F(*cand)
                if float(np.linalg.norm(fc)) < nf:
                    break
            t = t / 2
        else:
            break
        x, y, z, s = cand
        f = fc
    return tuple(v.astype(np.float64) for v in (x, y, z, s)), float(np.linalg.norm(f))


def exact_path(cones, prob, start, mus=MU_PATH):
    """exact_centre continued along `mus` from `start`: the last point and the worst residual."""
    pt, worst = start, 0.0
    for mu in mus:
        pt, r = exact_centre(cones, prob, *pt, mu)
        worst = max(worst, r)
    return pt, worst


def true_gradient(cones, prob, start, g):
    """The derivative of the exact solution: vjp_reference at the end of exact_path.
    (gradient dict, that point, the path's worst residual)."""
    pt, worst = exact_path(cones, prob, start)
    return vjp_reference(cones, prob, *pt, *g), pt, worst


# -------------------------------------------------------------- shared inputs
def upstream(name, nb, sing=False):
    """Seeded standard-normal gx, gy, gz, gs of a batch (gy = 0 for sing problems)."""
    sh = QC.SHAPES[name]
    rng = np.random.default_rng([sh.n, sh.m, sh.k, 7])
    g = [rng.standard_normal((nb, q)) for q in (sh.n, sh.m, sh.k, sh.k)]
    if sing:
        g[1][:] = 0.0
    return g


@functools.lru_cache(maxsize=None)
def table(name, nb=TABLE_B):
    """Shape `name`'s rows of the DESIGN table, computed once: per problem of
    qp_cases.batch(name, nb), from qp_reference(tol = 1e-5)'s final iterate,
    dict(status, start, pts, true, path_res, err[j], off[j]) -- pts the
    reference centring's iterates, err[j] the gradient error of vjp_reference
    at pts[j] against true_gradient, off[j] the off-centre measure there."""
    d = QC.batch(name, nb)
    cones = d.shape.cones
    g = upstream(name, nb, bool(d.shape.sing))
    rows = []
    for p, prob in enumerate(d.probs):
        r = QC.qp_reference(cones, prob, bool(d.shape.sing), tol=1e-5)
        start = (r["x"], r["y"], r["z"], r["s"])
        gp = [v[p] for v in g]
        row = dict(status=r["status"], start=start)
        if r["status"] == 0:
            true, pt, worst = true_gradient(cones, prob, start, gp)
            pts = centre_reference(cones, prob, *start)
            row.update(true=true, exact=pt, path_res=worst, pts=pts,
                       err=[grad_error(vjp_reference(cones, prob, *q, *gp), true) for q in pts],
                       off=[off_centre(cones, q[3], q[2]) for q in pts])
        rows.append(row)
    return rows


def flat_point(pts):
    """[(x, y, z, s)] per problem -> the library's four flat vectors."""
    return [np.concatenate([q[i] for q in pts]) for i in range(4)]


def unflatten(out, nb, n, m, k):
    """batch_vjp's flat outputs -> per problem dicts with matrices as matrices."""
    shape = dict(dc=(n,), db=(m,), dh=(k,), ux=(n,), uy=(m,), uz=(k,), dP=(n, n), dA=(m, n), dG=(k, n))
    res = []
    for p in range(nb):
        row = {}
        for key, sh in shape.items():
            if key not in out:
                continue
            cnt = int(np.prod(sh))
            v = np.asarray(out[key])[p * cnt:(p + 1) * cnt]
            row[key] = v.reshape(sh[::-1]).T if len(sh) == 2 else v
        res.append(row)
    return res
