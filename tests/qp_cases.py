"""Quadratic objectives (socp_batch_solve_qp): batches and a numpy restatement.

Problem: minimise x'Px/2 + c'x  s.t.  Ax = b, Gx + s = h, s in K.

``make_batch`` draws strictly feasible problems with tests/infeasible.py's
``feasible_problem`` and adds P = R'R/n (R of size n/2 x n, standard normal);
c is shifted by -P x0 so that the builder's pair (x0, s0), (y0, z0) stays dual
feasible: P x0 + c + A'y0 + G'z0 = 0.

``qp_reference`` restates the interior-point method in the kernels' operation
order on the CPU oracle's cone primitives:
  X = W^-1 G by iscale per column;  H = P + X'X (+A'A when sing);
  H = L L';  Z = L^-1 A';  S = Z'Z;  triangular solves;
  solve_kkt as densesolver.jl:61-89;  the driver as solver.jl:86-150 with
  rd = Px + A'y + G'z + c;  the initial point from the same KKT route with
  W = I and ds = 0.
It returns the outputs, the iterate at the start of every iteration, the exit
sum there and kappa_2(H) of every factorisation.
"""
import collections
import functools

import numpy as np

import oracle as O
from infeasible import feasible_problem

P_, Q_ = 0, 1  # cone kinds of include/socp.h: POC, SOC

Shape = collections.namedtuple("Shape", "cones n m k sing")
SHAPES = dict(
    c1=Shape(((Q_, 0, 48),), 32, 8, 48, 0),                               # one slot
    c2=Shape(((P_, 0, 32), (Q_, 32, 32), (Q_, 64, 32)), 64, 16, 96, 0),   # two slots, NQ = 4
    mq2=Shape(((P_, 0, 16), (Q_, 16, 48)), 48, 32, 64, 0),                # m > 16: the inverse by nature
    m0=Shape(((P_, 0, 8), (Q_, 8, 8)), 8, 0, 16, 0),                      # no equalities
    sing=Shape(((Q_, 0, 8),), 10, 4, 8, 1),                               # k < n: cholesky(G'G) fails
    # the same with G's last column zero: cholesky(G'G) meets an exactly zero pivot, whatever the rounding
    # (on "sing" the rank-deficient G'G fails or passes cholesky by rounding: 2 of 32 pass in numpy)
    singz=Shape(((Q_, 0, 8),), 10, 4, 8, 1),
    blk=Shape(((P_, 0, 40), (Q_, 40, 40), (Q_, 80, 40)), 80, 20, 120, 0),  # n > 64: the blocked kernel only
    # k = 1200: the vectors exceed a CU's LDS, the blocked kernel's global-vector instantiation.  (With three
    # 400-row cones 7 of 8 such problems ended in status 2 or 4 under the reference rule; this table converges.)
    gv=Shape(((P_, 0, 1136), (Q_, 1136, 64)), 16, 4, 1200, 0),
    s16=Shape(((P_, 0, 8), (Q_, 8, 16)), 16, 4, 24, 0),
    s8=Shape(((Q_, 0, 16),), 8, 2, 16, 0),
)
# the batches the GPU tests run under the reference stopping rule against the
# restatement; c2 and blk are compared over their first iterations only (at
# those sizes about a third of such random problems end in status 2 or 4 late
# in the solve, with or without P)
RULE_SHAPES = ("c1", "mq2", "m0", "s16", "s8")
# seeds chosen so that the restatement converges on every problem and at least
# 3/4 of each RULE_SHAPES batch is "clear" (test_qp_cpu.py checks both)
# (mq2: the register kernel forms Li = H^-1 for m > 16, and late in a solve, at
# kappa_2(H) >= 1e10, its iterates leave the restatement's Cholesky order by
# 1e-7; with seed 13 that kept one problem of 32 from the exit test at the
# restatement's last iteration and it ended in status 2 later in the solve.
# Seeds 22, 23 and 24 converge on all 32 there.)
SEEDS = dict(c1=11, c2=12, mq2=24, m0=14, sing=15, singz=19, blk=16, gv=20, s16=17, s8=18)
B = 32
TOL = 1e-5

Batch = collections.namedtuple("Batch", "shape B P c A b G h sing probs")


def make_batch(name, nb=B, zero_P=False):
    """nb problems of SHAPES[name] in the flat layout of include/socp.h, with
    probs[p] = (P, c, A, b, G, h) as matrices."""
    sh = SHAPES[name]
    cones, n, m, k, sing = sh
    rng = np.random.default_rng(SEEDS[name])
    probs = []
    for _ in range(nb):
        (c, A, b, G, h), (x0, y0, z0, s0) = feasible_problem(rng, cones, n, m, k)
        if name == "singz":
            G[:, -1] = 0.0
            h, c = G @ x0 + s0, -(A.T @ y0 + G.T @ z0)
        R = rng.standard_normal((n // 2, n))
        Pm = np.zeros((n, n)) if zero_P else R.T @ R / n
        probs.append((Pm, c - Pm @ x0, A, b, G, h))
    cat = lambda i, mat: np.concatenate([(p[i].ravel(order="F") if mat else p[i]) for p in probs])  # noqa: E731
    return Batch(sh, nb, cat(0, True), cat(1, False), cat(2, True) if m else np.zeros(0),
                 cat(3, False) if m else np.zeros(0), cat(4, True), cat(5, False),
                 np.full(nb, sing, np.uint8), probs)


@functools.lru_cache(maxsize=None)
def batch(name, nb=B, zero_P=False):
    return make_batch(name, nb, zero_P)


def _identity_scaling(cones, k):
    e = O.make_e(cones, k)
    sc = O.compute_scaling(cones, e, e)
    assert np.array_equal(sc["W"], np.eye(k)) and np.array_equal(sc["l"], e)
    return sc


class _Factor:
    """setup_iter in the kernels' order at scaling sc; status 2 / 3 where the
    Cholesky of H / S fails."""

    def __init__(self, cones, Pm, A, G, sing, sc):
        k, n = G.shape
        m = A.shape[0]
        self.cones, self.sc, self.A, self.G, self.sing, self.m = cones, sc, A, G, sing, m
        X = np.column_stack([O.scale(cones, sc["wbs"], sc["mu"], G[:, j], inverse=True) for j in range(n)])
        H = Pm + X.T @ X
        if sing:
            H = H + A.T @ A
        self.X, self.status = X, 0
        self.kappa = float(np.linalg.cond(H))
        try:
            self.L = np.linalg.cholesky(H)
        except np.linalg.LinAlgError:
            self.status = 2
            return
        if m:
            self.Z = np.linalg.solve(self.L, A.T)  # L^-1 A'
            try:
                self.LS = np.linalg.cholesky(self.Z.T @ self.Z)
            except np.linalg.LinAlgError:
                self.status = 3

    def iw(self, v):
        return O.scale(self.cones, self.sc["wbs"], self.sc["mu"], v, inverse=True)

    def w(self, v):
        return O.scale(self.cones, self.sc["wbs"], self.sc["mu"], v)

    def li(self, v):
        return np.linalg.solve(self.L.T, np.linalg.solve(self.L, v))

    def solve(self, dx, dy, dz, ds, init=False):
        k0 = O.iprod(self.cones, self.sc["l"], ds)
        k2 = dz - self.w(k0)
        n0 = self.X.T @ self.iw(k2) + dx
        if self.sing and self.m:
            n0 = n0 + self.A.T @ dy
        cy = np.zeros(0)
        if self.m:
            t = np.linalg.solve(self.L, n0)
            m0 = self.Z.T @ t - dy
            cy = np.linalg.solve(self.LS.T, np.linalg.solve(self.LS, m0))
            m0 = dy - cy if (self.sing and not init) else -cy
            n0 = n0 + self.A.T @ m0
        cx = self.li(n0)
        k1 = self.G @ cx - k2
        cz = self.iw(self.iw(k1))
        cs = self.w(k0 - self.w(cz))
        return cx, cy, cz, cs


def exit_terms(prob, x, y, z, s):
    """(|Px + c + A'y + G'z|, |Ax - b|, z's)."""
    Pm, c, A, b, G, h = prob
    rd = Pm @ x + c + G.T @ z + (A.T @ y if len(b) else 0.0)
    rp = A @ x - b if len(b) else np.zeros(0)
    return float(np.linalg.norm(rd)), float(np.linalg.norm(rp)), float(z @ s)


def qp_reference(cones, prob, sing, maxit=40, tol=TOL, step=0.99, sigma_exp=3, init_eps=1e-10):
    """One problem.  dict(x, y, z, s, iters, status, res, trace, exits, kappa):
    trace[t] the iterate at the start of iteration t, exits[t] the exit sum
    there, kappa the condition numbers of H in factorisation order (the initial
    point's first)."""
    Pm, c, A, b, G, h = prob
    k, n = G.shape
    m = A.shape[0]
    e = O.make_e(cones, k)
    kappa, trace, exits = [], [], []
    out = dict(iters=0, status=1, trace=trace, exits=exits, kappa=kappa)

    def done(x, y, z, s, status, iters):
        out.update(x=x, y=y, z=z, s=s, status=status, iters=iters, res=np.array(exit_terms(prob, x, y, z, s)))
        return out

    f = _Factor(cones, Pm, A, G, sing, _identity_scaling(cones, k))
    kappa.append(f.kappa)
    if f.status:
        return done(np.zeros(n), np.zeros(m), np.zeros(k), np.zeros(k), f.status, 0)
    x, y, iz, _ = f.solve(-c, b, h, np.zeros(k), init=True)
    ap, ad = O.max_step(cones, -iz), O.max_step(cones, iz)
    s = -iz if abs(ap) < init_eps else -iz + (1.0 + ap) * e
    z = iz if abs(ad) < init_eps else iz + (1.0 + ad) * e
    dg = O.deg(cones)
    for it in range(maxit):
        trace.append((x.copy(), y.copy(), z.copy(), s.copy()))
        sc = O.compute_scaling(cones, s, z)
        nd, np_, gap = exit_terms(prob, x, y, z, s)
        exits.append(nd + np_ + gap)
        if sc["status"]:
            return done(x, y, z, s, 4, it)
        l = sc["l"]
        if nd + np_ + gap < tol:
            return done(x, y, z, s, 0, it)
        dx = -(Pm @ x + c + G.T @ z + (A.T @ y if m else 0.0))
        dy = -(A @ x - b) if m else np.zeros(0)
        dz = -(G @ x + s - h)
        ds = -O.vprod(cones, l, l)
        f = _Factor(cones, Pm, A, G, sing, sc)
        kappa.append(f.kappa)
        if f.status:
            return done(x, y, z, s, f.status, it)
        rx, ry, rz, rs = f.solve(dx, dy, dz, ds)
        kt3, kt2 = f.w(rz), f.iw(rs)
        t, dom = O.compute_step(cones, l, kt3, kt2)
        if dom:
            return done(x, y, z, s, 4, it)
        ll = l @ l
        rho = 1.0 - t - t * t * (kt2 @ kt3) / ll
        sig = max(0.0, min(1.0, rho)) ** sigma_exp
        mu = ll / dg
        ds = ds + (sig * mu * e - O.vprod(cones, kt2, kt3))
        rx, ry, rz, rs = f.solve(dx * (1.0 - sig), dy * (1.0 - sig), dz * (1.0 - sig), ds)
        t, dom = O.compute_step(cones, l, f.w(rz), f.iw(rs))
        if dom:
            return done(x, y, z, s, 4, it)
        t *= step
        x, y, z, s = x + rx * t, y + ry * t, z + rz * t, s + rs * t
    nd, np_, gap = exit_terms(prob, x, y, z, s)
    trace.append((x.copy(), y.copy(), z.copy(), s.copy()))
    exits.append(nd + np_ + gap)
    return done(x, y, z, s, 1, maxit)


@functools.lru_cache(maxsize=None)
def reference(name, maxit=40, tol=TOL, nb=B):
    """qp_reference on every problem of batch(name): computed once per (name, maxit, tol)."""
    d = batch(name, nb)
    return [qp_reference(d.shape.cones, p, bool(d.shape.sing), maxit=maxit, tol=tol) for p in d.probs]


def clear(r, tol=TOL, margin=1.1):
    """The exit iteration is decided by more than rounding: the exit sum below
    tol / margin at the last iterate and above margin * tol at the one before."""
    ex = r["exits"]
    return r["status"] == 0 and ex[-1] < tol / margin and (len(ex) == 1 or ex[-2] > margin * tol)


Shared = collections.namedtuple("Shared", "shape B P c A b G h")


@functools.lru_cache(maxsize=None)
def shared_batch(name, nb, seed=20261020):
    """A parametric batch: ONE P, A and G, and per problem c, b, h around its
    own strictly feasible pair (tests/shared_cases.py's construction plus P)."""
    from shared_cases import interior
    sh = SHAPES[name]
    cones, n, m, k, _ = sh
    rng = np.random.default_rng(seed)
    A, G = rng.standard_normal((m, n)), rng.standard_normal((k, n))
    R = rng.standard_normal((n // 2, n))
    Pm = R.T @ R / n
    x0, y0 = rng.standard_normal((nb, n)), rng.standard_normal((nb, m))
    s0, z0 = interior(rng, cones, nb, k), interior(rng, cones, nb, k)
    flat = lambda M: np.ascontiguousarray(M).reshape(-1)  # noqa: E731
    col = lambda M: np.ascontiguousarray(M.ravel(order="F"))  # noqa: E731
    return Shared(sh, nb, col(Pm), flat(-(y0 @ A + z0 @ G) - x0 @ Pm), col(A), flat(x0 @ A.T), col(G),
                  flat(x0 @ G.T + s0))


def soc_projection(a):
    """Euclidean projection of a onto the second-order cone {(t, u): t >= |u|}."""
    t, u = a[0], a[1:]
    nu = np.linalg.norm(u)
    if nu <= t:
        return a.copy()
    if nu <= -t:
        return np.zeros_like(a)
    f = (t + nu) / 2.0
    return np.concatenate([[f], f * u / nu])


@functools.lru_cache(maxsize=None)
def projection_batch(n=64, nb=16, seed=7):
    """min |x - a|^2 / 2 over one second-order cone of n rows, as a QP:
    P = I, G = -I, h = 0, c = -a, m = 0.  a: one point inside K, one inside -K,
    the rest standard normal.  Returns (cones, a[nb, n], flat P, c, G, h)."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((nb, n))
    a[0, 0] = np.linalg.norm(a[0, 1:]) + 1.0
    a[1, 0] = -np.linalg.norm(a[1, 1:]) - 1.0
    eye = np.eye(n).ravel()
    return ((Q_, 0, n),), a, np.tile(eye, nb), -a.reshape(-1), np.tile(-eye, nb), np.zeros(nb * n)
