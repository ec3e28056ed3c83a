"""SOCP_F_EQUILIBRATE: the numpy restatement of the scaling rule, and the cases.

The rule (include/socp.h, socp_batch_equilibrate).  Integer exponents ed[n],
ee[m], ef[k] start at 0; D = 2^ed, E = 2^ee, F = 2^ef.  Each pass:
  scaled magnitudes ldexp(|A|, ee_i + ed_j), ldexp(|G|, ef_i + ed_j) and, with a
  P, ldexp(|P|, ed_i + ed_j) -- one ldexp each, so exact up to one rounding
  where a result is subnormal;
  cn_j the max over column j of all of them, ra_i / rg_i the row maxima of A /
  G; every row of an SOC cone gets the max of the cone's rg;
  a norm v finite and > 0 gives t = -floor((ilogb(v) + 1) / 2), any other 0;
  ed += t(cn), ee += t(ra), ef += t(rg), clamped to [-256, 256], all from the
  same pass's norms.
np.max propagates NaN, so a NaN entry freezes its row and its column, as an Inf
does.  ilogb comes from np.frexp (v = f 2^e with f in [1/2, 1): ilogb = e - 1),
not from log2.

Everything below is float64 / int64 numpy on matrices (rows x columns); the
flat arrays of a batch are in the layout of include/socp.h.
"""
import collections
import functools

import numpy as np

import oracle as O

P_, Q_ = 0, 1  # cone kinds of include/socp.h: POC, SOC
CLAMP = 256
PASSES = 8


def t_of(v):
    """The exponent increment of every norm in v."""
    v = np.asarray(v, dtype=np.float64)
    t = np.zeros(v.shape, np.int64)
    ok = np.isfinite(v) & (v > 0)
    _, e = np.frexp(v[ok])
    t[ok] = -(e.astype(np.int64) // 2)  # -floor((ilogb + 1) / 2), ilogb = e - 1
    return t


def norms(cones, Pm, A, G, ed, ee, ef):
    """(cn, ra, rg) of one pass; rg after the cone aggregation."""
    k, n = G.shape
    m = A.shape[0]
    Gh = np.ldexp(np.abs(G), ef[:, None] + ed[None, :])
    cn = Gh.max(axis=0)
    rg = Gh.max(axis=1)
    ra = np.zeros(0)
    if m:
        Ah = np.ldexp(np.abs(A), ee[:, None] + ed[None, :])
        cn = np.maximum(cn, Ah.max(axis=0))  # (np.maximum propagates NaN too)
        ra = Ah.max(axis=1)
    if Pm is not None:
        cn = np.maximum(cn, np.ldexp(np.abs(Pm), ed[:, None] + ed[None, :]).max(axis=0))
    for kind, o, d in cones:
        if kind == Q_:
            rg[o:o + d] = rg[o:o + d].max()
    return cn, ra, rg


def exponents(cones, Pm, A, G, passes=PASSES):
    """(ed, ee, ef) of one matrix set.  A is m x n (m may be 0), Pm n x n or None."""
    k, n = G.shape
    m = A.shape[0]
    ed, ee, ef = np.zeros(n, np.int64), np.zeros(m, np.int64), np.zeros(k, np.int64)
    for _ in range(passes):
        cn, ra, rg = norms(cones, Pm, A, G, ed, ee, ef)
        ed = np.clip(ed + t_of(cn), -CLAMP, CLAMP)
        ee = np.clip(ee + t_of(ra), -CLAMP, CLAMP)
        ef = np.clip(ef + t_of(rg), -CLAMP, CLAMP)
    return ed, ee, ef


def scale_set(Pm, A, G, ed, ee, ef):
    """(P^, A^, G^) = (D P D, E A D, F G D)."""
    return (None if Pm is None else np.ldexp(Pm, ed[:, None] + ed[None, :]),
            np.ldexp(A, ee[:, None] + ed[None, :]), np.ldexp(G, ef[:, None] + ed[None, :]))


# ------------------------------------------------------------------ batches
Shape = collections.namedtuple("Shape", "cones n m k")
SHAPES = dict(
    m0=Shape(((P_, 0, 3), (Q_, 3, 4)), 5, 0, 7),                          # no equalities
    s16=Shape(((P_, 0, 8), (Q_, 8, 8), (Q_, 16, 8)), 16, 4, 24),
    two=Shape(((P_, 0, 32), (Q_, 32, 32), (Q_, 64, 32)), 32, 8, 96),      # k > 64: the register kernel's two slots
    # the blocked kernel (n > 64); an SOC cone over rows 60..69 (a wavefront edge) and one over rows
    # 250..262 (the scaling kernel's 256-thread stride); the cone between them spans three wavefronts
    blk=Shape(((P_, 0, 60), (Q_, 60, 10), (Q_, 70, 180), (Q_, 250, 13), (Q_, 263, 37)), 70, 3, 300),
    # k above the scaling kernel's 4096-row LDS table of F's exponents (socp_batch_equilibrate only)
    tall=Shape(((P_, 0, 4000), (Q_, 4000, 101)), 3, 1, 4101),
)
B = 33  # more than one wavefront's worth of nothing in particular: odd, and > 32

# One batch in the flat layout; P is None or flat; MB = number of matrix sets (1: shared)
Batch = collections.namedtuple("Batch", "shape B MB P c A b G h")


def _pow2(rng, spread, size):
    return rng.integers(-spread, spread + 1, size)


def cone_exponents(rng, cones, k, spread):
    """Random row exponents, one per SOC cone (the same problem in other units)."""
    f = _pow2(rng, spread, k)
    for kind, o, d in cones:
        if kind == Q_:
            f[o:o + d] = f[o]
    return f


def mats(d, p):
    """(P, A, G) of matrix set p of a Batch as matrices (views of copies)."""
    cones, n, m, k = d.shape
    A = d.A[p * m * n:(p + 1) * m * n].reshape(n, m).T
    G = d.G[p * k * n:(p + 1) * k * n].reshape(n, k).T
    Pm = None if d.P is None else d.P[p * n * n:(p + 1) * n * n].reshape(n, n).T
    return Pm, A, G


def flat(M):
    return np.ascontiguousarray(M.ravel(order="F"))


@functools.lru_cache(maxsize=None)
def bad_batch(name, nb=B, seed=2, spread=12, with_P=False):
    """Generator problems (the oracle's restatement of socp_generate, `seed`)
    whose rows and columns are multiplied by powers of two within 2^+-spread
    drawn from default_rng(seed), one factor per SOC cone: the same problems in
    other units.  with_P adds P = R'R / n in the same units (D^-1-free: P is
    scaled like a Hessian in x's units, Dc P Dc)."""
    sh = SHAPES[name]
    cones, n, m, k = sh
    g = O.generate(list(cones), nb, n, m, k, seed)
    rng = np.random.default_rng(seed)
    c, A, b, G, h = (np.array(g[q], dtype=np.float64) for q in "cAbGh")
    Pf = np.zeros(nb * n * n) if with_P else None
    for p in range(nb):
        dc, er, fr = _pow2(rng, spread, n), _pow2(rng, spread, m), cone_exponents(rng, cones, k, spread)
        Am = A[p * m * n:(p + 1) * m * n].reshape(n, m).T
        Gm = G[p * k * n:(p + 1) * k * n].reshape(n, k).T
        A[p * m * n:(p + 1) * m * n] = flat(np.ldexp(Am, er[:, None] + dc[None, :]))
        G[p * k * n:(p + 1) * k * n] = flat(np.ldexp(Gm, fr[:, None] + dc[None, :]))
        c[p * n:(p + 1) * n] = np.ldexp(c[p * n:(p + 1) * n], dc)
        b[p * m:(p + 1) * m] = np.ldexp(b[p * m:(p + 1) * m], er)
        h[p * k:(p + 1) * k] = np.ldexp(h[p * k:(p + 1) * k], fr)
        if with_P:
            R = rng.standard_normal((max(n // 2, 1), n))
            Pf[p * n * n:(p + 1) * n * n] = flat(np.ldexp(R.T @ R / n, dc[:, None] + dc[None, :]))
    return Batch(sh, nb, nb, Pf, c, A, b, G, h)


@functools.lru_cache(maxsize=None)
def shared_batch(name, nb=B, seed=5, spread=12, with_P=False):
    """A parametric batch: the matrices of bad_batch's problem 0 for every
    problem, with c, b, h of that batch (b and h are then not those of a known
    feasible point; the bitwise contracts do not need one)."""
    d = bad_batch(name, nb, seed, spread, with_P)
    cones, n, m, k = d.shape
    return Batch(d.shape, nb, 1, None if d.P is None else d.P[:n * n].copy(), d.c, d.A[:m * n].copy(), d.b,
                 d.G[:k * n].copy(), d.h)


@functools.lru_cache(maxsize=None)
def decorated_batch(name, with_P=False):
    """bad_batch with, in problem 0 a zero column (A, G and P) and a zero POC
    row, in problem 1 one NaN entry, in problem 2 one Inf entry, in problem 3 a
    subnormal-only row (the last row of G, inside an SOC cone: the cone's max
    decides), in problem 4 a subnormal-only POC row."""
    d = bad_batch(name, 8, 3, 12, with_P)
    cones, n, m, k = d.shape
    G, A = d.G.copy(), d.A.copy()
    Pf = None if d.P is None else d.P.copy()
    Gv = lambda p: G[p * k * n:(p + 1) * k * n].reshape(n, k)  # noqa: E731  (transposed views: [column, row])
    Gv(0)[1, :] = 0.0
    Gv(0)[:, 0] = 0.0
    if m:
        A[0 * m * n:1 * m * n].reshape(n, m)[1, :] = 0.0
    if Pf is not None:
        Pf[:n * n].reshape(n, n)[1, :] = 0.0
        Pf[:n * n].reshape(n, n)[:, 1] = 0.0
    Gv(1)[2, min(5, k - 1)] = np.nan
    if m:
        A[2 * m * n:3 * m * n].reshape(n, m)[n - 1, m - 1] = -np.inf
    else:
        Gv(2)[n - 1, 1] = -np.inf
    tiny = 5e-324
    Gv(3)[:, k - 1] = tiny * np.arange(1, n + 1) * (-1.0) ** np.arange(n)
    Gv(4)[:, 2] = tiny * np.arange(n, 0, -1)
    return Batch(d.shape, d.B, d.MB, Pf, d.c, A, d.b, G, d.h)


@functools.lru_cache(maxsize=None)
def ones_batch(name="s16", nb=B, seed=9):
    """Strictly feasible problems whose every |A_ij| and |G_ij| lies in [1/2, 1):
    every norm does, so every increment is 0 and all factors are 1."""
    from infeasible import interior_point
    sh = SHAPES[name]
    cones, n, m, k = sh
    rng = np.random.default_rng(seed)
    out = dict(c=[], A=[], b=[], G=[], h=[])
    for _ in range(nb):
        A = rng.uniform(0.5, 1.0, (m, n)) * rng.choice([-1.0, 1.0], (m, n))
        G = rng.uniform(0.5, 1.0, (k, n)) * rng.choice([-1.0, 1.0], (k, n))
        s, z = interior_point(rng, cones, k), interior_point(rng, cones, k)
        x, y = rng.standard_normal(n), rng.standard_normal(m)
        out["c"].append(-(A.T @ y + G.T @ z))
        out["A"].append(flat(A))
        out["b"].append(A @ x)
        out["G"].append(flat(G))
        out["h"].append(G @ x + s)
    return Batch(sh, nb, nb, None, *(np.concatenate(out[q]) for q in "cAbGh"))


@functools.lru_cache(maxsize=None)
def spread20_batch(name="s16", nb=4, seed=0):
    """Standard-normal matrices with every row and every column multiplied by
    its own power of two within 2^+-20 (one per SOC cone): 6 passes reach the
    fixed point, 4 do not."""
    sh = SHAPES[name]
    cones, n, m, k = sh
    rng = np.random.default_rng(seed)
    As, Gs = [], []
    for _ in range(nb):
        dc = _pow2(rng, 20, n)
        As.append(flat(np.ldexp(rng.standard_normal((m, n)), _pow2(rng, 20, m)[:, None] + dc[None, :])))
        Gs.append(flat(np.ldexp(rng.standard_normal((k, n)), cone_exponents(rng, cones, k, 20)[:, None] + dc[None, :])))
    z = np.zeros
    return Batch(sh, nb, nb, None, z(nb * n), np.concatenate(As), z(nb * m), np.concatenate(Gs), z(nb * k))


@functools.lru_cache(maxsize=None)
def tall_batch(nb=2, seed=4):
    """k = 4101: F's exponents leave the scaling kernel's LDS table."""
    sh = SHAPES["tall"]
    cones, n, m, k = sh
    rng = np.random.default_rng(seed)
    A = np.ldexp(rng.standard_normal((nb, n, m)), _pow2(rng, 12, (nb, n, m)))
    G = np.ldexp(rng.standard_normal((nb, n, k)), _pow2(rng, 12, (nb, n, k)))
    return Batch(sh, nb, nb, None, rng.standard_normal(nb * n), A.reshape(-1), rng.standard_normal(nb * m),
                 G.reshape(-1), rng.standard_normal(nb * k))


Scaled = collections.namedtuple("Scaled", "ed ee ef D E F P c A b G h")


def restate(d, passes=PASSES):
    """The restatement on a whole Batch: exponents (MB x n, m, k), the factors
    as doubles and every scaled array, flat."""
    cones, n, m, k = d.shape
    ed, ee, ef = np.zeros((d.MB, n), np.int64), np.zeros((d.MB, m), np.int64), np.zeros((d.MB, k), np.int64)
    Ps, As, Gs = [], [], []
    for p in range(d.MB):
        Pm, A, G = mats(d, p)
        ed[p], ee[p], ef[p] = exponents(cones, Pm, A, G, passes)
        Ph, Ah, Gh = scale_set(Pm, A, G, ed[p], ee[p], ef[p])
        As.append(flat(Ah))
        Gs.append(flat(Gh))
        if Pm is not None:
            Ps.append(flat(Ph))
    per = lambda e: e if d.MB == d.B else np.broadcast_to(e, (d.B, e.shape[1]))  # noqa: E731
    one = np.ones(1)
    return Scaled(ed, ee, ef, np.ldexp(one, ed).reshape(-1), np.ldexp(one, ee).reshape(-1),
                  np.ldexp(one, ef).reshape(-1), np.concatenate(Ps) if Ps else None,
                  np.ldexp(d.c.reshape(d.B, n), per(ed)).reshape(-1), np.concatenate(As),
                  np.ldexp(d.b.reshape(d.B, m), per(ee)).reshape(-1), np.concatenate(Gs),
                  np.ldexp(d.h.reshape(d.B, k), per(ef)).reshape(-1))


def unscale(d, sc, x, y, z, s):
    """x = D x^, y = E y^, z = F z^, s = F^-1 s^ on flat batch-major arrays."""
    cones, n, m, k = d.shape
    per = lambda e: e if d.MB == d.B else np.broadcast_to(e, (d.B, e.shape[1]))  # noqa: E731
    return (np.ldexp(x.reshape(d.B, n), per(sc.ed)).reshape(-1), np.ldexp(y.reshape(d.B, m), per(sc.ee)).reshape(-1),
            np.ldexp(z.reshape(d.B, k), per(sc.ef)).reshape(-1), np.ldexp(s.reshape(d.B, k), -per(sc.ef)).reshape(-1))


def same_bits(u, v):
    """Bitwise equality of two arrays, except that a NaN matches any NaN (IEEE
    754 leaves the payload of ldexp(NaN) to the implementation)."""
    u, v = np.asarray(u), np.asarray(v)
    if u.shape != v.shape or u.dtype != v.dtype:
        return False
    if u.dtype != np.float64:
        return u.tobytes() == v.tobytes()
    nu, nv = np.isnan(u), np.isnan(v)
    return bool(np.array_equal(nu, nv) and np.array_equal(u.view(np.uint64)[~nu], v.view(np.uint64)[~nv]))
