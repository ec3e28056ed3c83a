"""SOCP_F_NORMALISE: a numpy restatement of the rule of include/socp.h and the
batches of tests/test_normalise_cpu.py and tests/test_gpu_normalise.py.

The rule, per problem: nc = max |c_j|, nb = max(max |b_i|, max |h_i|) (no b
term when m = 0); e(v) = -ilogb(v) for v finite and > 0, clamped to +-256, and
0 for every other v (zero, Inf, NaN anywhere in the vector); ec = e(nc),
eb = e(nb).  c^ = ldexp(c, ec), (b^, h^) = ldexp((b, h), eb), P^ = ldexp(P,
ec - eb); x^ = ldexp(x, eb), s^ = ldexp(s, eb), y^ = ldexp(y, ec), z^ =
ldexp(z, ec).  With shared matrices and a P the two norms are the maxima over
the whole batch.

``np.frexp`` returns v = f 2^q with f in [1/2, 1), subnormals included, so
ilogb(v) = q - 1.
"""
import collections
import functools

import numpy as np

import qp_cases as Q
from infeasible import feasible_problem

CLAMP = 256
TOL = 1e-5
NB = 16  # problems per solver batch


def e_of(v):
    """e(v) of one norm; NaN stands for "a NaN or an Inf somewhere in the vector"."""
    if not (np.isfinite(v) and v > 0):
        return 0
    return int(min(CLAMP, max(-CLAMP, 1 - int(np.frexp(v)[1]))))


def norm_of(*vectors):
    """The max-norm of the vectors together; NaN when any entry is a NaN or an Inf."""
    v = np.concatenate([np.abs(np.asarray(q, dtype=np.float64)).reshape(-1) for q in vectors])
    if not np.isfinite(v).all():
        return np.nan
    return float(v.max()) if v.size else 0.0


def exponents(n, m, k, c, b, h, batchwide=False):
    """expo[B, 2] = (ec, eb) per problem; batchwide: one pair from the maxima over the batch."""
    B = len(c) // n
    c, h = np.reshape(c, (B, n)), np.reshape(h, (B, k))
    b = np.reshape(b, (B, m)) if m else np.zeros((B, 0))
    if batchwide:
        pair = (e_of(norm_of(c)), e_of(norm_of(b, h)))
        return np.tile(np.array(pair, np.int32), (B, 1))
    return np.array([(e_of(norm_of(c[p])), e_of(norm_of(b[p], h[p]))) for p in range(B)], np.int32).reshape(B, 2)


Scaled = collections.namedtuple("Scaled", "expo c b h P")


def restate(n, m, k, c, b, h, P=None, shared=False):
    """The rule on flat arrays in the layout of include/socp.h (P: B matrices,
    or ONE with shared, which then takes the batch-wide pair)."""
    B = len(c) // n
    ex = exponents(n, m, k, c, b, h, batchwide=shared and P is not None)
    ec, eb = ex[:, 0].astype(np.int64), ex[:, 1].astype(np.int64)
    row = lambda v, w, e: np.ldexp(np.reshape(v, (B, w)), e[:, None]).reshape(-1)  # noqa: E731
    Ps = None
    if P is not None:
        MB = 1 if shared else B
        Ps = np.ldexp(np.reshape(P, (MB, n * n)), (ec - eb)[:MB, None]).reshape(-1)
    return Scaled(ex, row(c, n, ec), row(b, m, eb) if m else np.zeros(0), row(h, k, eb), Ps)


def scale_iterate(expo, n, m, k, x, y, z, s, sign=1):
    """sign = 1: the forward map of an iterate; -1: the unscaling."""
    B = expo.shape[0]
    ec, eb = sign * expo[:, 0].astype(np.int64), sign * expo[:, 1].astype(np.int64)
    row = lambda v, w, e: np.ldexp(np.reshape(v, (B, w)), e[:, None]).reshape(-1)  # noqa: E731
    return row(x, n, eb), (row(y, m, ec) if m else np.zeros(0)), row(z, k, ec), row(s, k, eb)


# ------------------------------------------------------------ rule batches
# (id, n, m, k) of the shapes socp_batch_normalise is checked on
RULE_SHAPES = dict(s8=(8, 2, 16), m0=(8, 0, 16), c1=(32, 8, 48), long=(16, 4, 1200))

Rule = collections.namedtuple("Rule", "n m k B c b h P")


@functools.lru_cache(maxsize=None)
def rule_batch(name, B, seed=5):
    """B problems whose per-problem exponents all differ (problem p's c is
    standard normal times 2^(3p - 40), its (b, h) times 2^(25 - 2p)); the
    largest entry of c is its last and negative, that of (b, h) the last of h
    and negative.  From B >= 5 on, problem 1 has c = 0, problem 2 a NaN in h,
    problem 3 an Inf in c and problem 4 a c of subnormals only."""
    n, m, k = RULE_SHAPES[name]
    rng = np.random.default_rng(seed)
    c, b, h = rng.standard_normal((B, n)), rng.standard_normal((B, m)), rng.standard_normal((B, k))
    c[:, -1] = -(np.abs(c).max(axis=1) + 0.25)
    h[:, -1] = -(max(np.abs(b).max(initial=0.0), np.abs(h).max()) + 0.25)
    p = np.arange(B)
    c, b, h = np.ldexp(c, (3 * p - 40)[:, None]), np.ldexp(b, (25 - 2 * p)[:, None]), np.ldexp(h, (25 - 2 * p)[:, None])
    if B >= 5:
        c[1] = 0.0
        h[2, k // 2] = np.nan
        c[3, 0] = np.inf
        c[4] = np.ldexp(rng.standard_normal(n), -1070)  # below 2^-1022 every one
        assert (np.abs(c[4]) < 2.0 ** -1022).all() and (c[4] != 0).any()
    R = rng.standard_normal((B, n, n))
    P = R + R.transpose(0, 2, 1)
    return Rule(n, m, k, B, c.reshape(-1), b.reshape(-1), h.reshape(-1), P.reshape(-1))


# ---------------------------------------------------------- solver batches
def scaled_by(d, a, b):
    """A qp_cases.Batch with c multiplied by 2^a, (b, h) by 2^b and P by
    2^(a - b); a and b are ints or one int per problem."""
    cones, n, m, k, _ = d.shape
    a = np.broadcast_to(np.asarray(a, np.int64), (d.B,))
    b = np.broadcast_to(np.asarray(b, np.int64), (d.B,))
    row = lambda v, w, e: np.ldexp(np.reshape(v, (d.B, w)), e[:, None]).reshape(-1)  # noqa: E731
    P = None if d.P is None else row(d.P, n * n, a - b)
    probs = []
    for p, pr in enumerate(d.probs):
        probs.append((None if pr[0] is None else np.ldexp(pr[0], a[p] - b[p]), np.ldexp(pr[1], a[p]), pr[2],
                      np.ldexp(pr[3], b[p]), pr[4], np.ldexp(pr[5], b[p])))
    return Q.Batch(d.shape, d.B, P, row(d.c, n, a), d.A, row(d.b, m, b) if m else d.b, d.G, row(d.h, k, b), d.sing,
                   probs)


# the seed of the linear batches; c1's gives a batch of which at least 3/4 is
# clear under the normalised reference (tests/test_normalise_cpu.py checks it)
LINEAR_SEED = 3


@functools.lru_cache(maxsize=None)
def linear_batch(name, nb=NB, seed=LINEAR_SEED):
    """nb strictly feasible linear problems of qp_cases.SHAPES[name] from
    tests/infeasible.py's feasible_problem, as a qp_cases.Batch with P = None
    and probs[p] = (None, c, A, b, G, h)."""
    sh = Q.SHAPES[name]
    cones, n, m, k, sing = sh
    rng = np.random.default_rng(seed)
    probs = [(None,) + feasible_problem(rng, cones, n, m, k)[0] for _ in range(nb)]
    cat = lambda i, mat: np.concatenate([(p[i].ravel(order="F") if mat else p[i]) for p in probs])  # noqa: E731
    return Q.Batch(sh, nb, None, cat(1, False), cat(2, True) if m else np.zeros(0), cat(3, False) if m else np.zeros(0),
                   cat(4, True), cat(5, False), np.full(nb, sing, np.uint8), probs)


@functools.lru_cache(maxsize=None)
def batch(name, qp, a=0, b=0, nb=NB):
    """The linear (qp=False) or quadratic (qp_cases.batch) batch of a shape, scaled by (2^a, 2^b)."""
    return scaled_by(Q.batch(name, nb) if qp else linear_batch(name, nb), a, b)


def normalised(d):
    """The batch the flagged solve hands to the kernels, and its exponents."""
    cones, n, m, k, _ = d.shape
    sc = restate(n, m, k, d.c, d.b, d.h, d.P)
    return scaled_by(d, sc.expo[:, 0], sc.expo[:, 1]), sc.expo


def linear_reference(O, cones, prob, sing, maxit=40, tol=TOL):
    """oracle.solve_trace in the kernels' operation order on one linear problem,
    in qp_cases.qp_reference's form: exits[t] is the exit sum at the start of
    iteration t, formed in numpy from the trace."""
    _, c, A, b, G, h = prob
    r = O.solve_trace(list(cones), c, A, b, G, h, sing=sing,
                      params=O.Params(maxit=maxit, tol=tol, flags=O.F_STRUCTURED | O.F_CHOLSOLVE))
    zero = np.zeros((len(c), len(c)))
    r["exits"] = [sum(Q.exit_terms((zero, c, A, b, G, h), *it)) for it in r["trace"]]
    return r


def _qp_reference(cones, prob, sing):
    """qp_cases.qp_reference; an H that is no longer finite (numpy's cond raises
    on it before the Cholesky is tried) counts as the failed factorisation it is."""
    try:
        return Q.qp_reference(cones, prob, sing)
    except np.linalg.LinAlgError:
        return dict(status=2, iters=-1, exits=[])


@functools.lru_cache(maxsize=None)
def reference(name, qp, a=0, b=0, normalise=True, nb=NB):
    """The CPU reference on every problem of batch(name, qp, a, b), normalised
    by the restatement first or as given: qp_cases.qp_reference for the
    quadratic batches, the oracle for the linear ones.  Computed once."""
    import oracle as O
    d = batch(name, qp, a, b, nb)
    if normalise:
        d, _ = normalised(d)
    cones, sing = d.shape.cones, bool(d.shape.sing)
    if qp:
        return [_qp_reference(cones, p, sing) for p in d.probs]
    return [linear_reference(O, cones, p, sing) for p in d.probs]


def unscaled(refs, expo, n, m, k):
    """x, y, z, s of a normalised batch's references, mapped back to the caller's units (flat)."""
    cat = lambda key: np.concatenate([np.asarray(r[key], dtype=np.float64) for r in refs])  # noqa: E731
    return scale_iterate(expo, n, m, k, cat("x"), cat("y"), cat("z"), cat("s"), sign=-1)
