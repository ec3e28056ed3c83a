"""Cases, inputs and the reference of the blocked kernel's KKT plugin entries
(test_kkt_cases_cpu.py, test_gpu_large_kkt.py): socp_batch_kkt_solve
(MODE_KKT) and socp_dense_setup_iter / socp_dense_solve_kkt (MODE_SETUP,
MODE_SOLVEKKT against per-problem records) at shapes only socp_large.hip takes.

The reference is not the oracle.  It is the KKT block system itself,

    A'cy + G'cz                = dx
    A cx                       = dy
    G cx + cs                  = dz
    lam o (W cz + W^-T cs)     = ds

in the unknowns u = (cx, cy, cz, cs): W, W^-1 and lam from
oracle.compute_scaling (both matrices are written down entry by entry from
w-bar and mu, scalings.jl:60-95: no inversion; iwiw=False skips the k^3 product
iW iW' that the reference forms next), the arrow operator of lam built
blockwise, the (n + m + 2k)-square matrix K factored once by LU in fp64 and
the solution refined with residuals formed in np.longdouble until the
correction stops shrinking.  It knows nothing of H, S or any operation order.

`sing` problems (H = G'W^-2 G + A'A, densesolver.jl:66-85 with m0 = dy - cy
and n0 += A'dy): with dy != 0 that formula does NOT solve the block system --
its cx leaves A cx - dy of dy's own size; at m65's shape with G's right half
zero the oracle's cx is 6e-3 .. 6e-2 relative from the block system's (cy, cz
and cs agree: G does not see the columns in which cx differs).  With dy = 0 both agree to rounding.  That is the reference's own
behaviour (harmless in the solver, where dy is the primal residual and goes to
zero), restated by the oracle and mirrored by the kernels; it is not to be
"fixed".  So a sing case is gated against the block system with dy = 0, and
run once more with dy != 0 against oracle.kkt_single(sing=True) in the
kernel's operation order.

The table: (n, m, k, cones, flags), each the smallest shape that reaches its
branch of socp_large.hip.  `kernel` is the name socp_last_kernel_name must
report; gv_kernel() restates large_layout's LDS arithmetic (the vectors go to
the HBM workspace when they exceed 160 KiB), and test_kkt_cases_cpu.py holds
every case to it, so no listed shape had to move.

Inputs: G and A standard normal, seeded from (n, m, k); (s, z) interior points
(POC entries in (0.3, 2), SOC heads above the tail norm by 0.2 .. 1); two
standard normal right-hand sides; B = 2 problems.  Singular cases zero G's
columns n//2.. (m >= n - n//2 keeps [G; A] of full column rank).
"""
import collections
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))

P_, Q_ = 0, 1  # cone kinds of include/socp.h: POC, SOC
B = 2
NRHS = 2
U = 2.0 ** -53
MAXC = 64  # socp_small.hpp: cone table size
LDS_BYTES = 160 * 1024

Case = collections.namedtuple("Case", "id n m k cones sing xi kernel")


def _table(*dims):
    """(kind, dim) pairs -> ((kind, offs, dim), ...)"""
    out, o = [], 0
    for kind, d in dims:
        out.append((kind, o, d))
        o += d
    return tuple(out)


def _small_cones():
    """POC 8 + SOC cones of 2, 3, 3, 2, 3, 3, ...: 72 rows in 27 cones (28 with the POC)."""
    dims = [(P_, 8)]
    left = 72
    while left:
        for d in (2, 3, 3):
            dims.append((Q_, d))
            left -= d
    return _table(*dims)


_EDGE = _table((P_, 10), (Q_, 56))
_M65 = _table((P_, 40), *[(Q_, 16)] * 10)
_WIDE = _table((Q_, 260), (Q_, 260))
_GV = _table((P_, 100), *[(Q_, 100)] * 10)

# sing: 0 / 1 the byte passed, None the device probe (which must find 1 here)
CASES = [
    # one column past a 64-block, m = 1
    Case("edge65", 65, 1, 66, _EDGE, 0, False, "socp_large_kernel"),
    # no equality rows; three ragged SOC cones
    Case("m0", 70, 0, 90, _table((Q_, 29), (Q_, 30), (Q_, 31)), 0, False, "socp_large_kernel"),
    # MPAD = 128: S spans two panels; 11 cones (> 8)
    Case("m65", 130, 65, 200, _M65, 0, False, "socp_large_kernel"),
    # G's right half zero: A'A in H, the At_dot term, m0 = dy - cy
    Case("sing", 130, 65, 200, _M65, 1, False, "socp_large_kernel"),
    # the same inputs, sing = NULL: the probe factors G'G with the matrix pointers at the record
    Case("probe", 130, 65, 200, _M65, None, False, "socp_large_kernel"),
    # tiny SOC cones, many of them
    Case("smallcones", 66, 4, 80, _small_cones(), 0, False, "socp_large_kernel"),
    # NPAD = 512 exactly: the last size factored without windows
    Case("n512", 512, 64, 528, _table((P_, 16), *[(Q_, 128)] * 4), 0, False, "socp_large_kernel"),
    # NPAD = 576: chol_wide / panel_chol_wide, then trsv against the factor in the record
    Case("wide", 513, 20, 520, _WIDE, 0, False, "socp_large_kernel"),
    # the vectors in the HBM workspace: load_record / store_record through gvec
    Case("gv", 80, 0, 1100, _GV, 0, False, "socp_large_gv_kernel"),
    # both
    Case("gv_wide", 513, 20, 900, _table((P_, 100), *[(Q_, 100)] * 8), 0, False, "socp_large_gv_kernel"),
    # MPAD = 576: S = L_S L_S' applied by two triangular solves on the record's Sm (GV by its size)
    Case("mwide", 600, 513, 640, _table((P_, 40), *[(Q_, 150)] * 4), 0, False, "socp_large_gv_kernel"),
    # SOCP_F_EXPLICIT_INVERSE: Li, Li A', S^-1 in the record
    Case("xi", 65, 1, 66, _EDGE, 0, True, "socp_large_xi_kernel"),
    Case("xi_wide", 513, 20, 520, _WIDE, 0, True, "socp_large_xi_kernel"),
    Case("xi_gv", 80, 0, 1100, _GV, 0, True, "socp_large_xi_gv_kernel"),
]
BY_ID = {c.id: c for c in CASES}


def case_id(c):
    return c.id


def singular(c):
    """Whether the problem runs the sing formulas (the probe finds G'G singular)."""
    return c.sing != 0


def sing_bytes(c, nb=B):
    return None if c.sing is None else np.full(nb, c.sing, np.uint8)


def gv_kernel(n, m, k):
    """large_layout's LDS total (socp_kernels.hpp) against a CU's 160 KiB, as
    socp_api.hip large_fits decides between the LDS and the GV kernels."""
    NPAD = (n + 63) // 64 * 64
    MPAD = (max(m, 1) + 63) // 64 * 64
    KP = (k + 15) // 16 * 16
    RW = max(NPAD, MPAD)
    o = 7 * KP + max(2 * RW, 1024) + 64 + 8 * MPAD
    # (the staged SYRK's padding to 16 NPAD at NPAD 256 / 512 is dropped by the layout when it would not fit)
    o += 8 * KP + KP + 12 * MAXC + 6 * NPAD + 5 * MPAD + 64 + 8 * 64
    return o * 8 + 64 > LDS_BYTES


def kernel_name(n, m, k, xi):
    return "socp_large_%s%skernel" % ("xi_" if xi else "", "gv_" if gv_kernel(n, m, k) else "")


def interior(rng, cones, nb, k):
    """nb interior points of the cone product (test_gpu_sqr.py's _interior)."""
    v = np.zeros((nb, k))
    for kind, o, d in cones:
        if kind == P_:
            v[:, o:o + d] = rng.uniform(0.3, 2.0, (nb, d))
        else:
            v[:, o + 1:o + d] = rng.uniform(-0.4, 0.4, (nb, d - 1))
            v[:, o] = np.linalg.norm(v[:, o + 1:o + d], axis=1) + rng.uniform(0.2, 1.0, nb)
    return v


def make_inputs(n, m, k, cones, zero_right, nb, dy_zero=()):
    """A (nb, m, n), G (nb, k, n), s, z (nb, k), rhs[j] = (dx, dy, dz, ds) with
    rows per problem.  zero_right: per problem, whether G's columns n//2.. are
    zeroed; dy_zero: the problems whose dy is 0."""
    rng = np.random.default_rng([n, m, k])
    G = rng.standard_normal((nb, k, n))
    A = rng.standard_normal((nb, m, n))
    for p in range(nb):
        if zero_right[p]:
            G[p][:, n // 2:] = 0.0
    s, z = interior(rng, cones, nb, k), interior(rng, cones, nb, k)
    rhs = []
    for _ in range(NRHS):
        r = [rng.standard_normal((nb, q)) for q in (n, m, k, k)]
        for p in dy_zero:
            r[1][p] = 0.0
        rhs.append(tuple(r))
    return dict(A=A, G=G, s=s, z=z, rhs=rhs)


@functools.lru_cache(maxsize=None)
def _inputs(n, m, k, cones, zero, dy0):
    return make_inputs(n, m, k, cones, (zero,) * B, B, range(B) if dy0 else ())


def inputs(c, dy0=None):
    """The case's batch.  Singular cases carry dy = 0 unless dy0=False (the run
    against the oracle's sing formula)."""
    if dy0 is None:
        dy0 = singular(c)
    return _inputs(c.n, c.m, c.k, c.cones, singular(c), bool(dy0))


def flat(d, nb=None):
    """The library's layout: column-major matrices, problems one after the other."""
    nb = len(d["G"]) if nb is None else nb
    Af = np.concatenate([d["A"][p].ravel(order="F") for p in range(nb)]) if d["A"].shape[1] else None
    Gf = np.concatenate([d["G"][p].ravel(order="F") for p in range(nb)])
    return Af, Gf


def flat_rhs(d, j, m):
    dx, dy, dz, ds = d["rhs"][j]
    return dx.ravel(), (dy.ravel() if m else None), dz.ravel(), ds.ravel()


# ------------------------------------------------------------------ reference
def arrow(cones, lam):
    """Arw(lam): vprod(lam, v) = Arw(lam) v, blockwise (POC: diag; SOC: [[l0, l1'], [l1, l0 I]])."""
    k = len(lam)
    M = np.zeros((k, k))
    for kind, o, d in cones:
        if kind == P_:
            M[np.arange(o, o + d), np.arange(o, o + d)] = lam[o:o + d]
        else:
            M[np.arange(o, o + d), np.arange(o, o + d)] = lam[o]
            M[o, o:o + d] = lam[o:o + d]
            M[o:o + d, o] = lam[o:o + d]
    return M


def kkt_matrix(cones, A, G, s, z):
    """K of the block system above at (s, z); unknowns (cx, cy, cz, cs)."""
    import oracle
    k, n = G.shape
    m = A.shape[0]
    sc = oracle.compute_scaling(list(cones), s, z, iwiw=False)
    assert sc["status"] == 0
    Arw = arrow(cones, sc["l"])
    N = n + m + 2 * k
    K = np.zeros((N, N))
    K[:n, n:n + m] = A.T
    K[:n, n + m:n + m + k] = G.T
    K[n:n + m, :n] = A
    K[n + m:n + m + k, :n] = G
    K[n + m:n + m + k, n + m + k:] = np.eye(k)
    K[n + m + k:, n + m:n + m + k] = Arw @ sc["W"]
    K[n + m + k:, n + m + k:] = Arw @ sc["iW"].T
    return K


def refined_solve(K, R, steps=6):
    """K u = R (columns) by LU in fp64, refined with np.longdouble residuals
    until the correction stops shrinking.  Returns (u, last correction relative
    to u per column, steps taken)."""
    import scipy.linalg as sl
    lu = sl.lu_factor(K)
    Kl = K.astype(np.longdouble)
    Rl = R.astype(np.longdouble)
    u = sl.lu_solve(lu, R).astype(np.longdouble)
    last = np.full(R.shape[1], np.inf)
    taken = 0
    for _ in range(steps):
        r = Rl - Kl @ u
        d = sl.lu_solve(lu, r.astype(np.float64))
        corr = np.linalg.norm(d, axis=0) / np.linalg.norm(u.astype(np.float64), axis=0)
        if (corr >= last).all():
            break
        u = u + d
        last = np.minimum(last, corr)
        taken += 1
    return u.astype(np.float64), last, taken


Ref = collections.namedtuple("Ref", "sol corr steps")


def split(u, n, m, k):
    return u[:n], u[n:n + m], u[n + m:n + m + k], u[n + m + k:]


def reference_of(cones, A, G, s, z, rhs):
    """The refined block-system solutions of one problem for each right-hand
    side (dx, dy, dz, ds) of `rhs`."""
    k, n = G.shape
    m = A.shape[0]
    K = kkt_matrix(cones, A, G, s, z)
    R = np.stack([np.concatenate(r) for r in rhs], axis=1)
    u, corr, steps = refined_solve(K, R)
    return Ref([split(u[:, j], n, m, k) for j in range(R.shape[1])], corr, steps)


def problem_rhs(d, p):
    return [tuple(v[p] for v in r) for r in d["rhs"]]


@functools.lru_cache(maxsize=None)
def _reference(n, m, k, cones, zero, dy0, p):
    d = _inputs(n, m, k, cones, zero, dy0)
    return reference_of(cones, d["A"][p], d["G"][p], d["s"][p], d["z"][p], problem_rhs(d, p))


def reference(c, p):
    """Problem p's refined reference (dy = 0 for singular cases): computed once
    per set of inputs, shared by the modes and the cases that run them."""
    return _reference(c.n, c.m, c.k, c.cones, singular(c), singular(c), p)


@functools.lru_cache(maxsize=None)
def _kappa(n, m, k, cones, zero, p):
    d = _inputs(n, m, k, cones, zero, zero)
    return float(np.linalg.cond(kkt_matrix(cones, d["A"][p], d["G"][p], d["s"][p], d["z"][p])))


def kappa(c, p):
    """kappa_2(K) of problem p."""
    return _kappa(c.n, c.m, c.k, c.cones, singular(c), p)


def oracle_of(cones, A, G, sing, s, z, rhs, xi):
    """oracle.kkt_single in the kernel's operation order, one result per right-hand side."""
    import oracle
    out = []
    for r in rhs:
        o = oracle.kkt_single(list(cones), A, G, sing, s, z, *r, structured=True, chol=not xi)
        out.append(o)
    return out


@functools.lru_cache(maxsize=None)
def _oracle(n, m, k, cones, zero, dy0, xi, p):
    d = _inputs(n, m, k, cones, zero, dy0)
    return oracle_of(cones, d["A"][p], d["G"][p], zero, d["s"][p], d["z"][p], problem_rhs(d, p), xi)


def oracle_solution(c, p, dy0=None):
    if dy0 is None:
        dy0 = singular(c)
    return _oracle(c.n, c.m, c.k, c.cones, singular(c), bool(dy0), c.xi, p)


KEYS = ("cx", "cy", "cz", "cs")


def rel_errors(got, ref):
    """||got - ref||_2 / ||ref||_2 per vector; None for an empty one."""
    out = []
    for g, r in zip(got, ref):
        out.append(float(np.linalg.norm(np.asarray(g) - r) / np.linalg.norm(r)) if len(r) else None)
    return out


def floor(n, m, k):
    """The rounding of one sum of n + m + 2k terms."""
    return (n + m + 2 * k) * U


def gates(n, m, k, e_or):
    """Per vector max(10 e_or, (n + m + 2k) 2^-53): ten times the oracle's own
    error against the refined reference in the kernel's order (the project's P6
    margin), never below the rounding of one sum of that many terms."""
    return [None if e is None else max(10.0 * e, floor(n, m, k)) for e in e_or]


@functools.lru_cache(maxsize=None)
def oracle_errors(c, p):
    """e_or[j][vector] of problem p (dy = 0 for singular cases)."""
    ref = reference(c, p)
    return tuple(tuple(rel_errors([o[key] for key in KEYS], ref.sol[j]))
                 for j, o in enumerate(oracle_solution(c, p)))
