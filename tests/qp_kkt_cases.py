"""Cases, inputs, reference and gate of the QP plugin entries
(test_qp_kkt_cases_cpu.py, test_gpu_qp_kkt.py): socp_batch_kkt_solve_qp
(MODE_KKT) and socp_dense_create_qp / socp_dense_setup_iter /
socp_dense_solve_kkt (MODE_SETUP, MODE_SOLVEKKT) on both dense kernels.

The reference is kkt_cases.py's block system with P in its first block row,

    P cx + A'cy + G'cz         = dx
    A cx                       = dy
    G cx + cs                  = dz
    lam o (W cz + W^-T cs)     = ds

i.e. kkt_cases.kkt_matrix with K[:n, :n] = P, solved by kkt_cases.refined_solve
(LU in fp64, residuals in np.longdouble).  It knows nothing of H, S or any
operation order.

The gate is kkt_cases.gates with the numpy restatement in the oracle's place:
per vector max(10 e_rs, (n + m + 2k) 2^-53), where e_rs is the relative error,
against the refined reference on the same inputs, of
qp_cases._Factor(...).solve -- setup_iter and solve_kkt in the kernels'
operation order with H = P + X'X (+A'A).  (oracle.kkt_single has no P; with
P = 0 the restatement agrees with it to 1e-11, test_qp_kkt_cases_cpu.py.)  The
factor ten is the project's P6 margin over something that is not the code
under test; no measurement of a kernel enters it.

Inputs are kkt_cases.make_inputs' (G, A standard normal, interior (s, z), two
right-hand sides, B = 2, seeded from (n, m, k)) plus P = R'R/n with R of n//2
rows, standard normal from a generator seeded (n, m, k, 1): positive
semidefinite of rank n//2, so singular.  The singular case takes sing = 1,
dy = 0 (kkt_cases.py's header: the sing formula solves the block system only
then), G's trailing m columns zeroed and P's rows and columns there zeroed as
well, so that A'A -- not P -- is what makes H definite.  (kkt_cases zeroes the
columns n//2..; at (10, 4, 8) that leaves five columns to A's four rows and H
singular, so the last m = 4 columns are zeroed here.)

The table: each shape the smallest that reaches its branch.  `kernel` is the
name socp_last_kernel_name must report; small_variant() restates
socp_api.hip's pick_variant over gen_inst.py's table.
"""
import collections
import functools
import os
import sys

import numpy as np

import kkt_cases as KC

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "socp.jl_amd", "csrc"))

P_, Q_ = KC.P_, KC.Q_
B, NRHS, KEYS = KC.B, KC.NRHS, KC.KEYS

Case = collections.namedtuple("Case", "id n m k cones sing force_large kernel")

_T = KC._table
CASES = [
    # NQ = 1, one slot
    Case("s8", 8, 2, 16, _T((Q_, 16)), 0, False, "socp_small_qp_kkt_kernel<1,4,1>"),
    # m = 0
    Case("m0", 8, 0, 16, _T((P_, 8), (Q_, 8)), 0, False, "socp_small_qp_kkt_kernel<1,4,1>"),
    # NQ = 2
    Case("c1", 32, 8, 48, _T((Q_, 48)), 0, False, "socp_small_qp_kkt_kernel<2,12,1>"),
    # two slots, NQ = 4: the variant at the register cap
    Case("c2", 64, 16, 96, _T((P_, 32), (Q_, 32), (Q_, 32)), 0, False, "socp_small_qp_kkt_kernel<4,24,1>"),
    # m > 16: the record holds the inverse of P + G'W^-2 G
    Case("mq2", 48, 32, 64, _T((P_, 16), (Q_, 48)), 0, False, "socp_small_qp_kkt_kernel<3,16,2>"),
    # sing: A'A in H, dy = 0
    Case("sing", 10, 4, 8, _T((Q_, 8)), 1, False, "socp_small_qp_kkt_kernel<1,2,1>"),
    # the blocked kernel on a register shape
    Case("c1_large", 32, 8, 48, _T((Q_, 48)), 0, True, "socp_large_qp_kernel"),
    # the blocked kernel, one column past a 64-block
    Case("edge65", 65, 1, 66, KC._EDGE, 0, False, "socp_large_qp_kernel"),
    # MPAD = 128
    Case("m65", 130, 65, 200, KC._M65, 0, False, "socp_large_qp_kernel"),
    # windowed panels, form_H_staged
    Case("wide", 513, 20, 520, KC._WIDE, 0, False, "socp_large_qp_kernel"),
    # the global-vector instantiation
    Case("gv", 80, 0, 1100, KC._GV, 0, False, "socp_large_qp_gv_kernel"),
]
BY_ID = {c.id: c for c in CASES}


def case_id(c):
    return c.id


def small_variant(n, m, k):
    """pick_variant (socp_api.hip) over gen_inst.VARIANTS: (NQ, NP, MQ) or None."""
    import gen_inst
    best = None
    for NQ, NP, MQ in gen_inst.VARIANTS:
        if 16 * NQ < n or 4 * NP < k or 16 * MQ < max(m, 1) or k > 128:
            continue
        cost = NQ * NQ * NP * 64 + MQ * 16
        if best is None or cost < best[0]:
            best = (cost, (NQ, NP, MQ))
    return best[1] if best else None


def kernel_name(c):
    v = None if (c.force_large or len(c.cones) > 8) else small_variant(c.n, c.m, c.k)
    if v:
        return "socp_small_qp_kkt_kernel<%d,%d,%d>" % v
    return "socp_large_qp_%skernel" % ("gv_" if KC.gv_kernel(c.n, c.m, c.k) else "")


def linear_kernel_name(c):
    """What socp_batch_kkt_solve / socp_dense_create report at the case's shape."""
    return c.kernel.replace("_qp_", "_")


def zeroed(c):
    """The columns of G (rows and columns of P) that the singular case zeroes."""
    return slice(c.n - c.m, c.n) if c.sing else slice(0, 0)


def sing_bytes(c, nb=B):
    return np.full(nb, c.sing, np.uint8)


@functools.lru_cache(maxsize=None)
def _inputs(n, m, k, cones, sing):
    d = KC.make_inputs(n, m, k, cones, (False,) * B, B, range(B) if sing else ())
    rng = np.random.default_rng([n, m, k, 1])
    P = np.zeros((B, n, n))
    for p in range(B):
        R = rng.standard_normal((n // 2, n))
        P[p] = R.T @ R / n
        if sing:
            d["G"][p][:, n - m:] = 0.0
            P[p][n - m:, :] = 0.0
            P[p][:, n - m:] = 0.0
    d["P"] = P
    return d


def inputs(c):
    """The case's batch: kkt_cases.make_inputs' dict plus P (B, n, n)."""
    return _inputs(c.n, c.m, c.k, c.cones, bool(c.sing))


def flat_P(d, nb=None):
    nb = len(d["P"]) if nb is None else nb
    return np.concatenate([d["P"][p].ravel(order="F") for p in range(nb)])


# ------------------------------------------------------------------ reference
def kkt_matrix(cones, P, A, G, s, z):
    K = KC.kkt_matrix(cones, A, G, s, z)
    n = G.shape[1]
    K[:n, :n] = P
    return K


def reference_of(cones, P, A, G, s, z, rhs):
    """kkt_cases.reference_of on the system with P."""
    k, n = G.shape
    m = A.shape[0]
    K = kkt_matrix(cones, P, A, G, s, z)
    R = np.stack([np.concatenate(r) for r in rhs], axis=1)
    u, corr, steps = KC.refined_solve(K, R)
    return KC.Ref([KC.split(u[:, j], n, m, k) for j in range(R.shape[1])], corr, steps)


@functools.lru_cache(maxsize=None)
def reference(c, p):
    """Problem p's refined reference: computed once, shared by every test."""
    d = inputs(c)
    return reference_of(c.cones, d["P"][p], d["A"][p], d["G"][p], d["s"][p], d["z"][p], KC.problem_rhs(d, p))


@functools.lru_cache(maxsize=None)
def kappa(c, p):
    d = inputs(c)
    return float(np.linalg.cond(kkt_matrix(c.cones, d["P"][p], d["A"][p], d["G"][p], d["s"][p], d["z"][p])))


def restatement_of(cones, P, A, G, sing, s, z, rhs):
    """qp_cases._Factor(...).solve per right-hand side: [(cx, cy, cz, cs), ...]."""
    import oracle
    import qp_cases as QC
    sc = oracle.compute_scaling(list(cones), s, z)
    assert sc["status"] == 0
    f = QC._Factor(list(cones), P, A, G, bool(sing), sc)
    assert f.status == 0, f.status
    return [f.solve(*r) for r in rhs]


@functools.lru_cache(maxsize=None)
def restatement(c, p):
    d = inputs(c)
    return restatement_of(c.cones, d["P"][p], d["A"][p], d["G"][p], c.sing, d["s"][p], d["z"][p],
                          KC.problem_rhs(d, p))


@functools.lru_cache(maxsize=None)
def restatement_errors(c, p):
    """e_rs[j][vector] of problem p: the restatement against the refined reference."""
    ref = reference(c, p)
    return tuple(tuple(KC.rel_errors(r, ref.sol[j])) for j, r in enumerate(restatement(c, p)))


def gates(c, p, j):
    """Per vector max(10 e_rs, (n + m + 2k) 2^-53) (kkt_cases.gates)."""
    return KC.gates(c.n, c.m, c.k, restatement_errors(c, p)[j])
