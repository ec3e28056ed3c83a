"""Cases that launch every compiled instantiation of the register-resident
kernel (test_variant_table_cpu.py, test_gpu_variants.py).

gen_inst.py emits one kernel per (variant, KM): 36 shape variants (NQ, NP, MQ)
-- NQ = ceil(n/16) column tiles, NP = ceil(k/4) row steps, MQ = ceil(m/16) row
tiles -- in 4 to 9 modes KM each (0 plain solver, 1 plugin entries, 2 / 3
explicit inverse, 4 detecting solver, 8 QP solver, 16 / 32 / 64 the plain
solver for pure slots), 220 kernels.  socp_api.hip's pick_variant chooses the
variant of a call by cost; ``pick_variant`` below restates it on gen_inst's own
table, so a changed table changes the cases with it.

Two shapes per variant, both selecting exactly that variant:
  full    one short of every tile edge (n = 16 NQ - 1, m = 16 MQ - 1,
          k = 4 NP - 1), n lowered to k - 1 where the variant's k range is
          below 16 NQ, m lowered where the system would be nearly square (m
          close to n leaves x almost fixed by Ax = b, and the one-rounding
          floor of such a trajectory exceeds FLOOR_CAP), n and m a few
          more where the conditioning asks for it (KAPPA_CAP below);
  sparse  the smallest n, m, k that still select the variant: one past the
          next smaller compiled NQ, MQ and NP, so that nearly a whole tile or
          row step is padding.
Variants with NP > 16 (k > 64, two slots) get a third shape, "sp", with k on
the tile edge: the one table layout that the slot plan rotates.

Seven variants have 4 NP < 16 (NQ - 1) + 1: no G with k >= n selects them.  Six
are reached with k < n through the sing path (H = G'W^-2 G + A'A, sing = 1),
at the shapes of SING_SHAPES.  EXEMPT = {(4, 8, 1)} holds no solvable problem:
n >= 49, m <= 16 and k <= 32 give rank(H) <= k + m <= 48 < n, and the oracle
ends every problem of (49, 16, 32) in status 2 (chol(H) failed).  Its kernels
are launched and their names checked, nothing is compared.

Cone tables (at most 8 cones, POC before SOC):
  mixed   k <= 4: one SOC cone; k <= 64: a POC head and two SOC cones of
          unequal, unaligned lengths; k > 64: the same, with both kinds in
          slot 0 -- the mixed kernel (KM 0);
  ps      POC 64 + SOC k - 64: slots pure as the table stands (KM 32);
  pp      one POC cone of k (KM 64);
  sp      POC then SOC cones of one common length 16 or 32 whose last 64 rows
          are SOC: rotated by 64 into an SOC slot and a POC slot (KM 16).
          k = 80 or 96 at NP = 24, k = 112 at NP = 32 (at k = 128 the last 64
          SOC rows leave 64 POC rows: pure as it stands, the ps kernel).

Data: B = 8 problems from oracle.generate with one fixed seed per case, K = 3
iterations, tol = 0.
"""
import collections
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "socp.jl_amd", "csrc"))
import gen_inst  # noqa: E402

import problems  # noqa: E402

P_, Q_ = 0, 1  # cone kinds of include/socp.h: POC, SOC
B, K, SEED = 8, 3, 20261020
KMAX = 128  # socp_kernels.hpp: the register kernel's largest k
VARIANTS = list(gen_inst.VARIANTS)
kms = gen_inst.kms
# the one-rounding floor (problems.order_floor_traces) allowed on any vector of
# any case: the floor gate 10 floor + 1e-13 then never exceeds gate P4 (1e-8)
FLOOR_CAP = 1e-9
# entry names of socp_last_kernel_name per KM (gen_inst.py's table; the slot
# kernels 16 / 32 / 64 carry the plain solver's name)
ENTRY = {0: "socp_small_kernel", 1: "socp_small_kkt_kernel", 2: "socp_small_xi_kernel",
         3: "socp_small_xi_kkt_kernel", 4: "socp_small_di_kernel", 8: "socp_small_qp_kernel",
         16: "socp_small_kernel", 32: "socp_small_kernel", 64: "socp_small_kernel"}
TABLE_KM = dict(mixed=0, sp=16, ps=32, pp=64)
# socp_debug_slot_plan's (rot, kind0, kind1) per table: kinds 0 mixed, 1 all SOC, 2 all POC
TABLE_PLAN = dict(mixed=(0, 0, 0), sp=(64, 1, 2), ps=(0, 2, 1), pp=(0, 2, 2))


def cost(v):
    return v[0] * v[0] * v[1] * 64 + v[2] * 16


def pick_variant(n, m, k, variants=None):
    """socp_api.hip pick_variant: the cheapest variant whose tiles hold the
    problem, the first one in table order among equals; None when none fits."""
    best = None
    for v in (VARIANTS if variants is None else variants):
        if 16 * v[0] < n or 4 * v[1] < k or 16 * v[2] < max(m, 1) or k > KMAX:
            continue
        if best is None or cost(v) < cost(best):
            best = v
    return best


def kernel_name(v, km):
    return "%s<%d,%d,%d>" % ((ENTRY[km],) + tuple(v))


# no G of full column rank (k >= n) selects these
UNREACHED_BY_FULL_RANK = [v for v in VARIANTS if 4 * v[1] < 16 * (v[0] - 1) + 1]
# (n, m, k) with k < n, run with sing = 1: first the ragged shape, then the small one.
# k + m >= n keeps H of full rank.  (33, 16, 17) and (49, 17, 32), where k + m = n
# makes [W^-1 G; A] square, are replaced by (33, 16, 18) and (49, 18, 32): in the
# orders that form H^-1 explicitly (F_STRUCTURED | F_INV_YTY at m = 16, F_STRUCTURED
# at m = 17) the oracle's one-rounding floor of s at K = 3 was 3.5e-8 .. 8.8e-5 and
# 2.1e-7 .. 9.1e-6 over 40 seeds there, above FLOOR_CAP on every seed.
SING_SHAPES = {
    (2, 4, 1): ((20, 10, 15), (31, 16, 16)),
    (2, 4, 2): ((30, 20, 15), (17, 17, 1)),
    (3, 8, 1): ((40, 16, 31), (33, 16, 18)),
    (3, 8, 2): ((47, 31, 31), (33, 17, 17)),
    (4, 8, 2): ((60, 32, 32), (49, 18, 32)),
    (4, 8, 4): ((63, 62, 31), (49, 33, 17)),
    # rank(H) <= k + m <= 48 < 49 <= n: no problem of this variant can be factored
    (4, 8, 1): ((63, 15, 31), (49, 16, 32)),
}
EXEMPT = {(4, 8, 1)}
# The kernels' order forms S^-1 (and H^-1 at m > 16) explicitly, so a kernel
# iterate carries an error of the size 2^-53 kappa, kappa the larger of the 2-norm
# conditions of H and S = A H^-1 A' (conditioning()); the oracle's kernel orders
# solve S by triangular solves, and their one-rounding floor does not grow with
# cond(S).  The floor gate therefore means what it says only at moderate kappa:
# every case keeps kappa <= KAPPA_CAP = 1e5 over the factorisations of its K
# iterations -- the window in which gates P3 and the trajectory fixtures hold
# the kernels to their tight bounds.  G one row from square
# (k = n + 1) and A nearly square (m close to n) are what breaks it.  Where the
# shape at the tile edges does, n and m step back from the edge inside the
# variant's ranges (SHAPE), k of a sparse shape gets rows to spare, or the case
# takes another seed (RESEED); k of the full shapes stays ragged.  The shapes of
# SING_SHAPES stand as given (H = G'W^-2 G + A'A with k + m barely above n): six of
# them lie above the cap on every seed tried (KAPPA_ABOVE, kappa 8e5 .. 4e6).
KAPPA_CAP = 1e5
KAPPA_ABOVE = {"q2_p4_m1-sparse-mixed", "q3_p8_m1-sparse-mixed", "q3_p8_m2-sparse-mixed", "q4_p8_m2-full-mixed",
               "q4_p8_m2-sparse-mixed", "q4_p8_m4-sparse-mixed"}
# (variant, shape) -> (n, m, k) where the rule's shape breaks FLOOR_CAP or KAPPA_CAP
SHAPE = {
    ((1, 2, 1), "full"): (5, 2, 7), ((1, 4, 1), "full"): (12, 6, 15),
    ((2, 8, 1), "full"): (27, 15, 31), ((2, 8, 2), "full"): (28, 19, 31),
    ((2, 12, 2), "full"): (31, 28, 47), ((2, 16, 2), "full"): (31, 28, 63),
    ((4, 16, 1), "full"): (57, 15, 63), ((4, 16, 2), "full"): (57, 27, 63), ((4, 16, 4), "full"): (59, 41, 63),
    ((4, 24, 4), "full"): (63, 58, 95), ((4, 24, 4), "sp"): (63, 54, 80),
    ((2, 8, 1), "sparse"): (17, 1, 19), ((2, 8, 2), "sparse"): (19, 17, 30),
    ((3, 16, 1), "sparse"): (33, 1, 36), ((3, 16, 2), "sparse"): (33, 17, 36),
    ((4, 16, 1), "sparse"): (49, 1, 54), ((4, 16, 2), "sparse"): (49, 17, 54), ((4, 16, 4), "sparse"): (49, 33, 53),
}
# per-case seed offsets where the default seed's batch breaks a precondition
# of test_variant_table_cpu.py (id -> offset)
RESEED = {"q1_p1_m1-full-mixed": 2, "q1_p2_m1-full-mixed": 1, "q1_p4_m1-full-mixed": 1, "q2_p4_m2-sparse-mixed": 2, "q2_p8_m1-full-mixed": 2, "q2_p8_m1-sparse-mixed": 2, "q2_p8_m2-full-mixed": 2,
          "q2_p12_m2-full-mixed": 1, "q2_p12_m2-sparse-mixed": 1, "q2_p24_m2-full-mixed": 6, "q2_p24_m2-full-pp": 4,
          "q2_p24_m2-sp-sp": 9, "q2_p32_m2-full-mixed": 6, "q2_p32_m2-full-pp": 2, "q3_p8_m1-sparse-mixed": 1,
          "q3_p16_m1-sparse-mixed": 2, "q3_p16_m2-sparse-mixed": 1, "q4_p8_m2-sparse-mixed": 4,
          "q4_p8_m4-full-mixed": 1, "q4_p8_m4-sparse-mixed": 1, "q4_p16_m2-sparse-mixed": 1,
          "q4_p16_m4-full-mixed": 4, "q4_p16_m4-sparse-mixed": 1, "q4_p24_m4-full-mixed": 1}


def _smaller(values, x):
    lo = [v for v in values if v < x]
    return max(lo) if lo else 0


def full_shape(v):
    NQ, NP, MQ = v
    if v in SING_SHAPES:
        return SING_SHAPES[v][0]
    if (v, "full") in SHAPE:
        return SHAPE[v, "full"]
    k = 4 * NP - 1
    n = min(16 * NQ - 1, k - 1)
    # (NQ = 1: 16 MQ - 1 = 15 is n or more; m = n / 2 keeps A from square, see KAPPA_CAP)
    return n, (n // 2 if NQ == 1 else min(16 * MQ - 1, n - 1)), k


def sparse_shape(v):
    NQ, NP, MQ = v
    if v in SING_SHAPES:
        return SING_SHAPES[v][1]
    if (v, "sparse") in SHAPE:
        return SHAPE[v, "sparse"]
    n = 16 * _smaller({u[0] for u in VARIANTS}, NQ) + 1
    m = 16 * _smaller({u[2] for u in VARIANTS if u[:2] == (NQ, NP)}, MQ) + 1
    k = 4 * _smaller({u[1] for u in VARIANTS if u[0] == NQ}, NP) + 1
    n = max(n, m + 2 if m > 1 else m)  # A of full row rank, and two unknowns that Ax = b leaves free
    k = max(k, n + 1)        # G of full column rank, one row to spare
    return n, m, k


def sp_shape(v):
    """k on the tile edge for the rotated table: 80 / 96 alternate over the NP = 24 variants."""
    NQ, NP, MQ = v
    if (v, "sp") in SHAPE:
        return SHAPE[v, "sp"]
    n, m, _ = full_shape(v)
    if NP == 32:
        return n, m, 112
    return n, m, (80, 96)[[u for u in VARIANTS if u[1] == 24].index(v) % 2]


def mixed_table(k):
    if k <= 4:
        return ((Q_, 0, k),)
    p = 21 if k > 64 else max(1, k // 4)
    rest = k - p
    b = (rest - 1) // 2
    a = rest - b  # a > b
    return ((P_, 0, p), (Q_, p, a), (Q_, p + a, b))


def ps_table(k):
    return ((P_, 0, 64), (Q_, 64, k - 64))


def pp_table(k):
    return ((P_, 0, k),)


def sp_table(k):
    d = 32 if k == 96 else 16
    npoc = (k - 64) // d
    return tuple((P_ if j < npoc else Q_, j * d, d) for j in range(k // d))


Case = collections.namedtuple("Case", "id variant shape table cones n m k sing seed")


def _cases():
    out = []
    probe_done = set()
    for v in VARIANTS:
        tag = "q%d_p%d_m%d" % v
        rows = [("full", "mixed", full_shape(v)), ("sparse", "mixed", sparse_shape(v))]
        if v[1] > 16:
            n, m, k = full_shape(v)
            rows += [("full", "ps", (n, m, k)), ("full", "pp", (n, m, k)), ("sp", "sp", sp_shape(v))]
        for shape, table, (n, m, k) in rows:
            cones = dict(mixed=mixed_table, ps=ps_table, pp=pp_table, sp=sp_table)[table](k)
            sing = 1 if v in SING_SHAPES else 0
            # one sparse case per NQ leaves sing to the device probe (G of full column rank: the probe says 0)
            if shape == "sparse" and sing == 0 and v[0] not in probe_done:
                probe_done.add(v[0])
                sing = None
            cid = "%s-%s-%s" % (tag, shape, table)
            out.append(Case(cid, v, shape, table, cones, n, m, k, sing, SEED + len(out) + 1000 * RESEED.get(cid, 0)))
    return out


CASES = _cases()
NUMERIC = [c for c in CASES if c.variant not in EXEMPT]
EXEMPT_CASES = [c for c in CASES if c.variant in EXEMPT]


def case_id(c):
    return c.id


def solver_km(c):
    """KM of the kernel a plain solve of the case launches."""
    return TABLE_KM[c.table]


def plugin_case(c):
    """The plugin entries and the explicit-inverse kernels keep their one
    kernel whatever the table: they run on the mixed-table cases."""
    return c.table == "mixed"


def launched(c):
    """Every (variant, KM) a case launches in test_gpu_variants.py."""
    out = {solver_km(c), 4, 8}
    if plugin_case(c):
        out |= {1} | ({2, 3} if c.variant[2] == 1 else set())
    return {(c.variant, km) for km in out}


def sing_bool(c):
    return bool(c.sing)  # None: the device probe, which says 0 on these cases


def sing_bytes(c):
    return None if c.sing is None else np.full(B, c.sing, np.uint8)


def kernel_order(oracle, c, explicit_inverse=False):
    """The oracle flags of the kernels' operation order at the case's m."""
    if explicit_inverse:
        return oracle.F_STRUCTURED | oracle.F_INV_YTY
    return oracle.F_STRUCTURED | (oracle.F_CHOLSOLVE if c.m <= 16 else 0)


@functools.lru_cache(maxsize=None)
def data(c):
    import oracle
    return oracle.generate(list(c.cones), B, c.n, c.m, c.k, c.seed)


def problem(c, p, d=None):
    """(c, A, b, G, h) of problem p as dense row-major matrices."""
    return problems.batch_problem(data(c) if d is None else d, B, c.n, c.m, c.k, p)


@functools.lru_cache(maxsize=None)
def reference(c, explicit_inverse=False):
    """Per problem (iterates 0..K, floors) of the oracle in the kernels' order
    (problems.floor_references): computed once per case and order."""
    import oracle
    return problems.floor_references(oracle, c, data(c), B, K, kernel_order(oracle, c, explicit_inverse),
                                     sing=sing_bool(c))


def qp_matrices(c):
    """P = R'R / n per problem (R of size n/2 x n, standard normal: qp_cases.make_batch's P;
    c stays the generator's, so the linear problem's strictly feasible pair is only primal feasible)."""
    rng = np.random.default_rng(c.seed)
    Ps = []
    for _ in range(B):
        R = rng.standard_normal((max(c.n // 2, 1), c.n))
        Ps.append(R.T @ R / c.n)
    return Ps


def conditioning(c):
    """The largest 2-norm condition of H and of S = A H^-1 A' over the case's
    factorisations (the initial point's and those of K iterations, at the
    oracle's iterates in the kernels' order)."""
    import oracle
    import qp_cases
    worst = 0.0
    for p in range(B):
        _, A, _, G, _ = problem(c, p)
        scs = [qp_cases._identity_scaling(list(c.cones), c.k)]
        scs += [oracle.compute_scaling(list(c.cones), s, z) for _, z, s in reference(c)[p][0][:K]]
        for sc in scs:
            f = qp_cases._Factor(list(c.cones), np.zeros((c.n, c.n)), A, G, sing_bool(c), sc)
            assert f.status == 0
            worst = max(worst, f.kappa, float(np.linalg.cond(f.Z.T @ f.Z)))
    return worst
