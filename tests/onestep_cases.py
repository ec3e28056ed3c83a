"""Cases of the one-step parity tests (test_onestep_cases_cpu.py,
test_gpu_onestep.py): from every iterate of the oracle's own solve of a
problem under the reference rule, one step of the implementation under test
against one step of the oracle in the same operation order
(problems.one_step_references).

The trajectory gates stop at the bench K and the teacher-forced test at
kappa(H) = 1e5; the iterates after that -- where a problem converges, loses
chol(H) or leaves sqrt's domain -- are otherwise compared only as histograms.
A single step is not chaotic: it replays the solve's next iterate bit for bit,
and under a one-ulp perturbation of G its status changes at under 1 % of the
steps, so the step at which an implementation parts from the oracle has a name:
(problem, t).

A reference set (REFS) is a shape, a problem list and an oracle order; a case
(CASES) is a reference set and the keyword arguments of the device call, so
the blocked kernel's cases reuse the register kernel's references.  gate() is
the whole check, shared by the device test and by the CPU test that runs an
independently rounded build of the oracle (oracle/Makefile `fma`) through it.
"""
import base64
import collections
import json
import os

import numpy as np

import problems
import shared_cases

HERE = os.path.dirname(os.path.abspath(__file__))
P, Q = 0, 1  # cone kinds of include/socp.h: POC, SOC
SEED0 = 0x534F4350  # socp_amd.configs: seed = SEED0 + config id

Shape = collections.namedtuple("Shape", "cones n m k")
C1 = Shape([(Q, 0, 48)], 32, 8, 48)
C2 = Shape([(P, 0, 32), (Q, 32, 32), (Q, 64, 32)], 64, 16, 96)
C4 = Shape([(Q, 80 * i, 80) for i in range(8)], 512, 64, 640)
LP = dict(n=32, m=8, k=48, cones=[(P, 0, 48)], seed=SEED0 + 9)  # test_gpu_xi.LP: chol(H) ends every solve in the Li order
MQ2_SEED = 20261020

# oracle orders by name (oracle.py's flag values are looked up at run time)
ORDERS = dict(chol=("F_STRUCTURED", "F_CHOLSOLVE"), xi=("F_STRUCTURED", "F_INV_YTY"))

# name -> (shape, problem source, order, seeds, steps)
#   ("outcomes", run): C2 problems picked by the oracle's outcome in tests/golden/c2_refrule_outcomes.json
#   ("generate", seed, count): the first `count` problems of the generator's stream
#   ("shared", key, seed, count): shared_cases.make(key, count, seed)
Ref = collections.namedtuple("Ref", "shape source order seeds steps")
REFS = {
    "c2-chol": Ref(C2, ("outcomes", "structured_chol"), "chol", range(1, 9), None),
    "c2-xi": Ref(C2, ("outcomes", "structured"), "xi", range(1, 9), None),
    "lp-xi": Ref(Shape(LP["cones"], LP["n"], LP["m"], LP["k"]), ("generate", LP["seed"], 16), "xi", range(1, 9), None),
    "mq2": Ref(Shape(*shared_cases.SHAPES["mq2"]), ("shared", "mq2", MQ2_SEED, 16), "xi", range(1, 9), None),
    "c1-chol": Ref(C1, ("generate", SEED0 + 1, 16), "chol", range(1, 9), None),
    # one C4 oracle step takes ~0.1 s: the last six iterates (the oracle's solve
    # loses chol(H) at iteration 13, so the failing step is among them), 4 seeds
    "c4-chol": Ref(C4, ("generate", SEED0 + 4, 1), "chol", range(1, 5), range(-6, 0)),
}
# how many problems of each oracle outcome the "outcomes" source takes, in problem order
PICK = ((2, 16), (4, 8), (0, 8))

# kernel: socp_last_kernel_name exactly, or up to the variant's "<" for a register kernel
Case = collections.namedtuple("Case", "name ref kw kernel min_failing stand_in")
CASES = [
    Case("c2-chol", "c2-chol", {}, "socp_small_kernel<", 12, True),
    Case("c2-chol-large", "c2-chol", dict(force_large=True), "socp_large_kernel", 12, True),
    Case("c2-xi", "c2-xi", dict(explicit_inverse=True), "socp_small_xi_kernel<", 12, True),
    Case("c2-xi-large", "c2-xi", dict(explicit_inverse=True, force_large=True), "socp_large_xi_kernel", 12, True),
    Case("lp-xi", "lp-xi", dict(explicit_inverse=True), "socp_small_xi_kernel<", 10, True),
    Case("lp-xi-large", "lp-xi", dict(explicit_inverse=True, force_large=True), "socp_large_xi_kernel", 10, True),
    Case("mq2", "mq2", {}, "socp_small_kernel<", 0, True),
    Case("c1-chol", "c1-chol", {}, "socp_small_kernel<", 0, True),
    Case("c4-chol", "c4-chol", {}, "socp_large_kernel", 1, False),
]
UNDECIDED_CAP = 0.05  # of a case's steps

# Where the kernels part from the oracle, measured on MI355X: only in the NAME
# of a failure, (problem, t, oracle status, kernel status), and only at iterates
# at which a second-order cone of s or z lies on the cone's boundary to within
# one rounding of v0^2: |v0^2 - |v1|^2| <= 3.3e-15 in exact arithmetic at every
# step listed, with v0^2 between 6 and 28.  compute_scaling takes the square
# root of that difference (scalings.jl:39-47).  The oracle subtracts the squares
# one after the other, as the reference does; scaling_op's cone lanes
# (socp_small.hpp) and the blocked kernel's scaling (socp_large.hip) subtract a
# tree sum of the squares from a fused v0 * v0.  One order ends below zero
# (DomainError, 4), the other at or above it (sqrt(0) = 0, 1 / 0 = Inf, H not
# finite: chol(H) fails, 2).  domain_by_order recomputes both on the host, and
# at EVERY decided failing step of the four cases (19 + 19 + 15 + 15) the
# oracle says 4 exactly where the serial difference is negative and the kernel
# says 4 exactly where its own tree's is (test_onestep_cases_cpu.py).  One ulp
# of G does not move s or z, so these steps count as decided; both sides fail
# at each.  Matching the name would take a serial sum of dim squares per cone
# and iteration on one lane of the kernel; it decides nothing but the name.
STAGE = "compute_scaling's v0^2 - |v1|^2 (scaling_op's cone lanes: tree sum and fma; the oracle subtracts serially)"
LOCATED = {
    "c2-chol": [(768, 22, 2, 4), (2982, 22, 4, 2), (4006, 21, 4, 2)],
    "c2-chol-large": [(768, 22, 2, 4), (1076, 20, 2, 4), (2982, 22, 4, 2), (4006, 21, 4, 2)],
    "c2-xi": [(2, 19, 4, 2), (12, 22, 4, 2), (10, 20, 4, 2), (223, 21, 2, 4), (383, 21, 4, 2)],
    "c2-xi-large": [(2, 19, 4, 2), (12, 22, 4, 2), (10, 20, 4, 2), (223, 21, 2, 4), (383, 21, 4, 2)],
}


def xfail_reason(name):
    return (f"{STAGE}: at an SOC within one rounding of its boundary the sign names the failure (domain 4 / "
            f"chol(H) 2) differently at (problem, t, oracle, kernel) {LOCATED[name]}")


def domain_by_order(shape, rec, head_lane):
    """(serial, tree): does v0^2 - |v1|^2 of an SOC of the iterate's s or z end
    below zero -- the DomainError of compute_scaling -- when the squares are
    subtracted one after the other (the oracle), and when a balanced tree sum
    of the tail's squares over the wave's lanes is subtracted from v0 * v0 in
    one fused operation (the kernels)?  head_lane: the cone's lanes start at its
    head, which adds 0 (the register kernel, a cone of 32 on lanes 0..31 or
    32..63); without it the tail starts at lane 0 (the blocked kernel)."""
    from fractions import Fraction
    serial = tree = False
    for v in (rec["iterate"][3], rec["iterate"][2]):
        for kind, o, dim in shape.cones:
            if kind != Q:
                continue
            w = [float(e) for e in v[o:o + dim]]
            q = w[0] * w[0]
            for e in w[1:]:
                q -= e * e
            serial = serial or q < 0.0
            a = ([0.0] if head_lane else []) + [e * e for e in w[1:]]
            while len(a) > 1:
                a = [a[i] + (a[i + 1] if i + 1 < len(a) else 0.0) for i in range(0, len(a), 2)]
            tree = tree or Fraction(w[0]) ** 2 - Fraction(a[0]) < 0
    return serial, tree


def order_flags(oracle, order):
    f = 0
    for name in ORDERS[order]:
        f |= getattr(oracle, name)
    return f


def outcome_problems(run):
    """Problem indices of the fixture's 4,096 C2 problems by the oracle's outcome in `run`."""
    with open(os.path.join(HERE, "golden", "c2_refrule_outcomes.json")) as f:
        fx = json.load(f)
    st = np.frombuffer(base64.b64decode(fx["runs"][run]["status"]), dtype="<i1")
    return fx["seed"], [int(p) for want, count in PICK for p in np.flatnonzero(st == want)[:count]]


def problem_list(oracle, ref):
    """[(label, c, A, b, G, h)] of a reference set, A and G dense row-major."""
    sh, src = ref.shape, ref.source
    if src[0] == "outcomes":
        seed, idx = outcome_problems(src[1])
        flats = [(p, oracle.generate(sh.cones, 1, sh.n, sh.m, sh.k, seed, first_problem=p), 1, 0) for p in idx]
    elif src[0] == "generate":
        d = oracle.generate(sh.cones, src[2], sh.n, sh.m, sh.k, src[1])
        flats = [(p, d, src[2], p) for p in range(src[2])]
    else:
        bt = shared_cases.make(src[1], src[3], src[2])
        A, G = shared_cases.replicated(bt)
        d = dict(c=bt.c, A=A, b=bt.b, G=G, h=bt.h)
        flats = [(p, d, src[3], p) for p in range(src[3])]
    return [(label,) + tuple(problems.batch_problem(d, B, sh.n, sh.m, sh.k, p)) for label, d, B, p in flats]


def references(oracle, name):
    """The reference set `name`: a flat list of steps, each problems.one_step_references'
    record plus `problem` (its label) and `data` (c, A, b, G, h)."""
    ref = REFS[name]
    flags = order_flags(oracle, ref.order)
    steps = []
    for label, c, A, b, G, h in problem_list(oracle, ref):
        for rec in problems.one_step_references(oracle, ref.shape.cones, c, A, b, G, h, flags, seeds=ref.seeds,
                                                steps=ref.steps):
            rec.update(problem=label, data=(c, A, b, G, h))
            steps.append(rec)
    return steps


def census(steps):
    """(steps, undecided, decided failing, decided continuing) of a reference set."""
    und = sum(not r["decided"] for r in steps)
    fail = sum(r["decided"] and r["status"] != 1 for r in steps)
    return len(steps), und, fail, len(steps) - und - fail


def stacked(shape, steps):
    """The steps as one batch in the include/socp.h layout: dict(c, A, b, G, h)
    with each step's problem repeated, and warm = (x, y, z, s) of the iterates."""
    cat = lambda vs: np.ascontiguousarray(np.concatenate([np.asarray(v, dtype=np.float64).reshape(-1) for v in vs]))  # noqa: E731
    d = dict(c=cat(r["data"][0] for r in steps), A=cat(r["data"][1].ravel(order="F") for r in steps),
             b=cat(r["data"][2] for r in steps), G=cat(r["data"][3].ravel(order="F") for r in steps),
             h=cat(r["data"][4] for r in steps))
    warm = tuple(cat(r["iterate"][i] for r in steps) for i in range(4))
    return d, warm


def oracle_steps(oracle, name, steps):
    """One step of another build of the oracle from every iterate of `steps`
    (the device's launch, on the CPU): dict(status, x, z, s), stacked."""
    ref = REFS[name]
    P1 = oracle.Params(maxit=1, tol=0.0, flags=order_flags(oracle, ref.order))
    got = [oracle.solve_trace(ref.shape.cones, *r["data"], sing=False, params=P1, max_trace=2, warm=r["iterate"])
           for r in steps]
    out = {key: np.concatenate([g[key] for g in got]) for key in "xzs"}
    out["status"] = np.array([g["status"] for g in got], np.int32)
    return out


def gate(shape, steps, got):
    """One launch's outputs `got` (status, x, z, s, stacked in the order of
    `steps`) against the references.  Returns
      rows   (ratio, problem, t, vector, error, floor), worst first: every vector
             of every decided step that both sides took; ratio = error /
             (FLOOR_FACTOR floor + FLOOR_ABS) must be <= 1
      fail   [(problem, t, oracle status, got status)] where a decided failing
             step got another status; at most one allowed
      cont   the same where a decided continuing step got a status other than 1
      allow  how many of `cont` are allowed: max(1, 0.5 % of the decided continuing steps)"""
    rows, fail, cont = [], [], []
    ncont = 0
    for i, r in enumerate(steps):
        st = int(got["status"][i])
        if not r["decided"]:
            continue
        if r["status"] != 1:
            if st != r["status"]:
                fail.append((r["problem"], r["t"], r["status"], st))
            continue
        ncont += 1
        if st != 1:
            cont.append((r["problem"], r["t"], 1, st))
            continue
        for j, (key, L) in enumerate((("x", shape.n), ("z", shape.k), ("s", shape.k))):
            a_, b_ = np.asarray(got[key][i * L:(i + 1) * L]), r["next"][j]
            e = float(np.linalg.norm(a_ - b_) / np.linalg.norm(b_))
            rows.append((e / (problems.FLOOR_FACTOR * r["floor"][key] + problems.FLOOR_ABS), r["problem"], r["t"], key,
                         e, r["floor"][key]))
    return sorted(rows, reverse=True), fail, cont, max(1, int(0.005 * ncont))


def check(name, shape, steps, got):
    """gate()'s assertions; returns its result for the caller's table."""
    rows, fail, cont, allow = gate(shape, steps, got)
    print(f"{name}: steps/undecided/failing/continuing {census(steps)}; status differences at failing steps {fail}, "
          f"at continuing steps {cont} (allowed {allow}); worst (ratio, problem, t, vector, error, floor): {rows[:4]}")
    assert not rows or rows[0][0] <= 1.0, [r for r in rows if r[0] > 1.0][:12]
    assert len(fail) <= 1 and len(cont) <= allow, ("(problem, t, oracle status, status)", fail + cont)
    return rows, fail, cont, allow


def check_located(name, shape, steps, got, head_lane):
    """What holds of a case of LOCATED while its check() is an expected
    failure: check() itself, except that a decided failing step may carry the
    other name of the pair domain / chol(H) where the oracle's and the kernel's
    order of v0^2 - |v1|^2 disagree in sign and the kernel's status follows its
    own.  A kernel that takes the step there, or names a failure differently
    anywhere else, counts against the one step check() allows."""
    rows, fail, cont, allow = gate(shape, steps, got)
    assert not rows or rows[0][0] <= 1.0, [r for r in rows if r[0] > 1.0][:12]
    rec = {(r["problem"], r["t"]): r for r in steps}
    other = []
    for p, t, want, st in fail:
        serial, tree = domain_by_order(shape, rec[p, t], head_lane)
        if not ({want, st} == {2, 4} and serial != tree and (st == 4) == tree):
            other.append((p, t, want, st))
    assert len(other) <= 1 and len(cont) <= allow, ("(problem, t, oracle status, status)", other + cont)
    return fail
