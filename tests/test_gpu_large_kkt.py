"""The blocked kernel's KKT plugin entries -- socp_batch_kkt_solve (MODE_KKT)
and socp_dense_setup_iter / socp_dense_solve_kkt (MODE_SETUP, MODE_SOLVEKKT
against per-problem factor records) -- at the shapes only socp_large.hip
takes, against the refined block-system reference of kkt_cases.py.
tests/test_kkt_cases_cpu.py holds the preconditions: the table, the kernel
each case must select, the oracle's status 0, the refinement's convergence and
the agreement of oracle and reference.

The gate, per vector cx, cy, cz, cs (empty ones skipped), with
e = ||got - ref||_2 / ||ref||_2 and e_or the same error of oracle.kkt_single
in the kernel's operation order (structured=True, chol=True; structured=True
with explicit_inverse) against the same reference:

    e <= max(10 e_or, (n + m + 2k) 2^-53)

10 is the project's P6 margin (test_large_kkt_backward_error), the floor the
rounding of one sum of that many terms, for cases where the oracle lands
within a few ulp.  No measurement of the kernel enters it.

sing cases (sing, probe): the sing formula of densesolver.jl:66-85 solves the
block system only for dy = 0 (kkt_cases.py, asserted in test_kkt_cases_cpu.py),
so they are gated against the block system with dy = 0, and run once more with
dy != 0 against oracle.kkt_single(sing=True) in the kernel's order.  That
second gate is the first one's, max(10 e_or, floor) with e_or of the dy = 0
run of the same problem, vector and right-hand side: kernel and oracle apply
one linear formula to the same factors in the same order, each within its own
rounding of the formula's exact value, and e_or measures that rounding for
these factors.

  fused     batch_kkt_solve against the gate, status 0, the kernel's name;
  split     setup_iter (status 0, 2k doubles per problem host-to-device) and
            solve_kkt of two right-hand sides (n + m + 2k doubles), each
            against the gate and bitwise the fused call (socp.h);
  scratch   the record does not depend on the workgroup's scratch slot: after
            another, larger blocked call on the same (fresh) context -- the
            workspace is reallocated -- and a second handle's setup_iter at
            the same shape on other problems, solve_kkt returns the same bits;
  several   a workgroup takes several problems: B = 2 CUs + 5 at (65, 40, 66)
            -- edge65's n, k and cones with m = 40, so that the odd problems,
            which have G's right half zero, sing = 1 and dy = 0, keep
            H + A'A definite (m >= n - n//2 = 33) -- every 97th problem with
            s outside its SOC cone: the failing problems report
            DOMAIN_ERROR and NaN, every problem has the bits of the same
            problem solved alone, split equals fused; the good problems
            against the gate in a test of its own (its docstring has the
            one raised gate and its reason);
  shared    SOCP_F_SHARED_MATRICES on the fused and the split entry returns
            the bits of the replicated call, on the LDS and the GV kernel.

Measured on MI355X: 36 tests in 7 s; worst e / gate per case 0.0055 (gv) to
0.42 (edge65), dy != 0 against the oracle 0.48, the batch of several 0.97
(DESIGN section 11a has the table).  With solve_matrix_part's m > 512 branch turned to symv, fused and
split of mwide fail; with store_record's sing word dropped, split of sing and
of probe fail (and the shared-matrices split at m65, which then reads an
unwritten word).
"""
import functools

import numpy as np
import pytest

import kkt_cases as KC
import socp_amd as S

pytestmark = pytest.mark.gpu

OUT = KC.KEYS + ("status",)
WORST = {}


def kernel_is(case, ctx=None):
    name = (ctx or S.default_context()).last_kernel_name()
    assert name == case.kernel, (case.id, name)


def same(a, b, keys=OUT):
    for key in keys:
        u, v = np.asarray(a[key]), np.asarray(b[key])
        assert u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes(), key


def vectors(out, p, n, m, k):
    return [out[key][p * q:(p + 1) * q] for key, q in zip(KC.KEYS, (n, m, k, k))]


def note(tag, case, ratio):
    key = (tag, case.id)
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    print(f"{tag} {case.id} on {case.kernel}: worst error / gate {WORST[key]:.3g}")


def check_gate(tag, case, out, j):
    """Every problem's four vectors of right-hand side j against the refined reference."""
    n, m, k = case.n, case.m, case.k
    assert (out["status"] == 0).all(), out["status"]
    worst = 0.0
    for p in range(KC.B):
        e = KC.rel_errors(vectors(out, p, n, m, k), KC.reference(case, p).sol[j])
        g = KC.gates(n, m, k, KC.oracle_errors(case, p)[j])
        for key, ev, gv in zip(KC.KEYS, e, g):
            if ev is None:
                continue
            print(f"  {case.id} p={p} rhs {j} {key}: e = {ev:.3g}, gate {gv:.3g}")
            worst = max(worst, ev / gv)
    note(tag, case, worst)
    assert worst <= 1.0, (case.id, j, worst)


def check_against_sing_oracle(tag, case, out, j):
    """dy != 0 on a sing case: against the oracle's sing formula (module docstring)."""
    n, m, k = case.n, case.m, case.k
    assert (out["status"] == 0).all(), out["status"]
    worst = 0.0
    for p in range(KC.B):
        o = KC.oracle_solution(case, p, dy0=False)[j]
        assert o["status"] == 0
        e = KC.rel_errors(vectors(out, p, n, m, k), [o[key] for key in KC.KEYS])
        g = KC.gates(n, m, k, KC.oracle_errors(case, p)[j])
        for key, ev, gv in zip(KC.KEYS, e, g):
            print(f"  {case.id} p={p} rhs {j} dy != 0 {key}: e = {ev:.3g}, gate {gv:.3g}")
            worst = max(worst, ev / gv)
    note(tag + "_dy", case, worst)
    assert worst <= 1.0, (case.id, j, worst)


def fused(case, d, j, ctx=None, **kw):
    Af, Gf = KC.flat(d)
    nb = len(d["G"])
    return S.batch_kkt_solve(list(case.cones), case.n, case.m, case.k, Af, Gf, kw.pop("sing", KC.sing_bytes(case, nb)),
                             d["s"].ravel(), d["z"].ravel(), *KC.flat_rhs(d, j, case.m),
                             explicit_inverse=case.xi, ctx=ctx, **kw)


def handle(case, d, ctx=None, **kw):
    Af, Gf = KC.flat(d)
    nb = len(d["G"])
    return S.DenseHandle(list(case.cones), case.n, case.m, case.k, Af, Gf, kw.pop("sing", KC.sing_bytes(case, nb)),
                         explicit_inverse=case.xi, ctx=ctx, **kw)


@functools.lru_cache(maxsize=None)
def fused_once(case, j, dy0):
    out = fused(case, KC.inputs(case, dy0), j)
    kernel_is(case)
    return out


# ---------------------------------------------------------------- 1. fused
@pytest.mark.parametrize("case", KC.CASES, ids=KC.case_id)
def test_fused(case):
    check_gate("fused", case, fused_once(case, 0, None), 0)
    if KC.singular(case):
        check_against_sing_oracle("fused", case, fused_once(case, 0, False), 0)


# ---------------------------------------------------------------- 2. split
@pytest.mark.parametrize("case", KC.CASES, ids=KC.case_id)
def test_split(case):
    n, m, k = case.n, case.m, case.k
    for dy0 in ((None, False) if KC.singular(case) else (None,)):
        d = KC.inputs(case, dy0)
        h = handle(case, d)
        try:
            st = h.setup_iter(d["s"].ravel(), d["z"].ravel())
            kernel_is(case)
            assert (st == 0).all(), st
            assert h.h2d_bytes == KC.B * 2 * k * 8
            for j in range(KC.NRHS):
                got = h.solve_kkt(*KC.flat_rhs(d, j, m))
                kernel_is(case)
                assert h.h2d_bytes == KC.B * (n + m + 2 * k) * 8
                if dy0 is None:
                    check_gate("split", case, got, j)
                else:
                    check_against_sing_oracle("split", case, got, j)
                same(got, fused_once(case, j, dy0))
        finally:
            h.close()


# -------------------------------------------- 3. record independent of scratch
OTHER = dict(edge65="m65", xi="m65", wide="gv_wide", gv="gv_wide")


@pytest.mark.parametrize("cid", sorted(OTHER))
def test_record_is_independent_of_the_scratch_slot(cid):
    """store_record's comment: X, the pivot rows and 1/d "stay in the
    workgroup's scratch slot".  solve_kkt must not read them: the slot belongs
    to whichever problem and call a workgroup ran last."""
    case, other = KC.BY_ID[cid], KC.BY_ID[OTHER[cid]]
    d = KC.inputs(case)
    ctx = S.Context()  # a fresh workspace buffer, sized by this test's calls
    h = h2 = None
    try:
        h = handle(case, d, ctx=ctx)
        assert (h.setup_iter(d["s"].ravel(), d["z"].ravel()) == 0).all()
        kernel_is(case, ctx)
        r = KC.flat_rhs(d, 0, case.m)
        first = h.solve_kkt(*r)
        same(first, fused_once(case, 0, None))
        # a larger shape on the same context: the workspace is reallocated, every slot overwritten
        out = fused(other, KC.inputs(other), 1, ctx=ctx)
        kernel_is(other, ctx)
        assert (out["status"] == 0).all()
        # the same shape, the problems in the other order at the other iterate: the same slots, another X
        rev = dict(A=d["A"][::-1], G=d["G"][::-1])
        h2 = handle(case, rev, ctx=ctx)
        assert (h2.setup_iter(d["z"][::-1].ravel(), d["s"][::-1].ravel()) == 0).all()
        kernel_is(case, ctx)
        same(h.solve_kkt(*r), first)
        # and the second handle's record is its own
        got2 = h2.solve_kkt(*r)
        assert (got2["status"] == 0).all() and got2["cx"].tobytes() != first["cx"].tobytes()
    finally:
        for x in (h, h2):
            if x is not None:
                x.close()
        ctx.close()


# ------------------------------------------ 4. a workgroup takes several problems
SEV = KC.Case("several", 65, 40, 66, KC.BY_ID["edge65"].cones, None, False, "socp_large_kernel")


@functools.lru_cache(maxsize=None)
def several_inputs():
    import torch
    nb = 2 * torch.cuda.get_device_properties(0).multi_processor_count + 5
    odd = [p % 2 == 1 for p in range(nb)]
    d = KC.make_inputs(SEV.n, SEV.m, SEV.k, SEV.cones, odd, nb, dy_zero=[p for p in range(nb) if odd[p]])
    bad = [p for p in range(nb) if p % 97 == 96]
    o = SEV.cones[1][1]  # the SOC cone's head
    for p in bad:
        d["s"][p, o + 3] = 10.0 * d["s"][p, o]
    return d, np.array(odd, np.uint8), bad


@functools.lru_cache(maxsize=None)
def several_run():
    """The batch through the fused and the split entry, once for both tests."""
    d, sing, bad = several_inputs()
    out = fused(SEV, d, 0, sing=sing)
    kernel_is(SEV)
    h = handle(SEV, d, sing=sing)
    try:
        st = h.setup_iter(d["s"].ravel(), d["z"].ravel())
        kernel_is(SEV)
        split = h.solve_kkt(*KC.flat_rhs(d, 0, SEV.m))
        kernel_is(SEV)
    finally:
        h.close()
    return out, split, st


def test_workgroup_takes_several_problems():
    """The grid is min(CUs x workgroups per CU, B): with B = 2 CUs + 5 the
    persistent loop carries sing, dm_aa and the LDS contents of one problem's
    KKT solve into the next, which may have the other sing byte or fail.  Every
    problem has the bits of the same problem solved alone (B = 1), failing
    problems report DOMAIN_ERROR and NaN in all four vectors on both entries,
    and split equals fused."""
    n, m, k = SEV.n, SEV.m, SEV.k
    d, sing, bad = several_inputs()
    nb = len(sing)
    assert nb > 256 and len(bad) >= 2 and {p % 2 for p in bad} == {0, 1}
    out, split, st = several_run()
    same(split, out)
    good = np.ones(nb, bool)
    good[bad] = False
    assert (out["status"][good] == 0).all() and (out["status"][bad] == S.DOMAIN_ERROR).all(), out["status"]
    assert np.array_equal(st, out["status"])
    for p in range(nb):
        got = vectors(out, p, n, m, k)
        one = dict(A=d["A"][p:p + 1], G=d["G"][p:p + 1], s=d["s"][p:p + 1], z=d["z"][p:p + 1],
                   rhs=[tuple(v[p:p + 1] for v in d["rhs"][0])])
        alone = fused(SEV, one, 0, sing=sing[p:p + 1])
        assert alone["status"][0] == out["status"][p], p
        for key, v in zip(KC.KEYS, got):
            assert alone[key].tobytes() == v.tobytes(), (p, key)
            assert good[p] or np.isnan(v).all(), (p, key)


def row_residual(K, R, sol):
    """The largest block-row residual of K u = R relative to ||R||_2, formed in np.longdouble."""
    n, m, k = len(sol[0]), len(sol[1]), len(sol[2])
    r = (K.astype(np.longdouble) @ np.concatenate(sol).astype(np.longdouble) - R).astype(np.float64)
    return max(float(np.linalg.norm(x)) for x in KC.split(r, n, m, k)) / float(np.linalg.norm(R))


def test_several_problems_meet_the_gate():
    """The good problems of the batch above against the gate, each with its
    own refined reference and its own e_or.

    This case's gate is raised, as far as the forward bound and only under a
    condition that shows the cause: a vector above max(10 e_or, floor) passes
    if e <= (n + m + 2k) 2^-53 kappa_2(K) AND the solution's largest block-row
    residual (formed in long double, relative to the right-hand side) is within
    10 x the oracle's on the same problem.  Reason: on the batch's singular
    problems (kappa_2(K) about 100, e_or of cx 2e-15 to 5e-15, at the floor)
    the kernel's cx is 2e-14 to 7e-14 from the reference, 1.2 and 1.4 x the gate
    on problems 427 and 5 of 517 on MI355X.  Its block-row residuals there
    equal the oracle's (problem 5: dual row 3.1e-13 against 2.3e-13, A cx
    1.3e-14 against 2.0e-14), so it solves the system as well; the forward
    error lies in the columns of cx that G does not see, which only A cx = 0
    fixes, where the direction of the rounding error decides and the oracle's
    own error varies 7 x under one-ulp changes of G (2e-15 to 1.5e-14).  A
    numpy restatement of the kernel's order with its inverted diagonal blocks
    gives the error of plain substitution (problem 5: 1.8e-14 against 1.7e-14),
    so it is the summation order and not a weaker algorithm.  Both figures of the condition come from the oracle and the
    number format, none from the kernel.

    Before S was kept as its Cholesky factor in the KKT entries
    (socp_large.hip s_factored), S^-1 applied by symv put 187 of the 512 good
    problems above the gate, the worst (problem 56, kappa_2(H) 5.8e9) at
    e(cx) = 8.5e-2 against e_or = 5.6e-8, far beyond the forward bound too."""
    n, m, k = SEV.n, SEV.m, SEV.k
    d, sing, bad = several_inputs()
    nb = len(sing)
    out = several_run()[0]
    rows, raised = [], []
    for p in range(nb):
        if p in bad:
            continue
        rhs = [tuple(v[p] for v in d["rhs"][0])]
        ref = KC.reference_of(SEV.cones, d["A"][p], d["G"][p], d["s"][p], d["z"][p], rhs)
        assert (ref.corr <= 4 * 2.0 ** -52).all(), (p, ref.corr)
        o = KC.oracle_of(SEV.cones, d["A"][p], d["G"][p], bool(sing[p]), d["s"][p], d["z"][p], rhs, False)[0]
        assert o["status"] == 0 and out["status"][p] == 0, p
        osol, got = [o[key] for key in KC.KEYS], vectors(out, p, n, m, k)
        e_or = KC.rel_errors(osol, ref.sol[0])
        e = KC.rel_errors(got, ref.sol[0])
        cond = None
        for key, ev, eo, gv in zip(KC.KEYS, e, e_or, KC.gates(n, m, k, e_or)):
            if ev > gv:  # the raised gate: the forward bound, for a solution with the oracle's backward error
                if cond is None:
                    K = KC.kkt_matrix(SEV.cones, d["A"][p], d["G"][p], d["s"][p], d["z"][p])
                    R = np.concatenate(rhs[0])
                    cond = (KC.floor(n, m, k) * float(np.linalg.cond(K)), row_residual(K, R, got),
                            row_residual(K, R, osol))
                raised.append((p, key, ev, gv) + cond)
                if cond[1] <= 10.0 * cond[2]:
                    gv = max(gv, cond[0])
            rows.append((ev / gv, p, key, ev, eo, gv))
    rows.sort(reverse=True)
    over = [r for r in rows if r[0] > 1.0]
    print(f"several: {nb} problems; (e / gate, problem, vector, e, e_or, gate), worst first:")
    for r in rows[:12]:
        print("  %.3g p=%d %s e=%.3g e_or=%.3g gate=%.3g" % r)
    for r in raised:
        print("  above max(10 e_or, floor): p=%d %s e=%.3g gate=%.3g; forward bound %.3g, row residual %.3g, "
              "the oracle's %.3g" % r)
    print(f"several: {len(over)} of {len(rows)} vectors above the gate, on {len({r[1] for r in over})} problems")
    note("several", SEV, rows[0][0])
    assert not over, over[:8]


# ------------------------------------------------------------ 5. shared matrices
@pytest.mark.parametrize("cid", ["m65", "gv"])
def test_shared_matrices(cid):
    """One A and one G for the batch (problem 0's): the bits of the call on
    the replicated matrices, on the fused and on the split entry."""
    case = KC.BY_ID[cid]
    n, m, k = case.n, case.m, case.k
    d = KC.inputs(case)
    rep = dict(d, A=np.repeat(d["A"][:1], KC.B, axis=0), G=np.repeat(d["G"][:1], KC.B, axis=0))
    A1, G1 = KC.flat(d, 1)
    one = np.zeros(1, np.uint8)
    s, z = d["s"].ravel(), d["z"].ravel()
    ref = fused(case, rep, 0)
    kernel_is(case)
    assert (ref["status"] == 0).all()
    # problem 0 is the case's own problem 0, problem 1 another iterate on the same matrices
    for key, v, w in zip(KC.KEYS, vectors(ref, 0, n, m, k), vectors(fused_once(case, 0, None), 0, n, m, k)):
        assert v.tobytes() == w.tobytes(), key
    got = S.batch_kkt_solve(list(case.cones), n, m, k, A1, G1, one, s, z, *KC.flat_rhs(d, 0, m),
                            explicit_inverse=case.xi, shared_matrices=True)
    kernel_is(case)
    same(got, ref)
    h = S.DenseHandle(list(case.cones), n, m, k, A1, G1, one, explicit_inverse=case.xi, shared_matrices=True,
                      batch=KC.B)
    try:
        assert (h.setup_iter(s, z) == 0).all()
        kernel_is(case)
        same(h.solve_kkt(*KC.flat_rhs(d, 0, m)), ref)
        kernel_is(case)
    finally:
        h.close()
