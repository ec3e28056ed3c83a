"""SOCP_F_EQUILIBRATE on the CPU: properties of the numpy restatement of the
scaling rule (tests/equil_cases.py), and what the scaling does to the CPU
oracle in the kernels' operation order on the batch the GPU rescue test uses.
"""
import numpy as np
import pytest

import equil_cases as Q
from infeasible import in_cone

CLEAN = [("m0", False), ("s16", False), ("two", False), ("blk", False), ("m0", True), ("s16", True), ("two", True),
         ("blk", True)]


@pytest.mark.parametrize("name,with_P", CLEAN)
def test_restatement_properties(name, with_P):
    """Every SOC cone has one factor; the fixed point is reached (one more pass
    on the scaled data gives all-ones factors); and there every column norm,
    every row norm of A, every POC row norm of G and every SOC cone's largest
    row norm lies in [1/2, 2)."""
    d = Q.bad_batch(name, 8, 2, 12, with_P)
    cones, n, m, k = d.shape
    sc = Q.restate(d)
    for p in range(d.B):
        for kind, o, dim in cones:
            if kind == Q.Q_:
                assert (sc.ef[p, o:o + dim] == sc.ef[p, o]).all()
        Pm, A, G = Q.mats(d, p)
        Ph, Ah, Gh = Q.scale_set(Pm, A, G, sc.ed[p], sc.ee[p], sc.ef[p])
        again = Q.exponents(cones, Ph, Ah, Gh, passes=1)
        assert all((e == 0).all() for e in again), (name, p)
        zero = np.zeros
        cn, ra, rg = Q.norms(cones, Ph, Ah, Gh, zero(n, np.int64), zero(m, np.int64), zero(k, np.int64))
        for v in (cn, ra, rg):
            assert ((v >= 0.5) & (v < 2.0)).all(), (name, p, v.min(), v.max())


def test_increment_of_special_norms():
    """Zero, Inf and NaN give 0; a subnormal is read by its true exponent; the
    powers of two around 1 land in [1/2, 2)."""
    v = np.array([0.0, np.inf, np.nan, 5e-324, 2.0 ** -1022, 0.5, 0.99, 1.0, 1.99, 2.0, 4.0, 2.0 ** 1023])
    want = [0, 0, 0, 537, 511, 0, 0, 0, 0, -1, -1, -512]
    assert Q.t_of(v).tolist() == want
    ok = np.isfinite(v) & (v > 0)
    after = np.ldexp(v[ok], 2 * Q.t_of(v)[ok])  # a row and a column both move
    assert ((after >= 0.5) & (after < 2.0)).all()


def test_decorated_inputs_freeze_their_factors():
    d = Q.decorated_batch("s16", True)
    cones, n, m, k = d.shape
    sc = Q.restate(d)
    assert sc.ed[0, 1] == 0 and sc.ef[0, 0] == 0          # zero column, zero POC row
    assert sc.ed[1, 2] == 0 and sc.ef[1, 5] == 0          # the NaN's column and (POC) row
    assert sc.ed[2, n - 1] == 0 and sc.ee[2, m - 1] == 0  # the Inf's column and row
    assert sc.ef[4, 2] == Q.CLAMP                         # a subnormal-only POC row runs into the clamp
    assert np.isfinite(sc.D).all() and (sc.D > 0).all()


def test_all_ones_factors():
    sc = Q.restate(Q.ones_batch())
    assert (sc.D == 1).all() and (sc.E == 1).all() and (sc.F == 1).all()


def test_passes_needed_on_spread_20():
    """2^+-20 per row and column: 6 passes reach the fixed point, 4 do not,
    and 1 pass differs from the default 8."""
    d = Q.spread20_batch()
    cones = d.shape.cones
    fixed = {}
    for passes in (1, 4, 6, 8):
        sc = Q.restate(d, passes)
        ok = True
        for p in range(d.B):
            Pm, A, G = Q.mats(d, p)
            _, Ah, Gh = Q.scale_set(Pm, A, G, sc.ed[p], sc.ee[p], sc.ef[p])
            ok = ok and all((e == 0).all() for e in Q.exponents(cones, None, Ah, Gh, passes=1))
        fixed[passes] = ok
    assert fixed == {1: False, 4: False, 6: True, 8: True}, fixed
    assert not np.array_equal(Q.restate(d, 1).ef, Q.restate(d, 8).ef)


def test_oracle_rescued_by_the_scaling(oracle):
    """(16,4,24), generator seed 2, 32 problems, spread 2^+-12, the oracle in
    the kernels' operation order (F_STRUCTURED | F_CHOLSOLVE, default params):
    as given at least 16 of 32 end with a non-zero status (measured 22 to 26
    over three seeds); after the restatement's scaling all 32 converge, and the
    unscaled outputs satisfy Gx + s = h and cone membership."""
    O = oracle
    d = Q.bad_batch("s16", 32, 2, 12)
    cones, n, m, k = d.shape
    pr = O.Params(flags=O.F_STRUCTURED | O.F_CHOLSOLVE)
    raw = O.batch_solve(list(cones), n, m, k, d.c, d.A, d.b, d.G, d.h, params=pr)
    nbad = int((np.asarray(raw["status"]) != 0).sum())
    print(f"as given: {nbad} of 32 not converged, statuses {sorted(set(np.asarray(raw['status']).tolist()))}")
    assert nbad >= 16
    sc = Q.restate(d)
    got = O.batch_solve(list(cones), n, m, k, sc.c, sc.A, sc.b, sc.G, sc.h, params=pr)
    assert (np.asarray(got["status"]) == 0).all(), got["status"]
    x, y, z, s = Q.unscale(d, sc, *(np.asarray(got[q], dtype=np.float64) for q in "xyzs"))
    for p in range(d.B):
        _, A, G = Q.mats(d, p)
        xp, sp, zp = x[p * n:(p + 1) * n], s[p * k:(p + 1) * k], z[p * k:(p + 1) * k]
        hp = d.h[p * k:(p + 1) * k]
        # F (Gx + s - h) is the scaled problem's third linear residual.  The exit test (solver.jl:122)
        # leaves it out; the initial point's cone shift makes it non-zero, and every Newton step
        # multiplies it by the factor that multiplies rd and rp.  It is held to the tolerance those two
        # meet, in the same scaled units (measured: at most 2.2e-7).
        r = np.ldexp(G @ xp + sp - hp, sc.ef[p])
        assert np.linalg.norm(r) < 1e-5, (p, np.linalg.norm(r))
        assert in_cone(cones, sp) and in_cone(cones, zp), p
