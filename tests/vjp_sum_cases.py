"""Gradients of a shared-matrix batch (socp_batch_vjp_sum): points, the
reference sums and the gate.  Helpers only, no tests.

points         random interior points of qp_cases.shared_batch(name, B), not
               solutions: the adjoint is defined at any interior (s, z), so no
               CPU solve is needed;
sum_reference  the three sums of include/socp.h in np.longdouble from the
               entry's own ux, uy, uz, status and the inputs x, y, z, gs, with
               w = uz + gs exact in that precision, and per element the sum of
               the absolute values of the terms, T;
gate           (2 B_on + 4) 2^-53 T per element, derived, not measured: a term
               passes through at most 2 (problems of its slab) accumulations of
               the matrix instruction, one addition per slab in the combine
               step, w's own rounding and dP's symmetrisation, and that count is
               at most 2 B + 4 for every B >= 1 with slabs of at least 4
               problems (the kernel keeps a tile's two chains in two
               accumulators, so its depth is (problems of the slab) + 1 there:
               smaller).  The reference's own error is B 2^-64 T: nothing here.
"""
import collections
import functools

import numpy as np

import qp_cases as QC
from shared_cases import interior

U = 2.0 ** -53
LD = np.longdouble
SUMS = ("dP", "dA", "dG")
VEC = ("dc", "db", "dh", "ux", "uy", "uz")

Points = collections.namedtuple("Points", "sh x y z s gx gy gz gs")


@functools.lru_cache(maxsize=None)
def points(name, B):
    """shared_batch(name, B) with (B, q) arrays: x, y, gx, gy, gz, gs seeded
    standard normals, z and s interior."""
    sh = QC.shared_batch(name, B)
    cones, n, m, k, _ = sh.shape
    rng = np.random.default_rng([n, m, k, B, 7])
    nrm = lambda q: rng.standard_normal((B, q))  # noqa: E731
    x, y = nrm(n), nrm(m)
    z, s = interior(rng, cones, B, k), interior(rng, cones, B, k)
    return Points(sh, x, y, z, s, nrm(n), nrm(m), nrm(k), nrm(k))


def col(M):
    """A matrix as the library lays it out: column-major, flat."""
    return np.ascontiguousarray(np.asarray(M).ravel(order="F"))


def sum_reference(x, y, z, gs, ux, uy, uz, status):
    """{key: (sum, T)} for dG, dA (absent when m = 0) and dP, flat column-major
    np.longdouble: the sums over the problems with status 0 and, per element,
    the sums of the absolute values of their terms.  All arguments (B, q)."""
    on = np.asarray(status) == 0
    f = lambda v: np.asarray(v, LD)[on]  # noqa: E731
    x, z, ux, w = f(x), f(z), f(ux), f(uz) + f(gs)
    out = {}
    out["dG"] = (-(z.T @ ux + w.T @ x), np.abs(z).T @ np.abs(ux) + np.abs(w).T @ np.abs(x))
    if np.asarray(y).shape[1]:
        y, uy = f(y), f(uy)
        out["dA"] = (-(y.T @ ux + uy.T @ x), np.abs(y).T @ np.abs(ux) + np.abs(uy).T @ np.abs(x))
    M, TM = ux.T @ x, np.abs(ux).T @ np.abs(x)
    out["dP"] = (-(M + M.T) / 2, (TM + TM.T) / 2)
    return {key: (col(v), col(t)) for key, (v, t) in out.items()}


def gate(B_on):
    """The allowance per unit of T."""
    return (2 * B_on + 4) * U


def worst(got, ref, T, B_on):
    """max |got - ref| / (gate(B_on) T) over the elements with T > 0; the others
    must be exactly zero."""
    got = np.asarray(got)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all()
    assert (got[T == 0] == 0.0).all()
    nz = T > 0
    if not nz.any():
        return 0.0
    return float(np.max(np.abs(got.astype(LD)[nz] - ref[nz]) / (gate(B_on) * T[nz])))
