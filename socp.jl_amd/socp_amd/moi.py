"""MathOptInterface-style adapter for the HIP dense path.

Mirror of the reference's `Socp.Optimizer` (`src/moi.jl`), whose data model is
ECOS's: every constraint is `f(x) = Fx + f0 ∈ K`, stored as `b - A x ∈ Zeros`
(rows of A, b) or `h - G x ∈ K` (rows of G, h) with `A, G = -F` and
`b, h = f0` (`moi.jl:142-160`).  Nonnegatives rows come first, then the
second-order cones in the order they were added (`moi.jl:101-116`), so the cone
tuple is `POC(0, l), SOC(l, q1), SOC(l+q1, q2), ...` (`moi.jl:212-217`).

Differences from the reference, each fixing a defect that keeps `moi.jl` from
running:

* `optimize!` builds `SolverState(prob, DenseSolver(prob))` and runs on the
  GPU (the reference calls `solve_socp(prob, SparseSolver(prob))`, a solver
  object where a `SolverState` is expected, `moi.jl:220`).
* No `POC(0, 0)` when the model has no Nonnegatives rows (`moi.jl:212`).
* `scalecoef` (undefined in the reference, `moi.jl:251,257`) is the identity:
  it only rescales PSD cones, which this solver does not support.
* The dual of a `Zeros` constraint is `y` (the reference reads `z`,
  `moi.jl:254`); termination/objective getters exist.

Beyond the reference: `optimize_batched(optimizers)` solves many models in
one device launch per structure class (same n, equality rows, Nonnegatives
length and SOC dimensions) — the batched dense path this framework exists for.
"""
from __future__ import annotations

from collections import OrderedDict
from dataclasses import dataclass, field

import numpy as np

from . import (CONVERGED, MAXIT, CHOL_H_FAILED, CHOL_S_FAILED, DOMAIN_ERROR, PRIMAL_INFEASIBLE, DUAL_INFEASIBLE,
               POC, SOC, batch_solve)

MIN_SENSE, MAX_SENSE, FEASIBILITY_SENSE = "MIN_SENSE", "MAX_SENSE", "FEASIBILITY_SENSE"
OPTIMIZE_NOT_CALLED = "OPTIMIZE_NOT_CALLED"
TERMINATION = {CONVERGED: "OPTIMAL", MAXIT: "ITERATION_LIMIT", CHOL_H_FAILED: "NUMERICAL_ERROR",
               CHOL_S_FAILED: "NUMERICAL_ERROR", DOMAIN_ERROR: "NUMERICAL_ERROR",
               PRIMAL_INFEASIBLE: "INFEASIBLE", DUAL_INFEASIBLE: "DUAL_INFEASIBLE"}
# MOI.PrimalStatus / MOI.DualStatus per solver status.  The optimizer solves
# with infeasibility detection on: a primal-infeasible model returns the
# certificate (y, z) as its dual (b'y + h'z = -1) and no primal point; a
# dual-infeasible one the ray (x, s) as its primal (c'x = -1) and no dual.
FEASIBLE_POINT, NO_SOLUTION, INFEASIBILITY_CERTIFICATE, UNKNOWN_RESULT_STATUS = (
    "FEASIBLE_POINT", "NO_SOLUTION", "INFEASIBILITY_CERTIFICATE", "UNKNOWN_RESULT_STATUS")
PRIMAL_STATUS = {CONVERGED: FEASIBLE_POINT, MAXIT: UNKNOWN_RESULT_STATUS, CHOL_H_FAILED: UNKNOWN_RESULT_STATUS,
                 CHOL_S_FAILED: UNKNOWN_RESULT_STATUS, DOMAIN_ERROR: UNKNOWN_RESULT_STATUS,
                 PRIMAL_INFEASIBLE: NO_SOLUTION, DUAL_INFEASIBLE: INFEASIBILITY_CERTIFICATE}
DUAL_STATUS = {CONVERGED: FEASIBLE_POINT, MAXIT: UNKNOWN_RESULT_STATUS, CHOL_H_FAILED: UNKNOWN_RESULT_STATUS,
               CHOL_S_FAILED: UNKNOWN_RESULT_STATUS, DOMAIN_ERROR: UNKNOWN_RESULT_STATUS,
               PRIMAL_INFEASIBLE: INFEASIBILITY_CERTIFICATE, DUAL_INFEASIBLE: NO_SOLUTION}


# ------------------------------------------------------------------ MOI types
@dataclass(frozen=True)
class VariableIndex:
    value: int  # 1-based, as MOI.VariableIndex


@dataclass(frozen=True)
class ScalarAffineTerm:
    coefficient: float
    variable: VariableIndex


@dataclass(frozen=True)
class VectorAffineTerm:
    output_index: int  # 1-based row of the vector function
    scalar_term: ScalarAffineTerm


@dataclass
class ScalarAffineFunction:
    terms: list
    constant: float = 0.0


@dataclass(frozen=True)
class ScalarQuadraticTerm:
    coefficient: float
    variable_1: VariableIndex
    variable_2: VariableIndex


@dataclass
class ScalarQuadraticFunction:
    """MOI's convention: the function is x'Qx/2 + a'x + constant with Q
    symmetric; a term (c, i, i) adds c to Q[i, i], a term (c, i, j), i != j,
    adds c to Q[i, j] and to Q[j, i] (so it contributes c x_i x_j)."""
    quadratic_terms: list
    affine_terms: list
    constant: float = 0.0


@dataclass
class VectorAffineFunction:
    terms: list
    constants: list


@dataclass(frozen=True)
class Zeros:
    dimension: int


@dataclass(frozen=True)
class Nonnegatives:
    dimension: int


@dataclass(frozen=True)
class SecondOrderCone:
    dimension: int


@dataclass(frozen=True)
class ConstraintIndex:
    set_type: type
    value: int  # the reference's ci.value: offset inside the set's row class (moi.jl:101-116)


@dataclass
class _Con:
    f: VectorAffineFunction
    s: object
    ci: ConstraintIndex


@dataclass
class _Solution:
    x: np.ndarray
    y: np.ndarray
    z: np.ndarray
    s: np.ndarray
    iters: int
    status: int


@dataclass
class ModelData:
    """The packed problem of one model (moi.jl:24-37, dense here)."""
    c: np.ndarray
    A: np.ndarray  # f x n, row-major
    b: np.ndarray
    G: np.ndarray  # (l + q) x n, row-major
    h: np.ndarray
    cones: tuple
    objconstant: float = 0.0
    signature: tuple = field(default=())
    P: np.ndarray | None = None  # n x n symmetric (the solver's: negated with c under MAX_SENSE); None: linear


class Optimizer:
    """`Socp.Optimizer` (moi.jl:57-66) over the GPU dense path.  Keyword options:
    `maxit` (default 40, solver.jl:105), `tol` (1e-5, solver.jl:122), `ctx`,
    `equilibrate` and `normalise` (default False; `optimize_batched`)."""

    def __init__(self, **options):
        self.options = dict(options)
        self.empty_()

    # -- MOI.SolverName / supports / is_empty / empty! (moi.jl:68-91)
    solver_name = "SOCP.jl (MI355X dense path)"

    @staticmethod
    def supports_constraint(ftype, stype) -> bool:
        return ftype is VectorAffineFunction and stype in (Zeros, Nonnegatives, SecondOrderCone)

    def is_empty(self) -> bool:
        return self.nvars == 0 and not self.cons and self.sense != MAX_SENSE and self.sol is None

    def empty_(self):
        self.nvars = 0
        self.cons: list[_Con] = []
        self.f = self.l = self.q = 0
        self.qa: list[int] = []
        self.sense = MIN_SENSE
        self.objective = ScalarAffineFunction([], 0.0)
        self.sol: _Solution | None = None
        self.data: ModelData | None = None

    # -- variables / objective
    def add_variable(self) -> VariableIndex:
        self.nvars += 1
        return VariableIndex(self.nvars)

    def add_variables(self, n: int) -> list:
        return [self.add_variable() for _ in range(n)]

    def set_objective_sense(self, sense):
        self.sense = sense  # MOIU.allocate(::ObjectiveSense) (moi.jl:187-189)

    def set_objective_function(self, f):
        """A ScalarAffineFunction or a ScalarQuadraticFunction (whose Q, in the
        solver's sense, must be positive semidefinite; unchecked)."""
        if not isinstance(f, (ScalarAffineFunction, ScalarQuadraticFunction)):
            raise TypeError(f"unsupported objective {type(f).__name__}")
        if isinstance(f, ScalarQuadraticFunction):
            for t in f.quadratic_terms:
                for v in (t.variable_1, t.variable_2):
                    if not (1 <= v.value <= self.nvars):
                        raise ValueError(f"unknown variable {v.value}")
        self.objective = f

    # -- constraints: _allocate_constraint (moi.jl:96-116)
    def add_constraint(self, f: VectorAffineFunction, s) -> ConstraintIndex:
        if not self.supports_constraint(type(f), type(s)):
            raise TypeError(f"unsupported constraint {type(f).__name__} in {type(s).__name__}")
        if len(f.constants) != s.dimension:
            raise ValueError("function output dimension does not match the set dimension")
        for t in f.terms:
            if not (1 <= t.output_index <= s.dimension):
                raise ValueError(f"output index {t.output_index} outside 1:{s.dimension}")
            if not (1 <= t.scalar_term.variable.value <= self.nvars):
                raise ValueError(f"unknown variable {t.scalar_term.variable.value}")
        if isinstance(s, Zeros):
            ci = ConstraintIndex(Zeros, self.f)
            self.f += s.dimension
        elif isinstance(s, Nonnegatives):
            ci = ConstraintIndex(Nonnegatives, self.l)
            self.l += s.dimension
        else:
            if s.dimension < 1:
                raise ValueError("SecondOrderCone needs dimension >= 1")
            self.qa.append(s.dimension)
            ci = ConstraintIndex(SecondOrderCone, self.q)
            self.q += s.dimension
        self.cons.append(_Con(f, s, ci))
        self.sol = None
        return ci

    def _constroffset(self, ci: ConstraintIndex) -> int:
        # constroffset (moi.jl:96,102,108): SOC rows follow all Nonnegatives rows
        return self.l + ci.value if ci.set_type is SecondOrderCone else ci.value

    # -- copy_to / load (moi.jl:142-200): the packed dense problem
    def build(self) -> ModelData:
        n, f, k = self.nvars, self.f, self.l + self.q
        if n == 0:
            raise ValueError("model has no variables")
        if k == 0:
            raise ValueError("the dense path needs at least one conic (Nonnegatives or SOC) row")
        A, b = np.zeros((f, n)), np.zeros(f)
        G, h = np.zeros((k, n)), np.zeros(k)
        for con in self.cons:
            off = self._constroffset(con.ci)
            M, v = (A, b) if con.ci.set_type is Zeros else (G, h)
            rows = off + np.arange(con.s.dimension)
            v[rows] = np.asarray(con.f.constants, dtype=np.float64)
            if con.f.terms:
                I = np.array([off + t.output_index - 1 for t in con.f.terms])
                J = np.array([t.scalar_term.variable.value - 1 for t in con.f.terms])
                V = np.array([-t.scalar_term.coefficient for t in con.f.terms], dtype=np.float64)
                np.add.at(M, (I, J), V)  # MOIU.canonical merges duplicate terms (moi.jl:143)
        c0 = np.zeros(n)
        quad = isinstance(self.objective, ScalarQuadraticFunction)
        for t in (self.objective.affine_terms if quad else self.objective.terms):
            c0[t.variable.value - 1] += t.coefficient
        c = -c0 if self.sense == MAX_SENSE else c0  # moi.jl:199
        P = None
        if quad:
            Q = np.zeros((n, n))
            for t in self.objective.quadratic_terms:
                i, j = t.variable_1.value - 1, t.variable_2.value - 1
                Q[i, j] += t.coefficient
                if i != j:
                    Q[j, i] += t.coefficient
            P = -Q if self.sense == MAX_SENSE else Q
        cones = ((POC(0, self.l),) if self.l else ()) + tuple(
            SOC(self.l + sum(self.qa[:i]), d) for i, d in enumerate(self.qa))
        sig = (n, f, self.l, tuple(self.qa))
        self.data = ModelData(c, A, b, G, h, cones, float(self.objective.constant), sig, P)
        return self.data

    # -- optimize! (moi.jl:203-222)
    def optimize(self):
        optimize_batched([self])

    def _set_solution(self, x, y, z, s, iters, status):
        self.sol = _Solution(np.array(x), np.array(y), np.array(z), np.array(s), int(iters), int(status))

    # -- getters (moi.jl:240-272)
    def _need_sol(self):
        if self.sol is None:
            raise RuntimeError("optimize() has not been called since the model last changed")
        return self.sol

    def termination_status(self) -> str:
        return TERMINATION[self.sol.status] if self.sol is not None else OPTIMIZE_NOT_CALLED

    def primal_status(self) -> str:
        return PRIMAL_STATUS[self.sol.status] if self.sol is not None else NO_SOLUTION

    def dual_status(self) -> str:
        return DUAL_STATUS[self.sol.status] if self.sol is not None else NO_SOLUTION

    def result_count(self) -> int:
        return 1 if self.sol is not None else 0  # moi.jl:272 (always 1 there)

    def barrier_iterations(self) -> int:
        return self._need_sol().iters

    def variable_primal(self, vi):
        sol = self._need_sol()
        if isinstance(vi, (list, tuple)):
            return np.array([sol.x[v.value - 1] for v in vi])
        return float(sol.x[vi.value - 1])

    def objective_value(self) -> float:
        sol = self._need_sol()
        c0 = -self.data.c if self.sense == MAX_SENSE else self.data.c
        val = float(c0 @ sol.x + self.data.objconstant)
        if self.data.P is not None:  # + x'Qx/2 in the model's sense
            q = 0.5 * float(sol.x @ (self.data.P @ sol.x))
            val += -q if self.sense == MAX_SENSE else q
        return val

    def _rows(self, ci: ConstraintIndex):
        for con in self.cons:
            if con.ci == ci:
                off = self._constroffset(ci)
                return off + np.arange(con.s.dimension)
        raise KeyError(ci)

    def constraint_primal(self, ci: ConstraintIndex) -> np.ndarray:
        sol, rows = self._need_sol(), self._rows(ci)
        if ci.set_type is Zeros:  # moi.jl:245-248
            return np.zeros(len(rows))
        return sol.s[rows].copy()  # moi.jl:253-257, scalecoef = identity

    def constraint_dual(self, ci: ConstraintIndex) -> np.ndarray:
        sol, rows = self._need_sol(), self._rows(ci)
        return (sol.y if ci.set_type is Zeros else sol.z)[rows].copy()


def optimize_batched(optimizers, ctx=None, shared_matrices=False):
    """`MOI.optimize!` for many models at once: models are grouped by structure
    (n, equality rows, Nonnegatives length, SOC dimensions) and each group is one
    `socp_batch_solve` launch, with infeasibility detection on
    (SOCP_F_DETECT_INFEASIBLE).  Per-model options `maxit`/`tol` must agree within a group.
    shared_matrices=True: a parametric batch -- within every group each model's A
    and G (and with them `sing`) must equal the group's first (ValueError
    otherwise), and one copy of them goes to the device (SOCP_F_SHARED_MATRICES).
    Models built with `Optimizer(equilibrate=True)` form groups of their own and
    are solved with SOCP_F_EQUILIBRATE (``batch_solve``'s equilibrate: `tol`
    then refers to the scaled problem, and `sing` is probed on the scaled G).
    The library refuses detection together with that flag, so these groups run
    without it: an infeasible model ends with a numerical status, not a certificate.
    Models built with `Optimizer(normalise=True)` group apart in the same way and
    are solved with SOCP_F_NORMALISE (``batch_solve``'s normalise: `tol` then
    refers to the normalised problem), likewise without detection.
    Models with a quadratic objective (ScalarQuadraticFunction) form groups of
    their own as well and run ``batch_solve(P=...)`` (socp_batch_solve_qp), for
    the same reason without detection: the library refuses that pair too.  With
    shared_matrices=True every such model's P must equal the group's first."""
    groups: "OrderedDict[tuple, list]" = OrderedDict()
    for o in optimizers:
        d = o.build()
        key = d.signature + (int(o.options.get("maxit", 40)), float(o.options.get("tol", 1e-5)),
                             bool(o.options.get("equilibrate", False)), d.P is not None,
                             bool(o.options.get("normalise", False)))
        groups.setdefault(key, []).append(o)
    for key, opts in groups.items():
        n, f, l, qa = key[:4]
        maxit, tol, equil, quad, norm = key[4], key[5], key[6], key[7], key[8]
        k = l + sum(qa)
        ds = [o.data for o in opts]
        if shared_matrices:
            for i, d in enumerate(ds):
                if (f and not np.array_equal(d.A, ds[0].A)) or not np.array_equal(d.G, ds[0].G):
                    raise ValueError(f"shared_matrices=True: model {i} of its group differs from the first in A or G")
                if quad and not np.array_equal(d.P, ds[0].P):
                    raise ValueError(f"shared_matrices=True: model {i} of its group differs from the first in P")
        ms = ds[:1] if shared_matrices else ds
        sing = None if equil else np.array([_sing(d.G) for d in ms], np.uint8)
        c = np.concatenate([d.c for d in ds])
        A = np.concatenate([d.A.ravel(order="F") for d in ms]) if f else None
        b = np.concatenate([d.b for d in ds]) if f else None
        G = np.concatenate([d.G.ravel(order="F") for d in ms])
        h = np.concatenate([d.h for d in ds])
        P = np.concatenate([d.P.ravel(order="F") for d in ms]) if quad else None
        out = batch_solve(ds[0].cones, n, f, k, c, A, b, G, h, sing, maxit=maxit, tol=tol,
                          detect_infeasible=not (equil or quad or norm), equilibrate=equil, normalise=norm,
                          shared_matrices=shared_matrices, P=P,
                          ctx=ctx if ctx is not None else opts[0].options.get("ctx"))
        for i, o in enumerate(opts):
            o._set_solution(out["x"][i * n:(i + 1) * n], out["y"][i * f:(i + 1) * f],
                            out["z"][i * k:(i + 1) * k], out["s"][i * k:(i + 1) * k],
                            out["iters"][i], out["status"][i])


def _sing(G) -> bool:
    """`sing` of Problem (Socp.jl:49-56): cholesky(G'G) throws."""
    try:
        np.linalg.cholesky(G.T @ G)
        return False
    except np.linalg.LinAlgError:
        return True


def vaf(rows, constants):
    """Shorthand: VectorAffineFunction from [(output_index, VariableIndex, coef), ...]."""
    return VectorAffineFunction([VectorAffineTerm(i, ScalarAffineTerm(float(a), v)) for i, v, a in rows],
                                [float(x) for x in constants])


def saf(terms, constant=0.0):
    """Shorthand: ScalarAffineFunction from [(VariableIndex, coef), ...]."""
    return ScalarAffineFunction([ScalarAffineTerm(float(a), v) for v, a in terms], float(constant))


def sqf(quadratic, affine=(), constant=0.0):
    """Shorthand: ScalarQuadraticFunction from [(VariableIndex, VariableIndex, coef), ...] and saf's terms."""
    return ScalarQuadraticFunction([ScalarQuadraticTerm(float(a), u, v) for u, v, a in quadratic],
                                   [ScalarAffineTerm(float(a), v) for v, a in affine], float(constant))
