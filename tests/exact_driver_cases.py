"""Cases of the exact-fit driver test (test_gpu_exact_driver.py) and the child
process that solves them, in the scheme of exact_fit_cases.py (the
SOCP_EXACT_FIT switch is read at launch, so each setting runs in a process of
its own; the geometry, the seed and the generated problems are that file's).

  python exact_driver_cases.py IN.npz OUT.npz    solve every case of IN.npz on the GPU

The cases are the paths of the exact-fit kernel's driver (socp_small.hpp
run_exact) that exact_fit_cases.py does not pin down: the exits of an
iteration trip before and after the residuals, one iteration, problems of one
batch leaving at different iterations with `res` written, the probe trip
followed by the rebuilt initial point and its failure, a warm start that only
forms the residual norms, and waves that take new problems after early exits.
"""
import collections
import sys

from exact_fit_cases import BAD_P, CONES, K, KEYS, M, N

# sing: "zeros" or "none" (the kernel probes G'G itself)
# warm_from: the warm start is that case's result of the same child
# zero_G / zero_A: problem BAD_P's column ZCOL of G / of A is zeroed
Case = collections.namedtuple("Case", "name batch maxit tol sing res warm_from zero_G zero_A healthy")


def case(name, batch, maxit, tol=0.0, sing="zeros", res=False, warm_from=None, zero_G=False, zero_A=False,
         healthy=None):
    return Case(name, batch, maxit, tol, sing, res, warm_from, zero_G, zero_A, healthy)


ZCOL = 17
CASES = [
    case("maxit0", 7, 0),                      # the initial point only: leaves before the residuals
    case("maxit0_res", 7, 0, res=True),        # ... after them: the initial point's residual norms
    case("maxit1", 7, 1),
    case("tol_res", 96, 40, tol=1e-5, res=True),  # the reference rule: leave at different iterations
    case("probe", 7, 3, sing="none"),
    # G'G singular (a zero column): the probe says so, the initial point is rebuilt with A'A
    case("probe_sing", 7, 3, sing="none", zero_G=True, healthy="probe"),
    # ... and A's column zero as well: chol(H) fails at the rebuilt initial point
    case("probe_fail", 7, 3, sing="none", zero_G=True, zero_A=True, healthy="probe"),
    case("warm_res_only", 7, 0, res=True, warm_from="maxit1"),  # enters at an iteration trip, forms res, leaves
]
ORACLE_CASES = ("maxit0", "maxit1")
# more problems than the device has waves of this kernel, under the reference rule at maxit = 3
MANY_RULE = dict(batch=1100, seed=83, maxit=3, tol=1e-5)
# (nothing converges within 3 iterations: every problem leaves through the maxit exit.)  The same batch at
# the rule's own maxit = 40: waves take their further problems after problems left at different iterations
MANY_RULE40 = dict(batch=1100, seed=83, maxit=40, tol=1e-5)


def main(inp, outp):
    import os

    import numpy as np

    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(here, "..", "socp.jl_amd"))
    import socp_amd as S
    import torch
    from socp_amd import _lib

    d = np.load(inp)
    out = {}
    for c in CASES:
        B = c.batch
        cv, A, b, G, h = (d[key][:B * L].copy() for key, L in (("c", N), ("A", M * N), ("b", M), ("G", K * N), ("h", K)))
        if c.zero_G:
            o = BAD_P * K * N + ZCOL * K  # column-major k x n per problem
            G[o:o + K] = 0.0
        if c.zero_A:
            o = BAD_P * M * N + ZCOL * M  # column-major m x n per problem
            A[o:o + M] = 0.0
        warm = tuple(out[f"{c.warm_from}/{q}"] for q in "xyzs") if c.warm_from else None
        fl = _lib.F_WARM_START if warm else 0
        out[f"{c.name}/exact"] = np.array(S.exact_fit(CONES, N, M, K, flags=fl))
        sing = None if c.sing == "none" else np.zeros(B, np.uint8)
        r = S.batch_solve(CONES, N, M, K, cv, A, b, G, h, sing, maxit=c.maxit, tol=c.tol, warm=warm, res=c.res)
        out[f"{c.name}/kernel"] = np.array(S.default_context().last_kernel_name())
        for key in KEYS + (("res",) if c.res else ()):
            out[f"{c.name}/{key}"] = np.asarray(r[key])
    L = MANY_RULE
    cv, A, b, G, h = S.generate(CONES, L["batch"], N, M, K, L["seed"])
    sing = torch.zeros(L["batch"], dtype=torch.uint8, device=G.device)
    for name, L in (("many_rule", MANY_RULE), ("many_rule40", MANY_RULE40)):
        r = S.batch_solve(CONES, N, M, K, cv, A, b, G, h, sing, maxit=L["maxit"], tol=L["tol"])
        S.default_context().sync()
        out[f"{name}/exact"] = np.array(S.exact_fit(CONES, N, M, K, flags=_lib.F_DEVICE_PTRS))
        out[f"{name}/kernel"] = np.array(S.default_context().last_kernel_name())
        for key in KEYS:
            out[f"{name}/{key}"] = r[key].cpu().numpy()
    np.savez(outp, **out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
