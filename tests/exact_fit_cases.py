"""Cases of the exact-fit test (test_gpu_exact_fit.py) and the child process
that solves them (the SOCP_EXACT_FIT switch is read at launch, so each setting
runs in a process of its own).

  python exact_fit_cases.py IN.npz OUT.npz      solve every case of IN.npz on the GPU

Every case is at the one geometry the kernel is compiled for: n = 64, m = 16,
k = 96, POC32 + SOC32 + SOC32.
"""
import collections
import sys

P, Q = 0, 1  # cone kinds of include/socp.h: POC, SOC
CONES = [(P, 0, 32), (Q, 32, 32), (Q, 64, 32)]
N, M, K = 64, 16, 96
SEED = 20261021
NGEN = 96  # host problems generated once; a case of B problems takes the first B

# sing: "zeros", "mixed" (ones and zeros in one batch: A'A added) or "none" (the kernel
# probes G'G itself)
# warm: K more iterations from the case `warm_from`'s result of the same child
# zero_col / nan_h: problem BAD_P's G has column BAD_J zeroed / its h a NaN at BAD_I
# healthy: the case with the same data and parameters and no defect
Case = collections.namedtuple("Case", "name batch maxit sing res warm_from zero_col nan_h shared healthy")


def case(name, batch, maxit=8, sing="zeros", res=False, warm_from=None, zero_col=False, nan_h=False, shared=False,
         healthy=None):
    return Case(name, batch, maxit, sing, res, warm_from, zero_col, nan_h, shared, healthy)


CASES = [
    case("b1", 1),
    case("b7", 7),
    case("b96", 96),
    case("b7_k2", 7, maxit=2),  # (also against the oracle)
    case("sing_mixed", 96, sing="mixed"),
    case("sing_none", 7, sing="none"),
    case("res", 7, res=True),
    case("warm", 7, maxit=3, warm_from="b7_k2"),  # enters at MP_ITER: no forming load
    case("zero_column", 7, zero_col=True, healthy="b7"),
    case("nan_in_h", 7, nan_h=True, healthy="b7"),
    case("shared", 96, shared=True),
]
BAD_P, BAD_J, BAD_I = 3, 17, 40
# more problems than the device has waves of this kernel (one per SIMD: 4 x 256 CUs):
# the persistent loop takes a second problem on a kernel that holds constants
MANY = dict(batch=1100, seed=81, maxit=2)
# the reference stopping rule: problems leave at different iterations
RULE = dict(batch=256, seed=82, maxit=40, tol=1e-5)
KEYS = ("x", "y", "z", "s", "iters", "status")


def sing_of(c):
    import numpy as np

    if c.sing == "none":
        return None
    s = np.zeros(1 if c.shared else c.batch, np.uint8)
    if c.sing == "mixed":
        s[[1, 2, 7, 11, 15, 64, 95]] = 1
    return s


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
        if c.zero_col:
            o = BAD_P * K * N + BAD_J * K  # column-major k x n per problem
            G[o:o + K] = 0.0
        if c.nan_h:
            h[BAD_P * K + BAD_I] = np.nan
        if c.shared:  # the batch's one A and G: problem 0's
            A, G = A[:M * N], G[:K * N]
        warm = tuple(out[f"{c.warm_from}/{q}"] for q in "xyzs") if c.warm_from else None
        fl = (_lib.F_WARM_START if warm else 0) | (_lib.F_SHARED_MATRICES if c.shared else 0)
        out[f"{c.name}/exact"] = np.array(S.exact_fit(CONES, N, M, K, flags=fl))
        r = S.batch_solve(CONES, N, M, K, cv, A, b, G, h, sing_of(c), maxit=c.maxit, tol=0.0, warm=warm, res=c.res,
                          shared_matrices=c.shared)
        out[f"{c.name}/kernel"] = np.array(S.default_context().last_kernel_name())
        for key in KEYS + (("res",) if c.res else ()):
            out[f"{c.name}/{key}"] = np.asarray(r[key])
    for name, L in (("many", MANY), ("rule", RULE)):
        cv, A, b, G, h = S.generate(CONES, L["batch"], N, M, K, L["seed"])
        sing = torch.zeros(L["batch"], dtype=torch.uint8, device=G.device)
        r = S.batch_solve(CONES, N, M, K, cv, A, b, G, h, sing, maxit=L["maxit"], tol=L.get("tol", 0.0))
        S.default_context().sync()
        out[f"{name}/exact"] = np.array(S.exact_fit(CONES, N, M, K, flags=_lib.F_DEVICE_PTRS))
        out[f"{name}/kernel"] = np.array(S.default_context().last_kernel_name())
        for key in KEYS:
            out[f"{name}/{key}"] = r[key].cpu().numpy()
    np.savez(outp, **out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
