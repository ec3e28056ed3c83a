"""Cases of the init-overlap test (test_gpu_init_overlap.py) and the child
process that solves them (the SOCP_INIT_OVERLAP switch is read at launch, so
each setting runs in a process of its own).

  python init_overlap_cases.py IN.npz OUT.npz      solve every case of IN.npz on the GPU
"""
import collections
import sys

P, Q = 0, 1  # cone kinds of include/socp.h: POC, SOC

C2_CONES = [(P, 0, 32), (Q, 32, 32), (Q, 64, 32)]
# sing: "zeros" (every problem 0), "mixed" (ones and zeros in one batch: A'A is
# added to a G'G that the load formed), "none" (the kernel probes G'G itself:
# the probe takes the load's H, the initial point rebuilds it)
# mixed: the mixed kernel (SOCP_SLOT_SPECIALISE=0) instead of the pure-slot pair
# zero_col: problem ZERO_COL_P's G has column ZERO_COL_J zeroed
Case = collections.namedtuple("Case", "name cones n m k maxit sing warm mixed zero_col oracle variant")


def case(name, cones=C2_CONES, n=64, m=16, k=96, maxit=2, sing="zeros", warm=False, mixed=False, zero_col=False,
         oracle=False, variant="<4,24,1>"):
    return Case(name, cones, n, m, k, maxit, sing, warm, mixed, zero_col, oracle, variant)


CASES = [
    # C2's shape: the initial point alone, and two iterations behind it
    case("c2_init", maxit=0, oracle=True),
    case("c2_k2", oracle=True),
    # the mixed kernel on C2's table
    case("c2_mixed_kernel", mixed=True),
    # padded columns and the padded diagonal of H
    case("n50_k96", n=50),
    # k = 90: the last row step is partial (rows 88, 89) and the 23rd is the variant's last but one
    case("k90_n64", cones=[(P, 0, 30), (Q, 30, 30), (Q, 60, 30)], k=90),
    case("sing_mixed", sing="mixed"),
    case("sing_none", sing="none"),
    # enters at MP_ITER: no initial factorisation takes the tiles
    case("c2_warm", warm=True),
    case("zero_column", zero_col=True),
]
BATCH, SEED, WARM_AT = 16, 20241020, 2
ZERO_COL_P, ZERO_COL_J = 5, 17
# A resident-G problem follows a loading one on the same wave: more problems
# than the device has waves of this kernel (one per SIMD: 4 x 256 CUs)
SHARED = dict(cones=C2_CONES, n=64, m=16, k=96, batch=2500, seed=78, maxit=2)
# Lifetime: every persistent wave loads several problems, which leave after
# different numbers of iterations (the reference rule: tol 1e-5, maxit 40)
LIFE = dict(cones=C2_CONES, n=64, m=16, k=96, batch=4096, seed=79)
KEYS = ("x", "y", "z", "s", "iters", "status")


def sing_of(c):
    import numpy as np

    if c.sing == "none":
        return None
    s = np.zeros(BATCH, np.uint8)
    if c.sing == "mixed":
        s[[1, 2, 7, 11, 15]] = 1
    return s


def main(inp, outp):
    import os

    import numpy as np

    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(here, "..", "socp.jl_amd"))
    import socp_amd as S
    import torch

    d = np.load(inp)
    out = {}
    for c in CASES:
        g = lambda key: d[f"{c.name}/{key}"]  # noqa: E731
        warm = tuple(g(f"w{q}") for q in "xyzs") if c.warm else None
        if c.mixed:
            os.environ["SOCP_SLOT_SPECIALISE"] = "0"
        else:
            os.environ.pop("SOCP_SLOT_SPECIALISE", None)
        r = S.batch_solve(c.cones, c.n, c.m, c.k, g("c"), g("A"), g("b"), g("G"), g("h"), sing_of(c),
                          maxit=c.maxit, tol=0.0, warm=warm)
        out[f"{c.name}/kernel"] = np.array(S.default_context().last_kernel_name())
        for key in KEYS:
            out[f"{c.name}/{key}"] = np.asarray(r[key])
    os.environ.pop("SOCP_SLOT_SPECIALISE", None)
    for name, L in (("shared", SHARED), ("life", LIFE)):
        cv, A, b, G, h = S.generate(L["cones"], L["batch"], L["n"], L["m"], L["k"], L["seed"])
        if name == "shared":  # the batch's one A and G: problem 0's
            A, G = A[:L["m"] * L["n"]].clone(), G[:L["k"] * L["n"]].clone()
            sing = torch.zeros(1, dtype=torch.uint8, device=G.device)
            r = S.batch_solve(L["cones"], L["n"], L["m"], L["k"], cv, A, b, G, h, sing, maxit=L["maxit"], tol=0.0,
                              shared_matrices=True)
        else:
            sing = torch.zeros(L["batch"], dtype=torch.uint8, device=G.device)
            r = S.batch_solve(L["cones"], L["n"], L["m"], L["k"], cv, A, b, G, h, sing)
        S.default_context().sync()
        out[f"{name}/kernel"] = np.array(S.default_context().last_kernel_name())
        for key in KEYS:
            out[f"{name}/{key}"] = r[key].cpu().numpy()
    np.savez(outp, **out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
