"""Cone tables of the fused-U test (test_gpu_fuse_u.py) and the child process
that solves them (the SOCP_FUSE_U switch is read at launch, so each setting
runs in a process of its own).

  python fuse_u_cases.py IN.npz OUT.npz      solve every case of IN.npz on the GPU
"""
import collections
import sys

P, Q = 0, 1  # cone kinds of include/socp.h: POC, SOC

Case = collections.namedtuple("Case", "name cones n m k warm variant")
# The residuals' G x pass forms U on tables whose cones are all 32 or all 64
# long (a G x chunk is 8 row steps = 32 rows, so a chunk lies in one cone).
CASES = [
    # C2's own variant, SOC+POC kernel by rotation: a cone is exactly one chunk
    Case("c2_n64", [(P, 0, 32), (Q, 32, 32), (Q, 64, 32)], 64, 16, 96, False, "<4,24,1>"),
    # the mixed kernel on a fused table
    Case("soc32x3", [(Q, 0, 32), (Q, 32, 32), (Q, 64, 32)], 32, 16, 96, False, "<2,24,1>"),
    # a cone spans two chunks: the accumulators cross the chunk boundary
    Case("k128_poc64_soc64", [(P, 0, 64), (Q, 64, 64)], 32, 16, 128, False, "<2,32,1>"),
    # no SOC cone: nothing is flushed, no U row is written
    Case("lp_poc96", [(P, 0, 96)], 32, 16, 96, False, "<2,24,1>"),
    # enters at MP_ITER: the first factorisation already takes a fused U
    Case("c2_n64_warm", [(P, 0, 32), (Q, 32, 32), (Q, 64, 32)], 64, 16, 96, True, "<4,24,1>"),
    # Tables that keep compute_U() under either setting.  Cones of 16 rows
    # (half a chunk; and the one-slot shape, chunks of 8 then 4 row steps):
    # aligned, but two cones share a chunk
    Case("poc16_soc16x5", [(P, 0, 16)] + [(Q, 16 + 16 * j, 16) for j in range(5)], 32, 16, 96, False, "<2,24,1>"),
    Case("k48_poc16_soc16x2", [(P, 0, 16), (Q, 16, 16), (Q, 32, 16)], 32, 16, 48, False, "<2,12,1>"),
    # unaligned cones; unequal dims
    Case("poc50_soc20_soc26", [(P, 0, 50), (Q, 50, 20), (Q, 70, 26)], 32, 16, 96, False, "<2,24,1>"),
    Case("poc32_soc64", [(P, 0, 32), (Q, 32, 64)], 32, 16, 96, False, "<2,24,1>"),
]
BATCH, SEED, FIXED_K, WARM_AT = 16, 20241019, 4, 2
# Flag lifetime: every persistent wave takes several problems, which leave
# MP_ITER at different iterations (the reference rule: tol 1e-5, maxit 40).
# Generated on the device by the child (the same generator, the same seed).
LIFE = dict(cones=[(P, 0, 32), (Q, 32, 32), (Q, 64, 32)], n=32, m=16, k=96, batch=4096, seed=77)
KEYS = ("x", "y", "z", "s", "iters", "status")


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
        r = S.batch_solve(c.cones, c.n, c.m, c.k, g("c"), g("A"), g("b"), g("G"), g("h"), np.zeros(BATCH, np.uint8),
                          maxit=FIXED_K - (WARM_AT if c.warm else 0), tol=0.0, warm=warm)
        out[f"{c.name}/kernel"] = np.array(S.default_context().last_kernel_name())
        for key in KEYS:
            out[f"{c.name}/{key}"] = np.asarray(r[key])
    L = LIFE
    cv, A, b, G, h = S.generate(L["cones"], L["batch"], L["n"], L["m"], L["k"], L["seed"])
    sing = torch.zeros(L["batch"], dtype=torch.uint8, device=G.device)
    for name, res in (("life", False), ("life_res", True)):
        r = S.batch_solve(L["cones"], L["n"], L["m"], L["k"], cv, A, b, G, h, sing, res=res)
        S.default_context().sync()
        for key in KEYS + (("res",) if res else ()):
            out[f"{name}/{key}"] = r[key].cpu().numpy()
    np.savez(outp, **out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
