"""Cone tables of the slot-plan tests (test_slot_plan.py, test_gpu_slot_kinds.py)
and the child process that solves them (the SOCP_SLOT_SPECIALISE switch is read
at launch, so each setting runs in a process of its own).

  python slot_cases.py IN.npz OUT.npz      solve every case of IN.npz on the GPU
"""
import collections
import sys

MIXED, SOC_ONLY, POC_ONLY = 0, 1, 2
P, Q = 0, 1  # cone kinds of include/socp.h: POC, SOC

Case = collections.namedtuple("Case", "name cones n m k warm")
# n = 32, m = 16: variant <2,24,1> for k = 96, <2,32,1> for k = 128.  The C API
# takes POC cones before SOC cones only (scalings.jl:102), so three tables of
# the kind SOC32+POC64, POC16+SOC48+POC32, SOC20+POC50+SOC26 cannot reach a
# kernel (INVALID_TABLES: SOCP_E_INVALID, test_slot_plan.py); what they would
# have covered runs on POC-first tables: a non-separable table of aligned
# cones, an unaligned table with both kinds in a slot, and a second row count.
CASES = [
    Case("c2_poc32_soc32_soc32", [(P, 0, 32), (Q, 32, 32), (Q, 64, 32)], 32, 16, 96, False),
    Case("soc32x3", [(Q, 0, 32), (Q, 32, 32), (Q, 64, 32)], 32, 16, 96, False),
    Case("lp_poc96", [(P, 0, 96)], 32, 16, 96, False),
    Case("poc32_soc64", [(P, 0, 32), (Q, 32, 64)], 32, 16, 96, False),
    Case("k128_poc64_soc64", [(P, 0, 64), (Q, 64, 64)], 32, 16, 128, False),
    Case("poc16_soc16x5", [(P, 0, 16)] + [(Q, 16 + 16 * j, 16) for j in range(5)], 32, 16, 96, False),
    Case("poc50_soc20_soc26", [(P, 0, 50), (Q, 50, 20), (Q, 70, 26)], 32, 16, 96, False),
    Case("poc16x2_soc16x4", [(P, 0, 16), (P, 16, 16)] + [(Q, 32 + 16 * j, 16) for j in range(4)], 32, 16, 96, False),
    Case("c2_warm", [(P, 0, 32), (Q, 32, 32), (Q, 64, 32)], 32, 16, 96, True),
]
INVALID_TABLES = [
    ([(Q, 0, 32), (P, 32, 64)], 96),
    ([(P, 0, 16), (Q, 16, 48), (P, 64, 32)], 96),
    ([(Q, 0, 20), (P, 20, 50), (Q, 70, 26)], 96),
]
BATCH, SEED, FIXED_K, WARM_AT = 16, 20240917, 4, 2


def main(inp, outp):
    import os

    import numpy as np

    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(here, "..", "socp.jl_amd"))
    import socp_amd as S

    d = np.load(inp)
    out = {}
    for c in CASES:
        g = lambda key: d[f"{c.name}/{key}"]  # noqa: E731
        warm = tuple(g(f"w{q}") for q in "xyzs") if c.warm else None
        r = S.batch_solve(c.cones, c.n, c.m, c.k, g("c"), g("A"), g("b"), g("G"), g("h"), np.zeros(BATCH, np.uint8),
                          maxit=FIXED_K - (WARM_AT if c.warm else 0), tol=0.0, warm=warm)
        out[f"{c.name}/kernel"] = np.array(S.default_context().last_kernel_name())
        for key in ("x", "y", "z", "s", "iters", "status"):
            out[f"{c.name}/{key}"] = np.asarray(r[key])
    np.savez(outp, **out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
