"""DESIGN.md §24's centring table from tests/vjp_cases.py (CPU only: the numpy /
oracle restatement, no GPU).

  python tools/vjp_table.py > profiles/r20_vjp_table.txt

Per shape of vjp_cases.TABLE_SHAPES, 8 problems with P from
qp_reference(tol = 1e-5)'s final iterate: the worst relative gradient error
against true_gradient (the largest over dc, db, dh, dP, dA, dG of
|g - g_true|_2 / |g_true|_2) and the worst off-centre measure
|lam o lam - mu e|_2 / mu after j = 0 .. 4 reference centring steps.
tests/test_vjp_cpu.py::test_centring_table asserts what the table shows.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for d in ("oracle", "tests", "socp.jl_amd"):
    sys.path.insert(0, os.path.join(HERE, "..", d))
import oracle as O  # noqa: E402

O.build()
import vjp_cases as V  # noqa: E402


def main():
    steps = range(V.STEPS + 1)
    print("worst relative gradient error over 8 problems, by centring steps")
    print("steps " + " ".join(f"{name:>8s}" for name in V.TABLE_SHAPES))
    tab = {name: V.table(name) for name in V.TABLE_SHAPES}
    for j in steps:
        print(f"{j:5d} " + " ".join(f"{max(r['err'][j] for r in tab[name]):8.1e}" for name in V.TABLE_SHAPES))
    print("worst off-centre measure, by centring steps")
    for j in steps:
        print(f"{j:5d} " + " ".join(f"{max(r['off'][j] for r in tab[name]):8.1e}" for name in V.TABLE_SHAPES))
    print("per problem: z's at the start and after 4 steps; |x - x_exact| / |x_exact| at the start and after 4 steps")
    import numpy as np
    for name in V.TABLE_SHAPES:
        for p, r in enumerate(tab[name]):
            xe = r["exact"][0]
            rel = [float(np.linalg.norm(r["pts"][j][0] - xe) / np.linalg.norm(xe)) for j in (0, V.STEPS)]
            gap = [float(r["pts"][j][2] @ r["pts"][j][3]) for j in (0, V.STEPS)]
            print(f"{name:4s} p={p} z's {gap[0]:.3e} {gap[1]:.3e}  x {rel[0]:.1e} {rel[1]:.1e}  "
                  f"errors {' '.join(f'{e:.1e}' for e in r['err'])}")


if __name__ == "__main__":
    main()
