"""What a quadratic objective costs (socp_batch_solve_qp; measuring tool, not a test).

  python tools/bench_qp.py [--shape c2] [--batch 65536] [--k 8] [--reps 11]

One seeded parametric batch (tests/qp_cases.py shared_batch) at fixed K, tol 0,
device pointers.  Four forms of the same data, interleaved in one process, two
series each (a1 b1 c1 d1 a2 b2 c2 d2 per round), medians of --reps after a
warm-up round; the difference of a form's two series is the A/A spread to read
the differences against:
  plain      per-problem A and G, linear objective (socp_batch_solve_ex)
  qp         the same with a per-problem P
  plain_sh   SOCP_F_SHARED_MATRICES, linear objective
  qp_sh      SOCP_F_SHARED_MATRICES with the batch's one P
Times are the solver kernel's (HIP events, socp_last_kernel_ms).
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "socp.jl_amd"))
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import socp_amd as S  # noqa: E402
from qp_cases import shared_batch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="c2")
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--reps", type=int, default=11)
    a = ap.parse_args()
    B, K = a.batch, a.k
    d = shared_batch(a.shape, B)
    cones, n, m, k = d.shape[:4]
    ctx = S.default_context()
    dev = torch.device("cuda", 0)
    t = lambda v: torch.from_numpy(v).to(dev)  # noqa: E731
    c, b, h, A1, G1, P1 = t(d.c), t(d.b), t(d.h), t(d.A), t(d.G), t(d.P)
    AB, GB, PB = A1.repeat(B), G1.repeat(B), P1.repeat(B)
    s1 = torch.zeros(1, dtype=torch.uint8, device=dev)
    sB = torch.zeros(B, dtype=torch.uint8, device=dev)
    forms = dict(plain=(AB, GB, sB, None, False), qp=(AB, GB, sB, PB, False), plain_sh=(A1, G1, s1, None, True),
                 qp_sh=(A1, G1, s1, P1, True))
    series = [(f, i) for i in (1, 2) for f in forms]
    times = {key: [] for key in series}
    outs, names = {}, {}
    for rnd in range(a.reps + 1):  # round 0 warms up
        for key in series:
            A, G, sing, P, sh = forms[key[0]]
            outs[key] = S.batch_solve(list(cones), n, m, k, c, A, b, G, h, sing, shared_matrices=sh, P=P,
                                      out=outs.get(key), maxit=K, tol=0.0, res=True)
            ctx.sync()
            names[key[0]] = ctx.last_kernel_name()
            if rnd:
                times[key].append(ctx.last_kernel_ms())
    med = {key: float(np.median(v)) for key, v in times.items()}
    print(f"device {torch.cuda.get_device_name(0)}; shape {a.shape} n={n} m={m} k={k}, batch {B}, K={K}, tol 0, "
          f"medians of {a.reps} (ms)")
    base = {}
    for f in forms:
        m1, m2 = med[(f, 1)], med[(f, 2)]
        base[f] = 0.5 * (m1 + m2)
        st = torch.bincount(outs[(f, 1)]["status"].long(), minlength=7).tolist()
        print(f"  {f:9s} {names[f]:34s} series {m1:8.3f} {m2:8.3f}  mean {base[f]:8.3f}  A/A spread {abs(m1 - m2):.3f}"
              f"  status counts {st}")
    for q, p in (("qp", "plain"), ("qp_sh", "plain_sh")):
        print(f"  {q} - {p} = {base[q] - base[p]:+.3f} ms ({100 * (base[q] - base[p]) / base[p]:+.2f} %)")


if __name__ == "__main__":
    main()
