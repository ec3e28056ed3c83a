"""What P costs in the fused KKT plugin entry (socp_batch_kkt_solve_qp against
socp_batch_kkt_solve; measuring tool, not a test).

  python tools/bench_qp_kkt.py [--shape c2] [--batch 65536] [--reps 11]

One seeded batch at an interior iterate (tests/kkt_cases.py interior, one
standard normal right-hand side), device pointers.  Four forms of the same
data, interleaved in one process, two series each (a1 b1 c1 d1 a2 b2 c2 d2 per
round), medians of --reps after a warm-up round; the difference of a form's two
series is the A/A spread to read the differences against:
  plain      per-problem A and G (socp_batch_kkt_solve)
  qp         the same with a per-problem P (socp_batch_kkt_solve_qp)
  plain_sh   SOCP_F_SHARED_MATRICES
  qp_sh      SOCP_F_SHARED_MATRICES with the batch's one P
Times are the kernel's (HIP events, socp_last_kernel_ms).
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
from socp_amd import _lib  # noqa: E402
from kkt_cases import interior  # noqa: E402
from qp_cases import SHAPES  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="c2")
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=11)
    a = ap.parse_args()
    B = a.batch
    cones, n, m, k = SHAPES[a.shape][:4]
    rng = np.random.default_rng(20261021)
    A1, G1 = rng.standard_normal(m * n), rng.standard_normal(k * n)
    R = rng.standard_normal((n // 2, n))
    P1 = (R.T @ R / n).ravel(order="F")
    dev = torch.device("cuda", 0)
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)  # noqa: E731
    s, z = t(interior(rng, cones, B, k).ravel()), t(interior(rng, cones, B, k).ravel())
    rhs = [t(rng.standard_normal(B * q)) for q in (n, m, k, k)]
    A1, G1, P1 = t(A1), t(G1), t(P1)
    AB, GB, PB = A1.repeat(B), G1.repeat(B), P1.repeat(B)
    s1 = torch.zeros(1, dtype=torch.uint8, device=dev)
    sB = torch.zeros(B, dtype=torch.uint8, device=dev)
    out = [torch.empty(B * q, dtype=torch.float64, device=dev) for q in (n, m, k, k)]
    st = torch.empty(B, dtype=torch.int32, device=dev)
    forms = dict(plain=(AB, GB, sB, None, False), qp=(AB, GB, sB, PB, False), plain_sh=(A1, G1, s1, None, True),
                 qp_sh=(A1, G1, s1, P1, True))
    ctx = S.default_context()
    ctx.bind_torch_stream()
    L = _lib.load()
    kind, offs, dim = S.cone_arrays(list(cones))
    dims = _lib.Dims(B, n, m, k, len(kind))
    p = _lib.ptr

    def run(A, G, sing, P, sh):
        flags = S.F_DEVICE_PTRS | (S.F_SHARED_MATRICES if sh else 0)
        head = (ctx.handle, dims, p(kind), p(offs), p(dim))
        tail = (p(A), p(G), p(sing), p(s), p(z), *[p(v) for v in rhs], *[p(v) for v in out], p(st), flags)
        _lib.check(L.socp_batch_kkt_solve(*head, *tail) if P is None else L.socp_batch_kkt_solve_qp(*head, p(P), *tail))
        ctx.sync()

    series = [(f, i) for i in (1, 2) for f in forms]
    times = {key: [] for key in series}
    names, bad = {}, {}
    for rnd in range(a.reps + 1):  # round 0 warms up
        for key in series:
            run(*forms[key[0]])
            names[key[0]] = ctx.last_kernel_name()
            bad[key[0]] = int((st != 0).sum())
            if rnd:
                times[key].append(ctx.last_kernel_ms())
    med = {key: float(np.median(v)) for key, v in times.items()}
    print(f"device {torch.cuda.get_device_name(0)}; shape {a.shape} n={n} m={m} k={k}, batch {B}, "
          f"medians of {a.reps} (ms)")
    base = {}
    for f in forms:
        m1, m2 = med[(f, 1)], med[(f, 2)]
        base[f] = 0.5 * (m1 + m2)
        print(f"  {f:9s} {names[f]:38s} series {m1:8.3f} {m2:8.3f}  mean {base[f]:8.3f}  A/A spread {abs(m1 - m2):.3f}"
              f"  nonzero status {bad[f]}")
    for q, pl in (("qp", "plain"), ("qp_sh", "plain_sh")):
        print(f"  {q} - {pl} = {base[q] - base[pl]:+.3f} ms ({100 * (base[q] - base[pl]) / base[pl]:+.2f} %)")


if __name__ == "__main__":
    main()
