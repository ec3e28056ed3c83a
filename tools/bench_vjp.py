"""What a gradient costs beside the solve it differentiates (measuring tool, not
a test; no pass/fail threshold).

  python tools/bench_vjp.py [--batch 65536] [--reps 9] [--steps 4] [--out FILE]

One C2 batch from the device generator (socp_amd.configs.C2: n = 64, m = 16,
k = 96), device pointers, all on torch's current stream:
  forward   batch_solve(tol = 1e-5): the solver kernel's time, from
            socp_last_kernel_ms (HIP events around the launch);
  backward  batch_centre(steps) on the solve's iterate, then batch_vjp with all
            six gradients: HIP events around the two calls (their kernels, the
            fused KKT solves' launches and the memsets between them).  The
            iterate is restored before the first event.
Both are run --reps times after a warm-up round, interleaved, in two series
each (f1 b1 f2 b2 per round); the figures are medians, and the difference of a
quantity's two series is the A/A spread to read the ratio against.  vjp_only is
the same with steps = 0 (the adjoint alone).  Prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "socp.jl_amd"))
import socp_amd as S  # noqa: E402
from socp_amd.configs import C2  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=C2.batch)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_vjp needs a GPU"
    cfg, B = C2, a.batch
    n, m, k = cfg.n, cfg.m, cfg.k
    ctx = S.default_context()
    c, A, b, G, h = S.generate(cfg.cones, B, n, m, k, cfg.seed)
    sing = torch.zeros(B, dtype=torch.uint8, device=G.device)
    gen = torch.Generator(device=G.device).manual_seed(7)
    g = [torch.randn(B * q, dtype=torch.float64, device=G.device, generator=gen) for q in (n, m, k, k)]
    sol = {}

    def forward():
        out = S.batch_solve(cfg.cones, n, m, k, c, A, b, G, h, sing, tol=1e-5)
        ms = ctx.last_kernel_ms()  # waits for the launch's second event
        sol.update(out, kernel=ctx.last_kernel_name())
        return ms

    def backward(steps):
        pt = [sol[key].clone() for key in "xyzs"]
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        cen = S.batch_centre(cfg.cones, n, m, k, c, A, b, G, h, sing, *pt, steps=steps)
        r = S.batch_vjp(cfg.cones, n, m, k, A, G, sing, *pt, *g, skip=sol["status"],
                        want=["dc", "db", "dh", "dA", "dG"])
        e1.record()
        e1.synchronize()
        bad = int((cen["status"] != 0).sum()) + int((r["status"] != 0).sum())
        return e0.elapsed_time(e1), bad, ctx.last_kernel_name()

    series = ("f1", "b1", "v1", "f2", "b2", "v2")
    times = {key: [] for key in series}
    bad = kkt = None
    for rnd in range(a.reps + 1):  # round 0 warms up
        for key in series:
            if key[0] == "f":
                ms = forward()
            else:
                ms, bad_now, kkt = backward(a.steps if key[0] == "b" else 0)
                if key[0] == "b":
                    bad = bad_now
            if rnd:
                times[key].append(ms)
    med = {key: float(np.median(v)) for key, v in times.items()}
    fwd, bwd, vjp = [0.5 * (med[q + "1"] + med[q + "2"]) for q in "fbv"]
    iters = sol["iters"].double().mean().item()
    rec = dict(device=torch.cuda.get_device_name(0), config="C2", n=n, m=m, k=k, batch=B, reps=a.reps,
               centre_steps=a.steps, solver_kernel=sol["kernel"], kkt_kernel=kkt,
               mean_iters=round(iters, 2), converged=int((sol["status"] == 0).sum()),
               forward_kernel_ms=round(fwd, 3), centre_plus_vjp_ms=round(bwd, 3), vjp_only_ms=round(vjp, 3),
               ratio_backward_over_forward=round(bwd / fwd, 3),
               forward_ms_per_iteration=round(fwd / max(iters, 1.0), 3),
               spread_ms=dict(forward=round(abs(med["f1"] - med["f2"]), 3),
                              backward=round(abs(med["b1"] - med["b2"]), 3),
                              vjp_only=round(abs(med["v1"] - med["v2"]), 3)),
               masked_problems=bad, gradient_bytes=8 * B * (n + m + k + m * n + k * n))
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
