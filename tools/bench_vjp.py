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

  python tools/bench_vjp.py --shared [--batch 65536] [--reps 9] [--out FILE]

The gradients of a shared-matrix batch (socp_batch_vjp_sum).  The same C2 batch
with problem 0's A and G and one P = R'R/n for every problem, at random interior
points (the adjoint is defined there; every KKT solve succeeds), device pointers,
HIP events, medians of --reps after a warm-up round, the three interleaved:
  vec    batch_vjp(shared_matrices=True) with dc, db, dh only;
  sums   the same call plus dP, dA, dG: the sum entry;
  repl   the route without that entry: the non-shared batch_vjp on the matrices
         replicated B times with dP, dA, dG, then torch sums over the batch.
sums - vec is what the two sum kernels cost; it is reported against the byte
floor 8 B (2n + 2m + 3k) / (HBM bandwidth measured here by a device copy of
1 GiB), and sums against repl.
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
from socp_amd.configs import C2, POC  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), r


def shared(a):
    cfg, B = C2, a.batch
    n, m, k = cfg.n, cfg.m, cfg.k
    _, A, _, G, _ = S.generate(cfg.cones, B, n, m, k, cfg.seed)
    dev = G.device
    gen = torch.Generator(device=dev).manual_seed(7)
    rnd = lambda *shape: torch.randn(*shape, dtype=torch.float64, device=dev, generator=gen)  # noqa: E731
    A1, G1 = A[:m * n].clone(), G[:k * n].clone()
    R = rnd(n // 2, n)
    P1 = (R.T @ R / n).contiguous().view(-1)

    def interior():
        v = rnd(B, k)
        for kind, o, d in cfg.cones:
            if kind == POC:
                v[:, o:o + d] = 1.0 + v[:, o:o + d].abs()
            else:
                v[:, o] = 1.0 + v[:, o + 1:o + d].norm(dim=1)
        return v.view(-1)

    x, y, z, s_ = rnd(B * n), rnd(B * m), interior(), interior()
    g = [rnd(B * q) for q in (n, m, k, k)]
    del A, G
    Ar, Gr, Pr = A1.repeat(B), G1.repeat(B), P1.repeat(B)
    sing1 = torch.zeros(1, dtype=torch.uint8, device=dev)
    singr = torch.zeros(B, dtype=torch.uint8, device=dev)
    new = lambda cnt: torch.empty(cnt, dtype=torch.float64, device=dev)  # noqa: E731
    vec = dict(dc=new(B * n), db=new(B * m), dh=new(B * k))
    one = dict(vec, dP=new(n * n), dA=new(m * n), dG=new(k * n))
    per = dict(dP=new(B * n * n), dA=new(B * m * n), dG=new(B * k * n))

    def run_vec():
        return S.batch_vjp(cfg.cones, n, m, k, A1, G1, sing1, x, y, z, s_, *g, P=P1, want=list(vec), out=vec,
                           shared_matrices=True)

    def run_sums():
        return S.batch_vjp(cfg.cones, n, m, k, A1, G1, sing1, x, y, z, s_, *g, P=P1, want=list(one), out=one,
                           shared_matrices=True)

    def run_repl():
        r = S.batch_vjp(cfg.cones, n, m, k, Ar, Gr, singr, x, y, z, s_, *g, P=Pr, want=list(per), out=per)
        return r, {key: per[key].view(B, -1).sum(0) for key in per}

    buf, dst = new(1 << 27), new(1 << 27)
    series = dict(vec=run_vec, sums=run_sums, repl=run_repl, copy=lambda: dst.copy_(buf))
    times = {key: [] for key in series}
    last = {}
    for it in range(a.reps + 1):  # round 0 warms up
        for key, fn in series.items():
            ms, last[key] = timed(fn)
            if it:
                times[key].append(ms)
    med = {key: float(np.median(v)) for key, v in times.items()}
    bw = 2.0 * 8 * (1 << 27) / (med["copy"] * 1e-3)  # bytes read and written per second
    floor_ms = 8.0 * B * (2 * n + 2 * m + 3 * k) / bw * 1e3
    bad = int((last["sums"]["status"] != 0).sum())
    # the two routes' numbers, relative to the largest entry of each gradient
    agree = {key: float(((one[key] - last["repl"][1][key]).abs().max() / one[key].abs().max()).item())
             for key in per}
    bitwise = all(torch.equal(run_sums()[key], one[key].clone()) for key in per)
    rec = dict(device=torch.cuda.get_device_name(0), config="C2 shared", n=n, m=m, k=k, batch=B, reps=a.reps,
               plan=S.vjp_sum_plan(B, n, m, k), kkt_kernel=S.default_context().last_kernel_name(),
               vec_only_ms=round(med["vec"], 3), with_sums_ms=round(med["sums"], 3),
               sum_kernels_ms=round(med["sums"] - med["vec"], 3), replicated_route_ms=round(med["repl"], 3),
               speedup_over_replicated=round(med["repl"] / med["sums"], 2),
               hbm_copy_GBps=round(bw / 1e9, 1), byte_floor_ms=round(floor_ms, 4),
               sum_kernels_over_floor=round((med["sums"] - med["vec"]) / floor_ms, 2),
               spread_ms={key: round(max(v) - min(v), 3) for key, v in times.items()},
               masked_problems=bad, max_rel_difference_from_replicated=agree, same_bits_again=bitwise,
               replicated_gradient_bytes=8 * B * (n * n + m * n + k * n))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=C2.batch)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--shared", action="store_true", help="the gradients of a shared-matrix batch (see above)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_vjp needs a GPU"
    if a.shared:
        line = json.dumps(shared(a))
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return
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
