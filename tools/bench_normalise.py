"""What SOCP_F_NORMALISE costs (measuring tool, not a test; run on an MI355X).

  python tools/bench_normalise.py [--config C2] [--reps 11] [--shift 10]

The config's generator batch (socp_generate, the config's seed; C2: 65,536
problems) with c and (b, h) multiplied by 2^shift, so that every exponent of
the rule is non-zero.  Device pointers, fixed K = the config's headline count
(C2: 8), tol 0, so both forms run the same iterations -- on the same numbers
up to the powers of two.  Two forms, interleaved in one process, two series
each (plain1 norm1 plain2 norm2 per round), medians of --reps after a warm-up
round; the difference of a form's two series is the A/A spread to read the
flag's cost against.  Times are whole calls between HIP events on the stream
the context issues on (the flag's work lies outside the solver kernel's own
event pair, which is printed beside it).

The three kernels' own times, between HIP events in the same rounds:
  norm      socp_batch_normalise with no scaled output (the norm kernel and the
            copy of 2 x batch exponents);
  forward   socp_batch_normalise with cs, bs, hs, less the line above;
  backward  the flag's cost less the two lines above (the kernel has no entry
            of its own).
The bytes they move are printed beside the solve's algorithmic bytes.
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "socp.jl_amd"))
import socp_amd as S  # noqa: E402
from socp_amd import _lib  # noqa: E402
from socp_amd.configs import CONFIGS  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def run(cfg, reps, shift):
    B, K = cfg.batch, cfg.fixed_k
    n, m, k = cfg.n, cfg.m, cfg.k
    c, A, b, G, h = S.generate(cfg.cones, B, n, m, k, cfg.seed)
    c, b, h = c * 2.0 ** shift, b * 2.0 ** shift, h * 2.0 ** shift  # (exact)
    ctx = S.default_context()
    L, p = _lib.load(), _lib.ptr
    dims = _lib.Dims(B, n, m, k, 0)
    expo = torch.empty(2 * B, dtype=torch.int32, device=c.device)
    cs, bs, hs = torch.empty_like(c), torch.empty_like(b), torch.empty_like(h)
    outs, names, kern = {}, {}, {}

    def solve(key, **kw):
        outs[key] = S.batch_solve(cfg.cones, n, m, k, c, A, b, G, h, None, normalise=key[0] == "norm",
                                  out=outs.get(key), res=True, **kw)
        names[key[0]] = ctx.last_kernel_name()

    def rule(scaled):
        o = (p(cs), p(bs), p(hs)) if scaled else (None, None, None)
        _lib.check(L.socp_batch_normalise(ctx.handle, dims, None, p(c), p(b), p(h), _lib.F_DEVICE_PTRS, p(expo), None,
                                          *o))

    ctx.bind_torch_stream()
    forms = ("plain", "norm", "rule", "rule+fw")
    series = [(f, i) for i in (1, 2) for f in forms]
    times = {key: [] for key in series}
    for rnd in range(reps + 1):  # round 0 warms up
        for key in series:
            if key[0].startswith("rule"):
                ms = timed(lambda: rule(key[0] == "rule+fw"))
            else:
                ms = timed(lambda: solve(key, maxit=K, tol=0.0))
                if rnd:
                    kern.setdefault(key, []).append(ctx.last_kernel_ms())
            if rnd:
                times[key].append(ms)
    med = {key: float(np.median(v)) for key, v in times.items()}
    mean = {f: 0.5 * (med[(f, 1)] + med[(f, 2)]) for f in forms}
    print(f"{cfg.name}: n={n} m={m} k={k}, batch {B}, K={K}, tol 0, c, b, h times 2^{shift}, medians of {reps} (ms)")
    for f in forms:
        what = names.get(f, "socp_batch_normalise, exponents only" if f == "rule" else "socp_batch_normalise, cs bs hs")
        print(f"  {f:8s} {what:38s} series {med[(f, 1)]:9.4f} {med[(f, 2)]:9.4f}  mean {mean[f]:9.4f}"
              f"  A/A spread {abs(med[(f, 1)] - med[(f, 2)]):.4f}")
    for f in ("plain", "norm"):
        ks = [float(np.median(kern[(f, i)])) for i in (1, 2)]
        print(f"  {f:8s} solver kernel's own event pair        series {ks[0]:9.4f} {ks[1]:9.4f}")
    cost = mean["norm"] - mean["plain"]
    vec = 8 * B * (n + m + k)
    print(f"  flag's cost {cost:+.4f} ms ({100 * cost / mean['plain']:+.3f} % of the plain call)")
    print(f"  norm kernel {mean['rule']:.4f} ms (reads {vec / 1e6:.1f} MB); forward kernel "
          f"{mean['rule+fw'] - mean['rule']:.4f} ms (reads and writes {vec / 1e6:.1f} MB); backward kernel, the "
          f"remainder, {cost - mean['rule+fw']:.4f} ms (reads and writes {8 * B * (n + m + 2 * k) / 1e6:.1f} MB)")
    moved = 8 * (3 * (n + m + k) + 2 * (n + m + 2 * k))
    algo = 8 * (k * n + m * n + 2 * (n + m + k) + n + m + 2 * k)
    print(f"  bytes per problem: the flag moves {moved} B; the solve's algorithmic bytes (A, G, c, b, h in; x, y, z, s "
          f"out) are {algo} B")
    same = all(torch.equal(outs[("plain", 1)][q], outs[("norm", 1)][q]) for q in ("iters", "status"))
    print(f"  iters and status of both forms equal: {same}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--shift", type=int, default=10)
    a = ap.parse_args()
    print(f"device {torch.cuda.get_device_name(0)}")
    run(CONFIGS[a.config], a.reps, a.shift)


if __name__ == "__main__":
    main()
