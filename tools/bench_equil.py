"""What SOCP_F_EQUILIBRATE costs (measuring tool, not a test; run on an MI355X).

  python tools/bench_equil.py [--configs C1,C2] [--reps 11] [--spread 12]

Per config one seeded badly scaled batch: the device generator's problems
(socp_generate, the config's seed) with every row and column multiplied by a
power of two within 2^+-spread drawn from torch's generator (seed 0), one
factor per SOC cone.  Device pointers, fixed K = the config's headline count,
tol 0, so both forms run the same iterations.  Two forms, interleaved in one
process, two series each (plain1 equil1 plain2 equil2 per round), medians of
--reps after a warm-up round; the difference of a form's two series is the A/A
spread to read the flag's cost against.  Times are whole calls between HIP
events on the stream the context issues on (the flag's work lies outside the
solver kernel's own event pair).

The flag's cost is set beside its byte floor -- one read plus one write of A
and G -- at the rate a device-to-device copy of the same bytes reaches in this
process (same two series), and as a multiple of it.  Under the reference rule
(tol 1e-5) the statuses of both forms are counted once at the end.
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "socp.jl_amd"))
import socp_amd as S  # noqa: E402
from socp_amd.configs import CONFIGS  # noqa: E402


def bad_units(cfg, B, spread, dev):
    """The config's generated batch in other units (exact: powers of two)."""
    n, m, k = cfg.n, cfg.m, cfg.k
    c, A, b, G, h = S.generate(cfg.cones, B, n, m, k, cfg.seed)
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    draw = lambda *shape: torch.randint(-spread, spread + 1, shape, generator=g, device=dev, dtype=torch.int32)  # noqa: E731
    dc, er, fr = draw(B, n), draw(B, m), draw(B, k)
    for kind, o, d in cfg.cones:
        if kind == S.CONE_SOC:
            fr[:, o:o + d] = fr[:, o:o + 1]
    A = torch.ldexp(A.view(B, n, m), dc[:, :, None] + er[:, None, :]).reshape(-1).contiguous()
    G = torch.ldexp(G.view(B, n, k), dc[:, :, None] + fr[:, None, :]).reshape(-1).contiguous()
    return (torch.ldexp(c.view(B, n), dc).reshape(-1).contiguous(), A, torch.ldexp(b.view(B, m), er).reshape(-1).contiguous(),
            G, torch.ldexp(h.view(B, k), fr).reshape(-1).contiguous())


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def run(cfg, reps, spread):
    dev = torch.device("cuda", 0)
    B, K = cfg.batch, cfg.fixed_k
    n, m, k = cfg.n, cfg.m, cfg.k
    c, A, b, G, h = bad_units(cfg, B, spread, dev)
    ctx = S.default_context()
    src = torch.cat([A, G])
    dst = torch.empty_like(src)
    outs, names = {}, {}

    def solve(key, **kw):
        outs[key] = S.batch_solve(cfg.cones, n, m, k, c, A, b, G, h, None, equilibrate=key[0] == "equil",
                                  out=outs.get(key), res=True, **kw)
        names[key[0]] = ctx.last_kernel_name()

    series = [(f, i) for i in (1, 2) for f in ("plain", "equil", "copy")]
    times = {key: [] for key in series}
    for rnd in range(reps + 1):  # round 0 warms up
        for key in series:
            ms, _ = timed((lambda: dst.copy_(src)) if key[0] == "copy" else (lambda: solve(key, maxit=K, tol=0.0)))
            if rnd:
                times[key].append(ms)
    med = {key: float(np.median(v)) for key, v in times.items()}
    mean = {f: 0.5 * (med[(f, 1)] + med[(f, 2)]) for f in ("plain", "equil", "copy")}
    print(f"{cfg.name}: n={n} m={m} k={k}, batch {B}, K={K}, tol 0, spread 2^+-{spread}, whole calls, medians of {reps} (ms)")
    for f in ("plain", "equil", "copy"):
        print(f"  {f:6s} {names.get(f, 'device-to-device copy of A and G'):34s} series {med[(f, 1)]:9.3f} {med[(f, 2)]:9.3f}"
              f"  mean {mean[f]:9.3f}  A/A spread {abs(med[(f, 1)] - med[(f, 2)]):.3f}")
    cost = mean["equil"] - mean["plain"]
    byts = 2 * src.numel() * 8
    print(f"  flag's cost {cost:+.3f} ms ({100 * cost / mean['plain']:+.2f} % of the plain call); byte floor "
          f"{byts / 1e6:.1f} MB (read + write of A and G) = {mean['copy']:.3f} ms at the copy's "
          f"{byts / mean['copy'] / 1e6:.0f} GB/s: the cost is {cost / mean['copy']:.2f} x the floor")
    for f in ("plain", "equil"):
        solve((f, 0))
        ctx.sync()
        st = torch.bincount(outs[(f, 0)]["status"].long(), minlength=7).tolist()
        print(f"  reference rule (tol 1e-5, maxit 40) {f:6s} status counts {st}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C1,C2")
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--spread", type=int, default=12)
    a = ap.parse_args()
    print(f"device {torch.cuda.get_device_name(0)}")
    for name in a.configs.split(","):
        run(CONFIGS[name], a.reps, a.spread)


if __name__ == "__main__":
    main()
