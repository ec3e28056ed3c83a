"""Parametric batches (SOCP_F_SHARED_MATRICES) against the same data with A, G
and sing replicated per problem, at C2's size (measuring tool, not a test).

  python tools/bench_shared.py [--batch 65536] [--k 8] [--reps 11] [--ingest-batches 8] [--seed 9]

One seeded parametric batch (tests/shared_cases.py) of C2's shape, fixed K,
tol 0.  Prints
  1. the solver kernel's time (HIP events), shared against replicated, device
     pointers, interleaved in one process: two series of each form per round
     (r1 s1 r2 s2), medians of --reps; |r1 - r2| and |s1 - s2| are the A/A
     spread to read the difference against;
  2. whether the two forms' outputs agree bitwise over the whole batch;
  3. problem-iterations/s through Ingest (PCIe-inclusive, pageable host
     arrays in, results out), shared against replicated, over
     --ingest-batches batches, with the input bytes per batch;
  4. the device and pinned bytes socp_ingest_create and socp_dense_create
     allocate in both forms, computed from the layouts (socp_api_ingest.hip, socp_api_dense.hip).
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "socp.jl_amd"))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import socp_amd as S  # noqa: E402
from shared_cases import make, replicated  # noqa: E402

KEYS = ("x", "y", "z", "s", "iters", "status", "res")


def al(v, a=256):
    return (v + a - 1) // a * a


def ingest_bytes(B, n, m, k, shared):
    """(pinned, device) bytes of socp_ingest_create: two slots of in_layout + out_layout, plus the shared block."""
    MB = 0 if shared else B
    inp = sum(al(8 * q) for q in (B * n, MB * m * n, B * m, MB * k * n, B * k)) + al(MB)
    out = sum(al(8 * q) for q in (B * n, B * m, B * k, B * k, 3 * B)) + 2 * al(4 * B) + 256
    mat = al(8 * m * n) + al(8 * k * n) + 256 if shared else 0
    return 2 * (inp + out), 2 * (inp + out) + 512 + mat


def dense_bytes(B, n, m, k, rec_bytes, shared):
    """Device bytes of socp_dense_create: A, G, sing, the zero c/b/h block, the factor records."""
    MB = 1 if shared else B
    return MB * (8 * (m * n + k * n) + 1) + 8 * B * (n + m + k) + B * rec_bytes + 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--ingest-batches", type=int, default=8)
    ap.add_argument("--seed", type=int, default=9)
    a = ap.parse_args()
    B, K = a.batch, a.k
    d = make("c2", B, a.seed)
    cones, n, m, k = d.shape
    ctx = S.default_context()
    dev = torch.device("cuda", 0)
    print(f"device {torch.cuda.get_device_name(0)}; C2 shape n={n} m={m} k={k}, batch {B}, K={K}, tol 0, seed {a.seed}")

    # ---- 1. kernel time, device pointers, interleaved
    t = lambda v: torch.from_numpy(v).to(dev)  # noqa: E731
    c, b, h, A1, G1 = t(d.c), t(d.b), t(d.h), t(d.A), t(d.G)
    AB, GB = A1.repeat(B), G1.repeat(B)
    sing1 = torch.zeros(1, dtype=torch.uint8, device=dev)
    singB = torch.zeros(B, dtype=torch.uint8, device=dev)
    kw = dict(maxit=K, tol=0.0, res=True)
    forms = dict(r1=(AB, GB, singB, False), s1=(A1, G1, sing1, True), r2=(AB, GB, singB, False),
                 s2=(A1, G1, sing1, True))
    times = {key: [] for key in forms}
    outs = {}
    for rnd in range(a.reps + 1):  # round 0 warms up
        for key, (A, G, sing, sh) in forms.items():
            outs[key] = S.batch_solve(cones, n, m, k, c, A, b, G, h, sing, shared_matrices=sh, out=outs.get(key), **kw)
            ctx.sync()
            if rnd:
                times[key].append(ctx.last_kernel_ms())
    kernel = ctx.last_kernel_name()
    med = {key: float(np.median(v)) for key, v in times.items()}
    print(f"1. kernel {kernel}, medians of {a.reps} (ms): " + "  ".join(f"{key} {v:.3f}" for key, v in med.items()))
    rep, shr = 0.5 * (med["r1"] + med["r2"]), 0.5 * (med["s1"] + med["s2"])
    print(f"   replicated {rep:.3f} ms (A/A spread {abs(med['r1'] - med['r2']):.3f}), shared {shr:.3f} ms "
          f"(A/A spread {abs(med['s1'] - med['s2']):.3f}): shared - replicated = {shr - rep:+.3f} ms "
          f"({100 * (shr - rep) / rep:+.2f} %); {B * K / shr * 1e3:.3e} problem-iterations/s shared, "
          f"{B * K / rep * 1e3:.3e} replicated (HBM-resident)")

    # ---- 2. outputs, bitwise
    bad = [key for key in KEYS if not torch.equal(outs["s1"][key], outs["r1"][key])]
    st = torch.bincount(outs["s1"]["status"].long(), minlength=7).tolist()
    print(f"2. shared against replicated over {B} problems, bitwise on {', '.join(KEYS)}: "
          f"{'EQUAL' if not bad else 'DIFFERENT in ' + ', '.join(bad)}; status counts {st}")
    host_ref = {key: outs["s1"][key].cpu().numpy() for key in KEYS}
    del AB, GB, outs
    torch.cuda.empty_cache()

    # ---- 3. ingest, PCIe-inclusive
    nb = a.ingest_batches
    rates = {}
    for sh in (True, False):
        ing = S.Ingest(cones, n, m, k, B, shared_matrices=sh)
        if sh:
            ing.set_matrices(d.A, d.G, np.zeros(1, np.uint8))
            args = (d.c, None, d.b, None, d.h, None)
            nbytes = 8 * B * (n + m + k)
        else:
            Ar, Gr = replicated(d)
            args = (d.c, Ar, d.b, Gr, d.h, np.zeros(B, np.uint8))
            nbytes = 8 * B * (n + m + k + m * n + k * n) + B
        ikw = dict(maxit=K, tol=0.0)
        last = ing.wait(ing.submit(*args, **ikw), res=True)  # warm-up batch
        t0 = time.perf_counter()
        tk = [ing.submit(*args, **ikw)]
        for i in range(1, nb):
            tk.append(ing.submit(*args, **ikw))
            last = ing.wait(tk[i - 1], res=True)
        last = ing.wait(tk[-1], res=True)
        dt = time.perf_counter() - t0
        ok = all(np.array_equal(last[key][:host_ref[key].size], host_ref[key][:last[key].size]) for key in KEYS)
        rates[sh] = nb * B * K / dt
        print(f"3. ingest {'shared    ' if sh else 'replicated'}: {nb} batches in {dt * 1e3:.1f} ms = "
              f"{rates[sh]:.3e} problem-iterations/s; input {nbytes / 1e6:.1f} MB per batch; "
              f"results {'equal to' if ok else 'DIFFER from'} the device-pointer solve")
        ing.close()
        del ing, args
    print(f"   shared / replicated = {rates[True] / rates[False]:.2f}x; shared ingest at "
          f"{100 * rates[True] / (B * K / shr * 1e3):.0f} % of the HBM-resident rate")

    # ---- 4. bytes from the layouts
    hd = S.DenseHandle(cones, n, m, k, d.A, d.G, np.zeros(1, np.uint8), shared_matrices=True, batch=B)
    rec = hd.record_bytes
    hd.close()
    for sh in (True, False):
        pin, dv = ingest_bytes(B, n, m, k, sh)
        print(f"4. {'shared    ' if sh else 'replicated'}: socp_ingest_create pins {pin / 1e6:.1f} MB and allocates "
              f"{dv / 1e6:.1f} MB on the device; socp_dense_create allocates "
              f"{dense_bytes(B, n, m, k, rec, sh) / 1e6:.1f} MB on the device (records {B * rec / 1e6:.1f} MB)")


if __name__ == "__main__":
    main()
