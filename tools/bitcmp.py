"""Bit-identity checks between two libsocp builds.
  bitcmp.py save|compare FILE   writes (or compares against) the C4 solution of a small batch
  bitcmp.py dirs A B            compares two bench.py --dump-outputs directories, file by file (no GPU)"""
import os
import sys

import numpy as np

if sys.argv[1] == "dirs":
    a, b = sys.argv[2], sys.argv[3]
    names = sorted(set(os.listdir(a)) | set(os.listdir(b)))
    bad = 0
    for nm in names:
        if not (os.path.exists(os.path.join(a, nm)) and os.path.exists(os.path.join(b, nm))):
            print(f"{nm}: only in one directory")
            bad += 1
            continue
        u, v = np.load(os.path.join(a, nm)), np.load(os.path.join(b, nm))
        same = u.dtype == v.dtype and u.shape == v.shape
        diff = int((u.view(np.uint8) != v.view(np.uint8)).reshape(u.size, -1).any(axis=1).sum()) if same else u.size
        bad += diff != 0
        print(f"{nm}: {diff} of {u.size} differ bitwise")
    sys.exit(1 if bad else 0)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "socp.jl_amd"))
import socp_amd as S  # noqa: E402
from socp_amd.configs import C4  # noqa: E402

mode, path = sys.argv[1], sys.argv[2]
B = 32
c, A, b, G, h = S.generate(C4.cones, B, C4.n, C4.m, C4.k, C4.seed)
import torch  # noqa: E402
sing = torch.zeros(B, dtype=torch.uint8, device=G.device)
out = S.batch_solve(C4.cones, C4.n, C4.m, C4.k, c, A, b, G, h, sing, maxit=5, tol=0.0)
S.default_context().sync()
x = np.concatenate([out[k].cpu().numpy().ravel() for k in ("x", "y", "z", "s")])
if mode == "save":
    with open(path, "wb") as f:
        f.write(x.tobytes())
else:
    ref = np.frombuffer(open(path, "rb").read(), dtype=np.float64)
    diff = int((ref.view(np.uint64) != x.view(np.uint64)).sum())
    print(f"{diff} of {x.size} values differ bitwise; max rel {np.max(np.abs(ref - x)) / np.max(np.abs(ref)):.3e}")
