"""Parametric batches for the shared-matrix tests (SOCP_F_SHARED_MATRICES):
one A and one G for the whole batch, built on the CPU from a seed.

A (m x n) and G (k x n) are standard normal.  Per problem x0, y0 are standard
normal and s0, z0 are interior to the cone (a POC element is 1 + |N|; an SOC
head is 1 + the norm of its standard-normal tail), and

    b = A x0,   h = G x0 + s0,   c = -(A'y0 + G'z0),

so every problem is strictly primal and dual feasible and differs from the
others.  Arrays come in the include/socp.h layout: A and G column-major, the
vectors stacked batch-major.
"""
import collections

import numpy as np

P, Q = 0, 1  # cone kinds of include/socp.h: POC, SOC

Shape = collections.namedtuple("Shape", "cones n m k")
# each the smallest shape that reaches its own code path of the register kernel
SHAPES = dict(
    c1=Shape([(Q, 0, 48)], 32, 8, 48),                           # one slot
    c2=Shape([(P, 0, 32), (Q, 32, 32), (Q, 64, 32)], 64, 16, 96),  # two slots, SOC+POC kernel, fused U
    mq2=Shape([(Q, 0, 48)], 32, 24, 48),                         # MQ = 2: the inverse by nature
    m0=Shape([(P, 0, 16), (Q, 16, 16)], 16, 0, 32),              # no equality rows
    sing=Shape([(Q, 0, 3)], 10, 8, 3),                           # G'G singular (k < n)
    wide=Shape([(P, 0, 32), (Q, 32, 64)], 80, 8, 96),            # n > 64: no register variant
)

Batch = collections.namedtuple("Batch", "shape B c A b G h")


def interior(rng, cones, B, k):
    v = np.zeros((B, k))
    for kind, offs, dim in cones:
        if kind == P:
            v[:, offs:offs + dim] = 1.0 + np.abs(rng.standard_normal((B, dim)))
        else:
            tail = rng.standard_normal((B, dim - 1))
            v[:, offs + 1:offs + dim] = tail
            v[:, offs] = 1.0 + np.linalg.norm(tail, axis=1)
    return v


def make(shape, B, seed):
    """A parametric batch of B problems of `shape` (a Shape or a key of SHAPES)."""
    if isinstance(shape, str):
        shape = SHAPES[shape]
    cones, n, m, k = shape
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((m, n))
    G = rng.standard_normal((k, n))
    x0 = rng.standard_normal((B, n))
    y0 = rng.standard_normal((B, m))
    s0 = interior(rng, cones, B, k)
    z0 = interior(rng, cones, B, k)
    b = x0 @ A.T
    h = x0 @ G.T + s0
    c = -(y0 @ A + z0 @ G)
    flat = lambda M: np.ascontiguousarray(M).reshape(-1)  # noqa: E731
    return Batch(shape, B, flat(c), np.ascontiguousarray(A.ravel(order="F")), flat(b),
                 np.ascontiguousarray(G.ravel(order="F")), flat(h))


def replicated(batch):
    """(A, G) of the batch replicated B times: the flag-off form of the same data."""
    return np.tile(batch.A, batch.B), np.tile(batch.G, batch.B)
