"""Inputs of the tile-factorisation tests (test_tile_cases_cpu.py,
test_gpu_tile_factor.py): batches in which one problem each loses a pivot of
the 16x16 tile factorisation (factor_tile) at a chosen position, and the
shapes of the parity sweep.

A zero column j of G makes row and column j of H = G' W^-2 G exactly zero, so
pivot j of chol(H) is exactly 0 and the factorisation fails there: in tile
j // 16, row block (j % 16) // 4, pivot j % 4 of the block.  A zero row r of A
does the same to S = A H^-1 A' (the S tile).  `sing` is passed as 0, so H takes
no A'A.  A wrong broadcast column or block index in the tile's pivot block
reads another (positive) entry instead and misses the failure.
"""
import collections

import numpy as np

P, Q = 0, 1  # cone kinds of include/socp.h: POC, SOC
FAIL_CLASS = (2, 3, 4)  # CHOL_H_FAILED, CHOL_S_FAILED, DOMAIN_ERROR: how the failure-isolation tests map a failure
MAXIT_ST, CHOL_H, CHOL_S = 1, 2, 3
K_ITERS = 3

Shape = collections.namedtuple("Shape", "cones n m k")
ONE_TILE = Shape([(P, 0, 16)], 16, 0, 16)
C2_SHAPE = Shape([(P, 0, 32), (Q, 32, 32), (Q, 64, 32)], 64, 16, 96)
C2_COLUMNS = (0, 3, 4, 15, 16, 21, 31, 32, 47, 48, 63)
S_ROWS = (0, 5, 15)
SEED = 20241020


def _gen(oracle, sh, B, seed):
    d = oracle.generate(sh.cones, B, sh.n, sh.m, sh.k, seed)
    return {key: v.copy() for key, v in d.items()}


def zero_G_column(d, sh, p, j):
    """Column j of problem p's G (k x n, column-major)."""
    o = p * sh.k * sh.n + j * sh.k
    d["G"][o:o + sh.k] = 0.0


def zero_A_row(d, sh, p, r):
    """Row r of problem p's A (m x n, column-major)."""
    o = p * sh.m * sh.n
    d["A"][o + r:o + sh.m * sh.n:sh.m] = 0.0


def one_tile_batch(oracle):
    """17 problems of ONE_TILE: problem j < 16 has column j of G zeroed, problem 16 is untouched."""
    sh = ONE_TILE
    d = _gen(oracle, sh, 17, SEED)
    for j in range(16):
        zero_G_column(d, sh, j, j)
    return sh, d, list(range(16)), [16]


def c2_column_batch(oracle):
    """C2's shape: problem i has column C2_COLUMNS[i] of G zeroed, then one
    untouched problem, then one with a NaN entry in G."""
    sh = C2_SHAPE
    nz = len(C2_COLUMNS)
    d = _gen(oracle, sh, nz + 2, SEED + 1)
    for i, j in enumerate(C2_COLUMNS):
        zero_G_column(d, sh, i, j)
    d["G"][(nz + 1) * sh.k * sh.n + 17 * sh.k + 40] = np.nan
    return sh, d, list(range(nz)), [nz], nz + 1


def s_tile_batch(oracle):
    """C2's shape: problem i has row S_ROWS[i] of A zeroed, then one untouched problem."""
    sh = C2_SHAPE
    d = _gen(oracle, sh, len(S_ROWS) + 1, SEED + 2)
    for i, r in enumerate(S_ROWS):
        zero_A_row(d, sh, i, r)
    return sh, d, list(range(len(S_ROWS))), [len(S_ROWS)]


def parity_cones(k):
    a = k // 4
    b = (k - a) // 2
    return [(P, 0, a), (Q, a, b), (Q, a + b, k - a - b)]


# n -> k: one to four column tiles of H, k no multiple of the row step where n is odd
PARITY_K = {10: 22, 17: 39, 33: 64, 48: 80, 64: 96}
# m = 0: no S tile; 3: a partial one; 16: a full one
PARITY = [Shape(parity_cones(k), n, m, k) for n, k in PARITY_K.items() for m in (0, 3, 16)]
# m = 20: two S tiles, the chol_inv / sweep path
PARITY_M20 = Shape(parity_cones(64), 32, 20, 64)
# the explicit inverse and the split plugin entries
PLUGIN = Shape(parity_cones(48), 32, 8, 48)
# the blocked kernel, forced, at the smallest shape the forced-large tests run (config C0b)
LARGE = Shape([(Q, 0, 3)], 10, 8, 3)
PARITY_B = 4


def shape_id(sh):
    return f"n{sh.n}_m{sh.m}_k{sh.k}"


def oracle_solve(oracle, sh, d, sing, flags=0, maxit=K_ITERS):
    return oracle.batch_solve(sh.cones, sh.n, sh.m, sh.k, d["c"], d["A"], d["b"], d["G"], d["h"], sing=sing,
                              params=oracle.Params(maxit=maxit, tol=0.0, flags=flags))
