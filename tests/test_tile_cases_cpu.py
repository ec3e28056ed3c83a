"""The CPU oracle gives the outcomes that the GPU tile-factorisation cases
(test_gpu_tile_factor.py, inputs in tile_cases.py) rely on: a problem with a
zeroed column of G, a zeroed row of A or a NaN in G stops in its first
factorisation (iteration 0), an untouched problem in the same batch runs its
3 iterations, and every shape of the parity sweep with m <= n runs them too.
"""
import numpy as np
import pytest

import tile_cases as T


def solve(oracle, sh, d):
    B = len(d["c"]) // sh.n
    return T.oracle_solve(oracle, sh, d, np.zeros(B, np.uint8))


def test_every_pivot_of_one_tile(oracle):
    sh, d, bad, good = T.one_tile_batch(oracle)
    assert bad == list(range(16)) and good == [16]
    G = d["G"].reshape(17, sh.n, sh.k)  # [problem, column, row]
    for j in bad:
        assert not G[j, j].any() and G[j, np.arange(sh.n) != j].all()
    assert G[16].all()
    r = solve(oracle, sh, d)
    assert (r["status"][bad] == T.CHOL_H).all() and (r["iters"][bad] == 0).all()
    assert r["status"][16] == T.MAXIT_ST and r["iters"][16] == T.K_ITERS
    assert np.isfinite(r["x"][16 * sh.n:]).all()


def test_one_position_per_tile_and_block_boundary(oracle):
    sh, d, bad, good, nan_p = T.c2_column_batch(oracle)
    # every tile of H (columns 0-15, 16-31, 32-47, 48-63), first and last pivot of a tile, both sides of a block boundary
    assert {j // 16 for j in T.C2_COLUMNS} == {0, 1, 2, 3}
    assert {3, 4} <= set(T.C2_COLUMNS) and {15, 16} <= set(T.C2_COLUMNS) and {0, 63} <= set(T.C2_COLUMNS)
    r = solve(oracle, sh, d)
    assert (r["status"][bad] == T.CHOL_H).all() and (r["iters"][bad] == 0).all()
    assert r["status"][good[0]] == T.MAXIT_ST and r["iters"][good[0]] == T.K_ITERS
    assert r["status"][nan_p] in T.FAIL_CLASS and r["iters"][nan_p] == 0


def test_s_tile_rows(oracle):
    sh, d, bad, good = T.s_tile_batch(oracle)
    A = d["A"].reshape(len(bad) + 1, sh.n, sh.m)  # [problem, column, row]
    for i, row in enumerate(T.S_ROWS):
        assert not A[i, :, row].any() and A[i][:, np.arange(sh.m) != row].all()
    r = solve(oracle, sh, d)
    assert np.isin(r["status"][bad], T.FAIL_CLASS).all() and (r["iters"][bad] == 0).all()
    assert r["status"][good[0]] == T.MAXIT_ST and r["iters"][good[0]] == T.K_ITERS


@pytest.mark.parametrize("sh", T.PARITY + [T.PARITY_M20, T.PLUGIN], ids=T.shape_id)
def test_parity_shapes_run_their_iterations(oracle, sh):
    d = T._gen(oracle, sh, T.PARITY_B, T.SEED + 3)
    r = solve(oracle, sh, d)
    if sh.m <= sh.n:
        assert (r["status"] == T.MAXIT_ST).all() and (r["iters"] == T.K_ITERS).all()
    else:  # more equality rows than unknowns: S = A H^-1 A' is singular, the first factorisation fails
        assert np.isin(r["status"], T.FAIL_CLASS).all() and (r["iters"] == 0).all()


def test_parity_sweep_covers_the_tile_counts():
    assert sorted({-(-sh.n // 16) for sh in T.PARITY}) == [1, 2, 3, 4]
    assert {sh.m for sh in T.PARITY} == {0, 3, 16} and len(T.PARITY) == 15
    assert T.PARITY_M20.m > 16 and T.PARITY_M20.n == 32
    for sh in T.PARITY + [T.PARITY_M20, T.PLUGIN, T.LARGE]:
        assert sum(c[2] for c in sh.cones) == sh.k and all(c[2] > 0 for c in sh.cones)
