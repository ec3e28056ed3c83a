"""The 16x16 tile factorisation (factor_tile) at every pivot position, and
parity with the CPU oracle across tile counts and paths.  Inputs:
tile_cases.py; that the oracle gives the outcomes relied on here:
test_tile_cases_cpu.py.

Pivot positions: a problem with column j of G zeroed loses pivot j of chol(H)
exactly (tile j // 16, row block (j % 16) // 4, pivot j % 4), a problem with
row r of A zeroed loses pivot r of the S tile.  The kernel must stop such a
problem where the oracle does (iteration 0), with the oracle's status (for
the S tile and the NaN: a status of the failure class, as the
failure-isolation tests of test_gpu_parity.py map it), and leave its
neighbours' results as they are when solved alone, bit for bit.

Parity: 3 iterations, same status and rel <= 1e-8 on x, y, z, s per problem
(test_gpu_parity.py's trajectory gate) for one to four tiles of H, no / a
partial / a full S tile, two S tiles (m = 20), the explicit inverse, the split
plugin entries (rel <= 1e-8 against the oracle's KKT solve, as smoke() holds
them) and the blocked kernel.
"""
import numpy as np
import pytest

import socp_amd as S
import tile_cases as T

pytestmark = pytest.mark.gpu
KEYS = (("x", "n"), ("y", "m"), ("z", "k"), ("s", "k"))


def rel(a, b):
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def gpu_solve(sh, d, sing, **kw):
    return S.batch_solve(sh.cones, sh.n, sh.m, sh.k, d["c"], d["A"], d["b"], d["G"], d["h"], sing,
                         maxit=T.K_ITERS, tol=0.0, **kw)


def one_problem(sh, d, p):
    sl = lambda v, L: v[p * L:(p + 1) * L]  # noqa: E731
    return dict(c=sl(d["c"], sh.n), A=sl(d["A"], sh.m * sh.n), b=sl(d["b"], sh.m), G=sl(d["G"], sh.k * sh.n),
                h=sl(d["h"], sh.k))


def assert_problem_parity(sh, g, r, p, tag):
    for key, dim in KEYS:
        L = getattr(sh, dim)
        if L == 0:
            continue
        e = rel(g[key][p * L:(p + 1) * L], r[key][p * L:(p + 1) * L])
        print(f"{tag} p={p} {key} rel={e:.3e}")
        assert e <= 1e-8, (tag, p, key, e)


def check_failures(oracle, sh, d, bad, good, exact_status, tag):
    """bad: problems that lose a pivot; good: untouched ones."""
    B = len(d["c"]) // sh.n
    sing = np.zeros(B, np.uint8)
    r = T.oracle_solve(oracle, sh, d, sing)
    g = gpu_solve(sh, d, sing)
    print(tag, "oracle status", r["status"].tolist(), "iters", r["iters"].tolist())
    print(tag, "kernel status", g["status"].tolist(), "iters", g["iters"].tolist())
    for p in bad:
        assert r["status"][p] in T.FAIL_CLASS and r["iters"][p] == 0  # test_tile_cases_cpu.py
        if exact_status:
            assert g["status"][p] == r["status"][p], (tag, p)
        else:
            assert g["status"][p] in T.FAIL_CLASS, (tag, p)
        assert g["iters"][p] == r["iters"][p], (tag, p)
    for p in good:
        assert g["status"][p] == r["status"][p] == T.MAXIT_ST and g["iters"][p] == r["iters"][p] == T.K_ITERS
        assert_problem_parity(sh, g, r, p, tag)
        alone = gpu_solve(sh, one_problem(sh, d, p), np.zeros(1, np.uint8))
        for key, dim in KEYS:
            L = getattr(sh, dim)
            assert np.array_equal(alone[key][:L], g[key][p * L:(p + 1) * L]), (tag, p, key)
    return g


def test_every_pivot_position_of_one_tile(oracle):
    sh, d, bad, good = T.one_tile_batch(oracle)
    check_failures(oracle, sh, d, bad, good, True, "one_tile")
    assert "<1,4,1>" in S.default_context().last_kernel_name()


def test_one_position_per_tile_and_block_boundary(oracle):
    sh, d, bad, good, nan_p = T.c2_column_batch(oracle)
    g = check_failures(oracle, sh, d, bad, good, True, "c2_columns")
    assert "<4,24,1>" in S.default_context().last_kernel_name()
    assert g["status"][nan_p] in T.FAIL_CLASS and g["iters"][nan_p] == 0


def test_s_tile_pivots(oracle):
    sh, d, bad, good = T.s_tile_batch(oracle)
    check_failures(oracle, sh, d, bad, good, False, "s_tile")


def check_parity(oracle, sh, sing, flags=0, **kw):
    d = T._gen(oracle, sh, T.PARITY_B, T.SEED + 3)
    r = T.oracle_solve(oracle, sh, d, sing, flags)
    g = gpu_solve(sh, d, sing, **kw)
    tag = T.shape_id(sh)
    print(tag, S.default_context().last_kernel_name(), "status", g["status"].tolist(), "oracle", r["status"].tolist())
    for p in range(T.PARITY_B):
        if r["status"][p] in T.FAIL_CLASS:  # m > n: S is singular, the first factorisation fails
            assert g["status"][p] in T.FAIL_CLASS and g["iters"][p] == r["iters"][p], (tag, p)
            continue
        assert g["status"][p] == r["status"][p] and g["iters"][p] == r["iters"][p], (tag, p)
        assert_problem_parity(sh, g, r, p, tag)


@pytest.mark.parametrize("sh", T.PARITY + [T.PARITY_M20], ids=T.shape_id)
def test_parity_across_tile_counts(oracle, sh):
    check_parity(oracle, sh, np.zeros(T.PARITY_B, np.uint8))


def test_parity_explicit_inverse(oracle):
    # the oracle's structured order with the kernels' Y'Y inverse, as test_gpu_xi.py compares it
    check_parity(oracle, T.PLUGIN, np.zeros(T.PARITY_B, np.uint8), oracle.F_STRUCTURED | oracle.F_INV_YTY,
                 explicit_inverse=True)


def test_parity_blocked_kernel(oracle):
    check_parity(oracle, T.LARGE, None, force_large=True)  # k < n: `sing` by the constructor's rule on both sides


def test_parity_setup_iter_solve_kkt(oracle):
    sh, B = T.PLUGIN, T.PARITY_B
    d = T._gen(oracle, sh, B, T.SEED + 3)
    sing = np.zeros(B, np.uint8)
    it = T.oracle_solve(oracle, sh, d, sing, maxit=2)  # interior iterates
    h = S.DenseHandle(sh.cones, sh.n, sh.m, sh.k, d["A"], d["G"], sing)
    assert (h.setup_iter(it["s"], it["z"]) == 0).all()
    rng = np.random.default_rng(7)
    dims = (sh.n, sh.m, sh.k, sh.k)
    rhs = [rng.standard_normal(B * q) for q in dims]
    got = h.solve_kkt(*rhs)
    assert (got["status"] == 0).all()
    for p in range(B):
        sl = lambda v, q: v[p * q:(p + 1) * q]  # noqa: E731
        A = sl(d["A"], sh.m * sh.n).reshape(sh.n, sh.m).T
        G = sl(d["G"], sh.k * sh.n).reshape(sh.n, sh.k).T
        ro = oracle.kkt_single(sh.cones, A, G, False, sl(it["s"], sh.k), sl(it["z"], sh.k),
                               *[sl(v, q) for v, q in zip(rhs, dims)])
        for key, q in zip(("cx", "cy", "cz", "cs"), dims):
            e = rel(sl(got[key], q), ro[key])
            print(f"split p={p} {key} rel={e:.3e}")
            assert e <= 1e-8, (p, key, e)
