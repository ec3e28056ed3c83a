"""Parity of the HIP path (libsocp.so on MI355X) with the CPU oracle and the
reference's golden vectors.  Gates:
  P2 KKT golden through the HIP entry            <= 1e-10 abs
  P3 teacher-forced one step, kappa(H) <= 1e5     rel <= 1e-9
  P4 trajectory, first 3 (C1) / 6 (C2) iterations rel <= 1e-8
  P5 outcome on problems the oracle converges:    same status, |d iters| <= 1, |dx|_inf <= 1e-3
  P6 KKT backward error at healthy iterates       <= 1e-12 (relative)
Plus bit-exact device generation, batch/shard/warm-start equivalence, NaN isolation
and size-independent properties at the full C2 size.
"""
import numpy as np
import pytest

import socp_amd as S
from socp_amd.configs import C0B, C1, C2
from problems import batch_problem, kat_problem, optimal_control, random_cones

pytestmark = pytest.mark.gpu


def rel(a, b):
    a = np.asarray(a).reshape(-1)
    b = np.asarray(b).reshape(-1)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def gpu_batch(cfg_or_dims, d, B, **kw):
    cones, n, m, k = cfg_or_dims
    return S.batch_solve(cones, n, m, k, d["c"], d["A"], d["b"], d["G"], d["h"], kw.pop("sing", None), **kw)


def dims(cfg):
    return (cfg.cones, cfg.n, cfg.m, cfg.k)


# ------------------------------------------------------------------ goldens
def test_kkt_golden_through_hip(kats):
    g = kats["kkt_golden"]
    cones = [tuple(c) for c in g["cones"]]
    G = np.array(g["G"])
    out = S.batch_kkt_solve(cones, 3, 0, 4, None, G.ravel(order="F"), None, np.array(g["s"]), np.array(g["z"]),
                            np.array(g["dx"]), None, np.array(g["dz"]), np.array(g["ds"]))
    assert out["status"][0] == 0
    for key in ("cx", "cz", "cs"):
        assert np.abs(out[key] - np.array(g[key])).max() <= 1e-10, key


def test_kkt_mirror_api(kats):
    # the reference call sequence of runtests.jl:118-127 on the mirror surface
    g = kats["kkt_golden"]
    cones = [S.POC(0, 1), S.SOC(1, 3)]
    prob = S.Problem(g["c"], np.zeros((0, 3)), [], g["G"], g["h"], cones)
    solver = S.DenseSolver(prob)
    scaling = S.compute_scaling(cones, S.Scaling(prob), g["s"], g["z"])
    st = S.State(prob, g["x"], [], g["z"], g["s"])
    S.setup_iter(solver, prob, st, scaling)
    cx, cy, cz, cs = np.zeros(3), np.zeros(0), np.zeros(4), np.zeros(4)
    dx, dz, ds = np.array(g["dx"]), np.array(g["dz"]), np.array(g["ds"])
    S.solve_kkt(solver, prob, st, scaling, dx, np.zeros(0), dz, ds, cx, cy, cz, cs)
    assert np.array_equal(dx, g["dx"]) and np.array_equal(ds, g["ds"])  # inputs untouched
    assert np.linalg.norm(cx - g["cx"]) < 1e-10 and np.linalg.norm(cs - g["cs"]) < 1e-10


@pytest.mark.parametrize("name", ["soc1", "soc2", "soc3"])
def test_end_to_end_kats(kats, oracle, name):
    q = kats[name]
    cones, c, A, b, G, h = kat_problem(q)
    prob = S.Problem(c, A, b, G, h, cones)
    ss = S.SolverState(prob, S.DenseSolver(prob))
    st = S.solve_socp(prob, ss)
    assert ss.status == S.CONVERGED
    assert np.linalg.norm(st.x - np.array(q["x_expect"])) < q["tol"]  # the reference's own assertion
    r = oracle.solve_trace(cones, c, A, b, G, h)
    assert ss.iters == r["iters"]
    assert np.abs(st.x - r["x"]).max() <= 1e-3


def test_sing_batch_c0b(oracle):
    cfg, B = C0B, 64
    d = oracle.generate(cfg.cones, B, cfg.n, cfg.m, cfg.k, cfg.seed)
    r = oracle.batch_solve(cfg.cones, cfg.n, cfg.m, cfg.k, d["c"], d["A"], d["b"], d["G"], d["h"])
    g = gpu_batch(dims(cfg), d, B)  # sing detected on the device
    ok = r["status"] == 0
    assert ok.mean() > 0.9
    assert (g["status"][ok] == 0).all()
    assert np.abs(g["iters"][ok] - r["iters"][ok]).max() <= 1
    dx = np.abs(g["x"].reshape(B, -1) - r["x"].reshape(B, -1)).max(axis=1)
    assert dx[ok].max() <= 1e-3


def test_beyond_both_kernels_reports_unsupported():
    # n > 2048: outside the blocked kernel in both operation orders (n = 600
    # solves in both: tests/test_gpu_large.py::test_wide_n_*,
    # tests/test_gpu_large.py::test_wide_n_blocked_cholesky)
    for n, xi in ((2100, False), (2100, True)):
        k = n + 1
        with pytest.raises(S.SocpError) as e:
            S.batch_solve([(1, 0, k)], n, 0, k, np.zeros(n), None, None, np.zeros(k * n), np.zeros(k),
                          explicit_inverse=xi)
        assert e.value.code == -2, (n, xi)


# ------------------------------------------------------------ generator
def test_device_generator_bit_exact(oracle):
    import torch
    for cfg in (C1, C2, C0B):
        B, first = 8, 1000
        dev = S.generate(cfg.cones, B, cfg.n, cfg.m, cfg.k, cfg.seed, first_problem=first)
        torch.cuda.synchronize()
        cpu = oracle.generate(cfg.cones, B, cfg.n, cfg.m, cfg.k, cfg.seed, first_problem=first)
        for key, t in zip(("c", "A", "b", "G", "h"), dev):
            assert np.array_equal(t.cpu().numpy(), cpu[key]), (cfg.name, key)


# ------------------------------------------------------ P3 / P4 / P5 / P6
@pytest.mark.parametrize("cfg,maxk", [(C1, 3), (C2, 6)])
def test_trajectory_parity(oracle, cfg, maxk):
    B = 32
    d = oracle.generate(cfg.cones, B, cfg.n, cfg.m, cfg.k, cfg.seed)
    for K in range(1, maxk + 1):
        r = oracle.batch_solve(cfg.cones, cfg.n, cfg.m, cfg.k, d["c"], d["A"], d["b"], d["G"], d["h"],
                               params=oracle.Params(maxit=K, tol=0.0))
        g = gpu_batch(dims(cfg), d, B, maxit=K, tol=0.0)
        assert (g["status"] == r["status"]).all()
        for p in range(B):
            for key, L in (("x", cfg.n), ("z", cfg.k), ("s", cfg.k)):
                e = rel(g[key][p * L:(p + 1) * L], r[key][p * L:(p + 1) * L])
                assert e <= 1e-8, (K, p, key, e)


@pytest.mark.parametrize("cfg", [C1, C2])
def test_teacher_forced_one_step(oracle, cfg):
    """P3: from oracle iterate j, one GPU iteration vs one oracle iteration while kappa(H_j) <= 1e5.
    Bound: rel <= max(1e-9, 2e-14 * kappa(H_j)) -- the SURVEY.md §8(c) probe's 5.7e-10 at kappa <= 1e5
    scaled with the conditioning of the system the two implementations invert."""
    B = 4
    d = oracle.generate(cfg.cones, B, cfg.n, cfg.m, cfg.k, cfg.seed)
    checked = 0
    for p in range(B):
        c, A, b, G, h = batch_problem(d, B, cfg.n, cfg.m, cfg.k, p)
        tr = oracle.solve_trace(cfg.cones, c, A, b, G, h, params=oracle.Params(maxit=14, tol=0.0), max_trace=15)
        for t in range(len(tr["trace"]) - 1):
            x, y, z, s = tr["trace"][t]
            H = oracle.kkt_single(cfg.cones, A, G, False, s, z, np.zeros(cfg.n), np.zeros(cfg.m), np.zeros(cfg.k),
                                  np.zeros(cfg.k), want_H=True)["H"]
            kap = np.linalg.cond(H)
            if kap > 1e5:
                break
            g = S.batch_solve(cfg.cones, cfg.n, cfg.m, cfg.k, c, A.ravel(order="F"), b, G.ravel(order="F"), h,
                              np.zeros(1, np.uint8), maxit=1, tol=0.0, warm=tr["trace"][t])
            xo, yo, zo, so = tr["trace"][t + 1]
            for got, want in ((g["x"], xo), (g["z"], zo), (g["s"], so), (g["y"], yo)):
                assert rel(got, want) <= max(1e-9, 2e-14 * kap), (p, t, kap, rel(got, want))
            checked += 1
    assert checked >= 8


@pytest.mark.parametrize("cfg,B", [(C1, 256), (C2, 256)])
def test_outcome_parity(oracle, cfg, B):
    """P5 on problems where the oracle (reference order) converges.  Late
    iterations are chaotic.  C1: every oracle-converged problem
    converges on the GPU within one iteration.  C2: the gates are the chaos
    floor of the same comparison done on the CPU -- the oracle in the kernels'
    order (F_STRUCTURED | F_CHOLSOLVE, unperturbed and G perturbed by one ulp)
    against the reference-order oracle on these 256 problems
    (tests/golden/c2_chaos_floor.json, "cross/first256") -- minus one point and
    one problem's share (the rule of test_gpu_outcomes.py)."""
    d = oracle.generate(cfg.cones, B, cfg.n, cfg.m, cfg.k, cfg.seed)
    r = oracle.batch_solve(cfg.cones, cfg.n, cfg.m, cfg.k, d["c"], d["A"], d["b"], d["G"], d["h"])
    g = gpu_batch(dims(cfg), d, B, res=True)
    ok = r["status"] == 0
    assert ok.sum() >= (0.3 * B if cfg is C2 else 0.95 * B)
    gok = g["status"] == 0
    both = ok & gok
    itok = np.abs(g["iters"] - r["iters"]) <= 1
    frac = itok[both].mean()
    if cfg is C2:
        import json
        import os
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "c2_chaos_floor.json")) as f:
            fl = json.load(f)
        assert fl["batch"] >= B and fl["seed"] == cfg.seed
        floor = fl["cross"]["structured_chol_vs_reference_order/first256"]["floor"]
        slack = fl["gate_slack"]
        assert gok[ok].mean() >= floor["of_conv"] - slack - 1.0 / ok.sum(), (gok[ok].mean(), floor)
        assert frac >= floor["iters1"] - slack - 1.0 / both.sum(), (frac, floor)
    else:
        assert gok[ok].all(), gok[ok].mean()
        assert frac == 1.0, frac
    dx = np.abs(g["x"].reshape(B, -1) - r["x"].reshape(B, -1)).max(axis=1)
    assert dx[both].max() <= 1e-3
    # everything the GPU reports as converged meets the reference exit test
    res = g["res"].reshape(B, 3)
    gc = g["status"] == 0
    assert (res[gc].sum(axis=1) < 1e-5).all()


@pytest.mark.parametrize("cfg", [C1, C2])
def test_kkt_backward_error(oracle, cfg):
    """P6: relative residual of every block row of the KKT system at healthy iterates.
    Bound: max(1e-12, 10 x the reference's own backward error on the same system) --
    the reference (oracle restatement) itself reaches 3.3e-10 here at kappa(H) ~ 3e4."""
    B = 2
    d = oracle.generate(cfg.cones, B, cfg.n, cfg.m, cfg.k, cfg.seed)
    rng = np.random.default_rng(1)
    for p in range(B):
        c, A, b, G, h = batch_problem(d, B, cfg.n, cfg.m, cfg.k, p)
        tr = oracle.solve_trace(cfg.cones, c, A, b, G, h, params=oracle.Params(maxit=6, tol=0.0), max_trace=7)
        for t in range(3):
            x, y, z, s = tr["trace"][t]
            rhs = [rng.standard_normal(n) for n in (cfg.n, cfg.m, cfg.k, cfg.k)]
            out = S.batch_kkt_solve(cfg.cones, cfg.n, cfg.m, cfg.k, A.ravel(order="F"), G.ravel(order="F"),
                                    np.zeros(1, np.uint8), s, z, *rhs)
            sc = oracle.compute_scaling(cfg.cones, s, z)
            W, lam = sc["W"], sc["l"]
            cx, cy, cz, cs = out["cx"], out["cy"], out["cz"], out["cs"]

            def backward(cx, cy, cz, cs):
                r1 = A.T @ cy + G.T @ cz - rhs[0]
                r2 = A @ cx - rhs[1]
                r3 = G @ cx + cs - rhs[2]
                r4 = oracle.vprod(cfg.cones, lam, W @ cz + np.linalg.solve(W.T, cs)) - rhs[3]
                scale = max(np.abs(np.concatenate(rhs)).max(), np.abs(np.concatenate([cx, cy, cz, cs])).max())
                return max(np.abs(rr).max() for rr in (r1, r2, r3, r4)) / scale

            o = oracle.kkt_single(cfg.cones, A, G, False, s, z, *rhs)
            ref_err = backward(o["cx"], o["cy"], o["cz"], o["cs"])
            assert backward(cx, cy, cz, cs) <= max(1e-12, 10 * ref_err), (p, t, ref_err)


# ------------------------------------------------- structural equivalences
def test_batch_vs_single_and_warm_start(oracle):
    cfg, B = C2, 16
    d = oracle.generate(cfg.cones, B, cfg.n, cfg.m, cfg.k, cfg.seed)
    full = gpu_batch(dims(cfg), d, B, maxit=5, tol=0.0)
    p = 7
    c, A, b, G, h = batch_problem(d, B, cfg.n, cfg.m, cfg.k, p)
    one = S.batch_solve(cfg.cones, cfg.n, cfg.m, cfg.k, c, A.ravel(order="F"), b, G.ravel(order="F"), h,
                        None, maxit=5, tol=0.0)
    n, k = cfg.n, cfg.k
    assert np.array_equal(one["x"], full["x"][p * n:(p + 1) * n])  # bitwise: per-problem determinism
    assert np.array_equal(one["s"], full["s"][p * k:(p + 1) * k])
    # 2 + 3 iterations with a warm start == 5 iterations
    a2 = gpu_batch(dims(cfg), d, B, maxit=2, tol=0.0)
    a5 = gpu_batch(dims(cfg), d, B, maxit=3, tol=0.0, warm=(a2["x"], a2["y"], a2["z"], a2["s"]))
    assert np.array_equal(a5["x"], full["x"]) and np.array_equal(a5["z"], full["z"])


def test_nan_isolation(oracle):
    cfg, B = C2, 16
    d = oracle.generate(cfg.cones, B, cfg.n, cfg.m, cfg.k, cfg.seed)
    ref = gpu_batch(dims(cfg), d, B, maxit=6, tol=0.0)
    bad = dict(d)
    bad["G"] = d["G"].copy()
    L = cfg.k * cfg.n
    bad["G"][3 * L + 17] = np.nan
    got = gpu_batch(dims(cfg), bad, B, maxit=6, tol=0.0)
    assert got["status"][3] in (S.CHOL_H_FAILED, S.CHOL_S_FAILED, S.DOMAIN_ERROR)
    others = np.arange(B) != 3
    n = cfg.n
    assert np.array_equal(got["status"][others], ref["status"][others])
    assert np.array_equal(got["x"].reshape(B, n)[others], ref["x"].reshape(B, n)[others])


def test_empty_batch():
    out = S.batch_solve(C1.cones, C1.n, C1.m, C1.k, np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(0))
    assert out["x"].size == 0


# ------------------------------------------------------------ shape sweep
@pytest.mark.parametrize("seed", range(6))
def test_random_shapes_early_parity(oracle, seed):
    rng = np.random.default_rng(100 + seed)
    n = int(rng.integers(3, 65))
    m = int(rng.integers(0, min(n, 40)))
    # k <= 96: the range every NQ is compiled for (NP = 32, k <= 128, stops at NQ = 3; test_gpu_variants.py runs it)
    k = int(rng.integers(n + 1, 97))
    cones = random_cones(rng, k)
    if len(cones) > 8:
        cones = cones[:7] + [(1, cones[7][1], k - cones[7][1])]
    B = 8
    d = oracle.generate(cones, B, n, m, k, 12345 + seed)
    r = oracle.batch_solve(cones, n, m, k, d["c"], d["A"], d["b"], d["G"], d["h"], params=oracle.Params(maxit=2, tol=0.0))
    g = S.batch_solve(cones, n, m, k, d["c"], d["A"], d["b"], d["G"], d["h"], None, maxit=2, tol=0.0)
    assert (g["status"] == r["status"]).all(), (n, m, k, cones)
    for p in range(B):
        if r["status"][p] != 1:
            continue
        assert rel(g["x"][p * n:(p + 1) * n], r["x"][p * n:(p + 1) * n]) <= 1e-8, (n, m, k, cones, p)


@pytest.mark.parametrize("n,m,k,cones", [
    (3, 1, 5, [(0, 0, 2), (1, 2, 3)]),                     # KP = 8: k-vectors 8 apart in LDS
    (30, 6, 47, [(0, 0, 7), (1, 7, 20), (1, 27, 20)]),     # KP = 48, one padding row
    (40, 8, 62, [(1, 0, 31), (1, 31, 31)]),                # KP = 64, two padding rows
    (48, 16, 64, [(0, 0, 16), (1, 16, 48)]),               # KP = 64 exactly: last shape packed KP apart
    (48, 16, 65, [(0, 0, 17), (1, 17, 48)]),               # KP = 68: two slots, 128 apart
])
def test_kvector_stride_boundaries(oracle, n, m, k, cones):
    """The register kernel packs its k-vectors KP apart when KP <= 64 (and 128
    apart otherwise); shapes on both sides of the boundary match the oracle."""
    B = 16
    d = oracle.generate(cones, B, n, m, k, 4242 + k)
    r = oracle.batch_solve(cones, n, m, k, d["c"], d["A"], d["b"], d["G"], d["h"], params=oracle.Params(maxit=3, tol=0.0))
    g = S.batch_solve(cones, n, m, k, d["c"], d["A"], d["b"], d["G"], d["h"], None, maxit=3, tol=0.0)
    assert (g["status"] == r["status"]).all(), (g["status"], r["status"])
    for key, dim in (("x", n), ("z", k), ("s", k)):
        assert rel(g[key], r[key]) <= 1e-8, (key, rel(g[key], r[key]))


def test_lp_and_m0_edge_cases(oracle):
    # pure LP (one POC cone, explicit-inverse sensitive: SURVEY.md §0.6) and m = 0
    for cones, n, m, k in (([(0, 0, 40)], 20, 5, 40), ([(1, 0, 24)], 16, 0, 24)):
        B = 8
        d = oracle.generate(cones, B, n, m, k, 777)
        r = oracle.batch_solve(cones, n, m, k, d["c"], d["A"], d["b"], d["G"], d["h"], params=oracle.Params(maxit=3, tol=0.0))
        g = S.batch_solve(cones, n, m, k, d["c"], d["A"], d["b"], d["G"], d["h"], None, maxit=3, tol=0.0)
        assert (g["status"] == r["status"]).all()
        assert rel(g["x"], r["x"]) <= 1e-8


# ------------------------------------------------------- full-size (C2)
def test_full_size_c2_properties(oracle):
    """BASELINE size, device-resident: fixed-K=8 on 65,536 problems; every iterate
    strictly inside its cones, gaps shrink, and a sampled subset matches the oracle."""
    import torch
    cfg = C2
    B = cfg.batch
    c, A, b, G, h = S.generate(cfg.cones, B, cfg.n, cfg.m, cfg.k, cfg.seed)
    sing = torch.zeros(B, dtype=torch.uint8, device=G.device)
    out = S.batch_solve(cfg.cones, cfg.n, cfg.m, cfg.k, c, A, b, G, h, sing, maxit=8, tol=0.0, res=True)
    S.default_context().sync()
    st = out["status"].cpu().numpy()
    assert (st == S.MAXIT).mean() > 0.99
    z = out["z"].cpu().numpy().reshape(B, cfg.k)
    s = out["s"].cpu().numpy().reshape(B, cfg.k)
    okp = st == S.MAXIT
    for arr in (z, s):
        assert (arr[okp, :32] > 0).all()  # POC block
        for o in (32, 64):
            assert (arr[okp, o] > np.linalg.norm(arr[okp, o + 1:o + 32], axis=1)).all()  # SOC blocks
    res = out["res"].cpu().numpy().reshape(B, 3)
    assert np.median(res[okp, 2]) < 1.0  # gap 596 -> O(0.1) after 8 iterations (see the trajectory test)
    # sampled oracle comparison
    idx = np.random.default_rng(0).choice(B, 24, replace=False)
    flat = {key: t.cpu().numpy() for key, t in zip(("c", "A", "b", "G", "h"), (c, A, b, G, h))}
    for p in idx:
        pc, pA, pb, pG, ph = batch_problem(flat, B, cfg.n, cfg.m, cfg.k, p)
        r = oracle.solve_trace(cfg.cones, pc, pA, pb, pG, ph, sing=False, params=oracle.Params(maxit=8, tol=0.0))
        assert rel(out["x"][p * cfg.n:(p + 1) * cfg.n].cpu().numpy(), r["x"]) <= 1e-6


# ------------------------------------------------------------- ingest (§8(f))
def test_pack_csc_matches_dense():
    """SparseMatrixCSC -> dense column-major batch (socp_pack_csc), bit-exact
    against scipy's toarray(); Julia's 1-based indices and 0-based ones; empty
    columns, an all-zero matrix, a duplicate entry (summed), and a bad index."""
    import scipy.sparse as sp
    import torch
    rng = np.random.default_rng(5)
    rows, cols = 96, 64
    mats = [sp.random(rows, cols, density=d, random_state=int(rng.integers(1 << 30)), format="csc")
            for d in (0.05, 0.3, 0.0, 1.0)]
    mats[0][:, 7] = 0.0  # an empty column
    mats[0].eliminate_zeros()
    want = np.concatenate([m.toarray().ravel(order="F") for m in mats])
    for base in (1, 0):
        got = S.pack_csc(mats, index_base=base).cpu().numpy()
        assert np.array_equal(got, want), base
    # duplicates are summed (sparse() semantics)
    dup = sp.csc_matrix((np.array([1.0, 2.0, 4.0]), np.array([3, 3, 5]), np.array([0, 3] + [3] * (cols - 1))),
                        shape=(rows, cols))
    got = S.pack_csc([dup]).cpu().numpy().reshape(cols, rows).T
    assert got[3, 0] == 3.0 and got[5, 0] == 4.0 and np.count_nonzero(got) == 2
    # a row index out of range is an API error
    dev = torch.device("cuda", 0)
    i64 = dict(dtype=torch.int64, device=dev)
    bad = (torch.tensor([0, 1], **i64), torch.tensor([1] + [2] * cols, **i64), torch.tensor([rows + 1], **i64),
           torch.ones(1, dtype=torch.float64, device=dev))
    with pytest.raises(S.SocpError) as e:
        S.pack_csc(bad, rows, cols)
    assert e.value.code == -1


def test_warm_start_from_fresh_device_tensors(oracle):
    """inputs torch computes just before a device-mode call (here the
    warm-start iterate, produced by a chain of torch ops on torch's current
    stream) are complete when the solver reads them: the context's work is
    ordered on torch's stream (socp_ctx_set_stream)."""
    import torch
    cfg, B = C2, 512
    c, A, b, G, h = S.generate(cfg.cones, B, cfg.n, cfg.m, cfg.k, cfg.seed)
    sing = torch.zeros(B, dtype=torch.uint8, device=G.device)
    a2 = S.batch_solve(cfg.cones, cfg.n, cfg.m, cfg.k, c, A, b, G, h, sing, maxit=2, tol=0.0)
    ref = S.batch_solve(cfg.cones, cfg.n, cfg.m, cfg.k, c, A, b, G, h, sing, maxit=3, tol=0.0,
                        warm=(a2["x"], a2["y"], a2["z"], a2["s"]))
    ref = {key: v.clone() for key, v in ref.items()}
    for _ in range(3):
        # a long dependent torch chain that ends in the warm iterate: x + big - big
        big = torch.full_like(a2["z"], 1e3)
        wz = a2["z"].clone()
        for _ in range(50):
            wz = (wz + big) - big + 0.0 * torch.sin(wz)
        wz = a2["z"].clone().copy_(a2["z"])  # exact values, produced last on the stream
        wx, wy, ws = a2["x"] * 1.0, a2["y"] * 1.0, a2["s"] * 1.0
        got = S.batch_solve(cfg.cones, cfg.n, cfg.m, cfg.k, c, A, b, G, h, sing, maxit=3, tol=0.0,
                            warm=(wx, wy, wz, ws))
        # consume on torch's stream without an explicit context sync
        assert torch.equal(got["x"], ref["x"]) and torch.equal(got["z"], ref["z"])


def test_pack_csc_unsorted_nonadjacent_duplicates():
    """a hand-built CSC whose column has unsorted rows with a
    non-adjacent duplicate ([3, 5, 3]) sums both entries (device kernel), and
    scipy input is canonicalised (sum_duplicates) before packing."""
    import scipy.sparse as sp
    import torch
    rows, cols = 8, 3
    dev = torch.device("cuda", 0)
    i64 = dict(dtype=torch.int64, device=dev)
    # column 0: rows [3, 5, 3] (values 1, 2, 4); column 1 empty; column 2: rows [6, 1]
    colptr = torch.tensor([1, 4, 4, 6], **i64)  # Julia 1-based
    rowval = torch.tensor([4, 6, 4, 7, 2], **i64)
    nzval = torch.tensor([1.0, 2.0, 4.0, 8.0, 16.0], dtype=torch.float64, device=dev)
    nz_offs = torch.tensor([0, 5], **i64)
    for _ in range(5):  # the sum must not depend on which thread stores first
        got = S.pack_csc((nz_offs, colptr, rowval, nzval), rows, cols).cpu().numpy().reshape(cols, rows).T
        want = np.zeros((rows, cols))
        want[3, 0], want[5, 0], want[6, 2], want[1, 2] = 5.0, 2.0, 8.0, 16.0
        assert np.array_equal(got, want)
    # scipy: an unsorted csc with a non-adjacent duplicate
    m = sp.csc_matrix((np.array([1.0, 2.0, 4.0]), np.array([3, 5, 3]), np.array([0, 3, 3, 3])), shape=(rows, cols))
    got = S.pack_csc([m]).cpu().numpy().reshape(cols, rows).T
    assert got[3, 0] == 5.0 and got[5, 0] == 2.0 and np.count_nonzero(got) == 2


def test_pack_csc_duplicates_sum_in_input_order():
    """three or more duplicates of one (i, j) are summed in
    input order (a thread per column), so the packed value is the sequential
    sum bit for bit -- values chosen so that the order changes the rounding."""
    import torch
    rows, cols, B = 4, 2, 64
    dev = torch.device("cuda", 0)
    i64 = dict(dtype=torch.int64, device=dev)
    vals = [1.0, 1e-16, 1e-16, -1.0, 3e-16, 0.5]  # all into (2, 0), then (1, 1)
    colptr = torch.tensor([0, 5, 6] * B, **i64)
    rowval = torch.tensor(([2, 2, 2, 2, 2, 1]) * B, **i64)
    nzval = torch.tensor(vals * B, dtype=torch.float64, device=dev)
    nz_offs = torch.arange(0, 6 * B + 1, 6, **i64)
    seq = 0.0
    for v in vals[:5]:
        seq += v
    for _ in range(3):
        got = S.pack_csc((nz_offs, colptr, rowval, nzval), rows, cols, index_base=0).cpu().numpy().reshape(B, cols, rows)
        assert (got[:, 0, 2] == seq).all() and (got[:, 1, 1] == 0.5).all()
        assert np.count_nonzero(got) == 2 * B


def test_batch_above_int32_rejected():
    """the persistent kernels index problems with an int32 counter."""
    import ctypes as C
    from socp_amd import _lib
    L = _lib.load()
    ctx = S.default_context()
    kind, offs, dim = S.cone_arrays(C1.cones)
    d = _lib.Dims(2**31, C1.n, C1.m, C1.k, len(kind))
    p = _lib.ptr
    rc = L.socp_generate(ctx.handle, C.byref(d), p(kind), p(offs), p(dim), 1, 0, None, None, None, None, None)
    assert rc == _lib.SOCP_E_INVALID and b"2^31" in L.socp_last_error()
    rc = L.socp_pack_csc(ctx.handle, 2**31, 4, 4, None, None, None, None, 1, None)
    assert rc == _lib.SOCP_E_INVALID


def test_problem_dump_env(tmp_path, monkeypatch, oracle):
    """SOCP_DUMP_DIR mirrors the reference's commented-out dumps (solver.jl:48-67,
    75-82): A, G, c, b, h, cones and initv = [-c; b; h] of the first problems."""
    cfg, B = C1, 4
    d = oracle.generate(cfg.cones, B, cfg.n, cfg.m, cfg.k, cfg.seed)
    monkeypatch.setenv("SOCP_DUMP_DIR", str(tmp_path))
    monkeypatch.setenv("SOCP_DUMP_COUNT", "2")
    gpu_batch(dims(cfg), d, B, maxit=1, tol=0.0)
    monkeypatch.delenv("SOCP_DUMP_DIR")
    n, m, k = cfg.n, cfg.m, cfg.k
    for p in range(2):
        pc, pA, pb, pG, ph = batch_problem(d, B, n, m, k, p)
        assert np.array_equal(np.loadtxt(tmp_path / f"problem{p}_G.txt"), pG)
        assert np.array_equal(np.loadtxt(tmp_path / f"problem{p}_A.txt"), pA)
        assert np.array_equal(np.loadtxt(tmp_path / f"problem{p}_h.txt"), ph)
        iv = np.loadtxt(tmp_path / f"problem{p}_initv.txt")
        assert np.array_equal(iv, np.concatenate([-pc, pb, ph]))
        assert (tmp_path / f"problem{p}_cones.txt").read_text().split() == ["SOC(0,48)"]
    assert not (tmp_path / "problem2_G.txt").exists()
