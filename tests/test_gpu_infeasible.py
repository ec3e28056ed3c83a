"""Infeasibility detection on the GPU (SOCP_F_DETECT_INFEASIBLE): the register
kernel, the blocked kernel (LDS and global-vector forms) and the rank-update
IPM.  Every batch holds 48 problems -- 16 feasible, 16 primal-infeasible, 16
dual-infeasible, interleaved (tests/infeasible.py) -- and every certificate is
checked in numpy from the returned arrays alone."""
import functools

import numpy as np
import pytest

import socp_amd as S
from socp_amd import _lib
from socp_amd import moi as M
from socp_amd.configs import C1
import infeasible as I

pytestmark = pytest.mark.gpu

CONES16 = [(0, 0, 6), (1, 6, 5), (1, 11, 5)]


def cones3(k):
    d = k // 3
    return [(0, 0, d), (1, d, d), (1, 2 * d, k - 2 * d)]


# name: (path, n, m, k, cones, compare iters with the oracle trace in this order (None: validity only))
SHAPES = {
    "small_8_2_16": ("dense", 8, 2, 16, CONES16, "kernel"),
    "small_8_0_16": ("dense", 8, 0, 16, CONES16, "kernel"),
    "small_32_8_48": ("dense", 32, 8, 48, cones3(48), "kernel"),
    "small_40_20_60_inverse": ("dense", 40, 20, 60, cones3(60), None),
    "forced_large_8_2_16": ("large", 8, 2, 16, CONES16, "kernel"),
    "large_80_20_120": ("dense", 80, 20, 120, cones3(120), "kernel"),
    "large_gv_64_16_4096": ("dense", 64, 16, 4096, [(0, 0, 1024), (1, 1024, 1024), (1, 2048, 1024), (1, 3072, 1024)],
                            None),
    "sqr_8_2_16": ("sqr", 8, 2, 16, CONES16, "sqr"),
    "sqr_80_20_120": ("sqr", 80, 20, 120, cones3(120), "sqr"),
    "sqr_200_50_240_record": ("sqr", 200, 50, 240, cones3(240), None),
}
KERNEL = {"small_8_2_16": "socp_small_di_kernel<1,4,1>", "small_8_0_16": "socp_small_di_kernel<1,4,1>",
          "small_32_8_48": "socp_small_di_kernel<2,12,1>", "small_40_20_60_inverse": "socp_small_di_kernel<3,16,2>",
          "forced_large_8_2_16": "socp_large_di_kernel", "large_80_20_120": "socp_large_di_kernel",
          "large_gv_64_16_4096": "socp_large_di_gv_kernel"}


def solve(name, flat, detect, ctx=None, **kw):
    path, n, m, k, cones, _ = SHAPES[name]
    B = flat["c"].size // n
    sing = np.zeros(B, np.uint8)
    if path == "sqr":
        h = S.SqrHandle(cones, n, m, k, flat["A"] if m else None, flat["G"], sing, ctx=ctx)
        out = h.solve_socp(flat["c"], flat["b"] if m else None, flat["h"], detect_infeasible=detect, **kw)
        out["kernel"] = None
        h.close()
        return out
    ctx = ctx or S.default_context()
    out = S.batch_solve(cones, n, m, k, flat["c"], flat["A"] if m else None, flat["b"] if m else None, flat["G"],
                        flat["h"], sing, res=True, force_large=path == "large", detect_infeasible=detect, ctx=ctx,
                        **kw)
    out["kernel"] = ctx.last_kernel_name()
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    """The shape's batch and its solves with and without the flag, once per session."""
    path, n, m, k, cones, _ = SHAPES[name]
    flat, kinds, probs, certs = I.make_batch(cones, n, m, k, per_kind=16, seed=sum(map(ord, name)))
    return dict(flat=flat, kinds=kinds, probs=probs, on=solve(name, flat, True), off=solve(name, flat, False))


def split(out, n, m, k, p):
    return (out["x"][p * n:(p + 1) * n], out["y"][p * m:(p + 1) * m], out["z"][p * k:(p + 1) * k],
            out["s"][p * k:(p + 1) * k])


@pytest.mark.parametrize("name", list(SHAPES))
def test_certificates_from_the_outputs(name):
    path, n, m, k, cones, _ = SHAPES[name]
    cs = case(name)
    on, off, kinds = cs["on"], cs["off"], cs["kinds"]
    if name in KERNEL:
        assert on["kernel"] == KERNEL[name] and off["kernel"] != on["kernel"]
    st = np.asarray(on["status"])
    print(name, "status", st.tolist(), "iters", np.asarray(on["iters"]).tolist())
    for p, (kind, prob) in enumerate(zip(kinds, cs["probs"])):
        c, A, b, G, h = prob
        x, y, z, s = split(on, n, m, k, p)
        if kind == I.FEASIBLE:
            # never a verdict, and bitwise the flag-off results: the neighbours do not disturb it
            assert st[p] not in (5, 6), (p, st[p])
            assert st[p] == off["status"][p] and on["iters"][p] == off["iters"][p]
            for key, a_, b_ in zip("xyzs", (x, y, z, s), split(off, n, m, k, p)):
                assert np.array_equal(a_, b_), (p, key)
            assert np.array_equal(on["res"][3 * p:3 * p + 3], off["res"][3 * p:3 * p + 3])
        elif kind == I.PRIMAL_INF:
            assert st[p] == S.PRIMAL_INFEASIBLE, (p, st[p], on["iters"][p])
            assert I.in_cone(cones, z)
            assert abs(b @ y + h @ z + 1.0) <= 1e-9
            assert np.linalg.norm(A.T @ y + G.T @ z) < I.TAU
        else:
            assert st[p] == S.DUAL_INFEASIBLE, (p, st[p], on["iters"][p])
            assert I.in_cone(cones, s)
            assert abs(c @ x + 1.0) <= 1e-9
            assert max(np.linalg.norm(A @ x), np.linalg.norm(G @ x + s)) < I.TAU
        if kind != I.FEASIBLE:
            # res[] holds the exit-test quantities before the scaling: not converged there
            assert 0 < on["iters"][p] < 40 and np.isfinite(on["res"][3 * p:3 * p + 3]).all()
            assert on["res"][3 * p:3 * p + 3].sum() >= 1e-5


@pytest.mark.parametrize("name", list(SHAPES))
def test_flag_off_reports_no_verdict(name):
    cs = case(name)
    st = np.asarray(cs["off"]["status"])
    assert ((st >= 0) & (st <= 4)).all()
    assert ((st[cs["kinds"] != I.FEASIBLE] >= 1)).all(), st.tolist()


@pytest.mark.parametrize("name", [q for q, v in SHAPES.items() if v[5]])
def test_firing_iteration_is_the_oracles(oracle, name):
    """iters equals the restated rule's iteration on the oracle's trace in the
    kernel's operation order, for every problem whose oracle ratio decides the
    iteration by a factor 1.1 on both sides; at least 60 % of the infeasible
    problems must be that clear (the filter reads the oracle alone: 20 of 32
    at (80, 20, 120), the lowest, to 30 of 32 at (8, 2, 16))."""
    O = oracle
    path, n, m, k, cones, order = SHAPES[name]
    flags = (O.F_STRUCTURED | O.F_CHOLSOLVE) if order == "kernel" else O.F_SQR
    cs = case(name)
    on = cs["on"]
    checked = total = 0
    rows = []
    for p, (kind, prob) in enumerate(zip(cs["kinds"], cs["probs"])):
        if kind == I.FEASIBLE:
            continue
        total += 1
        c, A, b, G, h = prob
        r = O.solve_trace(cones, c, A, b, G, h, sing=False, params=O.Params(flags=flags))
        st, it, ratios = I.rule_fire(prob, r)
        clear = st is not None and I.clear_firing(st, it, ratios)
        rows.append((p, int(kind), st, it, int(on["status"][p]), int(on["iters"][p]), clear))
        if not clear:
            continue
        checked += 1
    print(name, "(problem, kind, oracle status, oracle it, status, iters, clear):", rows)
    for p, kind, st, it, gst, git, clear in rows:
        if clear:
            assert (gst, git) == (st, it), (p, kind, st, it, gst, git)
    assert checked >= 0.6 * total, (checked, total)


def test_generator_batch_is_untouched():
    """4,096 feasible C1 generator problems: status, iters, x, y, z, s with the
    flag are bitwise those without it."""
    cfg, B = C1, 4096
    c, A, b, G, h = S.generate(cfg.cones, B, cfg.n, cfg.m, cfg.k, cfg.seed)
    import torch
    sing = torch.zeros(B, dtype=torch.uint8, device=G.device)
    outs = []
    for detect in (False, True):
        o = S.batch_solve(cfg.cones, cfg.n, cfg.m, cfg.k, c, A, b, G, h, sing, detect_infeasible=detect)
        S.default_context().sync()
        outs.append({key: v.cpu().numpy() for key, v in o.items()})
    off, on = outs
    assert (on["status"] <= 4).all()
    for key in ("status", "iters", "x", "y", "z", "s"):
        assert np.array_equal(on[key], off[key]), key


def test_looser_tolerance_fires_no_later():
    name = "small_8_2_16"
    cs = case(name)
    ctx = S.Context()
    try:
        ctx.set_infeasibility_tol(1e-3)
        loose = solve(name, cs["flat"], True, ctx=ctx)
        ctx.set_infeasibility_tol(1e-7)
        again = solve(name, cs["flat"], True, ctx=ctx)
        for bad in (0.0, -1.0, float("nan")):
            with pytest.raises(S.SocpError) as e:
                ctx.set_infeasibility_tol(bad)
            assert e.value.code == _lib.SOCP_E_INVALID
        kept = solve(name, cs["flat"], True, ctx=ctx)  # a refused value leaves the tolerance as it was
    finally:
        ctx.close()
    inf = cs["kinds"] != I.FEASIBLE
    tight = cs["on"]
    assert np.isin(loose["status"][inf], (5, 6)).all()
    assert (loose["iters"][inf] <= tight["iters"][inf]).all()
    assert (loose["iters"][inf] < tight["iters"][inf]).any()
    for key in ("status", "iters", "x", "y", "z", "s"):
        assert np.array_equal(again[key], tight[key]) and np.array_equal(kept[key], tight[key]), key


def test_sqr_tolerance_setter():
    name = "sqr_8_2_16"
    cs = case(name)
    ctx = S.Context()
    try:
        ctx.set_infeasibility_tol(1e-3)
        loose = solve(name, cs["flat"], True, ctx=ctx)
    finally:
        ctx.close()
    inf = cs["kinds"] != I.FEASIBLE
    assert np.isin(loose["status"][inf], (5, 6)).all()
    assert (loose["iters"][inf] <= cs["on"]["iters"][inf]).all()


def test_ingest_matches_batch_solve():
    name = "small_8_2_16"
    path, n, m, k, cones, _ = SHAPES[name]
    cs = case(name)
    flat, ref = cs["flat"], cs["on"]
    B = len(cs["kinds"])
    ing = S.Ingest(cones, n, m, k, B)
    try:
        t = ing.submit(flat["c"], flat["A"], flat["b"], flat["G"], flat["h"], np.zeros(B, np.uint8),
                       detect_infeasible=True)
        dense = ing.wait(t, res=True)
        nz = lambda rows, cols, v: (np.arange(B + 1, dtype=np.int64) * rows * cols,  # noqa: E731
                                    np.tile(np.arange(cols + 1, dtype=np.int64) * rows + 1, B),
                                    np.tile(np.tile(np.arange(rows, dtype=np.int64) + 1, cols), B), v)
        t = ing.submit_csc(flat["c"], flat["b"], flat["h"], np.zeros(B, np.uint8), nz(m, n, flat["A"]),
                           nz(k, n, flat["G"]), detect_infeasible=True)
        csc = ing.wait(t, res=True)
    finally:
        ing.close()
    for got in (dense, csc):
        for key in ("status", "iters", "x", "y", "z", "s", "res"):
            assert np.array_equal(got[key], ref[key]), key


def _model(c, A, b, G, h, cones):
    o = M.Optimizer()
    n = len(c)
    v = o.add_variables(n)
    o.set_objective_function(M.saf([(v[j], c[j]) for j in range(n)], 0.0))
    blocks = [(M.Zeros(len(b)), -A, b)] if len(b) else []
    for kind, offs, dim in cones:
        blocks.append((M.Nonnegatives(dim) if kind == S.CONE_POC else M.SecondOrderCone(dim), -G[offs:offs + dim],
                       h[offs:offs + dim]))
    cis = [o.add_constraint(M.vaf([(i + 1, v[j], F[i, j]) for i in range(F.shape[0]) for j in range(n)], f0), st)
           for st, F, f0 in blocks]
    return o, v, cis


def test_optimize_batched_matches_batch_solve():
    name = "small_8_2_16"
    path, n, m, k, cones, _ = SHAPES[name]
    cs = case(name)
    ref = cs["on"]
    models = [_model(*prob, cones) for prob in cs["probs"]]
    M.optimize_batched([mo[0] for mo in models])
    want = {I.FEASIBLE: ("OPTIMAL", "FEASIBLE_POINT", "FEASIBLE_POINT"),
            I.PRIMAL_INF: ("INFEASIBLE", "NO_SOLUTION", "INFEASIBILITY_CERTIFICATE"),
            I.DUAL_INF: ("DUAL_INFEASIBLE", "INFEASIBILITY_CERTIFICATE", "NO_SOLUTION")}
    for p, ((o, v, cis), kind) in enumerate(zip(models, cs["kinds"])):
        x, y, z, s = split(ref, n, m, k, p)
        assert (o.termination_status(), o.primal_status(), o.dual_status()) == want[int(kind)], p
        assert o.barrier_iterations() == ref["iters"][p]
        assert np.array_equal(o.variable_primal(v), x)
        assert np.array_equal(o.constraint_dual(cis[0]), y)
        assert np.array_equal(np.concatenate([o.constraint_dual(ci) for ci in cis[1:]]), z)
        assert np.array_equal(np.concatenate([o.constraint_primal(ci) for ci in cis[1:]]), s)


def test_explicit_inverse_with_detection_is_unsupported():
    name = "small_8_2_16"
    path, n, m, k, cones, _ = SHAPES[name]
    flat = case(name)["flat"]
    B = flat["c"].size // n
    for force_large in (False, True):
        with pytest.raises(S.SocpError) as e:
            S.batch_solve(cones, n, m, k, flat["c"], flat["A"], flat["b"], flat["G"], flat["h"],
                          np.zeros(B, np.uint8), explicit_inverse=True, detect_infeasible=True,
                          force_large=force_large)
        assert e.value.code == _lib.SOCP_E_UNSUPPORTED
        assert "EXPLICIT_INVERSE" in str(e.value)
    P = _lib.default_params(flags=_lib.F_EXPLICIT_INVERSE | _lib.F_DETECT_INFEASIBLE)
    ing = S.Ingest(cones, n, m, k, B)
    try:
        import ctypes as C
        t = C.c_int64()
        p = _lib.ptr
        rc = _lib.load().socp_ingest_submit(ing.handle, B, p(flat["c"]), p(flat["A"]), p(flat["b"]), p(flat["G"]),
                                            p(flat["h"]), None, P, C.byref(t))
        assert rc == _lib.SOCP_E_UNSUPPORTED
        # the refused submit claimed no slot: the ingest still takes two batches
        t0 = ing.submit(flat["c"], flat["A"], flat["b"], flat["G"], flat["h"], np.zeros(B, np.uint8))
        t1 = ing.submit(flat["c"], flat["A"], flat["b"], flat["G"], flat["h"], np.zeros(B, np.uint8))
        ing.wait(t0)
        ing.wait(t1)
    finally:
        ing.close()
