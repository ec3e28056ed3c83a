"""GPU tests of SOCP_F_EQUILIBRATE (include/socp.h).

The scaling rule is integer arithmetic on exponents and every scaled value is
one ldexp, so the checks are bitwise: socp_batch_equilibrate against the numpy
restatement of tests/equil_cases.py, and a flagged solve against the pipeline
equilibrate -> unflagged solve on the scaled data -> exact unscaling.  (A NaN
matches any NaN: the payload of ldexp(NaN) is the implementation's.)  The
rescue test runs the batch that tests/test_equil_cpu.py pins on the CPU oracle.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import equil_cases as Q
import socp_amd as S
from socp_amd import _lib

pytestmark = pytest.mark.gpu

KEYS = ("x", "y", "z", "s", "res", "iters", "status")
same_bits = Q.same_bits


def ctx():
    return S.default_context()


def equilibrate(d, device=False, what="PcAbGh"):
    """S.equilibrate on a Batch; device=True: torch tensors, results back as numpy."""
    cones, n, m, k = d.shape
    t = (lambda v: None if v is None else torch.from_numpy(np.ascontiguousarray(v)).cuda()) if device else (lambda v: v)
    pick = lambda q, v: t(v) if q in what else None  # noqa: E731
    out = S.equilibrate(list(cones), n, m, k, t(d.A) if m else None, t(d.G), P=pick("P", d.P), c=pick("c", d.c),
                        b=pick("b", d.b) if m else None, h=pick("h", d.h), shared_matrices=d.MB == 1)
    if device:
        ctx().sync()
        out = {key: v.cpu().numpy() for key, v in out.items()}
    return out


def check_against_restatement(d, got, sc):
    cones, n, m, k = d.shape
    want = dict(D=sc.D, E=sc.E, F=sc.F, Ps=sc.P, cs=sc.c, As=sc.A if m else None, bs=sc.b if m else None, Gs=sc.G,
                hs=sc.h)
    for key, w in want.items():
        if w is None:
            assert key not in got or got[key].size == 0, key
            continue
        assert same_bits(np.asarray(got[key]).reshape(-1), w), key


ALL = ([("bad", n, p) for n in ("m0", "s16", "two", "blk") for p in (False, True)]
       + [("dec", n, p) for n in ("m0", "s16", "two", "blk") for p in (False, True)]
       + [("ones", "s16", False), ("tall", "tall", False), ("spread20", "s16", False)])


@functools.lru_cache(maxsize=None)
def case(kind, name, with_P):
    if kind == "bad":
        return Q.bad_batch(name, Q.B, 2, 12, with_P)
    if kind == "dec":
        return Q.decorated_batch(name, with_P)
    return dict(ones=Q.ones_batch, tall=Q.tall_batch, spread20=Q.spread20_batch)[kind]()


@functools.lru_cache(maxsize=None)
def restated(kind, name, with_P):
    return Q.restate(case(kind, name, with_P))


# ------------------------------------------------------- 1. the scaling rule
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("kind,name,with_P", ALL, ids=[f"{a}-{b}{'-P' if c else ''}" for a, b, c in ALL])
def test_equilibrate_matches_the_restatement(kind, name, with_P, device):
    """D, E, F and the six scaled arrays, bitwise, on every case; with device
    pointers the caller's tensors are not written."""
    d = case(kind, name, with_P)
    got = equilibrate(d, device)
    check_against_restatement(d, got, restated(kind, name, with_P))
    if kind == "ones":
        assert (got["D"] == 1).all() and (got["E"] == 1).all() and (got["F"] == 1).all()


@pytest.mark.parametrize("name,with_P", [("s16", False), ("two", True), ("blk", False)])
def test_equilibrate_shared_against_replicated(name, with_P):
    """SOCP_F_SHARED_MATRICES: one factor set, the bits of every problem's set
    of the replicated call; cs, bs, hs index it for every problem."""
    d = Q.shared_batch(name, Q.B, 5, 12, with_P)
    cones, n, m, k = d.shape
    sh = equilibrate(d)
    check_against_restatement(d, sh, Q.restate(d))
    rep = Q.Batch(d.shape, d.B, d.B, None if d.P is None else np.tile(d.P, d.B), d.c, np.tile(d.A, d.B), d.b,
                  np.tile(d.G, d.B), d.h)
    rp = equilibrate(rep)
    for key in ("D", "E", "F", "As", "Gs") + (("Ps",) if with_P else ()):
        assert same_bits(np.tile(sh[key], d.B), rp[key]), key
    for key in ("cs", "bs", "hs"):
        assert same_bits(sh[key], rp[key]), key


def test_equilibrate_optional_arguments():
    """Outputs follow the inputs given: matrices only, and m = 0 without A."""
    d = case("bad", "s16", True)
    got = equilibrate(d, what="")
    assert sorted(got) == ["As", "D", "E", "F", "Gs"]
    sc = restated("bad", "s16", True)  # P takes part in the column norms, so without it the factors differ
    noP = Q.restate(Q.Batch(d.shape, d.B, d.MB, None, d.c, d.A, d.b, d.G, d.h))
    assert same_bits(got["D"], noP.D) and same_bits(got["Gs"], noP.G) and not same_bits(got["D"], sc.D)
    d0 = case("bad", "m0", False)
    got = equilibrate(d0, what="h")
    assert sorted(got) == ["D", "E", "F", "Gs", "hs"] and got["E"].size == 0
    assert same_bits(got["hs"], restated("bad", "m0", False).h)


def test_passes():
    """The setter rejects 0 and 65 and keeps its value; 1 pass differs from 8
    on the 2^+-20 data, and both match the restatement."""
    d = case("spread20", "s16", False)
    c = ctx()
    try:
        for bad in (0, 65, -3):
            with pytest.raises(S.SocpError) as e:
                c.set_equilibration_passes(bad)
            assert e.value.code == _lib.SOCP_E_INVALID
        eight = equilibrate(d)  # the rejected values left the default in place
        check_against_restatement(d, eight, Q.restate(d, 8))
        c.set_equilibration_passes(1)
        one = equilibrate(d)
        check_against_restatement(d, one, Q.restate(d, 1))
        assert not same_bits(one["F"], eight["F"])
        c.set_equilibration_passes(64)
        check_against_restatement(d, equilibrate(d), Q.restate(d, 64))
    finally:
        c.set_equilibration_passes(8)


# ------------------------------------------------- 2. the pipeline identity
def solve(d, equil, sing, arrays=None, **kw):
    cones, n, m, k = d.shape
    P, c, A, b, G, h = arrays if arrays is not None else (d.P, d.c, d.A, d.b, d.G, d.h)
    out = S.batch_solve(list(cones), n, m, k, c, A if m else None, b if m else None, G, h, sing, res=True, P=P,
                        equilibrate=equil, shared_matrices=d.MB == 1, **kw)
    return out, ctx().last_kernel_name()


def pipeline(d, sing, **kw):
    """equilibrate -> the unflagged solve on the scaled data -> unscaling in numpy."""
    cones, n, m, k = d.shape
    e = equilibrate(d)
    out, name = solve(d, False, sing, (e.get("Ps"), e["cs"], e.get("As"), e.get("bs"), e["Gs"], e["hs"]), **kw)
    ed, ee, ef = (np.frexp(e[q])[1].astype(np.int64).reshape(d.MB, w) - 1  # 2^e = 0.5 * 2^(e+1)
                  for q, w in zip("DEF", (n, m, k)))
    sc = Q.Scaled(ed, ee, ef, *([None] * 9))
    out["x"], y, out["z"], out["s"] = Q.unscale(d, sc, out["x"], out["y"][:d.B * m], out["z"], out["s"])
    out["y"] = y if m else out["y"]
    return out, name


def check_identity(d, sing=None, **kw):
    want, wname = pipeline(d, sing, **kw)
    got, gname = solve(d, True, sing, **kw)
    assert gname == wname, (gname, wname)
    for key in KEYS:
        assert same_bits(got[key], want[key]), (key, kw)
    return got, gname


PIPE = [("s16", False, {}), ("two", False, {}), ("blk", False, {}), ("s16", False, dict(force_large=True)),
        ("s16", False, dict(explicit_inverse=True)), ("two", True, {}), ("blk", True, {})]


@pytest.mark.parametrize("name,with_P,kw", PIPE,
                         ids=["s16", "two", "blk", "s16-large", "s16-xi", "two-P", "blk-P"])
def test_flagged_solve_is_the_pipeline(name, with_P, kw):
    """Every output and the kernel name, bitwise, under the reference rule
    (batch 33) and at a fixed iteration count (batch 1); sing probed on the
    scaled G, and given."""
    d = case("bad", name, with_P)
    _, kn = check_identity(d, None, **kw)
    large = name == "blk" or kw.get("force_large")
    assert kn.startswith("socp_large") == bool(large), kn
    d1 = Q.bad_batch(name, 1, 7, 12, with_P)
    check_identity(d1, np.zeros(1, np.uint8), maxit=3, tol=0.0, **kw)


@pytest.mark.parametrize("name,with_P,kw", [("s16", False, {}), ("two", True, {}), ("blk", False, {})],
                         ids=["s16", "two-P", "blk"])
def test_flagged_shared_against_replicated(name, with_P, kw):
    """SOCP_F_SHARED_MATRICES passes through: the pipeline identity holds, and
    the outputs are the bits of the replicated flagged call."""
    d = Q.shared_batch(name, Q.B, 5, 12, with_P)
    sh, kn = check_identity(d, None, maxit=4, tol=0.0, **kw)
    rep = Q.Batch(d.shape, d.B, d.B, None if d.P is None else np.tile(d.P, d.B), d.c, np.tile(d.A, d.B), d.b,
                  np.tile(d.G, d.B), d.h)
    rp, kr = solve(rep, True, None, maxit=4, tol=0.0, **kw)
    assert kn == kr
    for key in KEYS:
        assert same_bits(sh[key], rp[key]), key


def test_all_ones_factors_change_nothing():
    d = case("ones", "s16", False)
    sing = np.zeros(d.B, np.uint8)
    plain, kp = solve(d, False, sing)
    flagged, kf = solve(d, True, sing)
    assert kp == kf
    assert (plain["status"] == 0).all(), plain["status"]
    for key in KEYS:
        assert same_bits(flagged[key], plain[key]), key


@pytest.mark.parametrize("name,with_P", [("s16", True), ("blk", False)])
def test_device_inputs_are_not_written(name, with_P):
    """Device tensors in place: the flagged solve leaves every input bitwise as
    it was and returns the bits of the host-pointer call."""
    d = case("bad", name, with_P)
    cones, n, m, k = d.shape
    t = lambda v: None if v is None else torch.from_numpy(np.ascontiguousarray(v)).cuda()  # noqa: E731
    ins = dict(P=t(d.P), c=t(d.c), A=t(d.A), b=t(d.b), G=t(d.G), h=t(d.h))
    keep = {key: None if v is None else v.clone() for key, v in ins.items()}
    dev = S.batch_solve(list(cones), n, m, k, ins["c"], ins["A"], ins["b"], ins["G"], ins["h"], None, res=True,
                        P=ins["P"], equilibrate=True)
    ctx().sync()
    for key, v in ins.items():
        if v is not None:
            assert torch.equal(v.view(torch.int64), keep[key].view(torch.int64)), key
    host, _ = solve(d, True, None)
    for key in KEYS:
        assert same_bits(dev[key].cpu().numpy().reshape(-1)[:host[key].size], host[key]), key


# ----------------------------------------------------------------- 3. rescue
def term_scales(prob, x, y, z, s):
    """The magnitudes the three exit quantities are summed from (tests/test_gpu_qp.py)."""
    c, A, b, G, h = prob
    ab = np.abs
    return (np.linalg.norm(ab(c) + ab(A).T @ ab(y) + ab(G).T @ ab(z)), np.linalg.norm(ab(A) @ ab(x) + ab(b)),
            ab(z) @ ab(s))


def test_rescue_of_the_cpu_pinned_batch():
    """(16,4,24), generator seed 2, 32 problems, spread 2^+-12 -- the batch of
    tests/test_equil_cpu.py.  With the flag every status is 0 and res sums
    below tol; res equals the three exit quantities formed in numpy from the
    returned iterate mapped back to the scaled data, on the two scales of
    DESIGN.md section 18 (1e-13 of the magnitude of the terms each is summed
    from; 1e-9 of the quantity itself where it is at least N 2^-53 / 1e-9 of
    that magnitude).  Without the flag at least 8 of 32 stay unconverged: half
    the CPU floor of 16 (kernel and oracle outcomes differ by a few percent,
    DESIGN.md section 9); that bound only shows the test is not vacuous."""
    d = Q.bad_batch("s16", 32, 2, 12)
    cones, n, m, k = d.shape
    tol = 1e-5
    got, kn = solve(d, True, None)
    raw, _ = solve(d, False, None)
    nbad = int((raw["status"] != 0).sum())
    print(f"as given: {nbad} of 32 not converged; with the flag: statuses {sorted(set(got['status'].tolist()))}, "
          f"iterations {got['iters'].min()}..{got['iters'].max()} on {kn}")
    assert (got["status"] == S.CONVERGED).all(), got["status"]
    res = got["res"].reshape(d.B, 3)
    assert (res.sum(axis=1) < tol).all(), res.sum(axis=1).max()
    sc = Q.restate(d)
    thr = (n + m + k + 2) * 2.0 ** -53 / 1e-9
    worst = 0.0
    for p in range(d.B):
        A = sc.A[p * m * n:(p + 1) * m * n].reshape(n, m).T
        G = sc.G[p * k * n:(p + 1) * k * n].reshape(n, k).T
        c, b, h = sc.c[p * n:(p + 1) * n], sc.b[p * m:(p + 1) * m], sc.h[p * k:(p + 1) * k]
        x = np.ldexp(got["x"][p * n:(p + 1) * n], -sc.ed[p])
        y = np.ldexp(got["y"][p * m:(p + 1) * m], -sc.ee[p])
        z = np.ldexp(got["z"][p * k:(p + 1) * k], -sc.ef[p])
        s = np.ldexp(got["s"][p * k:(p + 1) * k], sc.ef[p])
        terms = (np.linalg.norm(c + A.T @ y + G.T @ z), np.linalg.norm(A @ x - b), float(z @ s))
        for q, scale in enumerate(term_scales((c, A, b, G, h), x, y, z, s)):
            err = abs(res[p, q] - terms[q])
            assert err <= 1e-13 * scale, (p, q, res[p, q], terms[q], scale)
            worst = max(worst, err / scale)
            if terms[q] > 0.0 and terms[q] >= thr * scale:
                assert err <= 1e-9 * terms[q], (p, q, res[p, q], terms[q])
        # z's is invariant under the scaling
        zs = float(got["z"][p * k:(p + 1) * k] @ got["s"][p * k:(p + 1) * k])
        assert abs(zs - res[p, 2]) <= 1e-13 * term_scales((c, A, b, G, h), x, y, z, s)[2], p
    print(f"res vs numpy on the scaled data: worst {worst:.2e} of the terms' magnitude")
    assert nbad >= 8, nbad


# -------------------------------------------------------------- 4. refusals
def test_refusals():
    """SOCP_E_UNSUPPORTED with warm start and with detection; from ingest and
    from the rank-update IPM, which ignored the bit before."""
    d = Q.bad_batch("s16", 4, 2, 12)
    cones, n, m, k = d.shape
    z = np.zeros
    with pytest.raises(S.SocpError) as e:
        solve(d, True, None, warm=(z(4 * n), z(4 * m), np.ones(4 * k), np.ones(4 * k)))
    assert e.value.code == _lib.SOCP_E_UNSUPPORTED and "WARM_START" in str(e.value)
    with pytest.raises(S.SocpError) as e:
        solve(d, True, None, detect_infeasible=True)
    assert e.value.code == _lib.SOCP_E_UNSUPPORTED and "DETECT_INFEASIBLE" in str(e.value)

    L, p = _lib.load(), _lib.ptr
    pr = _lib.default_params(flags=_lib.F_EQUILIBRATE)
    out = dict(x=z(4 * n), y=z(4 * m), z=z(4 * k), s=z(4 * k), iters=z(4, np.int32), status=z(4, np.int32))
    outp = [p(out[q]) for q in ("x", "y", "z", "s", "iters", "status")]
    hq = S.SqrHandle(list(cones), n, m, k, d.A, d.G, z(4, np.uint8))
    try:
        rc = L.socp_sqr_solve_socp(hq.handle, p(d.c), p(d.b), p(d.h), pr, *outp, None)
        assert rc == _lib.SOCP_E_UNSUPPORTED, rc
        assert "EQUILIBRATE" in L.socp_last_error().decode()
    finally:
        hq.close()
    ing = S.Ingest(list(cones), n, m, k, 4)
    try:
        ticket = C.c_int64()
        rc = L.socp_ingest_submit(ing.handle, 4, p(d.c), p(d.A), p(d.b), p(d.G), p(d.h), None, pr, C.byref(ticket))
        assert rc == _lib.SOCP_E_UNSUPPORTED, rc
        # the refused submit claimed no slot: two plain submits still fit
        t1 = ing.submit(d.c, d.A, d.b, d.G, d.h)
        t2 = ing.submit(d.c, d.A, d.b, d.G, d.h)
        ing.wait(t1)
        ing.wait(t2)
    finally:
        ing.close()


def test_python_layers_route_the_flag():
    """solve_socp_batched(equilibrate=True) returns what
    batch_solve(equilibrate=True) returns."""
    d = Q.bad_batch("s16", 4, 2, 12)
    cones, n, m, k = d.shape
    want, _ = solve(d, True, None)
    probs = []
    for p in range(d.B):
        _, A, G = Q.mats(d, p)
        probs.append(S.Problem(d.c[p * n:(p + 1) * n], A, d.b[p * m:(p + 1) * m], G, d.h[p * k:(p + 1) * k],
                               [S.POC(o, dm) if kd == Q.P_ else S.SOC(o, dm) for kd, o, dm in cones]))
    states, iters, status = S.solve_socp_batched(probs, equilibrate=True)
    assert same_bits(np.asarray(iters), want["iters"]) and same_bits(np.asarray(status), want["status"])
    assert same_bits(np.concatenate([st.x for st in states]), want["x"])
    # the MOI option: the models of one group, solved with the flag and without detection
    from socp_amd import moi as M
    from test_moi import model_from_dense
    models = [model_from_dense(pr.c, pr.A, pr.b, pr.G, pr.h, cones, equilibrate=True) for pr in probs]
    M.optimize_batched([mo[0] for mo in models])
    for p, (o, v, _) in enumerate(models):
        assert o.barrier_iterations() == want["iters"][p]
        assert same_bits(o.variable_primal(v), want["x"][p * n:(p + 1) * n]), p
