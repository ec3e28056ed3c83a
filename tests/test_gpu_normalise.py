"""GPU tests of SOCP_F_NORMALISE (include/socp.h).

The rule is integer arithmetic on exponents and every scaled value is one
ldexp, so the checks are bitwise: socp_batch_normalise against the numpy
restatement of tests/normalise_cases.py, and a flagged solve against the
pipeline normalise -> unflagged solve on the scaled data -> exact unscaling.
(A NaN matches any NaN: the payload of ldexp(NaN) is the implementation's.)
The rescue test runs the batches that tests/test_normalise_cpu.py pins on the
CPU references.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import equil_cases as E
import normalise_cases as N
import qp_cases as Q
import socp_amd as S
from socp_amd import _lib

pytestmark = pytest.mark.gpu

KEYS = ("x", "y", "z", "s", "res", "iters", "status")
same_bits = E.same_bits


def ctx():
    return S.default_context()


def t(v):
    return None if v is None else torch.from_numpy(np.ascontiguousarray(v)).cuda()


def back(out, dev):
    if dev:
        ctx().sync()
        out = {key: v.cpu().numpy() for key, v in out.items()}
    return out


# ------------------------------------------------------- 1. the scaling rule
def normalise(d, dev=False, P=None, shared=False):
    conv = t if dev else (lambda v: v)
    ins = [conv(d.c), conv(d.b) if d.m else None, conv(d.h), conv(P)]
    keep = [None if v is None or not dev else v.clone() for v in ins]
    out = S.normalise(d.n, d.m, d.k, ins[0], ins[1], ins[2], P=ins[3], shared_matrices=shared)
    out = back(out, dev)
    if dev:  # the caller's tensors are not written
        for v, v0 in zip(ins, keep):
            assert v is None or torch.equal(v.view(torch.int64), v0.view(torch.int64))
    return out


def check_rule(d, got, P=None, shared=False):
    sc = N.restate(d.n, d.m, d.k, d.c, d.b, d.h, P, shared)
    assert got["expo"].dtype == np.int32 and same_bits(got["expo"], sc.expo.reshape(-1))
    assert same_bits(got["cs"], sc.c) and same_bits(got["hs"], sc.h)
    if d.m:
        assert same_bits(got["bs"], sc.b)
    else:
        assert "bs" not in got
    if P is None:
        assert "Ps" not in got
    else:
        assert same_bits(got["Ps"], sc.P)
    return sc


RULE = [(name, B) for name in ("s8", "m0", "c1") for B in (1, 5, 67)] + [("long", 4)]


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name,B", RULE, ids=[f"{a}-{b}" for a, b in RULE])
def test_normalise_matches_the_restatement(name, B, dev):
    """expo and the four scaled arrays, bitwise: per-problem exponents that all
    differ, the maximum in the last element and negative, and from B = 5 on
    the problems with c = 0, a NaN in h, an Inf in c and a subnormal-only c;
    B = 1, 5, 67 leave the last workgroup ragged, and k = 1200 makes the
    strided loops longer than a wavefront."""
    d = N.rule_batch(name, B)
    sc = check_rule(d, normalise(d, dev, P=d.P), P=d.P)
    if B >= 5:
        assert sc.expo[1, 0] == 0 and sc.expo[2, 1] == 0 and sc.expo[3, 0] == 0 and sc.expo[4, 0] == N.CLAMP
    check_rule(d, normalise(d, dev))  # without P


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("B", [4, 67])
def test_normalise_shared_P_takes_one_pair(B, dev):
    """SOCP_F_SHARED_MATRICES with a P: one pair for the batch in all 2B
    entries, and ONE scaled matrix; a NaN or an Inf anywhere in the batch
    freezes its exponent; without P the pairs stay per problem."""
    d = N.rule_batch("c1", B)
    P1 = d.P[:d.n * d.n]
    sc = check_rule(d, normalise(d, dev, P=P1, shared=True), P=P1, shared=True)
    assert (sc.expo == sc.expo[0]).all()
    assert sc.P.size == d.n * d.n
    if B >= 5:  # frozen by problem 2's NaN and problem 3's Inf; then the same batch with the two made finite
        assert tuple(sc.expo[0]) == (0, 0)
        c, h = d.c.copy(), d.h.copy()
        c[3 * d.n] = 1.0
        h[2 * d.k + d.k // 2] = 0.0
        d = N.Rule(d.n, d.m, d.k, B, c, d.b, h, d.P)
        sc = check_rule(d, normalise(d, dev, P=P1, shared=True), P=P1, shared=True)
        assert sc.expo[0, 0] != 0 and sc.expo[0, 1] != 0
    check_rule(d, normalise(d, dev, shared=True), shared=True)


# ------------------------------------------------- 2. the pipeline identity
def solve(d, arrays=None, dev=False, shared=False, warm=None, sing="zeros", **kw):
    """batch_solve on a qp_cases Batch or Shared (or on `arrays` in its place); numpy back."""
    cones, n, m, k = d.shape[:4]
    P, c, A, b, G, h = arrays if arrays is not None else (d.P, d.c, d.A, d.b, d.G, d.h)
    conv = t if dev else (lambda v: v)
    sg = np.zeros(1 if shared else d.B, np.uint8) if isinstance(sing, str) else sing
    out = S.batch_solve(list(cones), n, m, k, conv(c), conv(A) if m else None, conv(b) if m else None, conv(G), conv(h),
                        conv(sg), res=True, P=conv(P), shared_matrices=shared,
                        warm=None if warm is None else tuple(conv(v) for v in warm), **kw)
    out = back(out, dev)
    out["y"] = out["y"][:d.B * m]
    return out, ctx().last_kernel_name()


def pipeline(d, dev=False, shared=False, warm=None, **kw):
    """normalise -> the unflagged solve on the scaled data (a warm start's
    iterate scaled forward) -> unscaling in numpy."""
    cones, n, m, k = d.shape[:4]
    nz = S.normalise(n, m, k, d.c, d.b if m else None, d.h, P=d.P, shared_matrices=shared)
    expo = nz["expo"].reshape(d.B, 2)
    if warm is not None:
        warm = N.scale_iterate(expo, n, m, k, *warm)
    out, name = solve(d, (nz.get("Ps"), nz["cs"], d.A, nz.get("bs", d.b), d.G, nz["hs"]), dev, shared, warm, **kw)
    out["x"], out["y"], out["z"], out["s"] = N.scale_iterate(expo, n, m, k, out["x"], out["y"], out["z"], out["s"], -1)
    return out, name, expo


def check_identity(d, dev=False, shared=False, warm=None, **kw):
    want, wname, expo = pipeline(d, dev, shared, warm, **kw)
    got, gname = solve(d, None, dev, shared, warm, normalise=True, **kw)
    assert gname == wname, (gname, wname)
    for key in KEYS:
        assert same_bits(got[key], want[key]), (key, kw)
    return got, gname, expo


def varied(name, qp, nb=N.NB):
    """The batch with every problem in units of its own: c times 2^(4p - 32), (b, h) times 2^(30 - 4p)."""
    p = np.arange(nb)
    return N.scaled_by(N.batch(name, qp, 0, 0, nb), 4 * p - 32, 30 - 4 * p)


# (id, shape, qp, batch_solve options, kernel family)
PIPE = [("c1", "c1", False, {}, "small"), ("c2", "c2", False, {}, "small"), ("blk", "blk", False, {}, "large"),
        ("c1-large", "c1", False, dict(force_large=True), "large"), ("c1-qp", "c1", True, {}, "small")]


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("case", PIPE, ids=[c[0] for c in PIPE])
def test_flagged_solve_is_the_pipeline(case, dev):
    """Every output and the kernel name, bitwise, under the reference rule and
    at a fixed iteration count: the register kernel at c1 and c2, the blocked
    kernel at blk and through SOCP_F_FORCE_LARGE, the QP kernel at c1."""
    _, name, qp, kw, family = case
    d = varied(name, qp, 8 if name == "blk" else N.NB)
    _, kn, expo = check_identity(d, dev, **kw)
    assert family in kn and ("qp" in kn) == qp, kn
    assert len({tuple(e) for e in expo.tolist()}) == d.B  # every problem its own pair
    check_identity(d, dev, maxit=3, tol=0.0, **kw)


def shared_c1(with_P):
    d = Q.shared_batch("c1", N.NB)
    p = np.arange(N.NB)
    row = lambda v, w, e: np.ldexp(v.reshape(N.NB, w), e[:, None]).reshape(-1)  # noqa: E731
    n, m, k = d.shape[1:4]
    return Q.Shared(d.shape, d.B, d.P if with_P else None, row(d.c, n, p + 3), d.A, row(d.b, m, 9 - p), d.G,
                    row(d.h, k, 9 - p))


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("with_P", [False, True], ids=["linear", "qp"])
def test_flagged_shared_matrices(with_P, dev):
    """SOCP_F_SHARED_MATRICES passes through: without P the pairs are per
    problem, with the one P the batch has one pair; in both the pipeline
    identity holds and the outputs are the bits of the replicated flagged
    call given the same exponents."""
    d = shared_c1(with_P)
    got, kn, expo = check_identity(d, dev, shared=True)
    assert ("qp" in kn) == with_P
    assert (len({tuple(e) for e in expo.tolist()}) == 1) == with_P
    if not with_P:  # per-problem pairs either way: the replicated call's bits
        rep = Q.Shared(d.shape, d.B, None, d.c, np.tile(d.A, d.B), d.b, np.tile(d.G, d.B), d.h)
        rp, kr = solve(rep, None, dev, normalise=True)
        assert kr == kn
        for key in KEYS:
            assert same_bits(got[key], rp[key]), key


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("qp", [False, True], ids=["linear", "qp"])
def test_flagged_warm_start(qp, dev):
    """SOCP_F_WARM_START from the K = 3 iterate of the caller's problem: the
    incoming iterate is scaled forward, and the outputs are the pipeline's."""
    d = varied("c1", qp)
    k3, _ = solve(d, None, False, maxit=3, tol=0.0, normalise=True)
    warm = tuple(k3[q] for q in "xyzs")
    got, _, _ = check_identity(d, dev, warm=warm)
    assert (got["status"] == 0).all(), got["status"]


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("with_P", [False, True], ids=["linear", "qp"])
def test_flag_together_with_equilibration(with_P, dev):
    """SOCP_F_EQUILIBRATE | SOCP_F_NORMALISE: equilibrate, normalise, solve,
    un-normalise, unscale -- every step exact, so the flagged call returns that
    pipeline's bits (sing probed on the scaled G in both)."""
    d0 = E.bad_batch("s16", 8, 2, 12, with_P)
    d = E.Batch(d0.shape, d0.B, d0.MB, d0.P, np.ldexp(d0.c, 12), d0.A, np.ldexp(d0.b, -7), d0.G, np.ldexp(d0.h, -7))
    cones, n, m, k = d.shape
    conv = t if dev else (lambda v: v)

    def run(P, c, A, b, G, h, **kw):
        out = S.batch_solve(list(cones), n, m, k, conv(c), conv(A), conv(b), conv(G), conv(h), None, res=True,
                            P=conv(P), **kw)
        return back(out, dev), ctx().last_kernel_name()

    for kw in (dict(), dict(maxit=3, tol=0.0)):
        e = S.equilibrate(list(cones), n, m, k, d.A, d.G, P=d.P, c=d.c, b=d.b, h=d.h)
        nz = S.normalise(n, m, k, e["cs"], e["bs"], e["hs"], P=e.get("Ps"))
        expo = nz["expo"].reshape(d.B, 2)
        assert (expo != 0).any()
        want, wname = run(nz.get("Ps"), nz["cs"], e["As"], nz["bs"], e["Gs"], nz["hs"], **kw)
        xyzs = N.scale_iterate(expo, n, m, k, want["x"], want["y"][:d.B * m], want["z"], want["s"], -1)
        ed, ee, ef = (np.frexp(e[q])[1].astype(np.int64).reshape(d.MB, w) - 1 for q, w in zip("DEF", (n, m, k)))
        want["x"], want["y"], want["z"], want["s"] = E.unscale(d, E.Scaled(ed, ee, ef, *([None] * 9)), *xyzs)
        got, gname = run(d.P, d.c, d.A, d.b, d.G, d.h, equilibrate=True, normalise=True, **kw)
        assert gname == wname
        for key in KEYS:
            assert same_bits(got[key].reshape(-1)[:want[key].size], want[key]), (key, kw)


def test_device_inputs_are_not_written():
    """Device tensors in place: the flagged solve leaves every input bitwise as
    it was -- the scaled copies live in the context."""
    d = varied("c1", True)
    cones, n, m, k = d.shape[:4]
    ins = dict(P=t(d.P), c=t(d.c), A=t(d.A), b=t(d.b), G=t(d.G), h=t(d.h))
    keep = {key: v.clone() for key, v in ins.items()}
    S.batch_solve(list(cones), n, m, k, ins["c"], ins["A"], ins["b"], ins["G"], ins["h"], None, res=True, P=ins["P"],
                  normalise=True)
    ctx().sync()
    for key, v in ins.items():
        assert torch.equal(v.view(torch.int64), keep[key].view(torch.int64)), key


# ------------------------------------------------------------- 3. the rescue
def term_scales(prob, x, y, z, s):
    """The magnitudes the three exit quantities are summed from (tests/test_gpu_qp.py)."""
    Pm, c, A, b, G, h = prob
    ab = np.abs
    return (np.linalg.norm(ab(Pm) @ ab(x) + ab(c) + ab(A).T @ ab(y) + ab(G).T @ ab(z)),
            np.linalg.norm(ab(A) @ ab(x) + ab(b)), ab(z) @ ab(s))


def with_zero_P(prob):
    return (np.zeros((len(prob[1]),) * 2) if prob[0] is None else prob[0],) + tuple(prob[1:])


@pytest.mark.parametrize("qp", [False, True], ids=["linear", "qp"])
def test_rescue_of_the_cpu_pinned_batch(qp):
    """c1 with c and (b, h) multiplied by 2^10 (and its QP twin) -- the batches
    of tests/test_normalise_cpu.py, on which the references converge on none
    as given and on all 16 normalised.  With the flag every status is 0; the
    exit test in the caller's units, 2^ec |rd| + 2^eb |rp| + 2^(ec+eb) z's <
    tol, holds when formed in numpy from the outputs and the caller's data;
    res equals the three exit quantities of the normalised problem at the
    normalised iterate, on the two scales of tests/test_gpu_qp.py (1e-13 of the
    magnitude of the terms each is summed from; 1e-9 of the quantity itself
    where it is at least N 2^-53 / 1e-9 of that magnitude); iters equals the
    normalised reference's on its clear problems.  Without the flag at most
    half converge (the references: none): that bound only shows the test is
    not vacuous."""
    d = N.batch("c1", qp, 10, 10)
    cones, n, m, k = d.shape[:4]
    tol = N.TOL
    got, kn = solve(d, normalise=True)
    raw, _ = solve(d)
    nconv = int((raw["status"] == 0).sum())
    print(f"as given: {nconv} of {d.B} converged; with the flag: statuses {sorted(set(got['status'].tolist()))}, "
          f"iterations {got['iters'].min()}..{got['iters'].max()} on {kn}")
    assert (got["status"] == S.CONVERGED).all(), got["status"]
    res = got["res"].reshape(d.B, 3)
    assert (res.sum(axis=1) < tol).all(), res.sum(axis=1).max()
    dn, expo = N.normalised(d)
    assert (expo != 0).all()
    xs, ys, zs, ss = N.scale_iterate(expo, n, m, k, got["x"], got["y"], got["z"], got["s"])
    refs = N.reference("c1", qp, 10, 10, True)
    thr = (n + m + k + 2) * 2.0 ** -53 / 1e-9
    rows = lambda v, w, p: v[p * w:(p + 1) * w]  # noqa: E731
    worst, nclear = 0.0, 0
    for p in range(d.B):
        ec, eb = int(expo[p, 0]), int(expo[p, 1])
        # the caller's units
        it = (rows(got["x"], n, p), rows(got["y"], m, p), rows(got["z"], k, p), rows(got["s"], k, p))
        rd, rp, gap = Q.exit_terms(with_zero_P(d.probs[p]), *it)
        total = np.ldexp(rd, ec) + np.ldexp(rp, eb) + np.ldexp(gap, ec + eb)
        print(f"problem {p}: caller's units |rd| {rd:.3e} |rp| {rp:.3e} z's {gap:.3e}; relative sum {total:.3e}")
        assert total < tol, (p, total)
        # the normalised units: what res holds
        prob = with_zero_P(dn.probs[p])
        itn = (rows(xs, n, p), rows(ys, m, p), rows(zs, k, p), rows(ss, k, p))
        terms = Q.exit_terms(prob, *itn)
        for q, scale in enumerate(term_scales(prob, *itn)):
            err = abs(res[p, q] - terms[q])
            assert err <= 1e-13 * scale, (p, q, res[p, q], terms[q], scale)
            worst = max(worst, err / scale)
            if terms[q] > 0.0 and terms[q] >= thr * scale:
                assert err <= 1e-9 * terms[q], (p, q, res[p, q], terms[q])
        if Q.clear(refs[p]):
            nclear += 1
            assert got["iters"][p] == refs[p]["iters"], (p, got["iters"][p], refs[p]["iters"])
    print(f"res vs numpy on the normalised data: worst {worst:.2e} of the terms' magnitude; {nclear} clear problems")
    assert nclear >= 3 * d.B // 4
    assert nconv <= d.B // 2, nconv


# ---------------------------------------------------- 4. scale invariance
@pytest.mark.parametrize("qp", [False, True], ids=["linear", "qp"])
def test_scale_invariance_on_the_device(qp):
    """The batch with problem p's c multiplied by 2^a_p and its (b, h) by 2^b_p
    (P by 2^(a_p - b_p)) returns, with the flag, the unscaled batch's x and s
    times 2^b_p and y and z times 2^a_p exactly, and the bits of its iters,
    status and res."""
    base = N.batch("c1", qp)
    rng = np.random.default_rng(4)
    a, b = rng.integers(-40, 41, base.B), rng.integers(-40, 41, base.B)
    want, kw = solve(base, normalise=True)
    got, kg = solve(N.scaled_by(base, a, b), normalise=True)
    assert kw == kg and (want["status"] == 0).all()
    cones, n, m, k = base.shape[:4]
    moved = N.scale_iterate(np.stack([a, b], axis=1), n, m, k, want["x"], want["y"], want["z"], want["s"])
    for key, v in zip("xyzs", moved):
        assert same_bits(got[key], v), key
    for key in ("iters", "status", "res"):
        assert same_bits(got[key], want[key]), key


# ------------------------------------------------------------------ 5. no-op
@pytest.mark.parametrize("qp", [False, True], ids=["linear", "qp"])
def test_zero_exponents_change_nothing(qp):
    """Data whose norms lie in [1, 2) already: the flag-off call's bits."""
    d, _ = N.normalised(N.batch("c1", qp))
    cones, n, m, k = d.shape[:4]
    assert (N.restate(n, m, k, d.c, d.b, d.h, d.P).expo == 0).all()
    for dev in (False, True):
        plain, kp = solve(d, None, dev)
        flagged, kf = solve(d, None, dev, normalise=True)
        assert kp == kf and (plain["status"] == 0).all()
        for key in KEYS:
            assert same_bits(flagged[key], plain[key]), (key, dev)


# -------------------------------------------------------------- 6. refusals
def test_refusals():
    """SOCP_E_UNSUPPORTED with detection, naming both flags; from ingest and
    from the rank-update IPM for the bit; and the same calls without the bit
    still run."""
    d = N.batch("s8", False, 10, 10, 4)
    cones, n, m, k = d.shape[:4]
    with pytest.raises(S.SocpError) as e:
        solve(d, normalise=True, detect_infeasible=True)
    assert e.value.code == _lib.SOCP_E_UNSUPPORTED
    assert "SOCP_F_NORMALISE" in str(e.value) and "SOCP_F_DETECT_INFEASIBLE" in str(e.value)
    out, _ = solve(d, detect_infeasible=True)  # the neighbour: detection alone still runs
    assert out["status"].shape == (4,)

    L, p, z = _lib.load(), _lib.ptr, np.zeros
    out = dict(x=z(4 * n), y=z(4 * m), z=z(4 * k), s=z(4 * k), iters=z(4, np.int32), status=z(4, np.int32))
    outp = [p(out[q]) for q in ("x", "y", "z", "s", "iters", "status")]
    hq = S.SqrHandle(list(cones), n, m, k, d.A, d.G, z(4, np.uint8))
    try:
        rc = L.socp_sqr_solve_socp(hq.handle, p(d.c), p(d.b), p(d.h), _lib.default_params(flags=_lib.F_NORMALISE),
                                   *outp, None)
        assert rc == _lib.SOCP_E_UNSUPPORTED, rc
        assert "NORMALISE" in L.socp_last_error().decode()
        assert L.socp_sqr_solve_socp(hq.handle, p(d.c), p(d.b), p(d.h), _lib.default_params(), *outp, None) == 0
    finally:
        hq.close()
    ing = S.Ingest(list(cones), n, m, k, 4)
    try:
        ticket = C.c_int64()
        rc = L.socp_ingest_submit(ing.handle, 4, p(d.c), p(d.A), p(d.b), p(d.G), p(d.h), None,
                                  _lib.default_params(flags=_lib.F_NORMALISE), C.byref(ticket))
        assert rc == _lib.SOCP_E_UNSUPPORTED, rc
        assert "NORMALISE" in L.socp_last_error().decode()
        # the refused submit claimed no slot: two plain submits still fit
        t1 = ing.submit(d.c, d.A, d.b, d.G, d.h)
        t2 = ing.submit(d.c, d.A, d.b, d.G, d.h)
        ing.wait(t1)
        ing.wait(t2)
    finally:
        ing.close()


# --------------------------------------------------------- 7. Python layers
def test_python_layers_route_the_flag():
    """solve_socp_batched(normalise=True), Optimizer(normalise=True) through
    optimize_batched and SocpLayer(normalise=True)'s forward return what
    batch_solve(normalise=True) returns; the layer's backward runs and is
    finite."""
    d = N.batch("s8", False, 10, 10, 4)
    cones, n, m, k = d.shape[:4]
    want, _ = solve(d, normalise=True)
    assert (want["status"] == 0).all()
    probs = [S.Problem(pr[1], pr[2], pr[3], pr[4], pr[5], [S.SOC(o, dm) for _, o, dm in cones]) for pr in d.probs]
    states, iters, status = S.solve_socp_batched(probs, normalise=True)
    assert same_bits(np.asarray(iters), want["iters"]) and same_bits(np.asarray(status), want["status"])
    for key in "xyzs":
        assert same_bits(np.concatenate([getattr(st, key) for st in states]), want[key]), key
    with pytest.raises(ValueError, match="normalise"):
        S.solve_socp_batched(probs, solver="sqr", normalise=True)

    from socp_amd import moi as M
    from test_moi import model_from_dense
    models = [model_from_dense(pr.c, pr.A, pr.b, pr.G, pr.h, cones, normalise=True) for pr in probs]
    plain = model_from_dense(probs[0].c, probs[0].A, probs[0].b, probs[0].G, probs[0].h, cones)
    M.optimize_batched([mo[0] for mo in models] + [plain[0]])  # the plain model groups apart
    for p, (o, v, _) in enumerate(models):
        assert o.barrier_iterations() == want["iters"][p]
        assert same_bits(o.variable_primal(v), want["x"][p * n:(p + 1) * n]), p

    from socp_amd.torch_layer import SocpLayer
    ins = [t(d.c).requires_grad_(), t(d.A), t(d.b).requires_grad_(), t(d.G), t(d.h).requires_grad_()]
    sing = t(np.zeros(d.B, np.uint8))
    x, y, z, s, st, it = SocpLayer(list(cones), n, m, k, centre_steps=0, normalise=True)(*ins, sing=sing)
    ctx().sync()
    for key, v in zip(KEYS, (x, y, z, s, None, it, st)):
        if v is not None:
            assert same_bits(v.detach().cpu().numpy(), want[key]), key
    x, y, z, s, st, it = SocpLayer(list(cones), n, m, k, normalise=True)(*ins, sing=sing)
    (x.sum() + z.sum()).backward()
    ctx().sync()
    for v in (ins[0], ins[2], ins[4]):
        assert v.grad is not None and torch.isfinite(v.grad).all()
