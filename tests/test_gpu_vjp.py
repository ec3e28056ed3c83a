"""Differentiable solves on the device: socp_batch_vjp, socp_batch_centre and
the torch layer, against vjp_cases.py's references.  test_vjp_cpu.py holds the
preconditions (the formulas against finite differences, the centring table).

  definition  every qp_kkt_cases case, with P and without: the kernel that the
              fused KKT entry selects; ux, uy, uz within qp_kkt_cases' gate for
              the right-hand side (gx - G'gs, gy, gz, 0) -- max(10 e_rs,
              (n + m + 2k) 2^-53), e_rs the numpy restatement's error against
              the refined block system, no kernel measurement in it; the six
              gradients within the rounding of their own formulas on the
              device's ux, uy, uz: |err| <= 3 * 2^-53 (|a_i b_j| + |c_i d_j|)
              per entry of a two-term outer product, one rounding for dh,
              equality for dc and db;
  masks       outputs not asked for leave canaries untouched; skip[1] = 7
              zeroes problem 1 and reports 7; a z outside the cone gives that
              problem a nonzero status and zeros, the other's bits unchanged;
  centring    batch_centre(4) from qp_reference(tol = 1e-5)'s iterates against
              centre_reference per problem; steps = 0; res; shared matrices;
  end to end  batch_solve, batch_centre(4), batch_vjp against true_gradient
              within ten times the CPU pipeline's own error, and not without
              the centring;
  layer       SocpLayer's .grad equals batch_vjp bit for bit, a MAXIT problem
              contributes zero, on a non-default stream.

The centring's per-problem gates hold on the problems that have a reference:
qp_reference converged and centre_reference took its four steps.  That is all 8
on s8, m0, s16, c1; on blk some random problems end in status 2 or 4 late in the
solve (qp_cases.py says so), and their last iterate has no centre to compare
with.  At least half of every batch must have one.
"""
import functools

import numpy as np
import pytest

import kkt_cases as KC
import oracle as O
import qp_cases as QC
import qp_kkt_cases as QK
import socp_amd as S
import vjp_cases as V

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble
VEC = ("dc", "db", "dh", "ux", "uy", "uz")


def bits(a, b):
    u, v = np.asarray(a), np.asarray(b)
    return u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes()


# ------------------------------------------------------------ the definition
@functools.lru_cache(maxsize=None)
def point(case):
    """Seeded standard-normal x, y, gx, gy, gz, gs of a case's batch (gy = 0 when sing)."""
    rng = np.random.default_rng([case.n, case.m, case.k, 5])
    v = {key: rng.standard_normal((QK.B, q)) for key, q in
         (("x", case.n), ("y", case.m), ("gx", case.n), ("gy", case.m), ("gz", case.k), ("gs", case.k))}
    if case.sing:
        v["gy"][:] = 0.0
    return v


def run_vjp(case, with_P, **kw):
    d, v = QK.inputs(case), point(case)
    Af, Gf = KC.flat(d)
    f = lambda key: v[key].ravel() if v[key].size else None  # noqa: E731
    z = kw.pop("z", d["z"])
    return S.batch_vjp(list(case.cones), case.n, case.m, case.k, Af, Gf, QK.sing_bytes(case), f("x"), f("y"),
                       z.ravel(), d["s"].ravel(), f("gx"), f("gy"), f("gz"), f("gs"),
                       P=QK.flat_P(d) if with_P else None, force_large=case.force_large, **kw)


@functools.lru_cache(maxsize=None)
def vjp_once(case, with_P):
    out = run_vjp(case, with_P)
    name = S.default_context().last_kernel_name()
    return out, name


@functools.lru_cache(maxsize=None)
def u_gate(case, with_P, p):
    """(refined (ux, uy, uz, .), the gate per vector) for problem p's right-hand side."""
    d, v = QK.inputs(case), point(case)
    Pm = d["P"][p] if with_P else np.zeros((case.n, case.n))
    G = d["G"][p]
    rx = (v["gx"][p].astype(LD) - G.T.astype(LD) @ v["gs"][p].astype(LD)).astype(np.float64)
    rhs = [(rx, v["gy"][p], v["gz"][p], np.zeros(case.k))]
    ref = QK.reference_of(case.cones, Pm, d["A"][p], G, d["s"][p], d["z"][p], rhs)
    rs = QK.restatement_of(case.cones, Pm, d["A"][p], G, case.sing, d["s"][p], d["z"][p], rhs)
    e_rs = KC.rel_errors(rs[0], ref.sol[0])
    return ref.sol[0], KC.gates(case.n, case.m, case.k, e_rs)


def outer_bound(got, a, b, c, d, scale=1.0):
    """got against -(a b' + c d') * scale: the worst |err| / (3 * 2^-53 (|a_i b_j| + |c_i d_j|) scale)."""
    al, bl, cl, dl = [np.asarray(v, LD) for v in (a, b, c, d)]
    exact = -(np.outer(al, bl) + np.outer(cl, dl)) * scale
    bound = 3.0 * U * (np.abs(np.outer(al, bl)) + np.abs(np.outer(cl, dl))) * scale
    err = np.abs(got.astype(LD) - exact)
    assert (err[bound == 0] == 0).all()
    return float(np.max(err[bound > 0] / bound[bound > 0])) if (bound > 0).any() else 0.0


@pytest.mark.parametrize("with_P", [True, False], ids=["P", "noP"])
@pytest.mark.parametrize("case", QK.CASES, ids=QK.case_id)
def test_definition(case, with_P):
    n, m, k = case.n, case.m, case.k
    out, name = vjp_once(case, with_P)
    assert name == (case.kernel if with_P else QK.linear_kernel_name(case)), name
    assert (out["status"] == 0).all(), out["status"]
    d, v = QK.inputs(case), point(case)
    rows = V.unflatten(out, QK.B, n, m, k)
    for p, r in enumerate(rows):
        ref, gates = u_gate(case, with_P, p)
        for key, e, g in zip(("ux", "uy", "uz"), KC.rel_errors([r["ux"], r["uy"], r["uz"]], ref[:3]), gates[:3]):
            if e is None:
                continue
            print(f"{case.id} {'P' if with_P else 'noP'} p={p} {key}: e = {e:.3g}, gate {g:.3g}")
            assert e <= g, (case.id, p, key, e, g)
        x, y, z, gs = v["x"][p], v["y"][p], d["z"][p], v["gs"][p]
        w = r["uz"] + gs
        assert np.array_equal(r["dc"], -r["ux"]) and np.array_equal(r["db"], r["uy"])
        assert (np.abs(r["dh"].astype(LD) - (r["uz"].astype(LD) + gs)) <= U * np.abs(w)).all()
        worst = dict(dP=outer_bound(r["dP"], r["ux"], x, x, r["ux"], 0.5),
                     dG=outer_bound(r["dG"], z, r["ux"], r["dh"], x))
        if m:
            worst["dA"] = outer_bound(r["dA"], y, r["ux"], r["uy"], x)
        print(f"{case.id} p={p} outer products, worst |err| / bound:", worst)
        assert max(worst.values()) <= 1.0, worst


def test_outputs_not_asked_for_are_not_written():
    """dc and dh alone, into slices of a canary-filled device buffer: the rest of
    the buffer is untouched and the two are the full call's bits."""
    import torch
    case = QK.BY_ID["c1"]
    n, m, k = case.n, case.m, case.k
    d, v = QK.inputs(case), point(case)
    Af, Gf = KC.flat(d)
    dev = lambda a, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dt)  # noqa: E731
    big = torch.full((4096,), 777.0, dtype=torch.float64, device="cuda")
    mine = dict(dc=big[100:100 + QK.B * n], dh=big[1000:1000 + QK.B * k])
    out = S.batch_vjp(list(case.cones), n, m, k, dev(Af), dev(Gf), dev(QK.sing_bytes(case), torch.uint8),
                      dev(v["x"].ravel()), dev(v["y"].ravel()), dev(d["z"].ravel()), dev(d["s"].ravel()),
                      dev(v["gx"].ravel()), dev(v["gy"].ravel()), dev(v["gz"].ravel()), dev(v["gs"].ravel()),
                      P=dev(QK.flat_P(d)), want=["dc", "dh"], out=mine)
    assert set(out) == {"dc", "dh", "status"}
    got = big.cpu().numpy()
    full, _ = vjp_once(case, True)
    assert bits(got[100:100 + QK.B * n], full["dc"]) and bits(got[1000:1000 + QK.B * k], full["dh"])
    keep = np.ones(4096, bool)
    keep[100:100 + QK.B * n] = keep[1000:1000 + QK.B * k] = False
    assert (got[keep] == 777.0).all()
    assert (out["status"].cpu().numpy() == 0).all()


@pytest.mark.parametrize("case", [QK.BY_ID["c1"], QK.BY_ID["edge65"]], ids=QK.case_id)
def test_masked_problems_are_zero(case):
    full, _ = vjp_once(case, True)
    cnt = lambda key: full[key].size // QK.B  # noqa: E731
    # skip[1] = 7
    out = run_vjp(case, True, skip=np.array([0, 7], np.int32))
    assert out["status"].tolist() == [0, 7]
    # a z outside its cone on problem 1
    z = QK.inputs(case)["z"].copy()
    kind, o, dim = case.cones[-1]
    z[1, o] = -1.0
    bad = run_vjp(case, True, z=z)
    assert bad["status"][0] == 0 and bad["status"][1] != 0, bad["status"]
    for res in (out, bad):
        for key in V.GRADS + ("ux", "uy", "uz"):
            if not full[key].size:
                continue
            assert bits(res[key][:cnt(key)], full[key][:cnt(key)]), key
            assert (res[key][cnt(key):] == 0.0).all(), key


# ---------------------------------------------------------------- centring
CENTRE_CASES = [("s8", False), ("m0", False), ("s16", False), ("c1", False), ("c1", True), ("blk", False),
                ("sing", False)]
NB = 8


@functools.lru_cache(maxsize=None)
def centre_inputs(name):
    """qp_reference(tol = 1e-5)'s final iterates of qp_cases.batch(name, 8), the
    reference centring from them, and which problems have a reference."""
    d = QC.batch(name, NB)
    cones = d.shape.cones
    start, pts, valid = [], [], []
    for prob in d.probs:
        r = QC.qp_reference(cones, prob, bool(d.shape.sing), tol=1e-5)
        st = (r["x"], r["y"], r["z"], r["s"])
        q = V.centre_reference(cones, prob, *st) if r["status"] == 0 else [st]
        start.append(st)
        pts.append(q)
        valid.append(r["status"] == 0 and len(q) == V.STEPS + 1)
    return d, start, pts, valid


def run_centre(name, force_large, steps, shared=None, **kw):
    d, start, _, _ = centre_inputs(name)
    cones, n, m, k, _ = d.shape
    x, y, z, s = V.flat_point(start)
    return S.batch_centre(list(cones), n, m, k, d.c, d.A if m else None, d.b if m else None, d.G, d.h, d.sing, x,
                          y if m else None, z, s, steps=steps, P=d.P, force_large=force_large, res=True, **kw)


@functools.lru_cache(maxsize=None)
def centred(name, force_large):
    return run_centre(name, force_large, V.STEPS)


def sum_of_terms(prob, x, y, z, s):
    """The sum of the norms of the terms of the three residuals."""
    Pm, c, A, b, G, h = prob
    nrm = np.linalg.norm
    t = nrm(Pm @ x) + nrm(c) + nrm(G.T @ z) + nrm(G @ x) + nrm(s) + nrm(h)
    if len(b):
        t += nrm(A.T @ y) + nrm(A @ x) + nrm(b)
    return float(t)


@pytest.mark.parametrize("name,force_large", CENTRE_CASES, ids=[n + ("_large" if f else "") for n, f in CENTRE_CASES])
def test_centre_against_reference(name, force_large):
    d, start, pts, valid = centre_inputs(name)
    cones, n, m, k, _ = d.shape
    assert sum(valid) >= NB // 2, valid
    if name in V.TABLE_SHAPES:
        assert all(valid)
    out = centred(name, force_large)
    kname = S.default_context().last_kernel_name()
    assert ("large" in kname) == (force_large or name == "blk"), kname
    for p in range(NB):
        if not valid[p]:
            print(f"{name} p={p}: no reference (status {out['status'][p]})")
            continue
        got = (out["x"][p * n:(p + 1) * n], out["y"][p * m:(p + 1) * m], out["z"][p * k:(p + 1) * k],
               out["s"][p * k:(p + 1) * k])
        ref = pts[p][-1]
        assert out["status"][p] == 0
        off, off_ref = V.off_centre(cones, got[3], got[2]), V.off_centre(cones, ref[3], ref[2])
        r3 = lambda q: sum(float(np.linalg.norm(v)) for v in V.residuals(d.probs[p], *q))  # noqa: E731
        res, res_ref = r3(got), r3(ref)
        floor = (n + m + 2 * k) * U * sum_of_terms(d.probs[p], *got)
        gap0, gap = float(start[p][2] @ start[p][3]), float(got[2] @ got[3])
        print(f"{name} p={p}: off-centre {off:.2e} (ref {off_ref:.2e}), residuals {res:.2e} (ref {res_ref:.2e}, "
              f"floor {floor:.2e}), z's {gap0:.3e} -> {gap:.3e}")
        assert off <= max(10.0 * off_ref, 1e-6)
        assert res <= max(10.0 * res_ref, floor)
        assert gap0 / 2.0 <= gap <= 2.0 * gap0
        # res[] is the returned point's.  z's cancels: its rounding is k 2^-53 of the sum of |s_i z_i| in either
        # order of summation, about 1e-9 of z's itself near a solution -- the size of the measure after four
        # steps.  So the measure is recomputed from compute_scaling's lam at the entry's own z's (res[2]).
        rr = out["res"][4 * p:4 * p + 4]
        assert abs(rr[2] - gap) <= 2 * k * U * float(np.abs(got[2] * got[3]).sum())
        off_at = V.off_centre(cones, got[3], got[2], gap=rr[2])
        print(f"{name} p={p}: res[3] {rr[3]:.6e}, recomputed {off_at:.6e}")
        assert abs(rr[3] - off_at) <= 1e-6 * off_at + 1e-12


def test_centre_zero_steps_returns_the_inputs():
    d, start, _, _ = centre_inputs("s16")
    out = run_centre("s16", False, 0)
    for key, v in zip("xyzs", V.flat_point(start)):
        assert bits(out[key], v), key
    assert (out["status"] == 0).all()
    cones, n, m, k, _ = d.shape
    for p in range(NB):
        off = V.off_centre(cones, start[p][3], start[p][2], gap=out["res"][4 * p + 2])
        assert abs(out["res"][4 * p + 3] - off) <= 1e-6 * off + 1e-12


@pytest.mark.parametrize("force_large", [False, True], ids=["small", "large"])
def test_centre_shared_matrices_are_the_replicated_call(force_large):
    sh = QC.shared_batch("c1", NB)
    cones, n, m, k, _ = sh.shape
    rng = np.random.default_rng(11)
    from shared_cases import interior
    x, y = rng.standard_normal(NB * n), rng.standard_normal(NB * m)
    z, s = interior(rng, cones, NB, k).ravel(), interior(rng, cones, NB, k).ravel()
    kw = dict(steps=3, force_large=force_large, res=True)
    one = S.batch_centre(list(cones), n, m, k, sh.c, sh.A, sh.b, sh.G, sh.h, np.zeros(1, np.uint8), x, y, z, s,
                         P=sh.P, shared_matrices=True, **kw)
    rep = S.batch_centre(list(cones), n, m, k, sh.c, np.tile(sh.A, NB), sh.b, np.tile(sh.G, NB), sh.h,
                         np.zeros(NB, np.uint8), x, y, z, s, P=np.tile(sh.P, NB), **kw)
    for key in ("x", "y", "z", "s", "status", "res"):
        assert bits(one[key], rep[key]), key
    assert not bits(one["x"], x)


# -------------------------------------------------------------- end to end
@functools.lru_cache(maxsize=None)
def solved(name):
    d = QC.batch(name, NB)
    cones, n, m, k, _ = d.shape
    out = S.batch_solve(list(cones), n, m, k, d.c, d.A if m else None, d.b if m else None, d.G, d.h, d.sing, P=d.P,
                        tol=1e-5)
    assert (out["status"] == 0).all(), out["status"]
    return out


def pipeline_errors(name, centre_steps):
    d = QC.batch(name, NB)
    cones, n, m, k, _ = d.shape
    o = solved(name)
    g = [v.ravel() if v.size else None for v in V.upstream(name, NB, bool(d.shape.sing))]
    r = S.batch_vjp(list(cones), n, m, k, d.A if m else None, d.G, d.sing, o["x"], o["y"] if m else None, o["z"],
                    o["s"], *g, P=d.P, centre_steps=centre_steps, c=d.c, b=d.b if m else None, h=d.h,
                    want=list(V.GRADS))
    assert (r["status"] == 0).all(), r["status"]
    rows = V.unflatten(r, NB, n, m, k)
    return [V.grad_error(rows[p], V.table(name)[p]["true"]) for p in range(NB)]


@pytest.mark.parametrize("name", V.TABLE_SHAPES)
def test_end_to_end_gradient(name):
    """GPU solve, four centring steps and the adjoint against the derivative of
    the exact solution: within ten times the CPU pipeline's own error after its
    four steps (below 1e-3 by test_vjp_cpu.py's cap).  Without the centring the
    same call misses that gate on at least one problem of the shape."""
    cpu = [r["err"][V.STEPS] for r in V.table(name)]
    got = pipeline_errors(name, V.STEPS)
    raw = pipeline_errors(name, 0)
    for p in range(NB):
        print(f"{name} p={p}: gradient error {got[p]:.2e} (CPU pipeline {cpu[p]:.2e}; uncentred {raw[p]:.2e})")
    assert all(e <= 10.0 * c for e, c in zip(got, cpu)), (got, cpu)
    assert any(e > 10.0 * c for e, c in zip(raw, cpu))


# ------------------------------------------------------------ the torch layer
def _layer_case(name, shared):
    import torch
    t = lambda a, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dt)  # noqa: E731
    if shared:
        d = QC.shared_batch(name, NB)
        sing = None
    else:
        d = QC.batch(name, NB)
        sing = t(d.sing, torch.uint8)
    return d, {key: t(getattr(d, key)) for key in ("c", "A", "b", "G", "h", "P")}, sing


@pytest.mark.parametrize("name,shared", [("s16", False), ("c1", True)], ids=["s16", "c1_shared"])
def test_layer_gradients_are_batch_vjp(name, shared):
    import torch
    from socp_amd.torch_layer import SocpLayer
    d, ten, sing = _layer_case(name, shared)
    cones, n, m, k, _ = d.shape
    diff = ("c", "b", "h") if shared else ("c", "A", "b", "G", "h", "P")
    rng = np.random.default_rng(3)
    with torch.cuda.stream(torch.cuda.Stream()):
        w = torch.from_numpy(rng.standard_normal(NB * n)).cuda()
        v = torch.from_numpy(rng.standard_normal(NB * k)).cuda()
        for key in diff:
            ten[key].requires_grad_(True)
        layer = SocpLayer(list(cones), n, m, k, shared_matrices=shared, tol=1e-5)
        x, y, z, s, status, iters = layer(ten["c"], ten["A"], ten["b"], ten["G"], ten["h"], ten["P"], sing)
        loss = (w * x).sum() + (v * z).sum()
        loss.backward()
        assert not status.requires_grad and not iters.requires_grad
        with torch.no_grad():
            ref = S.batch_vjp(list(cones), n, m, k, ten["A"].detach(), ten["G"].detach(), sing, x.detach(),
                              y.detach(), z.detach(), s.detach(), w, None, v, None, P=ten["P"].detach(),
                              skip=status, want=["d" + key for key in diff], shared_matrices=shared)
        assert (status.cpu().numpy() == 0).all()
        for key in diff:
            g = ten[key].grad
            assert g is not None and g.shape == ten[key].shape
            assert bits(g.cpu().numpy(), ref["d" + key].cpu().numpy()), key
            assert float(g.abs().max()) > 0.0
        for key in set(ten) - set(diff):
            assert ten[key].grad is None
        # the point the layer returns is batch_solve's, centred by batch_centre(4)
        with torch.no_grad():
            data = [ten[key].detach() for key in ("c", "A", "b", "G", "h")]
            o = S.batch_solve(list(cones), n, m, k, *data, sing, P=ten["P"].detach(), shared_matrices=shared,
                              tol=1e-5)
            assert not bits(o["x"].cpu().numpy(), x.detach().cpu().numpy())
            S.batch_centre(list(cones), n, m, k, *data, sing, o["x"], o["y"], o["z"], o["s"], steps=4,
                           P=ten["P"].detach(), shared_matrices=shared)
        for key, got in zip("xyzs", (x, y, z, s)):
            assert bits(o[key].cpu().numpy(), got.detach().cpu().numpy()), key


def test_layer_maxit_problem_contributes_zero():
    import torch
    from socp_amd.torch_layer import SocpLayer
    d, ten, sing = _layer_case("s16", False)
    cones, n, m, k, _ = d.shape
    with torch.cuda.stream(torch.cuda.Stream()):
        for key in ten:
            ten[key].requires_grad_(True)
        layer = SocpLayer(list(cones), n, m, k, maxit=1, tol=1e-5)
        x, y, z, s, status, iters = layer(ten["c"], ten["A"], ten["b"], ten["G"], ten["h"], ten["P"], sing)
        (x.sum() + y.sum() + z.sum() + s.sum()).backward()
        assert (status.cpu().numpy() == S.MAXIT).all()
        for key in ten:
            g = ten[key].grad.cpu().numpy()
            assert (g == 0.0).all() and np.isfinite(g).all(), key
