"""C2 under the reference's stopping rule (solver.jl:105,122: maxit 40,
absolute tol 1e-5): the HIP outcome of the first 4,096 C2 problems against the
oracle's (tests/golden/c2_refrule_outcomes.json, made by
tests/golden/make_outcomes.py), in the operation orders the oracle has.

Near the tolerance the iterates approach the cone boundary and whether a
problem converges, stalls at maxit, loses positive definiteness of H (chol(H))
or hits sqrt of a negative number (domain) is decided by rounding.  The
reference's own operation order (dense iW*iW', scalings.jl:108, and the
explicit Li = H^-1, densesolver.jl:48) loses the most there; the structured
order (X = W^-1 G) with the explicit inverse less; with triangular solves
against the Cholesky factor instead of Li (the register kernel's order for
m <= 16, oracle flags F_STRUCTURED | F_CHOLSOLVE) the least.  Measured on
MI355X (4,096 problems, [converged, maxit, chol(H), chol(S), domain]):
reference order [1517, 805, 138, 0, 1636], structured [3337, 2, 652, 0, 105],
structured + triangular solves [4037, 0, 53, 0, 6], HIP [4073, 0, 15, 0, 8].
Gates follow one rule instead of fitted thresholds: each
statistic must be no worse than its chaos floor -- its worst value when the
oracle is compared with itself under a one-ulp perturbation of G (three seeds,
tests/golden/c2_chaos_floor.json, made by tests/golden/make_chaos_floor.py) --
minus GATE_SLACK (one point) minus one problem's share of the statistic's
denominator (so a single problem never decides a small sample):
  * HIP against the oracle in the same operation order ("self" floor of that
    order): same outcome, of the oracle's converged the share HIP converges on,
    |d iters| <= 1 where both converge, and |d converged| / B, |d failures| / B
    (two-sided: a systematic shift of the histogram fails as much as a loss;
    for the explicit-inverse order one-sided -- DESIGN.md §9);
  * HIP (Cholesky order) against the reference-order oracle ("cross" floor:
    the oracle's own Cholesky-order runs against its reference-order run):
    of the reference's converged HIP converges on, its maxit share, and
    |d iters| <= 1 where both converge; HIP converges on at least as many;
  * every HIP "converged" problem meets the exit test (rd + rp + gap < 1e-5).
"""
import base64
import json
import os

import numpy as np
import pytest

import socp_amd as S
from socp_amd.configs import C2

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def chaos_floor():
    with open(os.path.join(HERE, "golden", "c2_chaos_floor.json")) as f:
        return json.load(f)


def stats(a, b):
    """Outcome agreement of run a (HIP) against run b (oracle): the statistics
    of make_chaos_floor.py, with each one's denominator."""
    sa, sb = a["status"], b["status"]
    ca, cb = sa == S.CONVERGED, sb == S.CONVERGED
    both = ca & cb
    di = np.abs(a["iters"][both] - b["iters"][both])
    fail = lambda st: int(((st >= 2) & (st <= 4)).sum())  # noqa: E731
    B = len(sa)
    return {"same": ((sa == sb).mean(), B), "of_conv": (ca[cb].mean(), int(cb.sum())),
            "maxit": ((sa[cb] == S.MAXIT).mean(), int(cb.sum())), "iters1": ((di <= 1).mean(), int(both.sum())),
            "dconv": (abs(int(ca.sum()) - int(cb.sum())) / B, B), "dfail": (abs(fail(sa) - fail(sb)) / B, B)}


def check_floor(st, floor, slack, keys):
    """Every statistic in `keys` no worse than its floor by more than
    slack + one problem's share of its denominator."""
    bad = []
    for key in keys:
        v, n = st[key]
        allow = slack + 1.0 / max(n, 1)
        if key in ("maxit", "dconv", "dfail"):
            ok = v <= floor[key] + allow
        else:
            ok = v >= floor[key] - allow
        if not ok:
            bad.append(f"{key}={v:.4f} (floor {floor[key]:.4f}, n={n})")
    assert not bad, bad


def _arr(s, dt):
    return np.frombuffer(base64.b64decode(s), dtype=dt)


@pytest.fixture(scope="module")
def outcomes():
    with open(os.path.join(HERE, "golden", "c2_refrule_outcomes.json")) as f:
        fx = json.load(f)
    cfg, B = C2, fx["batch"]
    c, A, b, G, h = S.generate(cfg.cones, B, cfg.n, cfg.m, cfg.k, fx["seed"])
    import torch
    sing = torch.zeros(B, dtype=torch.uint8, device=G.device)
    g = S.batch_solve(cfg.cones, cfg.n, cfg.m, cfg.k, c, A, b, G, h, sing, maxit=fx["maxit"], tol=fx["tol"],
                      res=True)
    torch.cuda.synchronize()
    hip = dict(status=g["status"].cpu().numpy(), iters=g["iters"].cpu().numpy(),
               res=g["res"].cpu().numpy().reshape(B, 3))
    # the reference's operation order on the same batch: Li = H^-1 formed
    # (SOCP_F_EXPLICIT_INVERSE, densesolver.jl:48) -- the oracle's "structured" run
    gx = S.batch_solve(cfg.cones, cfg.n, cfg.m, cfg.k, c, A, b, G, h, sing, maxit=fx["maxit"], tol=fx["tol"],
                       res=True, explicit_inverse=True)
    torch.cuda.synchronize()
    xi = dict(status=gx["status"].cpu().numpy(), iters=gx["iters"].cpu().numpy(),
              res=gx["res"].cpu().numpy().reshape(B, 3))
    runs = {name: dict(status=_arr(r["status"], "<i1").astype(np.int32), iters=_arr(r["iters"], "<i1").astype(np.int32),
                       res=_arr(r["res"], "<f8").reshape(B, 3))
            for name, r in fx["runs"].items()}
    hist = {name: np.bincount(r["status"], minlength=5) for name, r in runs.items()}
    hist["hip"] = np.bincount(hip["status"], minlength=5)
    hist["hip_xi"] = np.bincount(xi["status"], minlength=5)
    print("\nC2 reference rule, 4096 problems [converged, maxit, chol(H), chol(S), domain]:")
    for name, hh in hist.items():
        print(f"  {name:16s} {hh.tolist()}")
    for name, r in runs.items():
        same = (hip["status"] == r["status"]).mean()
        both = (hip["status"] == S.CONVERGED) & (r["status"] == S.CONVERGED)
        di = np.abs(hip["iters"][both] - r["iters"][both])
        rc = r["status"] == S.CONVERGED
        print(f"  vs {name}: same outcome {same:.4f}; of its converged, HIP converged "
              f"{(hip['status'][rc] == S.CONVERGED).mean():.4f} (HIP outcomes {np.bincount(hip['status'][rc], minlength=5).tolist()}); "
              f"both converged {both.sum()}: |d iters| = 0: {(di == 0).mean():.3f}, <= 1: {(di <= 1).mean():.3f}, "
              f"<= 2: {(di <= 2).mean():.3f}, max {di.max() if di.size else 0}")
    r = runs["structured"]
    same = (xi["status"] == r["status"]).mean()
    both = (xi["status"] == S.CONVERGED) & (r["status"] == S.CONVERGED)
    di = np.abs(xi["iters"][both] - r["iters"][both])
    rc = r["status"] == S.CONVERGED
    print(f"  explicit inverse vs structured: same outcome {same:.4f}; of its converged, HIP converged "
          f"{(xi['status'][rc] == S.CONVERGED).mean():.4f}; both converged {both.sum()}: |d iters| = 0: "
          f"{(di == 0).mean():.3f}, <= 1: {(di <= 1).mean():.3f}, <= 2: {(di <= 2).mean():.3f}, "
          f"max {di.max() if di.size else 0}")
    return dict(B=B, hip=hip, xi=xi, runs=runs, hist=hist)


def test_hip_exit_test_holds(outcomes):
    hip = outcomes["hip"]
    conv = hip["status"] == S.CONVERGED
    assert conv.any()
    assert (hip["res"][conv].sum(axis=1) < 1e-5).all()
    assert (hip["iters"][conv] <= 40).all()


SELF_KEYS = ("same", "of_conv", "iters1", "dconv", "dfail")


def test_vs_structured_oracle(outcomes):
    """HIP (default order: H = L L' + triangular solves) against the oracle in
    that order (F_STRUCTURED | F_CHOLSOLVE), at its chaos floor."""
    fl = chaos_floor()
    st = stats(outcomes["hip"], outcomes["runs"]["structured_chol"])
    print({key: round(v, 4) for key, (v, _) in st.items()})
    check_floor(st, fl["self"]["structured_chol"]["floor"], fl["gate_slack"], SELF_KEYS)


def test_vs_reference_order_oracle(outcomes):
    """HIP (Cholesky order) against the reference-order oracle, at the floor of
    the oracle's own Cholesky-order runs against that run (P5: |d iters| <= 1
    on the reference's converged problems)."""
    fl = chaos_floor()
    hip, r = outcomes["hip"], outcomes["runs"]["reference_order"]
    st = stats(hip, r)
    print({key: round(v, 4) for key, (v, _) in st.items()})
    check_floor(st, fl["cross"]["structured_chol_vs_reference_order/all"]["floor"], fl["gate_slack"],
                ("of_conv", "maxit", "iters1"))
    assert (hip["status"] == S.CONVERGED).sum() >= (r["status"] == S.CONVERGED).sum()


def test_explicit_inverse_vs_structured_oracle(outcomes):
    """SOCP_F_EXPLICIT_INVERSE (the reference's Li = H^-1: potrf, then
    triangular solves against I, densesolver.jl:47-48, used at :73,83) under
    the reference rule against the oracle run in the same operation order --
    X = W^-1 G per cone, H = X'X, Li by potrs(I) (the fixture's "structured"
    run, make_outcomes.py) -- at that order's chaos floor."""
    fl = chaos_floor()
    xi = outcomes["xi"]
    st = stats(xi, outcomes["runs"]["structured"])
    print({key: round(v, 4) for key, (v, _) in st.items()})
    # per-problem agreement at the floor; the histogram one-sided: HIP's
    # explicit inverse converges on ~3.7 % more of these problems than the
    # oracle's (a shift beyond the floor, DESIGN.md §9: not the inverse's
    # algorithm -- Y'Y and potrs(I) agree in the oracle -- nor S^-1 or the cx
    # form; nor any single step: test_gpu_onestep.py finds every kernel step from
    # the oracle's iterates at the rounding floor with the oracle's continue /
    # fail decision, DESIGN.md §9a -- a known deviation, a within-floor bias
    # accumulated over the late steps), so it may fail less, never more
    check_floor(st, fl["self"]["structured"]["floor"], fl["gate_slack"], ("same", "of_conv", "iters1"))
    hx, ho = outcomes["hist"]["hip_xi"], outcomes["hist"]["structured"]
    fail = lambda h: int(h[S.CHOL_H_FAILED] + h[S.CHOL_S_FAILED] + h[S.DOMAIN_ERROR])  # noqa: E731
    allow = (fl["self"]["structured"]["floor"]["dfail"] + fl["gate_slack"]) * outcomes["B"] + 1
    assert fail(hx) <= fail(ho) + allow, (hx.tolist(), ho.tolist())
    assert hx[S.CONVERGED] >= ho[S.CONVERGED] - allow, (hx.tolist(), ho.tolist())
    conv = xi["status"] == S.CONVERGED
    assert (xi["res"][conv].sum(axis=1) < 1e-5).all()  # the exit test holds where it says converged
