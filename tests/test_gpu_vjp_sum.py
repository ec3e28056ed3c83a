"""socp_batch_vjp_sum on the device: the gradients of a shared-matrix batch's one
P, A and G against vjp_sum_cases.sum_reference within its derived gate
(test_vjp_sum_cpu.py shows the gate has teeth), the per-problem outputs against
socp_batch_vjp's bits, determinism, masking, and the torch layer.

Shapes (qp_cases.SHAPES): s8 (every tile partial; the batch sizes around the
four problems of one matrix instruction and around the slab boundaries of
socp_debug_vjp_sum_plan), m0 (dA skipped), c1 (m is half a tile), blk (the
blocked kernel; n and k no multiples of 16, above 64), gv (75 row tiles of dG).
"""
import functools

import numpy as np
import pytest

import qp_cases as QC
import socp_amd as S
import vjp_sum_cases as VS

pytestmark = pytest.mark.gpu

ALL = VS.VEC + VS.SUMS
_, SLAB = S.vjp_sum_plan(1, 8, 2, 16)
B_EDGE = SLAB + 1          # ends one problem past a slab boundary
B_THREE = 2 * SLAB + 77    # three slabs, the last one ragged (and no multiple of 4)


def bits(a, b):
    u, v = np.asarray(a), np.asarray(b)
    return u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes()


def flat(v):
    return np.ascontiguousarray(v).reshape(-1) if v.size else None


def call(name, B, with_P=True, *, force_large=False, want=ALL, skip=None, z=None, device=False, out=None):
    pt = VS.points(name, B)
    sh = pt.sh
    cones, n, m, k, _ = sh.shape
    ins = dict(A=sh.A if m else None, G=sh.G, x=flat(pt.x), y=flat(pt.y), z=flat(pt.z if z is None else z),
               s=flat(pt.s), gx=flat(pt.gx), gy=flat(pt.gy), gz=flat(pt.gz), gs=flat(pt.gs),
               P=sh.P if with_P else None, skip=skip)
    if device:
        import torch
        ins = {key: None if v is None else torch.from_numpy(np.ascontiguousarray(v)).cuda()
               for key, v in ins.items()}
    r = S.batch_vjp(list(cones), n, m, k, ins["A"], ins["G"], None, ins["x"], ins["y"], ins["z"], ins["s"],
                    ins["gx"], ins["gy"], ins["gz"], ins["gs"], P=ins["P"], skip=ins["skip"], want=list(want),
                    out=out, force_large=force_large, shared_matrices=True)
    if device:
        r = {key: v.cpu().numpy() for key, v in r.items()}
    return r


@functools.lru_cache(maxsize=None)
def once(name, B, with_P=True, force_large=False):
    r = call(name, B, with_P, force_large=force_large)
    return r, S.default_context().last_kernel_name()


def ratios(name, B, r, z=None):
    """worst |err| / gate per sum, against the reference on r's own ux, uy, uz, status."""
    pt = VS.points(name, B)
    _, n, m, k, _ = pt.sh.shape
    rows = lambda key, q: r[key].reshape(B, q) if q else np.zeros((B, 0))  # noqa: E731
    ref = VS.sum_reference(pt.x, pt.y, pt.z if z is None else z, pt.gs, rows("ux", n), rows("uy", m), rows("uz", k),
                           r["status"])
    B_on = int((r["status"] == 0).sum())
    assert set(ref) == ({"dG", "dP"} | ({"dA"} if m else set()))
    return {key: VS.worst(r[key], *ref[key], B_on) for key in ref}


CASES = ([("s8", B, P, False) for B in (1, 3, 4, 5, B_EDGE, B_THREE) for P in (True, False)]
         + [(name, 8, P, False) for name in ("m0", "c1", "blk", "gv") for P in (True, False)]
         + [("c1", 8, True, True)])


@pytest.mark.parametrize("name,B,with_P,force_large", CASES,
                         ids=[f"{n}-B{B}-{'P' if P else 'noP'}{'-large' if f else ''}" for n, B, P, f in CASES])
def test_sums_against_reference(name, B, with_P, force_large):
    r, kname = once(name, B, with_P, force_large)
    _, n, m, k, _ = VS.points(name, B).sh.shape
    assert ("large" in kname) == (force_large or name in ("blk", "gv")), kname
    assert (r["status"] == 0).all(), r["status"]
    assert r["dG"].shape == (k * n,) and r["dP"].shape == (n * n,) and r["dA"].shape == (m * n,)
    worst = ratios(name, B, r)
    print(f"{name} B={B} {'P' if with_P else 'noP'}: worst |err| / gate {worst}, "
          f"plan {S.vjp_sum_plan(B, n, m, k)}")
    assert max(worst.values()) <= 1.0, worst
    assert all(np.abs(r[key]).max() > 0 for key in worst)
    dP = r["dP"].reshape(n, n)
    assert bits(dP, np.ascontiguousarray(dP.T))
    # the per-problem outputs are socp_batch_vjp's
    vec = call(name, B, with_P, force_large=force_large, want=VS.VEC)
    assert set(vec) == set(VS.VEC) | {"status"}
    for key in VS.VEC + ("status",):
        assert bits(r[key], vec[key]), key


def test_default_want_is_unchanged():
    pt = VS.points("s8", 4)
    cones, n, m, k, _ = pt.sh.shape
    r = S.batch_vjp(list(cones), n, m, k, pt.sh.A, pt.sh.G, None, flat(pt.x), flat(pt.y), flat(pt.z), flat(pt.s),
                    flat(pt.gx), P=pt.sh.P, shared_matrices=True)
    assert set(r) == set(VS.VEC) | {"status"}


@pytest.mark.parametrize("name,B", [("c1", 8), ("s8", B_THREE)])
def test_same_bits_again_on_the_device_and_alone(name, B):
    first, _ = once(name, B)
    again = call(name, B)
    dev = call(name, B, device=True)
    only = call(name, B, want=["dG"])
    assert set(only) == {"dG", "status"}
    for key in VS.SUMS:
        assert bits(first[key], again[key]) and bits(first[key], dev[key]), key
    assert bits(first["dG"], only["dG"])
    # each sum alone, and without the per-problem outputs
    for key in ("dP", "dA"):
        assert bits(first[key], call(name, B, want=[key], device=True)[key]), key


@pytest.mark.parametrize("name", ["c1", "blk"])
def test_masked_problems_contribute_nothing(name):
    B = 8
    pt = VS.points(name, B)
    cones = pt.sh.shape.cones
    full, _ = once(name, B)
    # skip[1] = 7
    skip = np.zeros(B, np.int32)
    skip[1] = 7
    r = call(name, B, skip=skip)
    assert r["status"].tolist() == [0, 7] + [0] * (B - 2)
    worst = ratios(name, B, r)
    print(name, "skip[1] = 7:", worst)
    assert max(worst.values()) <= 1.0, worst
    assert not bits(r["dG"], full["dG"])
    # a z outside its last cone on problem 1: the KKT solve fails there
    z = pt.z.copy()
    _, o, _ = cones[-1]
    z[1, o] = -1.0
    bad = call(name, B, z=z)
    assert bad["status"][1] != 0 and (np.delete(bad["status"], 1) == 0).all(), bad["status"]
    worst = ratios(name, B, bad, z=z)
    print(name, "z[1] outside the cone:", worst)
    assert max(worst.values()) <= 1.0, worst
    # the two masks leave the same problems: the same bits
    for key in VS.SUMS:
        assert np.isfinite(bad[key]).all() and bits(bad[key], r[key]), key
    # all skipped
    none = call(name, B, skip=np.full(B, 7, np.int32))
    assert (none["status"] == 7).all()
    for key in VS.SUMS:
        assert (none[key] == 0.0).all(), key


def test_only_the_outputs_are_written():
    """dG and dA into slices of a canary-filled device buffer."""
    import torch
    name, B = "c1", 8
    _, n, m, k, _ = VS.points(name, B).sh.shape
    big = torch.full((4096,), 777.0, dtype=torch.float64, device="cuda")
    mine = dict(dA=big[100:100 + m * n], dG=big[1000:1000 + k * n])
    r = call(name, B, want=["dA", "dG"], device=True, out=mine)
    assert set(r) == {"dA", "dG", "status"}
    got = big.cpu().numpy()
    full, _ = once(name, B)
    assert bits(got[100:100 + m * n], full["dA"]) and bits(got[1000:1000 + k * n], full["dG"])
    keep = np.ones(4096, bool)
    keep[100:100 + m * n] = keep[1000:1000 + k * n] = False
    assert (got[keep] == 777.0).all()


def test_layer_gradients_of_shared_matrices():
    import torch
    from socp_amd.torch_layer import SocpLayer
    name, B = "c1", 8
    sh = QC.shared_batch(name, B)
    cones, n, m, k, _ = sh.shape
    keys = ("c", "A", "b", "G", "h", "P")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    ten = {key: t(getattr(sh, key)).requires_grad_(True) for key in keys}
    rng = np.random.default_rng(3)
    w, v = t(rng.standard_normal(B * n)), t(rng.standard_normal(B * k))
    layer = SocpLayer(list(cones), n, m, k, shared_matrices=True, tol=1e-5)
    x, y, z, s, status, iters = layer(*[ten[key] for key in keys])
    ((w * x).sum() + (v * z).sum()).backward()
    assert (status.cpu().numpy() == 0).all()
    with torch.no_grad():
        ref = S.batch_vjp(list(cones), n, m, k, ten["A"].detach(), ten["G"].detach(), None, x.detach(), y.detach(),
                          z.detach(), s.detach(), w, None, v, None, P=ten["P"].detach(), skip=status,
                          want=["d" + key for key in keys], shared_matrices=True)
    for key in keys:
        g = ten[key].grad
        assert g is not None and g.shape == ten[key].shape, key
        assert bits(g.cpu().numpy(), ref["d" + key].cpu().numpy()), key
        assert float(g.abs().max()) > 0.0
    # the replicated, non-shared layer, summed over the batch
    rep = {key: (ten[key].detach().repeat(B) if key in ("A", "G", "P") else ten[key].detach().clone())
           .requires_grad_(True) for key in keys}
    sing = torch.zeros(B, dtype=torch.uint8, device="cuda")
    x2, _, z2, _, status2, _ = SocpLayer(list(cones), n, m, k, tol=1e-5)(*[rep[key] for key in keys], sing)
    ((w * x2).sum() + (v * z2).sum()).backward()
    assert (status2.cpu().numpy() == 0).all() and bits(x2.detach().cpu().numpy(), x.detach().cpu().numpy())
    for key in ("A", "G", "P"):
        per = rep[key].grad.view(B, -1)
        total = per.sum(0).cpu().numpy()
        allow = (2 * B + 8) * VS.U * per.abs().sum(0).cpu().numpy()
        err = np.abs(total - ten[key].grad.cpu().numpy())
        print(f"layer d{key}: worst |err| / allowance {float(np.max(err[allow > 0] / allow[allow > 0])):.3f}")
        assert (err <= allow).all(), key
