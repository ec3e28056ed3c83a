"""Parametric batches (SOCP_F_SHARED_MATRICES): one A, one G and one sing byte
for the whole batch.

Contract under test: a call with the flag returns, for every output array, the
bits of the same call without the flag on A, G and sing replicated B times
(np.tile), in the same process -- on the register kernel (where G and A then
stay resident across the problems of a wave), the blocked kernel, the
rank-update plugin and the ingest pipeline, and together with the other flags.

Register-kernel batches hold 16 problems per CU (4,096 on an MI355X): the
launch's grid is at most 8 waves per CU, so on average every wave takes two or
more problems and the resident G and A serve problems that did not load them.
Under the reference stopping rule (tol 1e-5, maxit 40) the problems leave at
different iterations.

Oracle gate, so that "equal to replicated" cannot hide two equal errors: the
first 16 problems of the C1 and C2 shapes at fixed K = 4 against the CPU oracle
in the kernels' operation order (F_STRUCTURED | F_CHOLSOLVE): same status and
rel <= 1e-8 on x, z, s per problem -- the gate of test_gpu_fuse_u.py.
"""
import functools

import numpy as np
import pytest

import socp_amd as S
from shared_cases import interior, make, replicated

pytestmark = pytest.mark.gpu

KEYS = ("x", "y", "z", "s", "iters", "status", "res")
KKT_KEYS = ("cx", "cy", "cz", "cs", "status")
SEED = 20261019


@functools.lru_cache(maxsize=None)
def num_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=None)
def batch(name, B, seed=SEED):
    return make(name, B, seed)


def same(got, ref, keys=KEYS):
    for key in keys:
        a, b = np.asarray(got[key]), np.asarray(ref[key])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), key


def solve_pair(d, sing=0, **kw):
    """(shared, replicated) batch_solve of the same data; sing: the one byte, or None (the probe)."""
    cones, n, m, k = d.shape
    A, G = replicated(d)
    s1 = None if sing is None else np.array([sing], np.uint8)
    sB = None if sing is None else np.full(d.B, sing, np.uint8)
    sh = S.batch_solve(cones, n, m, k, d.c, d.A, d.b, d.G, d.h, s1, res=True, shared_matrices=True, **kw)
    kernel = S.default_context().last_kernel_name()
    rp = S.batch_solve(cones, n, m, k, d.c, A, d.b, G, d.h, sB, res=True, **kw)
    assert S.default_context().last_kernel_name() == kernel
    return sh, rp, kernel


# ------------------------------------------------------------ register kernel
@pytest.mark.parametrize("name", ["c1", "c2", "mq2", "m0"])
def test_register_kernel_reference_rule_and_fixed_k(name):
    d = batch(name, 16 * num_cu())
    sh, rp, kernel = solve_pair(d)  # the reference rule: tol 1e-5, maxit 40
    assert kernel.startswith("socp_small")
    same(sh, rp)
    it = sh["iters"]
    print(f"{name}: {d.B} problems on {kernel}, iterations {it.min()}..{it.max()}, "
          f"status counts {np.bincount(sh['status'], minlength=7).tolist()}")
    assert it.min() < it.max()  # problems leave at different iterations
    sh, rp, _ = solve_pair(d, maxit=4, tol=0.0)
    same(sh, rp)


@pytest.mark.parametrize("sing", [1, None], ids=["sing_byte", "probe"])
def test_register_kernel_singular_shape(sing):
    d = batch("sing", 16 * num_cu())
    sh, rp, kernel = solve_pair(d, sing=sing)
    assert kernel.startswith("socp_small")
    same(sh, rp)
    assert sh["iters"].min() < sh["iters"].max()
    sh, rp, _ = solve_pair(d, sing=sing, maxit=4, tol=0.0)
    same(sh, rp)


def test_flag_warm_start(oracle):
    d = batch("c1", 16 * num_cu())
    cones, n, m, k = d.shape
    A, G = replicated(d)
    w = oracle.batch_solve(cones, n, m, k, d.c, A, d.b, G, d.h, sing=np.zeros(d.B, np.uint8),
                           params=oracle.Params(maxit=2, tol=0.0))
    warm = (w["x"], w["y"], w["z"], w["s"])
    sh, rp, _ = solve_pair(d, warm=warm)
    same(sh, rp)
    assert sh["iters"].min() < sh["iters"].max()


def test_flag_explicit_inverse():
    sh, rp, kernel = solve_pair(batch("c1", 16 * num_cu()), explicit_inverse=True)
    assert kernel.startswith("socp_small")
    same(sh, rp)


def test_flag_detect_infeasible():
    sh, rp, kernel = solve_pair(batch("c1", 16 * num_cu()), detect_infeasible=True)
    assert kernel.startswith("socp_small")
    same(sh, rp)


def test_torch_device_tensors():
    import torch
    d = batch("c1", 16 * num_cu())
    cones, n, m, k = d.shape
    A, G = replicated(d)
    t = lambda v: torch.from_numpy(v).cuda()  # noqa: E731
    c, b, h = t(d.c), t(d.b), t(d.h)
    sh = S.batch_solve(cones, n, m, k, c, t(d.A), b, t(d.G), h, torch.zeros(1, dtype=torch.uint8, device="cuda"),
                       res=True, shared_matrices=True)
    rp = S.batch_solve(cones, n, m, k, c, t(A), b, t(G), h, torch.zeros(d.B, dtype=torch.uint8, device="cuda"),
                       res=True)
    S.default_context().sync()
    same({key: v.cpu().numpy() for key, v in sh.items()}, {key: v.cpu().numpy() for key, v in rp.items()})
    host, _, _ = solve_pair(d)
    same({key: v.cpu().numpy()[:host[key].size] for key, v in sh.items()}, host)


def rhs(d, seed=5):
    cones, n, m, k = d.shape
    rng = np.random.default_rng(seed)
    s, z = interior(rng, cones, d.B, k).reshape(-1), interior(rng, cones, d.B, k).reshape(-1)
    return s, z, [rng.standard_normal(d.B * q) for q in (n, m, k, k)]


def test_plugin_batch_kkt_solve():
    d = batch("c1", 16 * num_cu())
    cones, n, m, k = d.shape
    A, G = replicated(d)
    s, z, r = rhs(d)
    sh = S.batch_kkt_solve(cones, n, m, k, d.A, d.G, np.zeros(1, np.uint8), s, z, *r, shared_matrices=True)
    assert S.default_context().last_kernel_name().startswith("socp_small")
    rp = S.batch_kkt_solve(cones, n, m, k, A, G, np.zeros(d.B, np.uint8), s, z, *r)
    same(sh, rp, KKT_KEYS)
    assert (sh["status"] == 0).all()


def test_plugin_dense_handle():
    d = batch("c1", 16 * num_cu())
    cones, n, m, k = d.shape
    A, G = replicated(d)
    s, z, r = rhs(d)
    _, _, r2 = rhs(d, seed=6)
    hs = S.DenseHandle(cones, n, m, k, d.A, d.G, np.zeros(1, np.uint8), shared_matrices=True, batch=d.B)
    assert hs.h2d_bytes == (m * n + k * n) * 8 + 1  # one A, one G, one byte
    hr = S.DenseHandle(cones, n, m, k, A, G, np.zeros(d.B, np.uint8))
    assert hr.h2d_bytes == d.B * ((m * n + k * n) * 8 + 1)
    assert np.array_equal(hs.setup_iter(s, z), hr.setup_iter(s, z))
    for q in (r, r2):  # two solves against the one setup
        same(hs.solve_kkt(*q), hr.solve_kkt(*q), KKT_KEYS)
    assert S.default_context().last_kernel_name().startswith("socp_small")


def test_second_launch_with_another_G():
    """Nothing of a launch outlives it: the same context, another shared G."""
    B = 16 * num_cu()
    first = solve_pair(batch("c1", B))
    d2 = batch("c1", B, SEED + 1)
    assert not np.array_equal(d2.G, batch("c1", B).G)
    sh, rp, _ = solve_pair(d2)
    same(sh, rp)
    assert sh["x"].tobytes() != first[0]["x"].tobytes()


# -------------------------------------------------------------- other kernels
def test_blocked_kernel_forced():
    sh, rp, kernel = solve_pair(batch("c1", 4 * num_cu()), force_large=True, maxit=6, tol=0.0)
    assert "large" in kernel
    same(sh, rp)


def test_blocked_kernel_shape_without_register_variant():
    sh, rp, kernel = solve_pair(batch("wide", 64))
    assert "large" in kernel
    same(sh, rp)


@pytest.mark.parametrize("name", ["c1", "wide"])
def test_rank_update_plugin(name):
    d = batch(name, 64)
    cones, n, m, k = d.shape
    A, G = replicated(d)
    s, z, r = rhs(d)
    hs = S.SqrHandle(cones, n, m, k, d.A, d.G, np.zeros(1, np.uint8), shared_matrices=True, batch=d.B)
    assert hs.h2d_bytes == (m * n + k * n) * 8 + 1
    hr = S.SqrHandle(cones, n, m, k, A, G, np.zeros(d.B, np.uint8))
    st = hs.setup_iter(s, z)
    assert np.array_equal(st, hr.setup_iter(s, z)) and (st == 0).all()
    same(hs.solve_kkt(*r), hr.solve_kkt(*r), KKT_KEYS)
    assert hs.factor(3).tobytes() == hr.factor(3).tobytes()
    same(hs.scaling(), hr.scaling(), ("l", "wbs", "mu"))
    same(hs.solve_socp(d.c, d.b, d.h), hr.solve_socp(d.c, d.b, d.h))


# --------------------------------------------------------------------- ingest
def test_ingest_shared_batches_and_misuse():
    B = 512
    d1, d2 = batch("c2", B), batch("c2", B, SEED + 2)  # two parametric batches, each with its own G
    cones, n, m, k = d1.shape
    kw = dict(maxit=8, tol=0.0)
    ing = S.Ingest(cones, n, m, k, B, shared_matrices=True)
    slot = ing.next_inputs()
    assert set(slot) == {"c", "b", "h"}  # no A / G / sing staging
    with pytest.raises(S.SocpError, match="set_matrices"):
        ing.submit(d1.c, None, d1.b, None, d1.h, **kw)  # before set_matrices
    ing.set_matrices(d1.A, d1.G, np.zeros(1, np.uint8))
    with pytest.raises(S.SocpError, match="NULL"):
        ing.submit(d1.c, np.tile(d1.A, B), d1.b, np.tile(d1.G, B), d1.h, **kw)  # A, G given
    with pytest.raises(S.SocpError, match="NULL"):
        ing.submit(d1.c, None, d1.b, None, d1.h, np.zeros(B, np.uint8), **kw)  # sing given
    with pytest.raises(S.SocpError, match="submit_csc"):
        ing.submit_csc(d1.c, d1.b, d1.h, None, (np.zeros(B + 1, np.int64),) * 4, (np.zeros(B + 1, np.int64),) * 4)
    t = ing.submit(d1.c, None, d1.b, None, d1.h, **kw)
    with pytest.raises(S.SocpError, match="outstanding"):
        ing.set_matrices(d2.A, d2.G)  # a ticket is outstanding
    got1 = ing.wait(t, res=True)
    ing.set_matrices(d2.A, d2.G, np.zeros(1, np.uint8))  # again between batches, another G
    got2 = ing.wait(ing.submit(d2.c, None, d2.b, None, d2.h, **kw), res=True)
    for d, got in ((d1, got1), (d2, got2)):
        A, G = replicated(d)
        same(got, S.batch_solve(cones, n, m, k, d.c, A, d.b, G, d.h, np.zeros(B, np.uint8), res=True, **kw))
        same(got, S.batch_solve(cones, n, m, k, d.c, d.A, d.b, d.G, d.h, np.zeros(1, np.uint8), res=True,
                                shared_matrices=True, **kw))
    plain = S.Ingest(cones, n, m, k, B)
    with pytest.raises(S.SocpError, match="SHARED_MATRICES"):
        plain.set_matrices(d1.A, d1.G)


# ---------------------------------------------------------------- oracle gate
def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


@pytest.mark.parametrize("name", ["c1", "c2"])
def test_oracle_gate(oracle, name):
    d = batch(name, 16 * num_cu())
    cones, n, m, k = d.shape
    nb = 16
    sh = S.batch_solve(cones, n, m, k, d.c, d.A, d.b, d.G, d.h, np.zeros(1, np.uint8), maxit=4, tol=0.0,
                       shared_matrices=True)
    want = oracle.batch_solve(cones, n, m, k, d.c[:nb * n], np.tile(d.A, nb), d.b[:nb * m], np.tile(d.G, nb),
                              d.h[:nb * k], sing=np.zeros(nb, np.uint8),
                              params=oracle.Params(maxit=4, tol=0.0, flags=oracle.F_STRUCTURED | oracle.F_CHOLSOLVE))
    assert (sh["status"][:nb] == want["status"]).all()
    for p in range(nb):
        for key, L in (("x", n), ("z", k), ("s", k)):
            e = rel(sh[key][p * L:(p + 1) * L], want[key][p * L:(p + 1) * L])
            print(f"{name} p={p} {key} rel={e:.3e}")
            assert e <= 1e-8, (name, p, key, e)
