"""SOCP_F_NORMALISE on the CPU: properties of the numpy restatement of the rule
(tests/normalise_cases.py), what the scaling does to the CPU references on the
batches the GPU tests use, and the refusals that need no device.
"""
import ctypes as C

import numpy as np
import pytest

import normalise_cases as N
import qp_cases as Q
import socp_amd as S
from socp_amd import _lib

SCALES = [(10, 10), (14, -6)]
SHAPES = ["c1", "s8", "m0"]


# ----------------------------------------------------------------- the rule
def test_exponent_of_special_norms():
    """Zero, Inf and NaN give 0; a subnormal is read by its true exponent and
    runs into the clamp, as does 2^1023 on the other side."""
    v = [0.0, np.inf, np.nan, -1.0, 5e-324, 2.0 ** -1022, 2.0 ** -256, 2.0 ** -255.5, 0.5, 0.99, 1.0, 1.99, 2.0, 4.0,
         2.0 ** 256, 2.0 ** 257, 2.0 ** 1023]
    want = [0, 0, 0, 0, 256, 256, 256, 256, 1, 1, 0, 0, -1, -2, -256, -256, -256]
    assert [N.e_of(q) for q in v] == want


@pytest.mark.parametrize("name", list(N.RULE_SHAPES))
def test_norms_lie_in_1_2_afterwards(name):
    """On the rule batch: every problem has its own pair; wherever a norm is
    finite, positive and unclamped the scaled vector's largest entry lies in
    [1, 2); the decorated problems keep exponent 0 (c = 0, a NaN in h, an Inf
    in c) or run into the clamp (a subnormal-only c)."""
    d = N.rule_batch(name, 5)
    sc = N.restate(d.n, d.m, d.k, d.c, d.b, d.h, d.P)
    ex = sc.expo
    assert ex.shape == (5, 2) and ex.dtype == np.int32
    assert len({tuple(e) for e in ex.tolist()}) == 5
    assert ex[1, 0] == 0 and ex[2, 1] == 0 and ex[3, 0] == 0 and ex[4, 0] == N.CLAMP
    cs, hs = sc.c.reshape(5, d.n), sc.h.reshape(5, d.k)
    bs = sc.b.reshape(5, d.m) if d.m else np.zeros((5, 0))
    for p in range(5):
        if p not in (1, 3, 4):
            assert 1.0 <= np.abs(cs[p]).max() < 2.0, p
            assert np.abs(cs[p]).argmax() == d.n - 1 and cs[p, -1] < 0
        if p != 2:
            assert 1.0 <= max(np.abs(bs[p]).max(initial=0.0), np.abs(hs[p]).max()) < 2.0, p
            assert np.abs(hs[p]).argmax() == d.k - 1 and hs[p, -1] < 0
    # exact both ways wherever nothing is subnormal
    back = np.ldexp(cs, -ex[:, :1].astype(np.int64)).reshape(-1)
    keep = np.ones(5, bool)
    keep[4] = False
    assert np.array_equal(back.reshape(5, -1)[keep], d.c.reshape(5, -1)[keep], equal_nan=True)
    # P follows ec - eb
    assert np.array_equal(sc.P.reshape(5, -1)[0], np.ldexp(d.P.reshape(5, -1)[0], int(ex[0, 0]) - int(ex[0, 1])))


def test_m0_has_no_b_term():
    d = N.rule_batch("m0", 5)
    assert d.m == 0 and d.b.size == 0
    ex = N.exponents(d.n, 0, d.k, d.c, d.b, d.h)
    h = d.h.reshape(5, d.k)
    assert [int(e) for e in ex[:, 1]] == [N.e_of(N.norm_of(h[p])) for p in range(5)]


def test_b_takes_part_in_nb():
    """A b larger than every h moves eb."""
    d = N.rule_batch("s8", 1)
    b = d.b.copy()
    b[0] = 2.0 ** 40
    assert N.exponents(d.n, d.m, d.k, d.c, b, d.h)[0, 1] == -40
    assert N.exponents(d.n, d.m, d.k, d.c, d.b, d.h)[0, 1] == N.e_of(N.norm_of(d.h)) > -40


def test_shared_P_takes_the_batch_wide_pair():
    """One pair for the batch from the maxima over it, a NaN anywhere freezing
    it; without P, or without sharing, the pairs stay per problem."""
    d = N.rule_batch("s8", 4)
    P1 = d.P[:d.n * d.n]
    sc = N.restate(d.n, d.m, d.k, d.c, d.b, d.h, P1, shared=True)
    assert (sc.expo == sc.expo[0]).all() and sc.expo.shape == (4, 2)
    # c grows and (b, h) shrink with p: the batch's nc is problem 3's, its nb problem 0's
    per = N.exponents(d.n, d.m, d.k, d.c, d.b, d.h)
    assert tuple(sc.expo[0]) == (per[3, 0], per[0, 1])
    assert sc.P.size == d.n * d.n
    assert np.array_equal(sc.P, np.ldexp(P1, int(sc.expo[0, 0]) - int(sc.expo[0, 1])))
    assert np.array_equal(N.restate(d.n, d.m, d.k, d.c, d.b, d.h, None, shared=True).expo, per)
    d5 = N.rule_batch("s8", 5)  # a NaN in problem 2's h, an Inf in problem 3's c
    assert tuple(N.restate(d5.n, d5.m, d5.k, d5.c, d5.b, d5.h, P1, shared=True).expo[0]) == (0, 0)


# ---------------------------------------------- the references, as assertions
def _converged(refs):
    return sum(r["status"] == 0 for r in refs)


@pytest.mark.parametrize("qp", [False, True], ids=["linear", "qp"])
@pytest.mark.parametrize("name", SHAPES)
def test_reference_rescued_and_scale_invariant(oracle, name, qp):
    """The (2^10, 2^10) and (2^14, 2^-6) batches of c1, s8 and m0 under the
    reference stopping rule, on the CPU oracle in the kernels' operation order
    (linear) and on qp_cases.qp_reference (quadratic, P times 2^(a - b)): as
    given 0 of 16 converge, normalised by the restatement 16 of 16 do, and the
    normalised run's iterate and iteration count are bitwise those of the
    normalised unscaled batch."""
    base = N.reference(name, qp, 0, 0, True)
    assert _converged(base) == N.NB
    for a, b in SCALES:
        assert _converged(N.reference(name, qp, a, b, False)) == 0, (a, b)
        got = N.reference(name, qp, a, b, True)
        assert _converged(got) == N.NB, (a, b)
        for r, r0 in zip(got, base):
            assert r["iters"] == r0["iters"]
            for key in "xyzs":
                assert np.asarray(r[key]).tobytes() == np.asarray(r0[key]).tobytes(), (a, b, key)


def _hist(refs):
    h = [0] * 5
    for r in refs:
        h[r["status"]] += 1
    return h


def _its(refs):
    return round(float(np.mean([r["iters"] for r in refs])), 1)


# DESIGN.md section 25's table: (shape, a, b, histogram as given); normalised, every row is [16,0,0,0,0]
TABLE = [("c1", 0, 0, [16, 0, 0, 0, 0]), ("c1", 10, 0, [0, 0, 11, 0, 5]), ("c1", 0, 10, [7, 0, 4, 0, 5]),
         ("c1", 10, 10, [0, 0, 8, 0, 8]), ("c1", 14, -6, [0, 0, 10, 0, 6]), ("c2", 0, 0, [11, 0, 3, 0, 2]),
         ("c2", 10, 10, [0, 0, 13, 0, 3]), ("s8", 10, 10, [0, 1, 11, 0, 4]), ("s8", 14, -6, [0, 0, 4, 0, 12]),
         ("m0", 10, 10, [0, 0, 7, 0, 9]), ("m0", 14, -6, [0, 0, 7, 0, 9])]


@pytest.mark.parametrize("name,a,b,given", TABLE, ids=[f"{r[0]}-{r[1]}-{r[2]}" for r in TABLE])
def test_table_rows(oracle, name, a, b, given):
    """Every row of DESIGN.md section 25's table on the CPU oracle in the
    kernels' operation order: the status histogram [converged, maxit, chol(H),
    chol(S), domain] as given and normalised, and the mean iteration counts
    that the table prints (c1 and c2 at (0, 0); the normalised counts are those
    of every other row of the shape, by the scale invariance above)."""
    assert _hist(N.reference(name, False, a, b, False)) == given
    assert _hist(N.reference(name, False, a, b, True)) == [16, 0, 0, 0, 0]
    its = dict(c1=(5.9, 4.6), c2=(15.4, 13.6))
    if (a, b) == (0, 0):
        assert (_its(N.reference(name, False, 0, 0, False)), _its(N.reference(name, False, 0, 0, True))) == its[name]
    elif name in its:
        assert _its(N.reference(name, False, a, b, True)) == its[name][1]


@pytest.mark.parametrize("qp", [False, True], ids=["linear", "qp"])
def test_three_quarters_of_the_iters_batches_are_clear(oracle, qp):
    """The GPU test compares iters on the c1 (10, 10) batch and its QP twin: at
    least 3/4 of each is decided by qp_cases.clear's margin of 1.1."""
    refs = N.reference("c1", qp, 10, 10, True)
    assert sum(Q.clear(r) for r in refs) >= 3 * N.NB // 4


# ---------------------------------------------------------------- refusals
@pytest.fixture()
def blank_ctx():
    """Zeroed memory in a context's place: the entries check their flags and
    dims before they touch the context, so these checks run without a device."""
    buf = C.create_string_buffer(1 << 16)
    return C.cast(buf, C.c_void_p)


def _cones():
    return np.array([0, 1], np.int32), np.array([0, 1], np.int32), np.array([1, 3], np.int32)


def _solve(ctx, flags, qp=False):
    L = _lib.load()
    kind, offs, dim = _cones()
    d = _lib.Dims(2, 3, 0, 4, 2)
    pr = _lib.default_params(flags=flags)
    head = (ctx, C.byref(d), kind.ctypes.data, offs.ctypes.data, dim.ctypes.data)
    one = np.zeros(64)
    if qp:
        return L.socp_batch_solve_qp(*head, one.ctypes.data, *[None] * 6, C.byref(pr), *[None] * 7)
    return L.socp_batch_solve_ex(*head, *[None] * 6, C.byref(pr), *[None] * 7)


def test_detection_with_the_flag_is_refused(blank_ctx):
    L = _lib.load()
    for qp in (False, True):
        flags = _lib.F_NORMALISE | _lib.F_DETECT_INFEASIBLE
        assert _solve(blank_ctx, flags, qp) == _lib.SOCP_E_UNSUPPORTED
        msg = L.socp_last_error().decode()
        if qp:  # the QP entry's own refusal of detection comes first and stays as it was
            assert "socp_batch_solve_qp with SOCP_F_DETECT_INFEASIBLE" in msg
        else:
            assert "SOCP_F_NORMALISE" in msg and "SOCP_F_DETECT_INFEASIBLE" in msg
    # the refusals that were there stay word for word
    assert _solve(blank_ctx, _lib.F_NORMALISE | _lib.F_EQUILIBRATE | _lib.F_WARM_START) == _lib.SOCP_E_UNSUPPORTED
    assert "SOCP_F_EQUILIBRATE with SOCP_F_WARM_START" in L.socp_last_error().decode()
    assert _solve(blank_ctx, _lib.F_NORMALISE | _lib.F_DETECT_INFEASIBLE | _lib.F_EXPLICIT_INVERSE) \
        == _lib.SOCP_E_UNSUPPORTED
    assert "SOCP_F_DETECT_INFEASIBLE with SOCP_F_EXPLICIT_INVERSE" in L.socp_last_error().decode()


def test_flag_bit_and_export():
    L = _lib.load()
    assert _lib.F_NORMALISE == 2048
    assert "socp_batch_normalise" in _lib.EXPORTED and hasattr(L, "socp_batch_normalise")
    with open(_lib.HEADER) as f:
        assert "#define SOCP_F_NORMALISE 2048" in f.read()


def _normalise(ctx, dims, flags, P=None, Ps=None):
    L = _lib.load()
    one = np.zeros(64)
    return L.socp_batch_normalise(ctx, C.byref(dims) if dims is not None else None, P, one.ctypes.data,
                                  one.ctypes.data, one.ctypes.data, flags, None, Ps, None, None, None)


def test_normalise_entry_argument_checks(blank_ctx):
    L = _lib.load()
    ok = _lib.Dims(2, 3, 1, 4, 0)  # ncones is not read
    assert _normalise(None, ok, 0) == _lib.SOCP_E_INVALID and b"ctx" in L.socp_last_error()
    assert _normalise(blank_ctx, None, 0) == _lib.SOCP_E_INVALID and b"dims" in L.socp_last_error()
    for bad in (_lib.Dims(-1, 3, 1, 4, 0), _lib.Dims(2, 0, 1, 4, 0), _lib.Dims(2, 3, -1, 4, 0),
                _lib.Dims(2, 3, 1, 0, 0)):
        assert _normalise(blank_ctx, bad, 0) == _lib.SOCP_E_INVALID
    assert _normalise(blank_ctx, _lib.Dims(2 ** 31, 3, 1, 4, 0), 0) == _lib.SOCP_E_INVALID
    assert b"2^31-1" in L.socp_last_error()
    for flags in (_lib.F_WARM_START, _lib.F_FORCE_LARGE, _lib.F_NORMALISE, _lib.F_EQUILIBRATE, 1 << 20):
        assert _normalise(blank_ctx, ok, flags) == _lib.SOCP_E_INVALID
        assert b"socp_batch_normalise" in L.socp_last_error()
    assert _normalise(blank_ctx, _lib.Dims(0, 3, 1, 4, 0), _lib.F_SHARED_MATRICES) == 0  # an empty batch
    one = np.zeros(64)
    assert _normalise(blank_ctx, ok, 0, P=None, Ps=one.ctypes.data) == _lib.SOCP_E_INVALID
    assert b"without its input" in L.socp_last_error()


def test_centre_and_vjp_answer_invalid_for_the_bit(blank_ctx):
    L = _lib.load()
    kind, offs, dim = _cones()
    d = _lib.Dims(2, 3, 0, 4, 2)
    head = (blank_ctx, C.byref(d), kind.ctypes.data, offs.ctypes.data, dim.ctypes.data)
    assert L.socp_batch_centre(*head, *[None] * 7, 4, _lib.F_NORMALISE, *[None] * 6) == _lib.SOCP_E_INVALID
    assert L.socp_batch_vjp(*head, *[None] * 13, _lib.F_NORMALISE, *[None] * 9, None) == _lib.SOCP_E_INVALID
    assert L.socp_batch_vjp_sum(*head, *[None] * 13, _lib.F_NORMALISE, *[None] * 9, None) == _lib.SOCP_E_INVALID


def test_python_layers_refuse_the_rank_update_solver():
    d = N.batch("s8", False, 0, 0, 2)
    cones, n, m, k, _ = d.shape
    probs = [S.Problem(pr[1], pr[2], pr[3], pr[4], pr[5], [S.SOC(o, dm) for _, o, dm in cones]) for pr in d.probs]
    with pytest.raises(ValueError, match="normalise"):
        S.solve_socp_batched(probs, solver="sqr", normalise=True)
