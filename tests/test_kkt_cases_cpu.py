"""CPU preconditions of test_gpu_large_kkt.py: the case table of kkt_cases.py,
its refined block-system reference and the oracle agree before any device is
involved.

  * every cone table is valid, the shape is one the library supports, and no
    register-kernel variant takes it (blocked-only by n, m, k or the cone count);
  * the kernel each case names is the one large_layout's LDS arithmetic selects;
  * the arrow operator built blockwise is oracle.vprod;
  * the oracle's status is 0 in the kernel's operation order;
  * the refinement converged: the last correction is at most 4 ulp relative;
  * e_or <= (n + m + 2k) 2^-53 kappa_2(K) per vector: the forward bound of one
    backward-stable solve, so the reference and the oracle agree;
  * the sing / dy finding (kkt_cases.py): with dy != 0 the oracle's sing
    formula is far from the block system, with dy = 0 it agrees.
"""
import numpy as np
import pytest

import kkt_cases as KC
import variant_cases as V


@pytest.mark.parametrize("case", KC.CASES, ids=KC.case_id)
def test_case_table(case):
    n, m, k = case.n, case.m, case.k
    o = 0
    for kind, offs, dim in case.cones:
        assert kind in (KC.P_, KC.Q_) and offs == o and dim >= (1 if kind == KC.P_ else 2)
        o += dim
    assert o == k
    kinds = [c[0] for c in case.cones]
    assert kinds == sorted(kinds), "POC cones come first"
    assert len(case.cones) <= KC.MAXC
    # blocked-only: no register variant holds the shape, or more cones than it takes (NCS = 8)
    assert V.pick_variant(n, m, k) is None or len(case.cones) > 8
    # socp_api.hip large_fits: NPAD, MPAD <= 2048
    assert n <= 2048 and m <= 2048
    assert KC.kernel_name(n, m, k, case.xi) == case.kernel
    if KC.singular(case):
        assert m >= n - n // 2
        d = KC.inputs(case)
        assert not d["G"][:, :, n // 2:].any() and not d["rhs"][0][1].any() and not d["rhs"][1][1].any()
        assert KC.inputs(case, dy0=False)["rhs"][0][1].any()


def test_case_table_reaches_its_branches():
    """The shapes hold what their comments say (socp_kernels.hpp large_layout: NPAD, MPAD
    are n, m rounded up to 64; windows beyond 512)."""
    pad = lambda v: (max(v, 1) + 63) // 64 * 64  # noqa: E731
    c = KC.BY_ID
    assert pad(c["edge65"].n) == 128 and c["edge65"].m == 1
    assert c["m0"].m == 0
    assert pad(c["m65"].m) == 128 and len(c["m65"].cones) > 8
    assert c["sing"].sing == 1 and c["probe"].sing is None
    assert c["sing"][1:5] == c["probe"][1:5] == c["m65"][1:5]
    assert len(c["smallcones"].cones) > 8 and min(d for _, _, d in c["smallcones"].cones) == 2
    assert pad(c["n512"].n) == 512
    assert pad(c["wide"].n) == 576 and pad(c["gv_wide"].n) == 576
    assert pad(c["mwide"].m) == 576
    for a, b in (("xi", "edge65"), ("xi_wide", "wide"), ("xi_gv", "gv")):
        assert c[a].xi and c[a][1:5] == c[b][1:5]
    assert {x.kernel for x in KC.CASES} == {"socp_large_kernel", "socp_large_gv_kernel", "socp_large_xi_kernel",
                                            "socp_large_xi_gv_kernel"}


def test_supported_by_the_library():
    """socp_supported (host code of libsocp.so) takes every case."""
    import ctypes as C
    from socp_amd import _lib
    L = _lib.load()
    for case in KC.CASES:
        assert L.socp_supported(C.byref(_lib.Dims(KC.B, case.n, case.m, case.k, len(case.cones)))) == 1, case.id


def test_arrow_is_vprod(oracle):
    case = KC.BY_ID["smallcones"]
    rng = np.random.default_rng(5)
    lam, v = rng.standard_normal(case.k), rng.standard_normal(case.k)
    got = KC.arrow(case.cones, lam) @ v
    ref = oracle.vprod(list(case.cones), lam, v)
    assert np.abs(got - ref).max() <= 8 * KC.U * np.abs(ref).max()


def test_compute_scaling_without_the_product(oracle):
    """iwiw=False returns the same W, iW, lam, w-bar and mu."""
    case = KC.BY_ID["m65"]
    d = KC.inputs(case)
    a = oracle.compute_scaling(list(case.cones), d["s"][0], d["z"][0])
    b = oracle.compute_scaling(list(case.cones), d["s"][0], d["z"][0], iwiw=False)
    for key in ("W", "iW", "l", "mu", "wbs"):
        assert np.array_equal(a[key], b[key]), key
    assert a["status"] == b["status"] == 0 and not b["iWiW"].any() and a["iWiW"].any()


@pytest.mark.parametrize("case", KC.CASES, ids=KC.case_id)
def test_reference_and_oracle_agree(oracle, case):
    n, m, k = case.n, case.m, case.k
    for p in range(KC.B):
        ref = KC.reference(case, p)
        assert ref.steps >= 1 and (ref.corr <= 4 * 2.0 ** -52).all(), (p, ref.corr, ref.steps)
        for o in KC.oracle_solution(case, p):
            assert o["status"] == 0, (p, o["status"])
        bound = KC.floor(n, m, k) * KC.kappa(case, p)
        e_or = KC.oracle_errors(case, p)
        print(f"{case.id} p={p}: kappa_2(K) = {KC.kappa(case, p):.3g}, refinement steps {ref.steps}, "
              f"worst e_or {max(e for r in e_or for e in r if e is not None):.3g}, bound {bound:.3g}")
        for j in range(KC.NRHS):
            for key, e in zip(KC.KEYS, e_or[j]):
                assert e is None or e <= bound, (p, j, key, e, bound)


def test_sing_formula_differs_from_the_block_system_when_dy_is_not_zero(oracle):
    """densesolver.jl:66-85 with sing (m0 = dy - cy, n0 += A'dy), restated by
    the oracle and mirrored by the kernels, solves the block system only for
    dy = 0: otherwise its cx leaves A cx - dy of dy's own size (6e-3 .. 6e-2
    relative on cx here).  Asserted here as the reason test_gpu_large_kkt.py
    gates sing cases against the block system with dy = 0 and against the
    oracle with dy != 0."""
    case = KC.BY_ID["sing"]
    n, m, k = case.n, case.m, case.k
    d0, d1 = KC.inputs(case), KC.inputs(case, dy0=False)
    assert np.array_equal(d0["G"], d1["G"]) and np.array_equal(d0["rhs"][0][0], d1["rhs"][0][0])
    for p in range(KC.B):
        # dy = 0: the two references agree within the forward bound (test_reference_and_oracle_agree)
        assert max(e for r in KC.oracle_errors(case, p) for e in r) <= KC.floor(n, m, k) * KC.kappa(case, p)
        # dy != 0: they do not
        rhs = KC.problem_rhs(d1, p)
        ref = KC.reference_of(case.cones, d1["A"][p], d1["G"][p], d1["s"][p], d1["z"][p], rhs)
        assert (ref.corr <= 4 * 2.0 ** -52).all()
        for j, o in enumerate(KC.oracle_solution(case, p, dy0=False)):
            assert o["status"] == 0
            e = KC.rel_errors([o[key] for key in KC.KEYS], ref.sol[j])
            print(f"sing p={p} rhs {j}, dy != 0: oracle against the block system {e}")
            assert e[0] >= 1e-3, (p, j, e)
            # the block system has A cx = dy; the formula's cx does not
            A, dy = d1["A"][p], rhs[j][1]
            assert np.linalg.norm(A @ ref.sol[j][0] - dy) <= 1e-9 * np.linalg.norm(dy)
            assert np.linalg.norm(A @ o["cx"] - dy) >= 1e-2 * np.linalg.norm(dy)
