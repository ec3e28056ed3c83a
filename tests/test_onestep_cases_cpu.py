"""The one-step parity cases (onestep_cases.py) and their gate, without a device.

  * replay: one oracle step from iterate t of the oracle's solve is iterate
    t + 1 of that solve, bit for bit -- the step is the solve's own;
  * the cases are what they claim: few undecided steps (the status under a
    one-ulp perturbation of G), and enough decided FAILING steps that an
    implementation whose pivot or domain test differs has steps to show it at;
  * the gate is attainable and not vacuous: a second build of the same oracle
    with fused multiply-adds (oracle/Makefile `fma`) -- an honest implementation
    of the same order with other roundings -- passes the assertions the device
    test makes (onestep_cases.check), on every case but C4 (cost).
"""
import importlib.util
import os
import subprocess

import numpy as np
import pytest

import onestep_cases as OC

REF_NAMES = list(OC.REFS)


@pytest.fixture(scope="module")
def refs(oracle):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = OC.references(oracle, name)
        return cache[name]
    return get


@pytest.fixture(scope="module")
def oracle_fma(oracle):
    """oracle.py once more, bound to build/liboracle_fma.so."""
    odir = os.path.dirname(os.path.abspath(oracle.__file__))
    subprocess.check_call(["make", "-s", "-C", odir, "fma"])
    old = os.environ.get("SOCP_ORACLE_LIB")
    os.environ["SOCP_ORACLE_LIB"] = os.path.join(odir, "build", "liboracle_fma.so")
    try:
        spec = importlib.util.spec_from_file_location("oracle_fma", os.path.join(odir, "oracle.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mod.lib()
    finally:
        if old is None:
            del os.environ["SOCP_ORACLE_LIB"]
        else:
            os.environ["SOCP_ORACLE_LIB"] = old
    assert mod.lib() is not oracle.lib()
    return mod


@pytest.mark.parametrize("name", REF_NAMES)
def test_replay_and_census(refs, name):
    steps = refs(name)
    for r in steps:
        if r["last"]:
            assert r["replay"] is None
            continue
        assert r["status"] == 1, (r["problem"], r["t"], r["status"])
        for got, want in zip(r["next"], r["replay"]):
            assert np.array_equal(got, want), (r["problem"], r["t"])
        if r["floor"] is not None:
            assert r["decided"] and all(np.isfinite(v) for v in r["floor"].values())
    n, und, fail, cont = OC.census(steps)
    print(f"{name}: steps {n}, undecided {und}, decided failing {fail}, decided continuing {cont}")
    assert und <= OC.UNDECIDED_CAP * n, (und, n)
    for case in OC.CASES:
        if case.ref == name:
            assert fail >= case.min_failing, (case.name, fail)


def test_selection_rule():
    """16 chol(H) failures, every domain error (at most 8) and 8 converged problems per C2 order."""
    for run in ("structured_chol", "structured"):
        _, idx = OC.outcome_problems(run)
        assert 24 < len(idx) <= 32 and len(set(idx)) == len(idx), (run, len(idx))


@pytest.mark.parametrize("name", list(OC.LOCATED))
def test_located_steps_lie_on_a_cone_boundary(refs, name):
    """The located cause of the kernels' status differences (measured on the
    device: onestep_cases.LOCATED, equal to the oracle's status at every other
    decided failing step): at every decided failing step of the case the
    oracle's status is domain exactly where v0^2 - |v1|^2 of an SOC of s or z is
    negative in the oracle's serial order, and the kernel's is domain exactly
    where it is negative in the kernel's own order."""
    case = next(c for c in OC.CASES if c.name == name)
    sh = OC.REFS[case.ref].shape
    kernel = {(p, t): (want, got) for p, t, want, got in OC.LOCATED[name]}
    seen = 0
    for r in refs(case.ref):
        if not r["decided"] or r["status"] == 1:
            continue
        want, got = kernel.get((r["problem"], r["t"]), (r["status"], r["status"]))
        seen += (want != got)
        assert want == r["status"] and {want, got} <= {2, 4}, (r["problem"], r["t"])
        serial, tree = OC.domain_by_order(sh, r, head_lane=not case.kernel.startswith("socp_large"))
        assert serial == (want == 4) and tree == (got == 4), (r["problem"], r["t"], want, got, serial, tree)
    assert seen == len(kernel)


@pytest.mark.parametrize("name", [n for n in REF_NAMES if any(c.ref == n and c.stand_in for c in OC.CASES)])
def test_fma_build_passes_the_gate(refs, oracle_fma, name):
    steps = refs(name)
    got = OC.oracle_steps(oracle_fma, name, steps)
    rows, fail, cont, allow = OC.check(name + " (fma stand-in)", OC.REFS[name].shape, steps, got)
    # another rounding, not the same library twice: some vector differs
    assert any(r[4] > 0.0 for r in rows)
