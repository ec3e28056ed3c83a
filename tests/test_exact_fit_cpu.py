"""The host rule of the exact-fit kernel (socp_api.hip small_exact_pair, through
socp_debug_exact_fit): which plain solves run the pure-slot solver compiled for
their exact launch geometry.  No device work.

One geometry is compiled: n = 64, m = 16, k = 96 with POC32 + SOC32 + SOC32 --
variant <4,24,1> filled exactly, the slot plan's SOC+POC pair at rot = 64,
cones of two 16-lane rows, the SYRK's cone rows fused into the residuals'
G x pass.  Every near miss keeps the generic kernel.  (The kernel keeps the
G'G probe, so the rule does not ask whether `sing` is given.)"""
import os

import pytest

import socp_amd as S
from socp_amd import _lib

P, Q = 0, 1  # cone kinds of include/socp.h: POC, SOC
C2_CONES = [(P, 0, 32), (Q, 32, 32), (Q, 64, 32)]
SWITCHES = ("SOCP_EXACT_FIT", "SOCP_FUSE_U", "SOCP_SLOT_SPECIALISE")


@pytest.fixture
def switch_env():
    old = {name: os.environ.pop(name, None) for name in SWITCHES}
    yield
    for name, v in old.items():
        os.environ.pop(name, None)
        if v is not None:
            os.environ[name] = v


def test_c2_is_eligible(switch_env):
    assert S.exact_fit(C2_CONES, 64, 16, 96) is True
    # the plan the kernel holds as constants
    assert S.slot_plan(C2_CONES, 96) == (64, 1, 2)


NEAR_MISSES = {
    # dims that do not fill <4,24,1>
    "n63": (C2_CONES, 63, 16, 96),
    "k92": ([(P, 0, 28), (Q, 28, 32), (Q, 60, 32)], 64, 16, 92),
    "m15": (C2_CONES, 64, 15, 96),
    "m0": (C2_CONES, 64, 0, 96),
    # another variant altogether
    "n48": (C2_CONES, 48, 16, 96),
    "m32": (C2_CONES, 64, 32, 96),
    # other cone tables on the same variant
    "poc32_soc64": ([(P, 0, 32), (Q, 32, 64)], 64, 16, 96),
    # POC + 2 x SOC32 with k padded differently: the last row steps hold padding
    "poc30_soc32_soc32_k94": ([(P, 0, 30), (Q, 30, 32), (Q, 62, 32)], 64, 16, 94),
    "poc31_soc32_soc32_k95": ([(P, 0, 31), (Q, 31, 32), (Q, 63, 32)], 64, 16, 95),
    # the same pair and rotation from cones of one 16-lane row: al_rows = 1, no fused U
    "poc16x2_soc16x4": ([(P, 0, 16), (P, 16, 16), (Q, 32, 16), (Q, 48, 16), (Q, 64, 16), (Q, 80, 16)], 64, 16, 96),
    # pure slots as the table stands (POC+POC, rot = 0)
    "lp_poc96": ([(P, 0, 96)], 64, 16, 96),
    "poc32x3": ([(P, 0, 32), (P, 32, 32), (P, 64, 32)], 64, 16, 96),
    # two SOC slots: the mixed kernel
    "soc32x3": ([(Q, 0, 32), (Q, 32, 32), (Q, 64, 32)], 64, 16, 96),
}


@pytest.mark.parametrize("name", sorted(NEAR_MISSES))
def test_near_misses_are_ineligible(name, switch_env):
    cones, n, m, k = NEAR_MISSES[name]
    assert S.exact_fit(cones, n, m, k) is False


def test_soc_before_poc_has_no_solve_at_all(switch_env):
    # SOC32 + POC32 + SOC32: the API rejects the table (POC cones come first), as a solve does
    with pytest.raises(S.SocpError) as e:
        S.exact_fit([(Q, 0, 32), (P, 32, 32), (Q, 64, 32)], 64, 16, 96)
    assert e.value.code == -1


def test_flags(switch_env):
    # the xi and di solvers keep their one kernel; the blocked kernel has none
    for fl in (_lib.F_EXPLICIT_INVERSE, _lib.F_DETECT_INFEASIBLE, _lib.F_FORCE_LARGE):
        assert S.exact_fit(C2_CONES, 64, 16, 96, flags=fl) is False
    # flags the kernel choice does not depend on: a warm start (init_overlap stays a run-time
    # argument), device pointers, one shared A and G, equilibrated data
    for fl in (_lib.F_WARM_START, _lib.F_DEVICE_PTRS, _lib.F_SHARED_MATRICES, _lib.F_EQUILIBRATE):
        assert S.exact_fit(C2_CONES, 64, 16, 96, flags=fl) is True


@pytest.mark.parametrize("name", SWITCHES)
def test_each_switch_off_makes_the_launch_ineligible(name, switch_env):
    os.environ[name] = "0"
    assert S.exact_fit(C2_CONES, 64, 16, 96) is False
    os.environ[name] = "1"
    assert S.exact_fit(C2_CONES, 64, 16, 96) is True
    del os.environ[name]
    assert S.exact_fit(C2_CONES, 64, 16, 96) is True
