"""The host rule of the slot plan (socp_small.hpp small_slot_plan, through
socp_debug_slot_plan): which rotation and slot kinds a plain solve of a k > 64
cone table takes on the register-resident kernel.  No device work.

Slot s, lane l holds element (64 s + l - rot) mod k.  Both slots pure as the
table stands: rot = 0 and the kernel compiled for that pair of kinds.  POC
elements followed by exactly 64 SOC elements in cones that are whole 16-lane
rows (all cones 16, 32 or 64 long): rot = 64, SOC slot + POC slot.  Otherwise
mixed slots, rot = 0."""
import os

import pytest

import socp_amd as S
from slot_cases import CASES, INVALID_TABLES, MIXED, POC_ONLY, SOC_ONLY

PLANS = {
    "c2_poc32_soc32_soc32": (64, SOC_ONLY, POC_ONLY),
    "soc32x3": (0, MIXED, MIXED),  # two SOC slots: left to the mixed kernel (small_slot_plan)
    "lp_poc96": (0, POC_ONLY, POC_ONLY),
    # cones of unequal length have no row-aligned reductions, so they are not rotated
    "poc32_soc64": (0, MIXED, MIXED),
    "k128_poc64_soc64": (0, POC_ONLY, SOC_ONLY),
    "poc16_soc16x5": (0, MIXED, MIXED),  # 80 SOC elements: no split into pure slots
    "poc50_soc20_soc26": (0, MIXED, MIXED),
    "poc16x2_soc16x4": (64, SOC_ONLY, POC_ONLY),
}


@pytest.fixture
def switch_env():
    old = os.environ.pop("SOCP_SLOT_SPECIALISE", None)
    yield
    os.environ.pop("SOCP_SLOT_SPECIALISE", None)
    if old is not None:
        os.environ["SOCP_SLOT_SPECIALISE"] = old


@pytest.mark.parametrize("case", [c for c in CASES if not c.warm], ids=lambda c: c.name)
def test_plan_of_case(case, switch_env):
    assert S.slot_plan(case.cones, case.k) == PLANS[case.name]


@pytest.mark.parametrize("case", [c for c in CASES if not c.warm], ids=lambda c: c.name)
def test_switch_forces_mixed(case, switch_env):
    os.environ["SOCP_SLOT_SPECIALISE"] = "0"
    assert S.slot_plan(case.cones, case.k) == (0, MIXED, MIXED)
    os.environ["SOCP_SLOT_SPECIALISE"] = "1"
    assert S.slot_plan(case.cones, case.k) == PLANS[case.name]


def test_rotation_properties(switch_env):
    # a rotation is 0 or 64 and moves a cone's first element to lane 0 of slot 0
    for c in CASES:
        rot, k0, k1 = S.slot_plan(c.cones, c.k)
        assert rot in (0, 64)
        assert (k0 == MIXED) == (k1 == MIXED)
        if rot:
            assert (k0, k1) == (SOC_ONLY, POC_ONLY) and (c.k - rot) in [cone[1] for cone in c.cones]
    # POC32 x2 + SOC32 x2 at k = 128: pure as it stands
    assert S.slot_plan([(0, 0, 32), (0, 32, 32), (1, 64, 32), (1, 96, 32)], 128) == (0, POC_ONLY, SOC_ONLY)
    # one slot (k <= 64): nothing to plan
    assert S.slot_plan([(0, 0, 32), (1, 32, 32)], 64) == (0, MIXED, MIXED)


@pytest.mark.parametrize("cones,k", INVALID_TABLES)
def test_tables_the_api_rejects_have_no_plan(cones, k, switch_env):
    # an SOC cone listed before a POC cone: SOCP_E_INVALID, as from a solve
    with pytest.raises(S.SocpError) as e:
        S.slot_plan(cones, k)
    assert e.value.code == -1
