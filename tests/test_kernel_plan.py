"""Which kernel a context would launch, asked of grlx_kernel_plan (no device): every row of the kernel table, every step of the precedence
order from both sides, the automatic layout's thresholds.  The cases and their literal expected values: tests/kernel_plan_cases.py."""
import re

import pytest

from tests import kernel_plan_cases as kc


@pytest.mark.parametrize("case", kc.CASES, ids=[c[0] for c in kc.CASES])
def test_plan(grlx, case):
    name, builder, n, over, flags, simds, _, want = case
    flags |= 0 if flags & (kc.FITS | kc.NOFIT) else kc.FITS       # (no device here: the runtime is not asked)
    rpw, rollout, server, variant, grid = grlx.capi.kernel_plan(kc.build(grlx, builder, n, over), simds, flags)
    assert (rpw, rollout, server, variant) == want
    if name in kc.GRIDS:
        assert grid == kc.GRIDS[name]


def test_cases_cover_every_row_of_the_table():
    import os
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "grl_amd", "csrc", "grlx_kernel_table.h")).read()
    rows = re.findall(r"^\s*\{FAM_\w+,.*?GRLX_K\((.*?)\), (?:GRLX_UNSERVED|GRLX_K\((.*?)\), k\w+)\},$", text, flags=re.M)
    assert len(rows) > 80
    rollouts = {c[7][1] for c in kc.CASES}
    servers = {c[7][2] for c in kc.CASES}
    assert {r for r, _ in rows} == rollouts
    assert {s for _, s in rows if s} == servers - {""}


def test_plan_refuses_what_create_refuses(grlx):
    capi = grlx.capi
    with pytest.raises(capi.GrlxError) as ei:
        capi.kernel_plan(grlx.pendulum_sarsa_config(5, action_steps=4), 1024)
    assert ei.value.code == capi.ERR_INVALID and "not built" in str(ei.value)
    with pytest.raises(capi.GrlxError) as ei:
        capi.kernel_plan(grlx.pendulum_sarsa_config(5, tap_replica=0, tap_capacity=8), 1024, capi.PLAN_SWEEP)
    assert ei.value.code == capi.ERR_INVALID and "taps" in str(ei.value)
