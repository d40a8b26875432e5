"""What a context launches: every launchable case of tests/kernel_plan_cases.py at its smallest shape (4-37 replicas, one trial, tables of
2^13 entries, the layout forced through the config).  After run(1) and sync(): the row of the kernel table, the variant and the layout."""
import numpy as np
import pytest

from tests import kernel_plan_cases as kc

LAUNCHED = [c for c in kc.CASES if c[6]]


@pytest.mark.gpu
@pytest.mark.parametrize("case", LAUNCHED, ids=[c[0] for c in LAUNCHED])
def test_launch(grlx, monkeypatch, case):
    name, builder, n, over, flags, _, _, (rpw, rollout, server, variant) = case
    monkeypatch.setenv("GRLX_ENV_SERVER", "0" if flags & kc.OFF else "1")
    monkeypatch.setenv("GRLX_ENV_SERVER_WALKER", "1" if flags & kc.WALKER else "0")
    cfg = kc.build(grlx, builder, n, dict(over, table_log2_capacity=13))
    r = grlx.Runner(cfg, np.arange(1, n + 1))
    try:
        if flags & kc.SWEEP:
            r.set_replica_params(alpha=[0.1 + 0.01 * k for k in range(n)])
        if flags & (kc.STAMPS1 | kc.STAMPS2):
            r.set_diag(2 if flags & kc.STAMPS2 else 1)
        assert r.last_kernel_name() == "" and r.last_kernel() == 0
        r.run(1)
        r.sync()
        assert (r.replicas_per_wave(), r.last_kernel_name(), r.last_kernel()) == (rpw, rollout, variant)
        served, fell_back = r.env_server_counts()
        assert (served + fell_back > 0) == (server != "")
    finally:
        r.close()
