"""What a context launches: every launchable case of tests/kernel_plan_cases.py at its smallest shape (4-37 replicas, one trial, tables of
2^13 entries, the layout forced through the config).  After run(1) and sync(): the row of the kernel table, the variant and the layout.
What the same cases compute: tests/test_gpu_kernel_plan_parity.py."""
import pytest

from tests import kernel_plan_cases as kc

LAUNCHED = kc.LAUNCHED


@pytest.mark.gpu
@pytest.mark.parametrize("case", LAUNCHED, ids=[c[0] for c in LAUNCHED])
def test_launch(grlx, monkeypatch, case):
    name, builder, n, over, flags, _, _, (rpw, rollout, server, variant) = case
    cfg = kc.build(grlx, builder, n, dict(over, table_log2_capacity=13))
    r, _ = kc.open_runner(grlx, monkeypatch, case, cfg)
    try:
        assert r.last_kernel_name() == "" and r.last_kernel() == 0
        r.run(1)
        r.sync()
        assert (r.replicas_per_wave(), r.last_kernel_name(), r.last_kernel()) == (rpw, rollout, variant)
        served, fell_back = r.env_server_counts()
        assert (served + fell_back > 0) == (server != "")
    finally:
        r.close()
