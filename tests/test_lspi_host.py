"""grlx_lspi_*: what the host decides before any device work (runs without a GPU)."""
import pytest

NAN, INF = float("nan"), float("inf")


def test_config_pendulum_gives_the_reference_files_values(grlx):
    for name, code in (("triangle", grlx.capi.RBF_TRIANGLE), ("gauss", grlx.capi.RBF_GAUSS)):
        c = grlx.pendulum_lspi_config(4, name)
        assert c.struct_size == 120 and c.n_replicas == 4 and c.projector == code and c.env == grlx.capi.ENV_PENDULUM
        assert list(c.steps) == [11, 11, 3] and c.gamma == 0.97 and c.iterations == 10 and c.cutoff == 0.01 and c.sigma == 1.0
        assert (c.batch_size, c.max_batches, c.action_steps, c.integration_steps) == (10000, 10, 3, 5)
        assert (c.control_step, c.timeout, c.action_min, c.action_max, c.init_min, c.init_max) == (0.03, 2.99, -3.0, 3.0, 0.0, 1.0)


@pytest.mark.parametrize("projector,over,word", [
    ("triangle", dict(env=1), "env"), ("triangle", dict(steps=[11, 1, 3]), "steps[1]"), ("triangle", dict(steps=[2, 2, 1]), "steps[2]"),
    ("triangle", dict(steps=[11, 11, 5]), "steps"), (2, dict(), "projector"),
    ("gauss", dict(sigma=0.0), "sigma"), ("gauss", dict(sigma=-1.0), "sigma"), ("gauss", dict(cutoff=0.0), "cutoff"), ("gauss", dict(cutoff=1.0), "cutoff"),
    ("gauss", dict(sigma=NAN), "sigma"), ("gauss", dict(cutoff=INF), "cutoff"), ("triangle", dict(gamma=NAN), "gamma"),
    ("triangle", dict(timeout=INF), "timeout"), ("triangle", dict(init_max=NAN), "init_max"), ("triangle", dict(action_min=-INF), "action_min"),
    ("triangle", dict(control_step=NAN), "control_step"), ("triangle", dict(struct_size=12), "struct_size")])
def test_refusals_name_their_field_before_any_device_work(grlx, projector, over, word):
    capi = grlx.capi
    with pytest.raises(capi.GrlxError) as ei:
        grlx.LspiRunner(grlx.pendulum_lspi_config(1, projector, **over), [1])
    assert ei.value.code == capi.ERR_INVALID and word in str(ei.value), str(ei.value)


def test_the_feature_bound_admits_the_reference_file(grlx):
    """F = 363 passes validation; 512 is the bound, 513 features are refused (8 x 8 x 8 = 512 passes, 9 x 19 x 3 = 513 does not)"""
    capi = grlx.capi
    for steps, refused in (([11, 11, 3], False), ([8, 8, 8], False), ([9, 19, 3], True)):
        try:
            grlx.LspiRunner(grlx.pendulum_lspi_config(1, steps=steps), [1]).close()
            code = capi.OK
        except capi.GrlxError as ex:
            code = ex.code
        assert (code == capi.ERR_INVALID) == refused and code in (capi.OK, capi.ERR_NO_DEVICE, capi.ERR_INVALID)


def test_no_cpu_fallback(grlx):
    capi = grlx.capi
    if capi.load().grlx_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(capi.GrlxError) as ei:
        grlx.LspiRunner(grlx.pendulum_lspi_config(2), [1, 2])
    assert ei.value.code == capi.ERR_NO_DEVICE
