"""CPU: the create-time answers around mppi_config.obstacle_motion = 2, the learned model's scene handle -- all made
before the device is looked for."""
import ctypes as C

import pytest

from test_fleet_abi import create, lib_and_config


def config(**over):
    return lib_and_config(**dict(dict(n_agents=1, fleet_radius=0.0, obstacle_motion=2, model=2), **over))


@pytest.mark.parametrize("model", [0, 1])
def test_value_2_is_refused_on_the_analytic_models_before_the_device_is_looked_for(model):
    lib, capi, c = config(model=model)
    rc, msg = create(lib, capi, c)
    assert rc == capi.ERR_BAD_ARG, (rc, msg)
    assert "obstacle_motion 2" in msg and "MPPI_MODEL_DIFFDRIVE_MLP" in msg, msg


def test_value_1_with_the_learned_model_is_still_refused_and_points_to_value_2():
    lib, capi, c = config(obstacle_motion=1)
    rc, msg = create(lib, capi, c)
    assert rc == capi.ERR_UNSUPPORTED, (rc, msg)
    assert "MPPI_MODEL_DIFFDRIVE_MLP" in msg and "obstacle_motion = 2" in msg, msg


def test_value_2_needs_an_obstacle_model():
    lib, capi, c = config(obstacle_model=0)
    rc, msg = create(lib, capi, c)
    assert rc == capi.ERR_BAD_ARG and "MPPI_OBSTACLE_NONE" in msg, (rc, msg)


def test_fleet_radius_with_value_2_is_refused():
    lib, capi, c = config(n_agents=3, fleet_radius=0.4)
    rc, msg = create(lib, capi, c)
    assert rc == capi.ERR_UNSUPPORTED, (rc, msg)
    assert "fleet" in msg and "analytic" in msg, msg


def test_sharding_and_f64_with_value_2_are_refused():
    lib, capi, c = config(K_global=512)
    rc, msg = create(lib, capi, c)
    assert rc == capi.ERR_UNSUPPORTED and "shard" in msg, (rc, msg)
    lib, capi, c = config(precision=1)
    assert capi.PREC_F64 == 1
    rc, msg = create(lib, capi, c)
    assert rc == capi.ERR_UNSUPPORTED, (rc, msg)


def test_a_valid_learned_scene_config_passes_validation():
    """Past every refusal: the handle is made, or -- on a machine without an MI355X -- the device check is what stops it."""
    for over in (dict(), dict(n_agents=3), dict(waypoint_mode=0)):
        lib, capi, c = config(**over)
        rc, msg = create(lib, capi, c)
        assert rc in (capi.OK, capi.ERR_NO_DEVICE), (rc, msg)


def test_no_symbol_and_no_config_field_came_with_it():
    lib, capi, _ = config()
    assert capi.OBSTACLE_MOTION_LEARNED == 2
    assert [f for f, _ in capi.MppiConfig._fields_][-3:] == ["obstacle_motion", "reserved0", "fleet_radius"]
    assert C.sizeof(capi.MppiConfig) == capi.config_size(lib)
