"""CPU: the create-time answers of mppi_config.obstacle_motion = 3 (the learned model's fleet handle) -- all made
before the device is looked for --, the unchanged answer of value 2 with a fleet radius, and the constant.  No symbol, no field:
MPPI_ABI_VERSION stays 8."""
import ctypes as C

import pytest

from test_fleet_abi import create, lib_and_config


def config(**over):
    return lib_and_config(**dict(dict(model=2, obstacle_motion=3, n_agents=3, fleet_radius=0.4, K=256, T=20), **over))


def test_the_fleet_handle_passes_validation():
    """Past every refusal: the handle is made, or -- on a machine without an MI355X -- the device check is what stops it.  A
    library without value 3 answers MPPI_ERR_BAD_ARG."""
    for over in (dict(), dict(n_agents=2), dict(n_agents=256, K=64), dict(obstacle_model=2), dict(waypoint_mode=2), dict(K=32768)):
        lib, capi, c = config(**over)
        rc, msg = create(lib, capi, c)
        assert rc in (capi.OK, capi.ERR_NO_DEVICE), (over, rc, msg)


@pytest.mark.parametrize("over,code,words", [
    (dict(model=0), "ERR_BAD_ARG", ("obstacle_motion 3", "MPPI_MODEL_DIFFDRIVE_MLP")),   # an analytic model
    (dict(model=1), "ERR_BAD_ARG", ("obstacle_motion 3", "MPPI_MODEL_DIFFDRIVE_MLP")),
    (dict(fleet_radius=0.0), "ERR_BAD_ARG", ("fleet_radius > 0", "obstacle_motion = 2")),
    (dict(n_agents=1), "ERR_BAD_ARG", ("n_agents >= 2",)),
    (dict(n_agents=0), "ERR_BAD_ARG", ("n_agents >= 2",)),
    (dict(fleet_radius=-0.1), "ERR_BAD_ARG", ("fleet_radius",)),
    (dict(fleet_radius=float("nan")), "ERR_BAD_ARG", ("fleet_radius",)),
    (dict(n_agents=257), "ERR_UNSUPPORTED", ("256",)),
    (dict(K_global=512), "ERR_UNSUPPORTED", ("sharded", "K_global = K")),
    (dict(precision=1), "ERR_UNSUPPORTED", ("f32",)),
    (dict(obstacle_model=0), "ERR_BAD_ARG", ("MPPI_OBSTACLE_NONE",)),
    (dict(waypoint_mode=0), "ERR_UNSUPPORTED", ("MPPI_WAYPOINT_FROZEN",)),                # what learned batches refuse
    (dict(K=32769), "ERR_UNSUPPORTED", ("512 rollout", "K <= 32768")),
])
def test_create_refuses_before_the_device_is_looked_for(over, code, words):
    lib, capi, c = config(**over)
    rc, msg = create(lib, capi, c)
    assert rc == getattr(capi, code), (rc, msg)
    for w in words:
        assert w in msg, msg


def test_value_2_with_a_fleet_radius_keeps_its_answer_and_points_to_value_3():
    lib, capi, c = config(obstacle_motion=2)
    rc, msg = create(lib, capi, c)
    assert rc == capi.ERR_UNSUPPORTED, (rc, msg)
    assert "fleet" in msg and "analytic" in msg and "obstacle_motion = 3" in msg, msg


def test_the_constant_and_the_abi_version():
    lib, capi, c = config()
    assert capi.OBSTACLE_MOTION_LEARNED_FLEET == 3 and capi.OBSTACLE_MOTION_LEARNED == 2
    assert capi.ABI_VERSION == 8 and lib.mppi_abi_version() == 8
    assert capi.config_size(lib) == C.sizeof(capi.MppiConfig)
    assert [f for f, _ in capi.MppiConfig._fields_][-3:] == ["obstacle_motion", "reserved0", "fleet_radius"]
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mppi_hip.h")).read()
    assert "#define MPPI_OBSTACLE_MOTION_LEARNED_FLEET 3" in header and "#define MPPI_ABI_VERSION 8" in header
