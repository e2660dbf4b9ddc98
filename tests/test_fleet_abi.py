"""CPU: the create-time refusals of mppi_config.fleet_radius -- all made before the device is looked for -- and the two entry
points that came with it (tests/test_abi_symbols.py holds the export list to the header by itself)."""
import ctypes as C

import numpy as np
import pytest


def lib_and_config(**over):
    import dnn_mppi_mpc_amd as pkg
    from dnn_mppi_mpc_amd import _capi as capi
    pkg.build_library()
    lib = capi.load_library(capi.LIB_PATH)
    c = capi.MppiConfig()
    c.struct_size = C.sizeof(capi.MppiConfig)
    c.model, c.precision, c.K, c.T = capi.MODEL_DIFFDRIVE, capi.PREC_F32, 256, 20
    c.delta_t, c.param_exploration, c.param_lambda, c.param_alpha = 0.1, 0.05, 1.0, 0.2
    c.u_max[0], c.u_max[1] = 5.0, 3.14
    c.sigma[0], c.sigma[3] = 0.1, 0.01
    c.waypoint_mode, c.search_window, c.filter_window = capi.WAYPOINT_FROZEN, 20, 10
    c.obstacle_model, c.safety_margin, c.collision_penalty = capi.OBSTACLE_CIRCLE, 0.8, 1e10
    c.n_agents, c.obstacle_motion, c.fleet_radius = 3, 1, 0.4
    for k, v in over.items():
        setattr(c, k, v)
    return lib, capi, c


def create(lib, capi, c):
    h = capi._H()
    rc = lib.mppi_create(C.byref(c), C.byref(h))
    msg = (lib.mppi_last_error(None) or b"").decode()
    if rc == capi.OK:
        lib.mppi_destroy(h)
    return rc, msg


@pytest.mark.parametrize("over,code,word", [
    (dict(fleet_radius=-0.1), "ERR_BAD_ARG", "fleet_radius"),
    (dict(fleet_radius=float("nan")), "ERR_BAD_ARG", "fleet_radius"),
    (dict(fleet_radius=float("inf")), "ERR_BAD_ARG", "fleet_radius"),
    (dict(n_agents=1), "ERR_BAD_ARG", "n_agents >= 2"),
    (dict(n_agents=0), "ERR_BAD_ARG", "n_agents >= 2"),
    (dict(obstacle_motion=0), "ERR_BAD_ARG", "obstacle_motion = 1"),
    (dict(n_agents=257), "ERR_UNSUPPORTED", "256"),
    (dict(obstacle_model=0), "ERR_BAD_ARG", "MPPI_OBSTACLE_NONE"),        # (inherited from obstacle_motion)
    (dict(model=2), "ERR_UNSUPPORTED", "MPPI_MODEL_DIFFDRIVE_MLP"),
    (dict(T=129), "ERR_UNSUPPORTED", "T <= 128"),
    (dict(K=16384), "ERR_UNSUPPORTED", "K <= 8192"),
])
def test_create_refuses_before_the_device_is_looked_for(over, code, word):
    lib, capi, c = lib_and_config(**over)
    rc, msg = create(lib, capi, c)
    assert rc == getattr(capi, code), (rc, msg)
    assert word in msg, msg


def test_a_valid_fleet_config_passes_validation():
    """Past every refusal: the handle is made, or -- on a machine without an MI355X -- the device check is what stops it."""
    lib, capi, c = lib_and_config()
    rc, msg = create(lib, capi, c)
    assert rc in (capi.OK, capi.ERR_NO_DEVICE), (rc, msg)
    lib, capi, c = lib_and_config(n_agents=256, K=64)
    rc, msg = create(lib, capi, c)
    assert rc in (capi.OK, capi.ERR_NO_DEVICE), (rc, msg)


def test_zero_radius_is_off_whatever_else_is_set():
    lib, capi, c = lib_and_config(fleet_radius=0.0, n_agents=1, obstacle_motion=0)
    rc, msg = create(lib, capi, c)
    assert rc in (capi.OK, capi.ERR_NO_DEVICE), (rc, msg)


def test_entry_points_are_exported_and_prototyped():
    lib, capi, _ = lib_and_config()
    assert capi.ABI_VERSION == 8 and lib.mppi_abi_version() == 8
    for name in ("mppi_get_agent_circles", "mppi_get_fleet_clearance"):
        assert hasattr(lib, name) and name in capi.PROTOTYPES
        assert getattr(lib, name).argtypes == capi.PROTOTYPES[name][1]
    assert [f for f, _ in capi.MppiConfig._fields_][-3:] == ["obstacle_motion", "reserved0", "fleet_radius"]
    # a NULL handle is refused before anything is read
    m = C.c_int32(-7)
    assert lib.mppi_get_agent_circles(None, 0, None, None, 0, C.byref(m)) == capi.ERR_BAD_ARG and m.value == -7
    assert lib.mppi_get_fleet_clearance(None, None, None, 0) == capi.ERR_BAD_ARG


def test_config_size_serves_older_libraries():
    from dnn_mppi_mpc_amd import _capi as capi

    class Lib:
        def __init__(self, v):
            self.v = v

        def mppi_abi_version(self):
            return self.v
    full = C.sizeof(capi.MppiConfig)
    assert [capi.config_size(Lib(v)) for v in (6, 7, 8)] == [full - 16, full - 8, full]
    assert np.dtype(np.float64).itemsize == 8 and capi.MppiConfig.fleet_radius.offset == full - 8
