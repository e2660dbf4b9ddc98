"""CPU: the per-agent scene entry points (mppi_set_agent_ref_path, mppi_set_agent_obstacles, mppi_get_agent_status) refuse a
NULL handle with MPPI_ERR_BAD_ARG before they touch a device -- no GPU needed, no crash."""
import ctypes as C

import numpy as np


def test_agent_scene_calls_refuse_a_null_handle():
    import dnn_mppi_mpc_amd as pkg
    from dnn_mppi_mpc_amd import _capi as capi
    pkg.build_library()
    lib = capi.load_library()
    path = np.zeros((4, 3))
    circles = np.array([[1.0, 1.0, 0.5]])
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    idx, end = (C.c_int32 * 2)(), (C.c_int32 * 2)()
    assert lib.mppi_set_agent_ref_path(None, 0, dp(path), 4, 3) == capi.ERR_BAD_ARG
    assert lib.mppi_set_agent_obstacles(None, 0, dp(circles), 1) == capi.ERR_BAD_ARG
    assert lib.mppi_get_agent_status(None, idx, end) == capi.ERR_BAD_ARG
    assert lib.mppi_get_agent_status(None, None, None) == capi.ERR_BAD_ARG


def test_engine_setters_take_an_agent():
    """The Python layer's signature: `agent=None` means every agent."""
    import inspect

    import dnn_mppi_mpc_amd as pkg
    for name in ("set_ref_path", "set_obstacles"):
        p = inspect.signature(getattr(pkg.Engine, name)).parameters
        assert "agent" in p and p["agent"].default is None
    assert callable(pkg.Engine.agent_status)
