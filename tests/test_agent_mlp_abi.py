"""CPU: the per-agent model entry points (mppi_set_agent_mlp, mppi_set_agent_mlp_scaled) refuse a NULL handle with
MPPI_ERR_BAD_ARG before they touch a device -- no GPU needed, no crash -- and Engine.set_mlp takes an agent."""
import ctypes as C

import numpy as np


def test_agent_mlp_calls_refuse_a_null_handle():
    import dnn_mppi_mpc_amd as pkg
    from dnn_mppi_mpc_amd import _capi as capi
    pkg.build_library()
    lib = capi.load_library()
    H, n = 64, 1
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    w_in, b_in = np.zeros((H, 5), np.float32), np.zeros(H, np.float32)
    w_h, b_h = np.zeros((H, H), np.float32), np.zeros(H, np.float32)
    w_out, b_out = np.zeros((3, H), np.float32), np.zeros(3, np.float32)
    PP = C.POINTER(C.c_float) * n
    args = (H, n, fp(w_in), fp(b_in), PP(fp(w_h)), PP(fp(b_h)), fp(w_out), fp(b_out))
    assert lib.mppi_set_agent_mlp(None, 0, *args) == capi.ERR_BAD_ARG
    m5, s5, m3, s3 = np.zeros(5), np.ones(5), np.zeros(3), np.ones(3)
    assert lib.mppi_set_agent_mlp_scaled(None, 0, *args, dp(m5), dp(s5), dp(m3), dp(s3)) == capi.ERR_BAD_ARG
    assert lib.mppi_set_agent_mlp_scaled(None, 0, *args, None, None, None, None) == capi.ERR_BAD_ARG


def test_engine_set_mlp_takes_an_agent():
    """The Python layer's signature: `agent=None` means every agent, as in set_ref_path."""
    import inspect

    import dnn_mppi_mpc_amd as pkg
    p = inspect.signature(pkg.Engine.set_mlp).parameters
    assert "agent" in p and p["agent"].default is None
    assert list(p)[:3] == ["self", "weights", "scalers"]  # (the positional order callers already use)
