"""CPU: what the callback controller's new models, terminal cost, options and two getters added to the C ABI -- declared,
exported and prototyped, NULL handles refused, the enum values, a config that grew at its end only (the struct_size handshake
tells the libraries apart, MPPI_ABI_VERSION stays 8), and the refusals that need no device."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mppi_cb_get_perturbed_actions", "mppi_cb_top_trajectories")
OLD_FIELDS = ["struct_size", "device", "dynamics", "obstacle_kind", "K", "T", "n_obs", "sample_null_action", "dt", "lambda_",
              "noise_sigma", "u_min", "u_max", "u_init", "goal", "q_diag", "r_diag", "obstacles", "safety_distance",
              "obstacle_weight", "skid_params", "seed"]
NEW_FIELDS = ["model_params", "terminal_cost", "noise_abs_cost", "terminal_goal", "terminal_q", "noise_mu", "u_scale"]
OLD_SIZE = 960  # sizeof(mppi_cb_config) before it grew: 8 int32, 115 doubles, one uint64


def lib_and_capi():
    import dnn_mppi_mpc_amd as pkg
    from dnn_mppi_mpc_amd import _capi as capi
    pkg.build_library()
    return capi.load_library(capi.LIB_PATH), capi


def header():
    return " ".join(open(os.path.join(ROOT, "include", "mppi_hip.h")).read().split())


def test_symbols_are_exported_prototyped_and_declared():
    lib, capi = lib_and_capi()
    want = {"mppi_cb_get_perturbed_actions": [capi._H, C.c_void_p, capi._D],
            "mppi_cb_top_trajectories": [capi._H, capi._D, C.c_void_p, C.c_int32, capi._D, C.POINTER(C.c_int32)]}
    for name in NAMES:
        assert capi.PROTOTYPES[name] == (C.c_int, want[name])
        assert hasattr(lib, name)
    text = header()
    assert "int mppi_cb_get_perturbed_actions(mppi_cb_handle *h, const float *eps, double *out);" in text
    assert ("int mppi_cb_top_trajectories(mppi_cb_handle *h, const double *state, const float *eps, int32_t n, double *traj_out, "
            "int32_t *index_out);") in text


def test_null_handles_are_refused_whatever_else_is_wrong():
    lib, capi = lib_and_capi()
    out = (C.c_double * 4)(-1.0, -1.0, -1.0, -1.0)
    idx = (C.c_int32 * 2)(-7, -7)
    state = (C.c_double * 5)()
    assert lib.mppi_cb_get_perturbed_actions(None, None, out) == capi.ERR_BAD_ARG
    assert lib.mppi_cb_get_perturbed_actions(None, None, None) == capi.ERR_BAD_ARG
    for n in (1, 0, -5, 1 << 30):
        assert lib.mppi_cb_top_trajectories(None, state, None, n, out, idx) == capi.ERR_BAD_ARG
    assert lib.mppi_cb_top_trajectories(None, None, None, 1, None, None) == capi.ERR_BAD_ARG
    assert lib.mppi_cb_eval(None, 2, state, None, 0, 1, out) == capi.ERR_BAD_ARG
    assert list(out) == [-1.0] * 4 and list(idx) == [-7, -7]  # nothing was written


def test_enum_values():
    text = header()
    for name, value in (("MPPI_CB_DYN_UNICYCLE", 0), ("MPPI_CB_DYN_SKID_STEER", 1), ("MPPI_CB_DYN_RACECAR", 2),
                        ("MPPI_CB_DYN_RACECAR_DYNAMIC", 3), ("MPPI_CB_DYN_DOUBLE_INTEGRATOR", 4)):
        assert re.search(rf"\b{name} = {value}\b", text), name
    from dnn_mppi_mpc_amd.callback_mppi import DYNAMICS
    assert DYNAMICS == {"unicycle": (0, 3, 2), "skid_steer": (1, 5, 4), "racecar": (2, 4, 2), "racecar_dynamic": (3, 4, 2),
                        "double_integrator": (4, 2, 1)}


def test_the_abi_version_stays_and_the_config_grew_at_its_end_only():
    lib, capi = lib_and_capi()
    from dnn_mppi_mpc_amd.callback_mppi import MppiCbConfig
    assert capi.ABI_VERSION == 8 and lib.mppi_abi_version() == 8
    names = [f[0] for f in MppiCbConfig._fields_]
    assert names == OLD_FIELDS + NEW_FIELDS
    assert MppiCbConfig.seed.offset + 8 == OLD_SIZE == MppiCbConfig.model_params.offset
    # the header through a C compiler: size and the offset of every new field against the mirror
    probes = ", ".join(f"offsetof(mppi_cb_config, {n})" for n in ["seed"] + NEW_FIELDS)
    fmt = " ".join(["%zu"] * (len(NEW_FIELDS) + 2))
    src = f'#include <stdio.h>\n#include <stddef.h>\n#include "mppi_hip.h"\nint main(){{printf("{fmt}", sizeof(mppi_cb_config), {probes});}}'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")])
        got = [int(v) for v in subprocess.check_output([os.path.join(d, "t")]).decode().split()]
    assert got[0] == C.sizeof(MppiCbConfig)
    assert got[1:] == [getattr(MppiCbConfig, n).offset for n in ["seed"] + NEW_FIELDS]


def test_a_config_of_the_old_size_is_refused_by_the_handshake():
    lib, capi = lib_and_capi()
    from dnn_mppi_mpc_amd.callback_mppi import MppiCbConfig
    c = MppiCbConfig()
    c.struct_size = OLD_SIZE
    h = C.c_void_p()
    assert lib.mppi_cb_create(C.byref(c), C.byref(h)) == capi.ERR_BAD_ARG and not h.value
    assert b"struct_size" in lib.mppi_cb_last_error(None)


def test_refusals_that_need_no_device():
    """rollout_samples / rollout_var_cost stay NotImplementedError and say why; "bicycle" stays a ValueError; u_scale = 0 and
    u_per_command outside [1, T] are ValueErrors; a non-positive wheelbase, l_r or mass and a u_scale of 0 or NaN handed to the
    library itself are MPPI_ERR_BAD_ARG before a device is looked for."""
    import dnn_mppi_mpc_amd as pkg
    from dnn_mppi_mpc_amd import _capi as capi
    from dnn_mppi_mpc_amd.callback_mppi import MPPI, RunningCost, TerminalCost
    rc, sig = RunningCost.racecar(), np.diag([0.05, 0.05])
    with pytest.raises(NotImplementedError, match="deterministic"):
        MPPI("racecar", rc, 4, sig, rollout_samples=2)
    with pytest.raises(NotImplementedError, match="deterministic"):
        MPPI("racecar", rc, 4, sig, rollout_var_cost=0.5)
    with pytest.raises(ValueError):
        MPPI("bicycle", rc, 4, sig)
    for kw in (dict(u_scale=0), dict(u_scale=float("nan")), dict(u_scale=float("inf")), dict(u_per_command=0),
               dict(u_per_command=16, horizon=15), dict(u_per_command=1.5), dict(terminal_state_cost=lambda s: 0),
               dict(terminal_state_cost=TerminalCost.double_integrator())):  # (two components for a model of four)
        with pytest.raises(ValueError):
            MPPI("racecar", rc, 4, sig, **kw)
    for dyn, params in (("racecar", [0.0]), ("racecar", [-0.3]), ("racecar", [float("nan")]),
                        ("racecar_dynamic", [0.0, 1.0, 1000.0, 1000.0, 1000.0]), ("racecar_dynamic", [1.5, 1.0, -1.0, 1000.0, 1000.0])):
        cost = RunningCost.racecar() if dyn == "racecar" else RunningCost.racecar_dynamic()
        with pytest.raises(pkg.MppiError) as e:
            MPPI(dyn, cost, 4, sig, model_params=params)
        assert e.value.code == capi.ERR_BAD_ARG, (dyn, params)
    lib = capi.load_library(capi.LIB_PATH)
    from dnn_mppi_mpc_amd.callback_mppi import MppiCbConfig
    for bad in (0.0, float("nan"), float("-inf")):
        c = MppiCbConfig()
        c.struct_size, c.dynamics, c.K, c.T, c.dt, c.lambda_, c.u_scale = C.sizeof(MppiCbConfig), 4, 8, 4, 0.1, 1.0, bad
        c.noise_sigma[0] = 0.5
        h = C.c_void_p()
        assert lib.mppi_cb_create(C.byref(c), C.byref(h)) == capi.ERR_BAD_ARG and not h.value
        assert b"u_scale" in lib.mppi_cb_last_error(None)


def test_presets_carry_the_scripts_numbers():
    from dnn_mppi_mpc_amd.callback_mppi import DEFAULT_DT, MODEL_PARAMS, RunningCost, TerminalCost
    import callback_models_checks as cm
    for dyn, make in (("racecar", RunningCost.racecar), ("racecar_dynamic", RunningCost.racecar_dynamic),
                      ("double_integrator", RunningCost.double_integrator)):
        rc, want = make(), cm.cost_of(dyn)
        np.testing.assert_array_equal(rc.goal, want["goal"])
        np.testing.assert_array_equal(rc.q_diag, want["q"])
        np.testing.assert_array_equal(rc.r_diag, want["r"])
        np.testing.assert_array_equal(rc.obstacles, want["obstacles"])
        assert (rc.safety_distance, rc.obstacle_weight, rc.kind) == (want["safety"], want["weight"], want["kind"])
        assert DEFAULT_DT[dyn] == cm.DT[dyn]
        assert tuple(MODEL_PARAMS.get(dyn, ())) == tuple(cm.MODEL[dyn].values())
    t = TerminalCost.double_integrator()
    np.testing.assert_array_equal(t.goal, [0, 0])
    np.testing.assert_array_equal(t.q_diag, [1, 1])
