"""CPU: the two entry points of the composed scenes (mppi_set_scene_mode / mppi_get_scene_mode) are declared, exported and
prototyped, refuse a null handle before anything else, and came without an ABI bump or a change to mppi_config
(tests/test_abi_symbols.py holds the export list to the header by itself)."""
import ctypes as C
import os

from test_cost_grid_abi import CONFIG_FIELDS, lib_and_capi

NAMES = ("mppi_set_scene_mode", "mppi_get_scene_mode")


def test_symbols_are_exported_and_prototyped():
    lib, capi = lib_and_capi()
    i32, H = C.c_int32, capi._H
    want = {"mppi_set_scene_mode": [H, i32], "mppi_get_scene_mode": [H, C.POINTER(i32)]}
    for name in NAMES:
        assert capi.PROTOTYPES[name] == (C.c_int, want[name])
        assert hasattr(lib, name)


def test_header_declares_them_and_the_constants():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = " ".join(open(os.path.join(root, "include", "mppi_hip.h")).read().split())
    assert "int mppi_set_scene_mode(mppi_handle *h, int32_t mode);" in text
    assert "int mppi_get_scene_mode(const mppi_handle *h, int32_t *mode);" in text
    assert "#define MPPI_SCENE_EXCLUSIVE 0" in text and "#define MPPI_SCENE_COMPOSED 1" in text
    from dnn_mppi_mpc_amd import _capi as capi
    assert (capi.SCENE_EXCLUSIVE, capi.SCENE_COMPOSED) == (0, 1)


def test_null_handles_are_refused_whatever_else_is_wrong():
    lib, capi = lib_and_capi()
    mode = C.c_int32(-7)
    for m in (0, 1, 2, -1):
        assert lib.mppi_set_scene_mode(None, m) == capi.ERR_BAD_ARG
    assert lib.mppi_get_scene_mode(None, C.byref(mode)) == capi.ERR_BAD_ARG
    assert lib.mppi_get_scene_mode(None, None) == capi.ERR_BAD_ARG
    assert mode.value == -7  # nothing was written


def test_the_abi_version_and_the_config_stay():
    lib, capi = lib_and_capi()
    assert capi.ABI_VERSION == 8 and lib.mppi_abi_version() == 8
    assert [f[0] for f in capi.MppiConfig._fields_] == CONFIG_FIELDS and C.sizeof(capi.MppiConfig) == 296


def test_engine_and_controllers_carry_the_feature():
    import inspect
    import dnn_mppi_mpc_amd as pkg
    assert callable(pkg.Engine.set_scene_mode) and isinstance(pkg.Engine.scene_mode, property)
    for cls in (pkg.MPPIAlgorithms, pkg.MPPIRacecarController):
        params = inspect.signature(cls.__init__).parameters
        assert list(params)[-1] == "compose_scene" and params["compose_scene"].default is False
