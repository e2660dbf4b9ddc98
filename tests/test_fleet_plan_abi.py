"""CPU: the two entry points of the fleet's plan mode are exported and prototyped, refuse a null handle before anything else,
and came without an ABI bump (tests/test_abi_symbols.py holds the export list to the header by itself)."""
import ctypes as C


def lib_and_capi():
    import dnn_mppi_mpc_amd as pkg
    from dnn_mppi_mpc_amd import _capi as capi
    pkg.build_library()
    return capi.load_library(capi.LIB_PATH), capi


def test_symbols_are_exported_and_prototyped():
    lib, capi = lib_and_capi()
    for name, args in (("mppi_set_fleet_prediction", [capi._H, C.c_int32]), ("mppi_get_fleet_plans", [capi._H, capi._D])):
        assert name in capi.PROTOTYPES
        assert capi.PROTOTYPES[name] == (C.c_int, args)
        assert hasattr(lib, name)
    assert (capi.FLEET_VELOCITY, capi.FLEET_PLAN) == (0, 1)


def test_null_handles_are_refused():
    lib, capi = lib_and_capi()
    assert lib.mppi_set_fleet_prediction(None, 1) == capi.ERR_BAD_ARG
    assert lib.mppi_get_fleet_plans(None, None) == capi.ERR_BAD_ARG


def test_the_abi_version_stays():
    lib, capi = lib_and_capi()
    assert capi.ABI_VERSION == 8 and lib.mppi_abi_version() == 8


def test_header_declares_the_modes():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "mppi_hip.h")).read()
    assert re.search(r"#define\s+MPPI_FLEET_VELOCITY\s+0\b", text) and re.search(r"#define\s+MPPI_FLEET_PLAN\s+1\b", text)
    assert "int mppi_set_fleet_prediction(mppi_handle *h, int32_t mode);" in text
    assert "int mppi_get_fleet_plans(mppi_handle *h, double *xy);" in text
