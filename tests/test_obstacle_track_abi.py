"""CPU: the three entry points of the obstacle tracks are declared, exported and prototyped, refuse a null handle before
anything else, and came without an ABI bump (tests/test_abi_symbols.py holds the export list to the header by itself)."""
import ctypes as C
import os

NAMES = ("mppi_set_obstacle_tracks", "mppi_set_agent_obstacle_tracks", "mppi_get_obstacle_tracks_at")


def lib_and_capi():
    import dnn_mppi_mpc_amd as pkg
    from dnn_mppi_mpc_amd import _capi as capi
    pkg.build_library()
    return capi.load_library(capi.LIB_PATH), capi


def test_symbols_are_exported_and_prototyped():
    lib, capi = lib_and_capi()
    i32, H, D = C.c_int32, capi._H, capi._D
    want = {"mppi_set_obstacle_tracks": [H, D, D, i32, i32], "mppi_set_agent_obstacle_tracks": [H, i32, D, D, i32, i32],
            "mppi_get_obstacle_tracks_at": [H, i32, i32, D, i32, C.POINTER(i32)]}
    for name in NAMES:
        assert capi.PROTOTYPES[name] == (C.c_int, want[name])
        assert hasattr(lib, name)


def test_header_declares_them():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "mppi_hip.h")).read()
    assert "int mppi_set_obstacle_tracks(mppi_handle *h, const double *xy, const double *radius, int32_t n, int32_t L);" in text
    assert ("int mppi_set_agent_obstacle_tracks(mppi_handle *h, int32_t agent, const double *xy, const double *radius, int32_t n, "
            "int32_t L);") in text
    assert ("int mppi_get_obstacle_tracks_at(mppi_handle *h, int32_t agent, int32_t step, double *xyr_out, int32_t cap, "
            "int32_t *n_out);") in text


def test_null_handles_are_refused_whatever_else_is_wrong():
    """The refusals that need no handle: NULL comes first, also with every other argument out of range."""
    lib, capi = lib_and_capi()
    xy, r = (C.c_double * 4)(0, 0, 1, 1), (C.c_double * 1)(0.4)
    n = C.c_int32(-7)
    for args in ((xy, r, 1, 2), (None, None, 1, 2), (xy, r, 257, 2), (xy, r, 1, 0), (xy, r, 1, 65537), (xy, r, -1, 2), (None, None, 0, 0)):
        assert lib.mppi_set_obstacle_tracks(None, *args) == capi.ERR_BAD_ARG
        assert lib.mppi_set_agent_obstacle_tracks(None, 0, *args) == capi.ERR_BAD_ARG
        assert lib.mppi_set_agent_obstacle_tracks(None, -3, *args) == capi.ERR_BAD_ARG
    out = (C.c_double * 3)(-1.0, -1.0, -1.0)
    assert lib.mppi_get_obstacle_tracks_at(None, 0, 0, out, 1, C.byref(n)) == capi.ERR_BAD_ARG
    assert lib.mppi_get_obstacle_tracks_at(None, 0, -1, None, 0, None) == capi.ERR_BAD_ARG
    assert n.value == -7 and list(out) == [-1.0, -1.0, -1.0]  # nothing was written


def test_the_abi_version_stays():
    lib, capi = lib_and_capi()
    assert capi.ABI_VERSION == 8 and lib.mppi_abi_version() == 8


def test_engine_and_controllers_carry_the_feature():
    import inspect
    import dnn_mppi_mpc_amd as pkg
    assert callable(pkg.Engine.set_obstacle_tracks) and callable(pkg.Engine.obstacle_tracks_at)
    for cls in (pkg.MPPIAlgorithms, pkg.MPPIRacecarController):
        assert "obstacle_tracks" in inspect.signature(cls.__init__).parameters
        assert isinstance(cls.obstacle_tracks, property)
