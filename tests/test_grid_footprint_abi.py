"""CPU: the three entry points of the cost-grid footprint are declared, exported and prototyped, refuse a null handle (and a null
out-pointer) before anything else, and came without an ABI bump or a change to mppi_config; the Python surface carries them."""
import ctypes as C
import os

from test_cost_grid_abi import CONFIG_FIELDS, lib_and_capi

NAMES = ("mppi_set_cost_grid_footprint", "mppi_get_cost_grid_footprint", "mppi_eval_cost_grid_footprint")


def test_symbols_are_exported_and_prototyped():
    lib, capi = lib_and_capi()
    i32, H, D = C.c_int32, capi._H, capi._D
    want = {"mppi_set_cost_grid_footprint": [H, i32], "mppi_get_cost_grid_footprint": [H, C.POINTER(i32)],
            "mppi_eval_cost_grid_footprint": [H, i32, D, i32, D, D]}
    for name in NAMES:
        assert capi.PROTOTYPES[name] == (C.c_int, want[name])
        assert hasattr(lib, name)
    assert (capi.GRID_FOOTPRINT_CENTRE, capi.GRID_FOOTPRINT_OUTLINE) == (0, 1)


def test_header_declares_them():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = " ".join(open(os.path.join(root, "include", "mppi_hip.h")).read().split())
    assert "#define MPPI_GRID_FOOTPRINT_CENTRE 0" in text and "#define MPPI_GRID_FOOTPRINT_OUTLINE 1" in text
    assert "int mppi_set_cost_grid_footprint(mppi_handle *h, int32_t mode);" in text
    assert "int mppi_get_cost_grid_footprint(const mppi_handle *h, int32_t *mode);" in text
    assert ("int mppi_eval_cost_grid_footprint(mppi_handle *h, int32_t agent, const double *pose, int32_t n, double *value, "
            "double *points);") in text
    # the semantics the tests hold the device to are written down: the order of the rotation, the fold, the refusals
    for words in ("px = fma(qx, cs, fma(-qy, sn, x))", "py = fma(qx, sn, fma(qy, cs, y))", "g_foot = fmax over q",
                  "inflating the map by its radius", "(-a, 0), (-a, b), (0, b), (a, b), (a, 0), (a, -b), (0, -b), (-a, -b)"):
        assert words in text, words


def test_null_pointers_are_refused_whatever_else_is_wrong():
    lib, capi = lib_and_capi()
    for mode in (0, 1, 2, -7):
        assert lib.mppi_set_cost_grid_footprint(None, mode) == capi.ERR_BAD_ARG
    m = C.c_int32(-5)
    assert lib.mppi_get_cost_grid_footprint(None, C.byref(m)) == capi.ERR_BAD_ARG
    assert lib.mppi_get_cost_grid_footprint(None, None) == capi.ERR_BAD_ARG
    assert m.value == -5  # nothing was written
    pose = (C.c_double * 3)(0, 0, 0)
    out = (C.c_double * 1)(-1.0)
    pts = (C.c_double * 18)(*([-1.0] * 18))
    assert lib.mppi_eval_cost_grid_footprint(None, 0, pose, 1, out, pts) == capi.ERR_BAD_ARG
    assert lib.mppi_eval_cost_grid_footprint(None, -1, None, 0, None, None) == capi.ERR_BAD_ARG
    assert list(out) == [-1.0] and list(pts) == [-1.0] * 18


def test_the_abi_version_and_the_config_stay():
    lib, capi = lib_and_capi()
    assert capi.ABI_VERSION == 8 and lib.mppi_abi_version() == 8
    assert [f[0] for f in capi.MppiConfig._fields_] == CONFIG_FIELDS and C.sizeof(capi.MppiConfig) == 296


def test_engine_and_controllers_carry_the_feature():
    import inspect
    import dnn_mppi_mpc_amd as pkg
    assert callable(pkg.Engine.set_cost_grid_footprint) and callable(pkg.Engine.cost_grid_footprint_at)
    assert isinstance(pkg.Engine.cost_grid_footprint, property)
    sig = inspect.signature(pkg.Engine.cost_grid_footprint_at).parameters
    assert list(sig)[1:] == ["poses", "agent", "points"] and sig["agent"].default == 0 and sig["points"].default is False
    for cls in (pkg.MPPIAlgorithms, pkg.MPPIRacecarController):
        params = list(inspect.signature(cls.__init__).parameters)
        assert params[-1] == "compose_scene" and "footprint" not in params  # the key lives in the cost_grid mapping
        assert "footprint" in cls.cost_grid.__doc__
