"""The mesh binding of the convolutional path (psm_unet_mesh_*, psm_unet_solve*) at the C boundary, without a GPU: every new
prototype of include/psm_unet.h is bound by _lib.py and exported by the built library, PSM_ABI_VERSION is still 4, a C99 file that
includes the header can take the address of each (tests/native/abi_c_check_unet_solve.c), psm_unet_canvas_shape gives the canvas of
the test networks and of the reference's 400 x 3000 grid, a NULL handle is refused by every entry, and the Python mirrors refuse bad
arguments before any library call."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from psm_amd import UNetSolverEnsemble, UNetSolverModule, _lib, unet_solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("psm_unet_canvas_shape", "psm_unet_mesh_create", "psm_unet_mesh_destroy", "psm_unet_mesh_last_error",
               "psm_unet_mesh_set_geometry", "psm_unet_solve", "psm_unet_solve_device", "psm_unet_mesh_prime", "psm_unet_mesh_reset",
               "psm_unet_mesh_state", "psm_unet_mesh_read")


def test_new_entries_are_declared_bound_and_exported():
    txt = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_UNET).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(psm_[a-z_0-9]+)\s*\(", txt)))
    assert declared == sorted(_lib.SIGNATURES_UNET)         # the header and the binding agree, name for name
    lib = _lib.load()
    for name in NEW_ENTRIES:
        assert name in declared and name in _lib.SIGNATURES_UNET and hasattr(lib, name), name
    assert _lib.PSM_ABI_VERSION == 4 and lib.psm_abi_version() == 4
    for macro, value in (("PSM_UNET_STEP_ABSOLUTE", _lib.UNET_STEPS["absolute"]), ("PSM_UNET_STEP_DELTA", _lib.UNET_STEPS["delta"]),
                         ("PSM_UNET_READ_CANVAS", _lib.UNET_READ["canvas"]), ("PSM_UNET_READ_FIELD", _lib.UNET_READ["field"]),
                         ("PSM_UNET_READ_UMAX", _lib.UNET_READ["umax"])):
        assert re.search(rf"#define\s+{macro}\s+{value}\b", txt), macro
    assert "BUILD-DEFINED" in open(_lib.HEADER_UNET).read()   # the header says that the padding rule has no reference


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_header_compiles_as_c99_with_the_mesh_entries(tmp_path):
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                        os.path.join(ROOT, "tests", "native", "abi_c_check_unet_solve.c"), "-o", str(tmp_path / "a.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("levels, grid, canvas", [(4, (138, 300), (144, 304)), (3, (138, 300), (140, 300)), (2, (138, 300), (138, 300)),
                                                  (5, (400, 3000), (400, 3008)), (4, (400, 3000), (400, 3000)), (2, (1, 1), (2, 2))])
def test_canvas_shape(levels, grid, canvas):
    lib = _lib.load()
    a, b = C.c_int32(-1), C.c_int32(-1)
    assert lib.psm_unet_canvas_shape(levels, *grid, C.byref(a), C.byref(b)) == 0
    assert (a.value, b.value) == canvas == unet_solver.canvas_shape(levels, *grid)
    assert a.value % 2 ** (levels - 1) == 0 and b.value % 2 ** (levels - 1) == 0
    assert 0 <= a.value - grid[0] < 2 ** (levels - 1) and 0 <= b.value - grid[1] < 2 ** (levels - 1)


def test_canvas_shape_refuses_bad_arguments():
    lib = _lib.load()
    a, b = C.c_int32(), C.c_int32()
    for levels, ny, nx in ((1, 8, 8), (8, 8, 8), (3, 0, 8), (3, 8, -1)):
        assert lib.psm_unet_canvas_shape(levels, ny, nx, C.byref(a), C.byref(b)) == -1
    assert lib.psm_unet_canvas_shape(3, 8, 8, None, C.byref(b)) == -1
    with pytest.raises(ValueError):
        unet_solver.canvas_shape(1, 8, 8)


def test_null_handle_is_refused_by_every_entry():
    lib = _lib.load()
    out = C.c_void_p(1)
    assert lib.psm_unet_mesh_create(None, 0, 144, 304, 1, 0, C.byref(out)) == -1 and not out.value
    assert b"null" in lib.psm_unet_mesh_last_error(None)
    assert lib.psm_unet_mesh_create(None, 0, 144, 304, 1, 0, None) == -1
    lib.psm_unet_mesh_destroy(None)
    n = (C.c_int64 * 1)(10)
    none = (C.c_void_p * 1)(None)
    assert lib.psm_unet_mesh_set_geometry(None, 1, n, 4, 4, none, none, none, none, none, none, None, 0, 0, 0.05) == -1
    assert lib.psm_unet_solve(None, None, None) == -1
    assert lib.psm_unet_solve_device(None, None, None, None) == -1
    assert lib.psm_unet_mesh_prime(None, None) == -1
    assert lib.psm_unet_mesh_reset(None) == -1
    assert lib.psm_unet_mesh_state(None, None, None) == -1
    assert lib.psm_unet_mesh_read(None, 0, None, 0) == -1


def test_python_argument_checks_come_before_any_library_call():
    """The mirrors refuse bad arguments on objects that hold no network and no binding: any call into the library would raise
    AttributeError instead."""
    for cls in (UNetSolverModule, UNetSolverEnsemble):
        with pytest.raises(ValueError, match="step"):
            cls(None, step="relative")
        with pytest.raises(ValueError, match="geometry"):
            cls(None, geometry="qhull")
        with pytest.raises(ValueError, match="precision"):
            cls(None, precision="fp8")
        for maxs in ((1.0, 1.0, 1.0), (1.0,) * 5):
            with pytest.raises(ValueError, match="maxs"):
                cls(None, maxs=maxs)
        assert cls(None).step == "absolute" and cls(None, step="delta").step == "delta"
        for name in ("init_func", "py_func", "prime", "reset_state", "read", "close"):
            assert callable(getattr(cls, name, None)), (cls, name)
        assert isinstance(cls.state, property)
    with pytest.raises(ValueError, match="max_cases"):
        UNetSolverEnsemble(None, max_cases=0)
    sm = UNetSolverModule(None, step="delta")
    for call in (lambda: sm.py_func(np.zeros((4, 5))), lambda: sm.prime(np.zeros((4, 5))), sm.reset_state, lambda: sm.state, lambda: sm.read("canvas")):
        with pytest.raises(RuntimeError, match="init_func"):
            call()
    sm.tables, sm.cell_off = "native", [0, 4]               # as after init_func; the binding stays None
    for bad in (np.zeros((4, 4)), np.zeros(20), np.zeros((2, 2, 5)), np.zeros((5, 5))):
        for call in (sm.py_func, sm.prime):
            with pytest.raises(ValueError, match=r"\[N,5\]"):
                call(bad)
    for out in (np.zeros(4, np.float32), np.zeros(5), np.zeros((4, 2))[:, 0], [0.0] * 4):
        with pytest.raises(ValueError, match="out"):
            sm.py_func(np.zeros((4, 5)), out=out)
    sm.tables = None                                        # nothing to close
    absolute = UNetSolverModule(None)
    absolute.tables, absolute.cell_off = "native", [0, 4]
    for call in (lambda: absolute.prime(np.zeros((4, 5))), absolute.reset_state, lambda: absolute.state):
        with pytest.raises(RuntimeError, match="step='delta'"):
            call()
    absolute.tables = None
    ens = UNetSolverEnsemble(None, step="delta", max_cases=2)
    with pytest.raises(ValueError, match="per case"):
        ens.init_func([np.zeros((4, 5))] * 3, [None] * 3, [None] * 3)      # more than max_cases
    with pytest.raises(RuntimeError, match="init_func"):
        ens.py_func([np.zeros((4, 5))])
    ens.tables, ens.cell_off = "native", [0, 4, 7]
    with pytest.raises(ValueError, match="2 cases"):
        ens.prime([np.zeros((4, 5))])
    with pytest.raises(ValueError, match=r"\[N,5\]"):
        ens.py_func([np.zeros((4, 5)), np.zeros((3, 4))])
    ens.tables = None
