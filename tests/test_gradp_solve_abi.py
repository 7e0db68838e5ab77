"""The gradient-model step at the solver boundary (psm_solve_gradp*, psm_solve_cases_gradp*) at the C boundary, without a GPU: every
new prototype of include/psm.h is bound by _lib.py and exported by the built library, PSM_ABI_VERSION is still 4, a C99 file that
includes the header can take the address of each (tests/native/abi_c_check_gradp_solve.c), a NULL handle is refused by every entry,
and the Python mirrors ``SolverModule(step="gradp")`` / ``SolverEnsemble(step="gradp")`` refuse bad arguments before any library call."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from psm_amd import GridSurrogate, SolverEnsemble, SolverModule, _lib, solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("psm_bind_gradp_solve", "psm_bind_gradp_solve_cases", "psm_unbind_gradp_solve", "psm_solve_gradp", "psm_solve_gradp_device",
               "psm_solve_cases_gradp", "psm_solve_cases_gradp_device")
NEW_METHODS = ("bind_gradp_solve", "bind_gradp_solve_cases", "unbind_gradp_solve", "solve_gradp", "solve_gradp_device", "solve_cases_gradp",
               "solve_cases_gradp_device")
MAXS5 = (2.5, 0.6, 0.35, 40.0, 25.0)


def test_new_entries_are_declared_bound_and_exported():
    raw = open(_lib.HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(psm_[a-z_0-9]+)\s*\(", txt))
    lib = _lib.load()
    for name in NEW_ENTRIES:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert re.search(r"#define\s+PSM_GRADP_REF_NONE\s+0\b", txt) and re.search(r"#define\s+PSM_GRADP_REF_OUTLET\s+1\b", txt)
    assert GridSurrogate.GRADP_REFERENCES == {"none": 0, "outlet": 1}
    assert re.search(r"#define\s+PSM_ABI_VERSION\s+4\b", txt) and _lib.PSM_ABI_VERSION == 4 and lib.psm_abi_version() == 4
    for name in NEW_METHODS:
        assert callable(getattr(GridSurrogate, name, None)), name
    assert "gradp" in solver.MODULE_STEPS
    for cls in (SolverModule, SolverEnsemble):
        obj = cls(None, MAXS5, step="gradp")
        assert obj.step == "gradp" and obj.reference == "outlet" and obj.cut is None and obj.apply_filter is False
        assert callable(obj.py_func) and callable(obj.init_func)
    # the header says what the step does not provide
    comment = raw[raw.index("the gradient-model step at the solver boundary"):raw.index("#define PSM_GRADP_REF_NONE")]
    for word in ("_begin / _end", "psm_pin_buffers", "no atomics", "PSM_ERR_UNSUPPORTED"):
        assert word in comment, word


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_header_compiles_as_c99_with_the_gradp_solve_entries(tmp_path):
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                        os.path.join(ROOT, "tests", "native", "abi_c_check_gradp_solve.c"), "-o", str(tmp_path / "a.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_null_handle_is_refused_by_every_entry():
    lib = _lib.load()
    assert lib.psm_bind_gradp_solve(None, 50, 40, 0.005, 0.005, 1.5, 0.7, None, 0, 1) == -1
    assert lib.psm_bind_gradp_solve_cases(None, None, None, 0.005, 0.005, 1.5, 0.7, None, 0, 1) == -1
    assert lib.psm_unbind_gradp_solve(None) == -1
    assert lib.psm_solve_gradp(None, None, 0, 0, None) == -1
    assert lib.psm_solve_gradp_device(None, None, None, None, None, None, None, None) == -1
    assert lib.psm_solve_cases_gradp(None, None, None) == -1
    assert lib.psm_solve_cases_gradp_device(None, None, None, None, None, None, None, None) == -1


def test_python_argument_checks_come_before_any_library_call():
    """The mirrors refuse bad arguments on objects whose surrogate does not exist: any call into the library would raise
    AttributeError instead.  prime, reset_state, state and the begin / end halves raise for this step."""
    for cls in (SolverModule, SolverEnsemble):
        with pytest.raises(ValueError, match=r"step='gradp'.*five maxs"):
            cls(None, maxs=(1.0, 1.0, 1.0, 1.0), step="gradp")
        with pytest.raises(ValueError, match="reference"):
            cls(None, maxs=MAXS5, step="gradp", reference="inlet")
        with pytest.raises(ValueError, match="step"):
            cls(None, step="relative")
    sm = SolverModule(None, MAXS5, step="gradp", cut=(50, 40), reference="none", apply_filter=True)
    assert sm.cut == (50, 40) and sm.reference == "none" and sm.apply_filter is True
    with pytest.raises(RuntimeError, match="init_func"):
        sm.py_func(np.zeros((4, 5)))
    ens = SolverEnsemble(None, MAXS5, 4, step="gradp")
    with pytest.raises(RuntimeError, match="init_func"):
        ens.py_func([np.zeros((4, 5))])
    sm.tables, ens.tables, ens.cell_off = "native", "native", [0, 4, 7]          # as after init_func; _sur stays None
    one, two = np.zeros((4, 5)), [np.zeros((4, 5)), np.zeros((3, 5))]
    for call in (lambda: sm.prime(one), sm.reset_state, lambda: sm.state, lambda: ens.prime(two), ens.reset_state, lambda: ens.state):
        with pytest.raises(RuntimeError, match=r"step='gradp' has no state"):
            call()
    for call in (lambda: sm.py_func_begin(one), sm.py_func_end, lambda: ens.py_func_begin(two), ens.py_func_end):
        with pytest.raises(RuntimeError, match=r"step='gradp' has no begin / end"):
            call()
    with pytest.raises(ValueError, match=r"\[N,5\]"):
        sm.py_func(np.zeros((4, 4)))
    with pytest.raises(ValueError, match="2 cases"):
        ens.py_func([one])
    # the Poisson step keeps its default filter
    assert SolverModule(None, (2.7, 0.004, 0.004, 0.35, 0.005), step="poisson", phi=0.16, k=0.5).apply_filter is True


def test_default_cut_rule():
    """cut=None: center_y is the middle row, rounded up, of the rows that hold a zero of sdfunct off the grid's rim; center_x is the
    rule of Eval_dual_Dense_onlycil.py:599 on that row."""
    ny, nx, delta = 60, 80, 0.01
    sd = np.full((ny, nx), 0.1)
    sd[0, :] = 0.0; sd[:, -1] = 0.0                       # rim cells outside the mesh's hull
    sd[20:31, 30:41] = 0.0                                 # the obstacle: rows 20 .. 30, columns 30 .. 40
    a = np.zeros((4, 5))
    a[:, 2] = (0.0, 0.8, 0.0, 0.8); a[:, 3] = (0.0, 0.0, 0.6, 0.6)
    dx, dy, extents, x_min = solver.gradp_grid_metrics(a, ny, nx)
    xl = np.linspace(0.0, 0.8, nx)
    assert dx == float(np.diff(xl)[0]) and dy == float(np.diff(np.linspace(0.0, 0.6, ny))[0]) and extents == (0.8, 0.6) and x_min == 0.0
    cy, cx = solver.gradp_default_cut(sd, a, delta)
    solid = sd[25] == 0
    assert cy == 25 and cx == int(((xl[solid].max() + xl[solid].min()) / 2 - delta / 2) / delta)
    sd[31, 30:41] = 0.0                                    # an even number of rows: rounded up
    assert solver.gradp_default_cut(sd, a, delta)[0] == 26
    with pytest.raises(ValueError, match="no solid cell"):
        solver.gradp_default_cut(np.full((ny, nx), 0.1), a, delta)
