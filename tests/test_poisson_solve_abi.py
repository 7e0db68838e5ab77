"""The entries of the Poisson-model step at the solver boundary at the C boundary, without a GPU: every new prototype of
include/psm.h is bound by _lib.py and exported by the built library, PSM_ABI_VERSION is still 4, a C99 file that includes the header
can take the address of each (tests/native/abi_c_check_poisson_solve.c), a NULL handle is refused by every entry, and the Python
mirrors refuse bad arguments before any library call."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from psm_amd import GridSurrogate, SolverEnsemble, SolverModule, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("psm_bind_poisson_solve", "psm_unbind_poisson_solve", "psm_poisson_solve_push", "psm_poisson_solve_reset",
               "psm_poisson_solve_state", "psm_solve_poisson", "psm_solve_poisson_device")
NEW_METHODS = ("bind_poisson_solve", "unbind_poisson_solve", "poisson_solve_push", "poisson_solve_reset", "solve_poisson",
               "solve_poisson_device")
MAXS5 = (2.7, 0.004, 0.004, 0.35, 0.005)


def test_new_entries_are_declared_bound_and_exported():
    raw = open(_lib.HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(psm_[a-z_0-9]+)\s*\(", txt))
    lib = _lib.load()
    for name in NEW_ENTRIES:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert re.search(r"#define\s+PSM_ABI_VERSION\s+4\b", txt) and _lib.PSM_ABI_VERSION == 4 and lib.psm_abi_version() == 4
    for name in NEW_METHODS:
        assert callable(getattr(GridSurrogate, name, None)), name
    assert isinstance(GridSurrogate.poisson_solve_state, property)
    # the header says what this entry does not provide
    comment = raw[raw.index("the Poisson-model step at the solver boundary"):raw.index("int psm_bind_poisson_solve")]
    for word in ("_begin / _end", "psm_pin_buffers", "case sets"):
        assert word in comment, word


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_header_compiles_as_c99_with_the_poisson_solve_entries(tmp_path):
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                        os.path.join(ROOT, "tests", "native", "abi_c_check_poisson_solve.c"), "-o", str(tmp_path / "a.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_null_handle_is_refused_by_every_entry():
    lib = _lib.load()
    assert lib.psm_bind_poisson_solve(None, 0.16, 0.005, 1, 1) == -1
    assert lib.psm_unbind_poisson_solve(None) == -1
    assert lib.psm_poisson_solve_push(None, None, 1) == -1
    assert lib.psm_poisson_solve_reset(None) == -1
    assert lib.psm_poisson_solve_state(None, None, None) == -1
    assert lib.psm_solve_poisson(None, None, 1, 0, None) == -1
    assert lib.psm_solve_poisson_device(None, None, None, None, None, None) == -1


def test_python_argument_checks_come_before_any_library_call():
    """The mirror refuses bad arguments on objects whose surrogate does not exist: any call into the library would raise
    AttributeError instead."""
    with pytest.raises(ValueError, match="five maxs"):
        SolverModule(None, maxs=(1.0, 1.0, 1.0, 1.0), step="poisson", phi=0.16, k=0.5)
    with pytest.raises(ValueError, match="phi and k"):
        SolverModule(None, maxs=MAXS5, step="poisson")
    with pytest.raises(ValueError, match="step"):
        SolverModule(None, step="relative")
    with pytest.raises(ValueError, match="step"):
        SolverEnsemble(None, step="poisson")                # no case-batch form
    sm = SolverModule(None, maxs=MAXS5, step="poisson", phi=0.16, k=0.5)
    assert sm.step == "poisson" and sm.weighting and sm.apply_filter and sm.sigma_field == (10, 10) and sm.sigma_weight == (50, 50)
    for call in (lambda: sm.py_func(np.zeros((4, 5))), lambda: sm.prime(np.zeros((4, 5))), sm.reset_state, lambda: sm.state):
        with pytest.raises(RuntimeError, match="init_func"):
            call()
    sm.tables = "native"                                    # as after init_func; _sur stays None
    for bad in (np.zeros((4, 4)), np.zeros(20), np.zeros((2, 2, 5))):
        for call in (sm.py_func, sm.prime):
            with pytest.raises(ValueError, match=r"\[N,5\]"):
                call(bad)
    with pytest.raises(ValueError, match="out"):
        sm.py_func(np.zeros((4, 5)), out=np.zeros(4, np.float32))
    with pytest.raises(RuntimeError, match="begin / end"):
        sm.py_func_begin(np.zeros((4, 5)))
