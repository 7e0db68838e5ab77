"""The case-set entries of the Poisson-model step at the solver boundary at the C boundary, without a GPU: every new prototype of
include/psm.h is bound by _lib.py and exported by the built library, PSM_ABI_VERSION is still 4, a C99 file that includes the header
can take the address of each (tests/native/abi_c_check_poisson_cases.c), a NULL handle is refused by every entry, and the Python
mirror ``SolverEnsemble(step="poisson")`` refuses bad arguments before any library call."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from psm_amd import GridSurrogate, SolverEnsemble, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("psm_bind_poisson_solve_cases", "psm_poisson_solve_push_cases", "psm_solve_cases_poisson", "psm_solve_cases_poisson_device")
NEW_METHODS = ("bind_poisson_solve_cases", "poisson_solve_push_cases", "solve_cases_poisson", "solve_cases_poisson_device")
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
    # the header says what the case-set entries do not provide
    comment = raw[raw.index("int psm_solve_poisson_device"):raw.index("int psm_bind_poisson_solve_cases")]
    for word in ("_begin / _end", "psm_pin_buffers", "ONE frame counter"):
        assert word in comment, word


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_header_compiles_as_c99_with_the_poisson_cases_entries(tmp_path):
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                        os.path.join(ROOT, "tests", "native", "abi_c_check_poisson_cases.c"), "-o", str(tmp_path / "a.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_null_handle_is_refused_by_every_entry():
    lib = _lib.load()
    assert lib.psm_bind_poisson_solve_cases(None, 0.16, 0.005, 1, 1) == -1
    assert lib.psm_poisson_solve_push_cases(None, None) == -1
    assert lib.psm_solve_cases_poisson(None, None, None) == -1
    assert lib.psm_solve_cases_poisson_device(None, None, None, None, None, None) == -1


def test_python_argument_checks_come_before_any_library_call():
    """The mirror refuses bad arguments on objects whose surrogate does not exist: any call into the library would raise
    AttributeError instead."""
    with pytest.raises(ValueError, match=r"step='poisson'.*five maxs"):
        SolverEnsemble(None, maxs=(1.0, 1.0, 1.0, 1.0), step="poisson", phi=0.16, k=0.5)
    for kw in (dict(), dict(phi=0.16), dict(k=0.5)):
        with pytest.raises(ValueError, match=r"step='poisson'.*phi and k"):
            SolverEnsemble(None, maxs=MAXS5, step="poisson", **kw)
    with pytest.raises(ValueError, match="step"):
        SolverEnsemble(None, step="relative")
    ens = SolverEnsemble(None, MAXS5, 4, step="poisson", phi=0.16, k=0.5)
    assert ens.step == "poisson" and ens.weighting and ens.apply_filter and ens.sigma_field == (10, 10) and ens.sigma_weight == (50, 50)
    assert ens.max_cases == 4 and ens.phi == 0.16 and ens.k == 0.5
    for call in (lambda: ens.py_func([np.zeros((4, 5))]), lambda: ens.prime([np.zeros((4, 5))]), ens.reset_state, lambda: ens.state):
        with pytest.raises(RuntimeError, match="init_func"):
            call()
    ens.tables, ens.cell_off = "native", [0, 4, 7]          # as after init_func with two cases; _sur stays None
    for bad in ([np.zeros((4, 4)), np.zeros((3, 5))], [np.zeros(20), np.zeros((3, 5))], [np.zeros((4, 5)), np.zeros((4, 5))]):
        for call in (ens.py_func, ens.prime):
            with pytest.raises(ValueError, match=r"\[N,5\]"):
                call(bad)
    with pytest.raises(ValueError, match="2 cases"):
        ens.py_func([np.zeros((4, 5))])
    with pytest.raises(RuntimeError, match="begin / end"):
        ens.py_func_begin([np.zeros((4, 5)), np.zeros((3, 5))])
