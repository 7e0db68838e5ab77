"""The delta-step entries at the C boundary, without a GPU: every new prototype of include/psm.h is bound by _lib.py and exported
by the built library, PSM_ABI_VERSION is still 4, a C99 file that includes the header can take the address of each
(tests/native/abi_c_check_delta.c), a NULL handle is refused by every entry, and the Python mirrors refuse bad arguments before
any library call."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from psm_amd import SolverEnsemble, SolverModule, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("psm_delta_prime", "psm_delta_reset", "psm_delta_state", "psm_solve_delta", "psm_solve_delta_begin",
               "psm_solve_delta_end", "psm_delta_prime_cases", "psm_solve_cases_delta_device", "psm_solve_cases_delta",
               "psm_solve_cases_delta_begin", "psm_solve_cases_delta_end")


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
    for cls in (SolverModule, SolverEnsemble):
        for name in ("prime", "reset_state"):
            assert callable(getattr(cls, name, None)), (cls, name)
        assert isinstance(cls.state, property)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_header_compiles_as_c99_with_the_delta_entries(tmp_path):
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                        os.path.join(ROOT, "tests", "native", "abi_c_check_delta.c"), "-o", str(tmp_path / "a.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_null_handle_is_refused_by_every_entry():
    lib = _lib.load()
    assert lib.psm_delta_prime(None, None, 1) == -1
    assert lib.psm_delta_reset(None) == -1
    assert lib.psm_delta_state(None, None, None) == -1
    assert lib.psm_solve_delta(None, None, 1, 0, None) == -1
    assert lib.psm_solve_delta_begin(None, None, 1, 0, None) == -1
    assert lib.psm_solve_delta_end(None) == -1
    assert lib.psm_delta_prime_cases(None, None) == -1
    assert lib.psm_solve_cases_delta_device(None, None, None, None) == -1
    assert lib.psm_solve_cases_delta(None, None, None) == -1
    assert lib.psm_solve_cases_delta_begin(None, None, None) == -1
    assert lib.psm_solve_cases_delta_end(None) == -1


def test_python_argument_checks_come_before_any_library_call():
    """The mirrors refuse bad arguments on objects whose surrogate does not exist: any call into the library would raise
    AttributeError instead."""
    for cls in (SolverModule, SolverEnsemble):
        with pytest.raises(ValueError, match="step"):
            cls(None, step="relative")
        assert cls(None).step == "absolute" and cls(None, step="delta").step == "delta"
    sm = SolverModule(None, step="delta")
    with pytest.raises(RuntimeError, match="init_func"):
        sm.py_func(np.zeros((4, 5)))
    with pytest.raises(RuntimeError, match="init_func"):
        sm.prime(np.zeros((4, 5)))
    sm.tables = "native"                                    # as after init_func; _sur stays None
    for bad in (np.zeros((4, 4)), np.zeros(20), np.zeros((2, 2, 5))):
        for call in (sm.py_func, sm.py_func_begin, sm.prime):
            with pytest.raises(ValueError, match=r"\[N,5\]"):
                call(bad)
    for out in (np.zeros(4, np.float32), np.zeros(5), np.zeros((4, 2))[:, 0], [0.0] * 4):
        with pytest.raises(ValueError, match="out"):
            sm.py_func(np.zeros((4, 5)), out=out)
        with pytest.raises(ValueError, match="out"):
            sm.py_func_begin(np.zeros((4, 5)), out=out)
    absolute = SolverModule(None)
    absolute.tables = "native"
    for call in (lambda: absolute.prime(np.zeros((4, 5))), absolute.reset_state, lambda: absolute.state):
        with pytest.raises(RuntimeError, match="step='delta'"):
            call()
    ens = SolverEnsemble(None, step="delta")
    with pytest.raises(RuntimeError, match="init_func"):
        ens.py_func([np.zeros((4, 5))])
    with pytest.raises(RuntimeError, match="init_func"):
        ens.prime([np.zeros((4, 5))])
    ens.tables, ens.cell_off = "native", [0, 4, 7]
    with pytest.raises(ValueError, match="2 cases"):
        ens.prime([np.zeros((4, 5))])
    with pytest.raises(ValueError, match=r"\[N,5\]"):
        ens.py_func([np.zeros((4, 5)), np.zeros((3, 4))])
    with pytest.raises(RuntimeError, match="step='delta'"):
        SolverEnsemble(None).reset_state()
