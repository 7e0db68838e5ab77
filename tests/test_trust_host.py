"""The input-trust score without a device: the entries exist in header, binding and the Python mirrors; the oracle's identity
holds on a basis that is not orthonormal; the solver classes with ``trust=False`` ask nothing new of the library."""
import importlib
import inspect

import numpy as np
import pytest

import trust_oracle as to
from psm_amd import GridSurrogate, SolverEnsemble, SolverModule, _lib
from test_abi import declared_functions
from test_solver_boundary_calls import Lib, build_geometry_standin, cells, surrogate_class

ENTRIES = ("psm_bind_trust", "psm_unbind_trust", "psm_trust_last_device", "psm_trust_last")


def test_entries_exist_in_header_binding_and_python():
    names = declared_functions()
    for e in ENTRIES:
        assert e in names and e in _lib.SIGNATURES, e
    lib = _lib.load()
    for e in ENTRIES:
        assert hasattr(lib, e), e
    for m in ("bind_trust", "unbind_trust", "trust_last", "trust_last_device"):
        assert callable(getattr(GridSurrogate, m)), m
    for cls in (SolverModule, SolverEnsemble):
        assert inspect.signature(cls.__init__).parameters["trust"].default is False
        assert callable(cls.trust)


def test_identity_on_a_non_orthonormal_basis():
    """n - 2 |z|^2 + z^T G z == |x - mu - C^T z|^2 at z = C (x - mu), to 1e-12 n."""
    rng = np.random.default_rng(11)
    B, P, K = 6, 17, 3 * 24 * 24
    C = rng.standard_normal((P, K)) / np.sqrt(K) * (1.0 + rng.random((P, 1)))
    mu, x = 0.05 * rng.standard_normal(K), rng.standard_normal((B, K))
    G = C @ C.T
    assert np.abs(G - np.eye(P)).max() > 0.1
    z = to.encode(x, mu, C)
    n, spe = to.score(x, mu, C, z)
    n2, spe2 = to.score_identity(x, mu, C, z)
    assert np.array_equal(n, n2) and (spe > 0.1 * n).all()
    assert (np.abs(spe - spe2) <= 1e-12 * n).all(), (np.abs(spe - spe2) / n).max()
    x[2] = mu
    n, spe = to.score_identity(x, mu, C, to.encode(x, mu, C))
    assert n[2] == 0.0 and spe[2] == 0.0


def _record(cls, step, trust, **kw):
    """The library and GridSurrogate calls of construct + init_func + py_func + trust(), with the recorders of
    test_solver_boundary_calls (and, like them, on the solver module as it is imported now)."""
    from psm_amd import solver
    cls = getattr(solver, cls)
    geometry = importlib.import_module(solver.__package__ + ".geometry")
    log = []
    lib = Lib(log)
    saved = solver.GridSurrogate, solver._lib.load, geometry.build_geometry
    solver.GridSurrogate, solver._lib.load, geometry.build_geometry = surrogate_class(log, lib, saved[0]), (lambda: lib), build_geometry_standin(log)
    try:
        ens = cls is solver.SolverEnsemble
        maxs = (7.0, 1.5, 2.5, 0.5, 4.0) if step == "poisson" else (1.5, 2.5, 0.5, 3.0, 6.0) if step == "gradp" else (1.5, 2.5, 0.5, 4.0)
        args = dict(maxs=maxs, step=step, geometry="scipy", **kw)
        if trust is not None:
            args["trust"] = trust
        if ens:
            args["max_cases"] = 3
        m = cls("model", **args)
        top, obst = np.zeros((3, 2)), np.ones((4, 2))
        if ens:
            m.init_func([cells(6, 1), cells(7, 2)], [top, top], [obst, obst])
            m.py_func([cells(6, 3), cells(7, 4)])
        else:
            m.init_func(cells(6, 1), top, obst)
            m.py_func(cells(6, 3))
        try:
            m.trust()
            log.append("    trust() returned")
        except RuntimeError as e:
            log.append("    trust() ! " + str(e))
        except AttributeError:
            log.append("    trust() reached the surrogate")       # the stand-in has no trust_last
    finally:
        solver.GridSurrogate, solver._lib.load, geometry.build_geometry = saved
    return log


@pytest.mark.parametrize("cls", ("SolverModule", "SolverEnsemble"))
@pytest.mark.parametrize("step,kw", (("absolute", {}), ("delta", {}), ("poisson", dict(phi=0.1, k=2.0)), ("gradp", {})))
def test_trust_false_issues_no_trust_call(cls, step, kw):
    default, off, on = _record(cls, step, None, **kw), _record(cls, step, False, **kw), _record(cls, step, True, **kw)
    assert default == off
    assert not any("trust" in line for line in off[:-1]), [l for l in off if "trust" in l]
    assert "without trust=True" in off[-1]
    # on: the same calls and one bind_trust, behind the kind's own binds and in front of the priming call
    extra = [l for l in on[:-1] if "trust" in l]
    assert len(extra) == 1 and extra[0].endswith(".bind_trust()"), extra
    assert [l for l in on[:-1] if "trust" not in l] == off[:-1]
    at = on.index(extra[0])
    assert not any(".bind_" in l for l in on[at + 1:-1])
    assert on[-1] == "    trust() reached the surrogate"
