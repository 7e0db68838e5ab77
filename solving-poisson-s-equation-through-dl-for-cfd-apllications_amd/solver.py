"""The Chapter-5 solver module on top of ``GridSurrogate``: ``SolverModule`` (one case: ``init_func`` / ``py_func`` with the
reference's signatures, python_module.py:172, :249, and the grid-native body of ``py_func``, :299-473, as ``py_func_grid``) and
``SolverEnsemble`` (K cases on one handle).  ``surrogate.py`` re-exports both.

Everything that differs between the step kinds is one ``StepKind`` record in ``_KINDS``; everything the two classes share is
``_SolverBase``.  A class keeps what one mesh and a case set differ in: the geometry entries, pack / split, pin / unpin."""
from __future__ import annotations

import ctypes as C
from typing import Callable, NamedTuple, Optional, Tuple

import numpy as np

from . import _lib
from .surrogate import GridSurrogate, _f64, _p
from .synthetic import SurrogateModel

STEPS = ("absolute", "delta")
_F64, _F64P = np.dtype(np.float64), C.POINTER(C.c_double)   # made once: a step's path makes neither again
MODULE_STEPS = STEPS + ("poisson", "gradp")   # the Poisson-model step: psm_solve_poisson (SolverModule), psm_solve_cases_poisson (SolverEnsemble); the gradient-model step: psm_solve_gradp / psm_solve_cases_gradp


def _check_step(step, allowed=STEPS):
    if step not in allowed:
        raise ValueError("step must be 'absolute' or 'delta'" + (" or 'poisson' or 'gradp'" if "poisson" in allowed else ""))
    return step


def _check_cells(array_in, out):
    """The [N,5] float64 view of a step's input and its output array, refused before any library call."""
    a = np.ascontiguousarray(array_in, _F64)
    if a.ndim != 2 or a.shape[1] != 5:
        raise ValueError("array must be [N,5] = (Ux, Uy, Cx, Cy, p)")
    if out is None:
        out = np.empty(a.shape[0], _F64)
    elif not isinstance(out, np.ndarray) or out.dtype != _F64 or not out.flags.c_contiguous or out.shape != (a.shape[0],):
        raise ValueError("out must be a contiguous float64 array [N]")
    return a, out


def gradp_grid_metrics(array, ny, nx, round_digits=2):
    """(dx, dy, (extent_x, extent_y), x_min) of the grid ``build_geometry`` makes for ``array``: the bounds rounded as it rounds them,
    ``np.diff(np.linspace(min, max, n))[0]`` as Eval_dual_Dense_onlycil.py:594-595 takes the spacings."""
    a = np.asarray(array, np.float64)
    x_min, x_max = round(np.min(a[:, 2]), round_digits), round(np.max(a[:, 2]), round_digits)
    y_min, y_max = round(np.min(a[:, 3]), round_digits), round(np.max(a[:, 3]), round_digits)
    xl, yl = np.linspace(x_min, x_max, nx), np.linspace(y_min, y_max, ny)
    return float(np.diff(xl)[0]), float(np.diff(yl)[0]), (float(x_max - x_min), float(y_max - y_min)), float(x_min)


def gradp_default_cut(sdfunct, array, delta, round_digits=2):
    """The cut of step='gradp' with ``cut=None``: center_y is the middle row of the obstacle's solid rows -- the rows of ``sdfunct``
    [ny,nx] that hold a zero off the grid's rim --, rounded up; center_x is the rule of Eval_dual_Dense_onlycil.py:599 on that row,
    ``int(((xl[solid].max() + xl[solid].min()) / 2 - X0.min()) / delta)`` with ``xl = np.linspace(min_x, max_x, nx)``.  (The
    reference's literal row 200 fits only its own grid.)"""
    sd = np.asarray(sdfunct, np.float64)
    ny, nx = sd.shape
    rows = 1 + np.flatnonzero((sd[1:-1, 1:-1] == 0).any(axis=1))      # not the grid's rim, where cells outside the mesh's hull are zero too
    if rows.size == 0:
        raise ValueError("sdfunct holds no solid cell: pass the cut")
    cy = int((rows.min() + rows.max() + 1) // 2)
    _, _, (ex, _), x_min = gradp_grid_metrics(array, ny, nx, round_digits)
    xl = np.linspace(x_min, x_min + ex, nx)
    solid = sd[cy] == 0
    cx = int(((xl[solid].max() + xl[solid].min()) / 2 - (x_min + delta / 2)) / delta)
    return cy, cx


# -- the step kinds.  An entry pair is (single mesh, case set): a class reads the half of its own form, once, in its constructor.
def _configure_poisson(m, phi, k, weighting, apply_filter, sigma_field, sigma_weight, **_):
    if phi is None or k is None:
        raise ValueError("step='poisson' needs phi and k")
    m.phi, m.k, m.weighting, m.apply_filter = float(phi), float(k), bool(weighting), apply_filter is None or bool(apply_filter)
    m.sigma_field, m.sigma_weight = tuple(sigma_field), tuple(sigma_weight)


def _configure_gradp(m, apply_filter, sigma_field, sigma_weight, cut, reference, **_):
    if reference not in GridSurrogate.GRADP_REFERENCES:
        raise ValueError("reference must be 'none' or 'outlet'")
    m.cut, m.reference, m.apply_filter = cut, reference, bool(apply_filter)
    m.sigma_field, m.sigma_weight = tuple(sigma_field), tuple(sigma_weight)


def _bind_poisson(m, sur, sdfs, arrays):
    """Everything a Poisson-model step stands on, in the order the library asks for it; after it a step allocates nothing.  A case
    set binds the features with its K SDF planes and takes no ``bind_frames``."""
    sur.bind_features(np.stack(sdfs) if m.CASES else sdfs[0], m.k, m.maxs[:4])
    sur.bind_poststeps(m.sigma_field, m.sigma_weight)
    if not m.CASES:
        sur.bind_frames(1, 6)
    (sur.bind_poisson_solve_cases if m.CASES else sur.bind_poisson_solve)(m.phi, m.maxs[4], m.weighting, m.apply_filter)


def _bind_gradp(m, sur, sdfs, arrays):
    """Everything a gradient-model step stands on; after it a step allocates nothing.  The grid is case 0's (all cases share its
    shape and bounds); one cut per case."""
    dx, dy, extents, _ = gradp_grid_metrics(arrays[0], sur.ny, sur.nx)
    if m.cut is None:
        cuts = [gradp_default_cut(sd, a, m.delta) for sd, a in zip(sdfs, arrays)]
    else:
        cuts = [tuple(int(v) for v in c) for c in (m.cut if m.CASES else [m.cut])]
    if m.apply_filter:
        sur.bind_poststeps(m.sigma_field, m.sigma_weight)
    if m.CASES:
        m.cuts_used = cuts
        sur.bind_gradp_solve_cases(cuts, dx, dy, extents, m.maxs[3:5], m.apply_filter, m.reference)
    else:
        m.cut_used = cuts[0]
        sur.bind_gradp_solve(cuts[0], dx, dy, extents, m.maxs[3:5], m.apply_filter, m.reference)


class StepKind(NamedTuple):
    """One step kind at the solver boundary.  An entry pair that is None does not exist for the kind: the method raises the text
    beside it ({noun}: 'module' or 'ensemble')."""
    solve: Tuple[str, str]
    begin: Optional[Tuple[str, str]]
    end: Optional[Tuple[str, str]]
    no_halves: Optional[str]                              # what a missing begin or end half raises
    prime: Optional[Tuple[str, str]]
    reset: Optional[str]
    state: Optional[str]
    state_first: Optional[Callable]                       # the type of the state's first field: primed (bool) or frames held (int)
    no_state: Optional[str]                               # what prime, reset_state and state raise for a kind without a state
    sdf_model: int = 0                                    # normalise_sdf = fill_input of psm_set_geometry*: the deltas model's convention (SM_call.py:441-443)
    five_maxs: Optional[str] = None                       # the kind takes five maxs: what another count raises (None: the last four are taken as they come)
    maxs4: Callable = lambda maxs: maxs[-4:]              # the four maxs of psm_set_geometry*
    configure: Callable = lambda m, **_: None             # the kind's constructor arguments and their checks
    bind: Optional[Callable] = None                       # what init_func binds behind the geometry
    primes: bool = False                                  # init_func primes the state with its own cells


_GRADP_HAS_NO = "step='gradp' has no {}: a step depends on its cells alone, use py_func"
_KINDS = {
    "absolute": StepKind(
        solve=("psm_solve", "psm_solve_cases"), begin=("psm_solve_begin", "psm_solve_cases_begin"), end=("psm_solve_end", "psm_solve_cases_end"),
        no_halves=None, prime=None, reset=None, state=None, state_first=None,
        no_state="this {noun} was built with step='absolute': the state belongs to step='delta'"),
    "delta": StepKind(
        solve=("psm_solve_delta", "psm_solve_cases_delta"), begin=("psm_solve_delta_begin", "psm_solve_cases_delta_begin"),
        end=("psm_solve_delta_end", "psm_solve_cases_delta_end"), no_halves=None,
        prime=("psm_delta_prime", "psm_delta_prime_cases"), reset="psm_delta_reset", state="psm_delta_state", state_first=bool, no_state=None,
        sdf_model=1, primes=True),
    "poisson": StepKind(                                  # no begin half; the end half has never refused (it is the 'absolute' one)
        solve=("psm_solve_poisson", "psm_solve_cases_poisson"), begin=None, end=("psm_solve_end", "psm_solve_cases_end"),
        no_halves="step='poisson' has no begin / end halves: use py_func",
        prime=("psm_poisson_solve_push", "psm_poisson_solve_push_cases"), reset="psm_poisson_solve_reset", state="psm_poisson_solve_state",
        state_first=int, no_state=None, sdf_model=1,
        five_maxs="step='poisson' takes five maxs: (max_abs_Poisson_term_1, max_abs_delta_Ux, max_abs_delta_Uy, max_abs_dist, max_abs_delta_p)",
        configure=_configure_poisson, bind=_bind_poisson, primes=True),
    "gradp": StepKind(
        solve=("psm_solve_gradp", "psm_solve_cases_gradp"), begin=None, end=None, no_halves=_GRADP_HAS_NO.format("begin / end halves"),
        prime=None, reset=None, state=None, state_first=None, no_state=_GRADP_HAS_NO.format("state"), sdf_model=1,
        five_maxs="step='gradp' takes five maxs: (max_abs_Ux, max_abs_Uy, max_abs_dist, max_abs_dPdx, max_abs_dPdy)",
        maxs4=lambda maxs: maxs[:3] + (1.0,),             # (max_abs_Ux, max_abs_Uy, max_abs_dist, unused)
        configure=_configure_gradp, bind=_bind_gradp),
}
assert tuple(_KINDS) == MODULE_STEPS

# the six tables of psm_set_geometry*: (field of build_geometry's tables, rows per grid point (0: per cell), width, dtype, C type)
_TABLES = (("vtx_m2g", 1, 3, np.int32, C.c_int32), ("wts_m2g", 1, 3, np.float64, C.c_double), ("indices", 1, 2, np.int32, C.c_int32),
           ("sdfunct", 1, 1, np.float64, C.c_double), ("vtx_g2m", 0, 3, np.int32, C.c_int32), ("wts_g2m", 0, 3, np.float64, C.c_double))


class _SolverBase:
    """What ``SolverModule`` (CASES = 0) and ``SolverEnsemble`` (CASES = 1) share.  A class gives ``_take`` (a call's input -> the cells
    and p arrays), ``_cells_args`` and ``_step`` (their marshalling into a library call), ``_give`` (p -> what the call returns), ``_set_geometry``, ``_init_native``
    and ``_one`` (a per-case list -> what its own signature calls it)."""
    CASES = 0
    NOUN = "module"

    def __init__(self, model, maxs, max_cases, geometry, device, delta, step, trust=False, **step_args):
        if geometry not in ("scipy", "native"):
            raise ValueError("geometry must be 'scipy' or 'native'")
        self.step = _check_step(step, MODULE_STEPS)
        kind = self._kind = _KINDS[self.step]
        self.model, self.maxs, self.max_cases = model, tuple(float(v) for v in maxs), int(max_cases)
        self.geometry, self.device, self.delta = geometry, device, delta
        if kind.five_maxs and len(self.maxs) != 5:
            raise ValueError(kind.five_maxs)
        kind.configure(self, **step_args)
        form = lambda pair: pair and pair[self.CASES]
        self._solve, self._begin, self._end, self._prime = form(kind.solve), form(kind.begin), form(kind.end), form(kind.prime)
        self._sur = None
        self.tables = None
        self._inflight = None
        self._trust = bool(trust)

    def _call(self, entry, *args):
        sur = self._sur
        return sur._chk(getattr(sur.lib, entry)(sur.h, *args))

    def _need_init(self):
        if self.tables is None:
            raise RuntimeError("init_func has not been called")

    # -- init_func: the tables, the geometry entry of the class, then what the kind binds, then its first frame
    def _init(self, arrays, tops, obsts):
        kind, K = self._kind, len(arrays)
        a, t, o = [_f64(x) for x in arrays], [_f64(x) for x in tops], [_f64(x) for x in obsts]
        mx = _f64(kind.maxs4(self.maxs))
        if self.geometry == "native":
            lib = _lib.load()
            ny, nx = C.c_int32(), C.c_int32()
            if lib.psm_geometry_shape(_p(a[0], C.c_double), a[0].shape[0], self.delta, C.byref(ny), C.byref(nx), None):
                raise ValueError(lib.psm_geometry_last_error().decode())
            ny, nx, tables = ny.value, nx.value, "native"
        else:
            from .geometry import build_geometry
            tables = [build_geometry(a[k], t[k], o[k], self.delta) for k in range(K)]
            ny, nx = tables[0].ny, tables[0].nx
            if any((g.ny, g.nx) != (ny, nx) for g in tables):
                raise ValueError("the cases of an ensemble must share one grid shape")
        if self._sur is not None:
            self._sur.close()
        self._sur = sur = GridSurrogate(self.model, ny, nx, self.max_cases, self.device)
        keep = None
        if tables == "native" and not kind.sdf_model:      # the library builds and installs the tables (with the flags 0, 0)
            self._init_native(sur, mx, a, t, o)
        else:                                              # the six tables per case, handed over with the kind's two flags
            keep = (self._native_tables(a, t, o, ny * nx) if tables == "native" else
                    [[np.ascontiguousarray(getattr(g, f), dt) for g in tables] for f, _, _, dt, _ in _TABLES])
            self._set_geometry(sur, [x.shape[0] for x in a], ny, nx, keep, mx, kind.sdf_model)
        self.tables = tables if tables == "native" else self._one(tables)
        if kind.bind:
            kind.bind(self, sur, [np.asarray(sd, np.float64).reshape(ny, nx) for sd in keep[3]], a)
        if self._trust:
            sur.bind_trust()
        if kind.primes:
            self.prime(self._one(a))
        return 0

    def _native_tables(self, a, t, o, ng):
        """psm_geometry_build per case: the tables the library would install itself, for psm_set_geometry* with the kind's flags."""
        lib = _lib.load()
        keep = [[np.empty((ng if per_point else x.shape[0]) * width, dt) for x in a] for _, per_point, width, dt, _ in _TABLES]
        for k in range(len(a)):
            if lib.psm_geometry_build(_p(a[k], C.c_double), a[k].shape[0], _p(t[k], C.c_double), t[k].shape[0], _p(o[k], C.c_double),
                                      o[k].shape[0], self.delta, 10, *[_p(col[k], ct) for col, (_, _, _, _, ct) in zip(keep, _TABLES)]):
                raise ValueError((f"case {k}: " if self.CASES else "") + lib.psm_geometry_last_error().decode())
        return keep

    # -- trust=True: the input-trust score of the last step (psm_bind_trust / psm_trust_last of include/psm.h)
    def trust(self):
        """Per case of the last ``py_func``, how much of the network's input the model's retained input components represent: a
        dict of ``n`` = |x - mean|^2 and ``spe`` (the PCA reconstruction residual) per block [B], ``explained`` = 1 - spe / n [B],
        ``explained_min`` and ``explained_total`` = 1 - sum(spe) / sum(n).  Compare with the var_in the model was trained to; what a
        low value means for the step (keep the solver's own p as the initial guess) is the caller's decision.  The scored image is
        the one the last launch chain ran on: a priming step runs none and leaves the chain before it."""
        if not self._trust:
            raise RuntimeError(f"this {self.NOUN} was built without trust=True")
        self._need_init()
        t = self._sur.trust_last()
        with np.errstate(invalid="ignore", divide="ignore"):
            return self._one([{"n": n, "spe": spe, "explained": ex, "explained_min": float(np.min(ex)),
                               "explained_total": float(1.0 - spe.sum() / n.sum())}
                              for n, spe, ex in zip(t["n"], t["spe"], t["explained"])])

    # -- the state of step='delta' (psm_delta_prime* / _reset / _state) and of step='poisson' (psm_poisson_solve_push* / _reset / _state)
    def _need_state(self):
        if self._kind.no_state:
            raise RuntimeError(self._kind.no_state.format(noun=self.NOUN))
        self._need_init()

    def prime(self, arrays):
        """U(t-1) := array[:,0:2] (of every case).  ``init_func`` does this with the start fields; a restart primes again.
        step='poisson': one frame (U and p) is pushed into the two-frame state; a restart primes with two."""
        self._need_state()
        self._call(self._prime, *self._cells_args(self._take(arrays, None)[0]))

    def reset_state(self):
        """Forget U(t-1): the next ``py_func`` is the priming step and returns ``array[:,4]``."""
        self._need_state()
        self._call(self._kind.reset)

    @property
    def state(self):
        """(primed, steps) of psm_delta_state; step='poisson': (frames held, steps) of psm_poisson_solve_state."""
        self._need_state()
        first, steps = C.c_int32(), C.c_int64()
        self._call(self._kind.state, C.byref(first), C.byref(steps))
        return self._kind.state_first(first.value), int(steps.value)

    # -- the halves of a step
    def _step_begin(self, arrays, out):
        if self._begin is None:
            raise RuntimeError(self._kind.no_halves)
        self._inflight = self._step(self._begin, arrays, out, 0)  # keeps both arrays alive until the end call (set only once the step is in flight)

    def py_func_end(self):
        if self._end is None:
            raise RuntimeError(self._kind.no_halves)
        self._call(self._end)
        _, out = self._inflight
        self._inflight = None
        return self._give(out)


class SolverModule(_SolverBase):
    """Chapter-5 ``python_module`` (python_module.py): ``init_func`` / ``py_func`` with the
    reference's signatures on one rank (the serial solver, singleCore/test_Case/python_module.py:
    139,199; in the parallel solver the mpi4py gather/scatter of python_module.py:179-185,258,511
    stays around these calls).  ``maxs`` = (max_abs_Ux, max_abs_Uy, max_abs_dist, max_abs_p) of
    the ``maxs`` file (python_module.py:106-109)."""

    def __init__(self, model: SurrogateModel, maxs=(1.0, 1.0, 1.0, 1.0), device: int = 0, delta: float = 5e-3,
                 geometry: str = "scipy", step: str = "absolute", phi: float = None, k: float = None, weighting: bool = True,
                 apply_filter: bool = None, sigma_field=(10, 10), sigma_weight=(50, 50), cut=None, reference: str = "outlet",
                 trust: bool = False):
        """``step``: 'absolute' (U -> p, the Chapter-5 module) or 'delta' (the deltas model behind the same two calls:
        [U(t) - U(t-1)], SDF -> p(t) - p(t-1), psm_solve_delta* of include/psm.h).  With 'delta', ``maxs`` are
        (max_abs_dUx, max_abs_dUy, max_abs_dist, max_abs_dp), ``init_func`` installs the tables with the deltas model's
        convention (SDF divided by max_abs_dist, interpolate_fill) and primes U(t-1) with its own ``array`` -- the fields of
        the start time -- and ``py_func`` returns ``array[:,4] + dp``.
        ``step='poisson'``: pressureSM_Poisson's time step behind the same two calls (psm_solve_poisson of include/psm.h): ``maxs`` =
        (max_abs_Poisson_term_1, max_abs_delta_Ux, max_abs_delta_Uy, max_abs_dist, max_abs_delta_p), ``phi`` the length scale of
        the features, ``k`` the arcsinh smoothing's constant, ``weighting`` / ``apply_filter`` and the two filter widths as in the
        reference's ``timeStep``.  ``init_func`` installs the tables, binds features, post-steps, frames and the step, and pushes
        its own ``array`` as the first frame; the state is U, dU and p of the previous call, on the device: with the weighting the
        first ``py_func`` is a priming step too (it returns ``array[:,4]``), then every call returns ``array[:,4] + dp``.
        ``step='gradp'``: the U_to_gradP model behind the same two calls (psm_solve_gradp of include/psm.h): ``maxs`` = (max_abs_Ux,
        max_abs_Uy, max_abs_dist, max_abs_dPdx, max_abs_dPdy), the ``maxs`` file of the reference (Eval_dual_Dense_onlycil.py:54);
        ``init_func`` installs the tables with normalise_sdf = fill_input = 1, takes the extents and spacings from the grid bounds it
        built (``max_x - min_x``, ``np.diff(xl)[0]``, :594-595) and binds the step (with ``apply_filter``, default off for this step,
        the post-steps with ``sigma_field`` first).  ``cut`` = (center_y, center_x) of the integration; None:
        :func:`gradp_default_cut` (the reference's literal row 200 fits only its own grid).  ``reference``: 'outlet' (p = 0 at the
        outlet) or 'none'.  There is no state: ``prime``, ``reset_state``, ``state`` and the begin / end halves raise.
        ``geometry``: who builds init_func's tables -- 'scipy' (default in this Python mirror: the routines the reference
        itself calls, qhull Delaunay in both directions, so that the tables -- including qhull's arbitrary choice of diagonal
        in every cocircular lattice square of the grid -> mesh step -- are the reference's) or 'native' (the library's C++
        builder behind ``psm_init_geometry``, csrc/psm_geometry.cpp: what a C++ solver gets; no SciPy).  The two differ only
        where the reference's own result is an accident of qhull (include/psm.h): fixed lattice diagonals -- a second-order
        difference on smooth fields, O(1) per cell on the white-noise fields of randomly initialised test networks
        (tests/measure/mesh_native_vs_scipy.py) -- and the simplex used for lattice points outside the hull.
        ``trust=True``: ``init_func`` also binds the input-trust score behind the step's own bindings and :meth:`trust` reports it for
        the last step; off, the module makes exactly the library calls it makes without the option."""
        super().__init__(model, maxs, 1, geometry, device, delta, step, trust=trust, phi=phi, k=k, weighting=weighting, apply_filter=apply_filter,
                         sigma_field=sigma_field, sigma_weight=sigma_weight, cut=cut, reference=reference)

    # -- grid-native body (python_module.py:299-473)
    def py_func_grid(self, grid: np.ndarray) -> np.ndarray:
        if self._sur is None or (self._sur.ny, self._sur.nx) != grid.shape[:2]:
            if self._sur is not None:
                self._sur.close()
            self._sur = GridSurrogate(self.model, grid.shape[0], grid.shape[1], 1, self.device)
        return self._sur.solve(grid)[0, :, :, 0]

    # -- the solver boundary
    def init_func(self, array, top_boundary, obst_boundary, placeholder=0):
        """python_module.py:172: one-time tables (host, SciPy qhull like the reference; geometry='native': built inside the
        library, csrc/psm_geometry.cpp), handed to the GPU library with psm_set_geometry.  Returns 0."""
        return self._init([array], [top_boundary], [obst_boundary])

    @staticmethod
    def _one(per_case):
        return per_case[0]

    def _set_geometry(self, sur, n_cells, ny, nx, keep, mx, sdf_model):
        sur._chk(sur.lib.psm_set_geometry(sur.h, int(n_cells[0]), ny, nx, *[_p(col[0], ct) for col, (_, _, _, _, ct) in zip(keep, _TABLES)],
                                          _p(mx, C.c_double), sdf_model, sdf_model, 0.05))

    def _init_native(self, sur, mx, a, t, o):
        """psm_set_case + psm_init_geometry: the tables are built inside the library (csrc/psm_geometry.cpp)."""
        sur._chk(sur.lib.psm_set_case(sur.h, _p(mx, C.c_double), self.delta, 10, 0.05))
        sur._chk(sur.lib.psm_init_geometry(sur.h, _p(a[0], C.c_double), a[0].shape[0], _p(t[0], C.c_double), t[0].shape[0],
                                           _p(o[0], C.c_double), o[0].shape[0], 0))

    _take = staticmethod(_check_cells)

    @staticmethod
    def _cells_args(a):
        return _p(a, C.c_double), a.shape[0]

    def _step(self, entry, array_in, out, rank):
        """One library call cells [N,5] -> p [N] -> (cells, p)."""
        if self.tables is None:
            raise RuntimeError("init_func has not been called")
        a, out = _check_cells(array_in, out)
        sur = self._sur
        sur._chk(getattr(sur.lib, entry)(sur.h, a.ctypes.data_as(_F64P), a.shape[0], rank, out.ctypes.data_as(_F64P)))
        return a, out

    @staticmethod
    def _give(out):
        return out

    def pin(self, array: np.ndarray, out: np.ndarray = None):
        """psm_pin_buffers: register the caller's persistent [N,5] float64 array (and optionally a persistent output
        array) for direct DMA; later ``py_func(array, out=out)`` calls with exactly these arrays skip the staging copies.
        The caller keeps both arrays alive until ``unpin()`` / a new ``init_func``."""
        if array.dtype != np.float64 or not array.flags.c_contiguous or (out is not None and (out.dtype != np.float64 or not out.flags.c_contiguous)):
            raise ValueError("contiguous float64 arrays expected")
        self._call("psm_pin_buffers", _p(array, C.c_double), _p(out, C.c_double) if out is not None else None)
        self._pinned = (array, out)

    def unpin(self):
        self._call("psm_unpin_buffers")
        self._pinned = None

    def py_func_begin(self, array_in, out: np.ndarray = None):
        """First half of :meth:`py_func` (psm_solve_begin): enqueue the step and return; several SolverModules (cases)
        can be advanced from one thread by calling begin on all of them, then :meth:`py_func_end` on each."""
        self._need_init()
        self._step_begin(array_in, out)

    def py_func(self, array_in, placeholder=0, out: np.ndarray = None) -> np.ndarray:
        """python_module.py:249: cells [N,5] float64 -> p [N] float64.  step='delta': p = array[:,4] + dp (psm_solve_delta);
        step='poisson': likewise through psm_solve_poisson."""
        return self._step(self._solve, array_in, out, int(placeholder))[1]


class SolverEnsemble(_SolverBase):
    """``SolverModule`` for an ensemble of cases that share one grid shape: K meshes with their own obstacles on ONE handle,
    all advanced by one call (``psm_set_geometry_cases`` / ``psm_solve_cases``: one launch chain per step instead of one per
    case).  ``init_func`` takes one (array, top, obst) per case, ``py_func`` one ``[N_i,5]`` array per case and returns the
    list of ``p_i``.  ``geometry``: 'native' (``psm_init_geometry_cases``, the library's C++ table builder) or 'scipy'
    (``geometry.build_geometry`` per case, handed over with ``psm_set_geometry_cases``) -- see :class:`SolverModule`.
    ``step``: 'absolute' or 'delta' as for :class:`SolverModule`, on ``psm_solve_cases_delta*``: one state for the set; or
    'poisson' with the further arguments of :class:`SolverModule` (five ``maxs``, ``phi``, ``k``, the weighting, the filter and its
    widths), on ``psm_solve_cases_poisson``: ``init_func`` installs the K table sets, binds the features with the K SDF planes, the
    post-steps and the step, and pushes its own ``arrays`` as the first frame; one two-frame state, one frame counter and one step
    counter for the set; no begin / end halves.  Or 'gradp' with ``cut`` (None, or one (center_y, center_x) per case), ``reference``
    and ``apply_filter`` (default off) of :class:`SolverModule`, on ``psm_solve_cases_gradp``: no state, no begin / end halves.
    ``trust=True``: as for :class:`SolverModule`; :meth:`trust` returns one dict per case."""
    CASES = 1
    NOUN = "ensemble"

    def __init__(self, model: SurrogateModel, maxs=(1.0, 1.0, 1.0, 1.0), max_cases: int = 8, geometry: str = "native",
                 device: int = 0, delta: float = 5e-3, step: str = "absolute", phi: float = None, k: float = None, weighting: bool = True,
                 apply_filter: bool = None, sigma_field=(10, 10), sigma_weight=(50, 50), cut=None, reference: str = "outlet",
                 trust: bool = False):
        super().__init__(model, maxs, max_cases, geometry, device, delta, step, trust=trust, phi=phi, k=k, weighting=weighting, apply_filter=apply_filter,
                         sigma_field=sigma_field, sigma_weight=sigma_weight, cut=cut, reference=reference)
        self.cell_off = None

    @staticmethod
    def _ptrs(arrays):
        return (C.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])

    def init_func(self, arrays, tops, obsts):
        """One-time tables of every case; all cases must give the same grid shape.  Returns 0."""
        if not (len(arrays) == len(tops) == len(obsts)) or not 1 <= len(arrays) <= self.max_cases:
            raise ValueError("one (array, top, obst) per case, 1..max_cases cases")
        return self._init(arrays, tops, obsts)

    @staticmethod
    def _one(per_case):
        return per_case

    def _set_geometry(self, sur, n_cells, ny, nx, keep, mx, sdf_model):
        sur._chk(sur.lib.psm_set_geometry_cases(sur.h, len(n_cells), (C.c_int64 * len(n_cells))(*n_cells), ny, nx, *[self._ptrs(col) for col in keep],
                                                _p(mx, C.c_double), sdf_model, sdf_model, 0.05))
        self._read_cell_off(sur, len(n_cells))

    def _init_native(self, sur, mx, a, t, o):
        """psm_set_case + psm_init_geometry_cases: the K table sets are built inside the library."""
        counts = lambda xs: (C.c_int64 * len(xs))(*[x.shape[0] for x in xs])
        sur._chk(sur.lib.psm_set_case(sur.h, _p(mx, C.c_double), self.delta, 10, 0.05))
        sur._chk(sur.lib.psm_init_geometry_cases(sur.h, len(a), self._ptrs(a), counts(a), self._ptrs(t), counts(t), self._ptrs(o), counts(o)))
        self._read_cell_off(sur, len(a))

    def _read_cell_off(self, sur, K):
        off = (C.c_int64 * (K + 1))()
        sur._chk(sur.lib.psm_mesh_cases(sur.h, None, off))
        self.cell_off = [int(v) for v in off]

    def _take(self, arrays, out):
        """The cases' cells packed in case order, and p for all of them."""
        K = len(self.cell_off) - 1
        if len(arrays) != K:
            raise ValueError(f"{K} cases were initialised")
        cells = np.empty((self.cell_off[-1], 5), np.float64)
        for k, x in enumerate(arrays):
            x = np.asarray(x)
            if x.shape != (self.cell_off[k + 1] - self.cell_off[k], 5):
                raise ValueError("array must be [N,5] = (Ux, Uy, Cx, Cy, p) with the cell count of init_func")
            cells[self.cell_off[k]:self.cell_off[k + 1]] = x
        return cells, np.empty(self.cell_off[-1], np.float64)

    @staticmethod
    def _cells_args(cells):
        return (_p(cells, C.c_double),)

    def _step(self, entry, arrays, out, rank):
        """One library call on the packed cells of all cases -> (cells, p)."""
        if self.tables is None:
            raise RuntimeError("init_func has not been called")
        cells, p = self._take(arrays, None)
        sur = self._sur
        sur._chk(getattr(sur.lib, entry)(sur.h, cells.ctypes.data_as(_F64P), p.ctypes.data_as(_F64P)))
        return cells, p

    def _give(self, p):
        return [p[self.cell_off[k]:self.cell_off[k + 1]] for k in range(len(self.cell_off) - 1)]

    def py_func_begin(self, arrays):
        """First half of :meth:`py_func` (psm_solve_cases_begin): enqueue the step of all cases and return."""
        self._step_begin(arrays, None)

    def py_func(self, arrays):
        """One step of every case: list of cells [N_i,5] float64 -> list of p_i [N_i] float64."""
        return self._give(self._step(self._solve, arrays, None, 0)[1])
