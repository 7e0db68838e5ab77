"""The Chapter-5 solver module on top of ``GridSurrogate``: ``SolverModule`` (one case: ``init_func`` / ``py_func`` with the
reference's signatures, python_module.py:172, :249, and the grid-native body of ``py_func``, :299-473, as ``py_func_grid``) and
``SolverEnsemble`` (K cases on one handle).  ``surrogate.py`` re-exports both."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .surrogate import GridSurrogate, _f64, _p
from .synthetic import SurrogateModel

STEPS = ("absolute", "delta")
MODULE_STEPS = STEPS + ("poisson", "gradp")   # the Poisson-model step: psm_solve_poisson (SolverModule), psm_solve_cases_poisson (SolverEnsemble); the gradient-model step: psm_solve_gradp / psm_solve_cases_gradp


def _check_step(step, allowed=STEPS):
    if step not in allowed:
        raise ValueError("step must be 'absolute' or 'delta'" + (" or 'poisson' or 'gradp'" if "poisson" in allowed else ""))
    return step


def _check_cells(array_in, out):
    """The [N,5] float64 view of a step's input and its output array, refused before any library call."""
    a = _f64(array_in)
    if a.ndim != 2 or a.shape[1] != 5:
        raise ValueError("array must be [N,5] = (Ux, Uy, Cx, Cy, p)")
    if out is None:
        out = np.empty(a.shape[0], np.float64)
    elif not isinstance(out, np.ndarray) or out.dtype != np.float64 or not out.flags.c_contiguous or out.shape != (a.shape[0],):
        raise ValueError("out must be a contiguous float64 array [N]")
    return a, out


def _check_poisson(maxs, phi, k):
    """The argument checks of step='poisson', of SolverModule and SolverEnsemble alike, before any library call."""
    if len(maxs) != 5:
        raise ValueError("step='poisson' takes five maxs: (max_abs_Poisson_term_1, max_abs_delta_Ux, max_abs_delta_Uy, max_abs_dist, max_abs_delta_p)")
    if phi is None or k is None:
        raise ValueError("step='poisson' needs phi and k")


def _check_gradp(maxs, reference):
    """The argument checks of step='gradp', of SolverModule and SolverEnsemble alike, before any library call."""
    if len(maxs) != 5:
        raise ValueError("step='gradp' takes five maxs: (max_abs_Ux, max_abs_Uy, max_abs_dist, max_abs_dPdx, max_abs_dPdy)")
    if reference not in GridSurrogate.GRADP_REFERENCES:
        raise ValueError("reference must be 'none' or 'outlet'")


def _no_gradp_state(what):
    raise RuntimeError(f"step='gradp' has no {what}: a step depends on its cells alone, use py_func")


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


def _poisson_state(sur):
    frames, steps = C.c_int32(), C.c_int64()
    sur._chk(sur.lib.psm_poisson_solve_state(sur.h, C.byref(frames), C.byref(steps)))
    return int(frames.value), int(steps.value)


def _delta_state(sur):
    primed, steps = C.c_int32(), C.c_int64()
    sur._chk(sur.lib.psm_delta_state(sur.h, C.byref(primed), C.byref(steps)))
    return bool(primed.value), int(steps.value)


class SolverModule:
    """Chapter-5 ``python_module`` (python_module.py): ``init_func`` / ``py_func`` with the
    reference's signatures on one rank (the serial solver, singleCore/test_Case/python_module.py:
    139,199; in the parallel solver the mpi4py gather/scatter of python_module.py:179-185,258,511
    stays around these calls).  ``maxs`` = (max_abs_Ux, max_abs_Uy, max_abs_dist, max_abs_p) of
    the ``maxs`` file (python_module.py:106-109)."""

    def __init__(self, model: SurrogateModel, maxs=(1.0, 1.0, 1.0, 1.0), device: int = 0, delta: float = 5e-3,
                 geometry: str = "scipy", step: str = "absolute", phi: float = None, k: float = None, weighting: bool = True,
                 apply_filter: bool = None, sigma_field=(10, 10), sigma_weight=(50, 50), cut=None, reference: str = "outlet"):
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
        (tests/measure/mesh_native_vs_scipy.py) -- and the simplex used for lattice points outside the hull."""
        if geometry not in ("scipy", "native"):
            raise ValueError("geometry must be 'scipy' or 'native'")
        self.step = _check_step(step, MODULE_STEPS)
        self.model, self.maxs, self.device, self.delta = model, tuple(float(v) for v in maxs), device, delta
        self.geometry = geometry
        if self.step == "poisson":
            _check_poisson(self.maxs, phi, k)
            self.phi, self.k, self.weighting, self.apply_filter = float(phi), float(k), bool(weighting), apply_filter is None or bool(apply_filter)
            self.sigma_field, self.sigma_weight = tuple(sigma_field), tuple(sigma_weight)
        if self.step == "gradp":
            _check_gradp(self.maxs, reference)
            self.cut, self.reference, self.apply_filter = cut, reference, bool(apply_filter)
            self.sigma_field, self.sigma_weight = tuple(sigma_field), tuple(sigma_weight)
        self._sur = None
        self.tables = None

    # -- grid-native body (python_module.py:299-473)
    def py_func_grid(self, grid: np.ndarray) -> np.ndarray:
        if self._sur is None or (self._sur.ny, self._sur.nx) != grid.shape[:2]:
            if self._sur is not None:
                self._sur.close()
            self._sur = GridSurrogate(self.model, grid.shape[0], grid.shape[1], 1, self.device)
        return self._sur.solve(grid)[0, :, :, 0]

    # -- the solver boundary
    def init_func(self, array, top_boundary, obst_boundary, placeholder=0):
        """python_module.py:172: one-time tables (host, SciPy qhull like the reference), handed
        to the GPU library with psm_set_geometry.  Returns 0."""
        from .geometry import build_geometry
        if self.geometry == "native":
            return self._init_func_native(array, top_boundary, obst_boundary)
        t = build_geometry(np.asarray(array, np.float64), top_boundary, obst_boundary, self.delta)
        if self._sur is not None:
            self._sur.close()
        self._sur = GridSurrogate(self.model, t.ny, t.nx, 1, self.device)
        v1, w1 = np.ascontiguousarray(t.vtx_m2g, np.int32), _f64(t.wts_m2g)
        v2, w2 = np.ascontiguousarray(t.vtx_g2m, np.int32), _f64(t.wts_g2m)
        idx, sdf, mx = np.ascontiguousarray(t.indices, np.int32), _f64(t.sdfunct), self._maxs4()
        smd = int(self.step != "absolute")       # the deltas model's convention: normalise_sdf = fill_input = 1 (SM_call.py:441-443)
        self._sur._chk(self._sur.lib.psm_set_geometry(
            self._sur.h, int(np.asarray(array).shape[0]), t.ny, t.nx, _p(v1, C.c_int32), _p(w1, C.c_double),
            _p(idx, C.c_int32), _p(sdf, C.c_double), _p(v2, C.c_int32), _p(w2, C.c_double), _p(mx, C.c_double),
            smd, smd, 0.05))
        self.tables = t
        if self.step == "poisson":
            self._bind_poisson(sdf.reshape(t.ny, t.nx))
        if self.step == "gradp":
            self._bind_gradp(sdf.reshape(t.ny, t.nx), array)
        elif smd:
            self.prime(array)
        return 0

    def _maxs4(self):
        """The four maxs of psm_set_geometry: the last four; step='gradp': (max_abs_Ux, max_abs_Uy, max_abs_dist, unused)."""
        return _f64(self.maxs[:3] + (1.0,)) if self.step == "gradp" else _f64(self.maxs[-4:])

    def _bind_gradp(self, sdfunct, array):
        """Everything a gradient-model step stands on; after it a step allocates nothing."""
        sur = self._sur
        dx, dy, extents, _ = gradp_grid_metrics(array, sur.ny, sur.nx)
        self.cut_used = tuple(int(v) for v in self.cut) if self.cut is not None else gradp_default_cut(sdfunct, array, self.delta)
        if self.apply_filter:
            sur.bind_poststeps(self.sigma_field, self.sigma_weight)
        sur.bind_gradp_solve(self.cut_used, dx, dy, extents, self.maxs[3:5], self.apply_filter, self.reference)

    def _bind_poisson(self, sdfunct):
        """Everything a Poisson-model step stands on, in the order the library asks for it; after it a step allocates nothing."""
        sur = self._sur
        sur.bind_features(sdfunct, self.k, self.maxs[:4])
        sur.bind_poststeps(self.sigma_field, self.sigma_weight)
        sur.bind_frames(1, 6)
        sur.bind_poisson_solve(self.phi, self.maxs[4], self.weighting, self.apply_filter)

    def _init_func_native(self, array, top_boundary, obst_boundary):
        """psm_set_case + psm_init_geometry: the tables are built inside the library (csrc/psm_geometry.cpp).  step='delta':
        psm_geometry_build + psm_set_geometry, which takes the deltas model's two flags (psm_init_geometry passes 0, 0)."""
        a, t, o = _f64(array), _f64(top_boundary), _f64(obst_boundary)
        lib = _lib.load()
        ny, nx = C.c_int32(), C.c_int32()
        if lib.psm_geometry_shape(_p(a, C.c_double), a.shape[0], self.delta, C.byref(ny), C.byref(nx), None):
            raise ValueError(lib.psm_geometry_last_error().decode())
        if self._sur is not None:
            self._sur.close()
        self._sur = GridSurrogate(self.model, ny.value, nx.value, 1, self.device)
        mx = self._maxs4()
        if self.step != "absolute":
            n, ng = a.shape[0], ny.value * nx.value
            v1, w1, idx, sdf = np.empty((ng, 3), np.int32), np.empty((ng, 3)), np.empty((ng, 2), np.int32), np.empty(ng)
            v2, w2 = np.empty((n, 3), np.int32), np.empty((n, 3))
            if lib.psm_geometry_build(_p(a, C.c_double), n, _p(t, C.c_double), t.shape[0], _p(o, C.c_double), o.shape[0], self.delta, 10,
                                      _p(v1, C.c_int32), _p(w1, C.c_double), _p(idx, C.c_int32), _p(sdf, C.c_double),
                                      _p(v2, C.c_int32), _p(w2, C.c_double)):
                raise ValueError(lib.psm_geometry_last_error().decode())
            self._sur._chk(lib.psm_set_geometry(self._sur.h, n, ny.value, nx.value, _p(v1, C.c_int32), _p(w1, C.c_double),
                                                _p(idx, C.c_int32), _p(sdf, C.c_double), _p(v2, C.c_int32), _p(w2, C.c_double),
                                                _p(mx, C.c_double), 1, 1, 0.05))
            self.tables = "native"
            if self.step == "poisson":
                self._bind_poisson(sdf.reshape(ny.value, nx.value))
            if self.step == "gradp":
                self._bind_gradp(sdf.reshape(ny.value, nx.value), a)
            else:
                self.prime(a)
            return 0
        self._sur._chk(lib.psm_set_case(self._sur.h, _p(mx, C.c_double), self.delta, 10, 0.05))
        self._sur._chk(lib.psm_init_geometry(self._sur.h, _p(a, C.c_double), a.shape[0], _p(t, C.c_double), t.shape[0],
                                             _p(o, C.c_double), o.shape[0], 0))
        self.tables = "native"
        return 0

    # -- the state of step='delta' (psm_delta_prime / _reset / _state) and of step='poisson' (psm_poisson_solve_push / _reset / _state)
    def _need_delta(self, what="state"):
        if self.step == "absolute":
            raise RuntimeError("this module was built with step='absolute': the state belongs to step='delta'")
        if self.step == "gradp":
            _no_gradp_state(what)
        if self.tables is None:
            raise RuntimeError("init_func has not been called")

    def prime(self, array):
        """U(t-1) := array[:,0:2].  ``init_func`` does this with the start fields; a restart primes again.  step='poisson': one
        frame (U and p) is pushed into the two-frame state; a restart primes with two."""
        self._need_delta()
        a = _f64(array)
        if a.ndim != 2 or a.shape[1] != 5:
            raise ValueError("array must be [N,5] = (Ux, Uy, Cx, Cy, p)")
        if self.step == "poisson":
            self._sur._chk(self._sur.lib.psm_poisson_solve_push(self._sur.h, _p(a, C.c_double), a.shape[0]))
            return
        self._sur._chk(self._sur.lib.psm_delta_prime(self._sur.h, _p(a, C.c_double), a.shape[0]))

    def reset_state(self):
        """Forget U(t-1): the next ``py_func`` is the priming step and returns ``array[:,4]``."""
        self._need_delta()
        if self.step == "poisson":
            self._sur._chk(self._sur.lib.psm_poisson_solve_reset(self._sur.h))
            return
        self._sur._chk(self._sur.lib.psm_delta_reset(self._sur.h))

    @property
    def state(self):
        """(primed, steps) of psm_delta_state; step='poisson': (frames held, steps) of psm_poisson_solve_state."""
        self._need_delta()
        return _poisson_state(self._sur) if self.step == "poisson" else _delta_state(self._sur)

    def pin(self, array: np.ndarray, out: np.ndarray = None):
        """psm_pin_buffers: register the caller's persistent [N,5] float64 array (and optionally a persistent output
        array) for direct DMA; later ``py_func(array, out=out)`` calls with exactly these arrays skip the staging copies.
        The caller keeps both arrays alive until ``unpin()`` / a new ``init_func``."""
        if array.dtype != np.float64 or not array.flags.c_contiguous or (out is not None and (out.dtype != np.float64 or not out.flags.c_contiguous)):
            raise ValueError("contiguous float64 arrays expected")
        self._sur._chk(self._sur.lib.psm_pin_buffers(self._sur.h, _p(array, C.c_double), _p(out, C.c_double) if out is not None else None))
        self._pinned = (array, out)

    def unpin(self):
        self._sur._chk(self._sur.lib.psm_unpin_buffers(self._sur.h))
        self._pinned = None

    def py_func_begin(self, array_in, out: np.ndarray = None):
        """First half of :meth:`py_func` (psm_solve_begin): enqueue the step and return; several SolverModules (cases)
        can be advanced from one thread by calling begin on all of them, then :meth:`py_func_end` on each."""
        if self.tables is None:
            raise RuntimeError("init_func has not been called")
        if self.step == "poisson":
            raise RuntimeError("step='poisson' has no begin / end halves: use py_func")
        if self.step == "gradp":
            _no_gradp_state("begin / end halves")
        if self.step == "delta":
            a, out = _check_cells(array_in, out)
            self._sur._chk(self._sur.lib.psm_solve_delta_begin(self._sur.h, _p(a, C.c_double), a.shape[0], 0, _p(out, C.c_double)))
            self._inflight = (a, out)
            return
        a = _f64(array_in)
        if a.ndim != 2 or a.shape[1] != 5:
            raise ValueError("array must be [N,5] = (Ux, Uy, Cx, Cy, p)")
        if out is None:
            out = np.empty(a.shape[0], np.float64)
        self._sur._chk(self._sur.lib.psm_solve_begin(self._sur.h, _p(a, C.c_double), a.shape[0], 0, _p(out, C.c_double)))
        self._inflight = (a, out)                       # keeps both arrays alive until the end call (set only once the step is in flight)

    def py_func_end(self) -> np.ndarray:
        if self.step == "gradp":
            _no_gradp_state("begin / end halves")
        end = self._sur.lib.psm_solve_delta_end if self.step == "delta" else self._sur.lib.psm_solve_end
        self._sur._chk(end(self._sur.h))
        a, out = self._inflight
        self._inflight = None
        return out

    def py_func(self, array_in, placeholder=0, out: np.ndarray = None) -> np.ndarray:
        """python_module.py:249: cells [N,5] float64 -> p [N] float64.  step='delta': p = array[:,4] + dp (psm_solve_delta);
        step='poisson': likewise through psm_solve_poisson."""
        if self.tables is None:
            raise RuntimeError("init_func has not been called")
        if self.step == "poisson":
            a, out = _check_cells(array_in, out)
            self._sur._chk(self._sur.lib.psm_solve_poisson(self._sur.h, _p(a, C.c_double), a.shape[0], int(placeholder), _p(out, C.c_double)))
            return out
        if self.step == "gradp":
            a, out = _check_cells(array_in, out)
            self._sur._chk(self._sur.lib.psm_solve_gradp(self._sur.h, _p(a, C.c_double), a.shape[0], int(placeholder), _p(out, C.c_double)))
            return out
        if self.step == "delta":
            a, out = _check_cells(array_in, out)
            self._sur._chk(self._sur.lib.psm_solve_delta(self._sur.h, _p(a, C.c_double), a.shape[0], int(placeholder), _p(out, C.c_double)))
            return out
        a = _f64(array_in)
        if a.ndim != 2 or a.shape[1] != 5:
            raise ValueError("array must be [N,5] = (Ux, Uy, Cx, Cy, p)")
        if out is None:
            out = np.empty(a.shape[0], np.float64)
        self._sur._chk(self._sur.lib.psm_solve(self._sur.h, _p(a, C.c_double), a.shape[0], int(placeholder),
                                                _p(out, C.c_double)))
        return out


class SolverEnsemble:
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
    and ``apply_filter`` (default off) of :class:`SolverModule`, on ``psm_solve_cases_gradp``: no state, no begin / end halves."""

    def __init__(self, model: SurrogateModel, maxs=(1.0, 1.0, 1.0, 1.0), max_cases: int = 8, geometry: str = "native",
                 device: int = 0, delta: float = 5e-3, step: str = "absolute", phi: float = None, k: float = None, weighting: bool = True,
                 apply_filter: bool = None, sigma_field=(10, 10), sigma_weight=(50, 50), cut=None, reference: str = "outlet"):
        if geometry not in ("scipy", "native"):
            raise ValueError("geometry must be 'scipy' or 'native'")
        self.step = _check_step(step, MODULE_STEPS)
        self.model, self.maxs, self.max_cases = model, tuple(float(v) for v in maxs), int(max_cases)
        self.geometry, self.device, self.delta = geometry, device, delta
        if self.step == "poisson":
            _check_poisson(self.maxs, phi, k)
            self.phi, self.k, self.weighting, self.apply_filter = float(phi), float(k), bool(weighting), apply_filter is None or bool(apply_filter)
            self.sigma_field, self.sigma_weight = tuple(sigma_field), tuple(sigma_weight)
        if self.step == "gradp":
            _check_gradp(self.maxs, reference)
            self.cut, self.reference, self.apply_filter = cut, reference, bool(apply_filter)
            self.sigma_field, self.sigma_weight = tuple(sigma_field), tuple(sigma_weight)
        self._sur = None
        self.tables = None
        self.cell_off = None
        self._inflight = None

    @staticmethod
    def _ptrs(arrays):
        return (C.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])

    def init_func(self, arrays, tops, obsts):
        """One-time tables of every case; all cases must give the same grid shape.  Returns 0."""
        if not (len(arrays) == len(tops) == len(obsts)) or not 1 <= len(arrays) <= self.max_cases:
            raise ValueError("one (array, top, obst) per case, 1..max_cases cases")
        lib = _lib.load()
        K = len(arrays)
        a, t, o = [_f64(x) for x in arrays], [_f64(x) for x in tops], [_f64(x) for x in obsts]
        mx = _f64(self.maxs[:3] + (1.0,)) if self.step == "gradp" else _f64(self.maxs[-4:])
        if self.geometry == "native":
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
        n = (C.c_int64 * K)(*[x.shape[0] for x in a])
        smd = int(self.step != "absolute")       # the deltas model's convention: normalise_sdf = fill_input = 1 (SM_call.py:441-443)
        if self.geometry == "native" and smd:    # psm_init_geometry_cases passes 0, 0: build the tables, hand them over with 1, 1
            ng = ny * nx
            keep = [[np.empty((rows or x.shape[0]) * width, dt) for x in a]      # vtx_m2g, wts_m2g, indices, sdfunct, vtx_g2m, wts_g2m
                    for rows, width, dt in ((ng, 3, np.int32), (ng, 3, np.float64), (ng, 2, np.int32), (ng, 1, np.float64),
                                            (0, 3, np.int32), (0, 3, np.float64))]
            for k in range(K):
                v1, w1, idx, sdf, v2, w2 = (col[k] for col in keep)
                if lib.psm_geometry_build(_p(a[k], C.c_double), a[k].shape[0], _p(t[k], C.c_double), t[k].shape[0], _p(o[k], C.c_double),
                                          o[k].shape[0], self.delta, 10, _p(v1, C.c_int32), _p(w1, C.c_double), _p(idx, C.c_int32),
                                          _p(sdf, C.c_double), _p(v2, C.c_int32), _p(w2, C.c_double)):
                    raise ValueError(f"case {k}: " + lib.psm_geometry_last_error().decode())
            sur._chk(lib.psm_set_geometry_cases(sur.h, K, n, ny, nx, *[self._ptrs(col) for col in keep], _p(mx, C.c_double), 1, 1, 0.05))
        elif self.geometry == "native":
            sur._chk(lib.psm_set_case(sur.h, _p(mx, C.c_double), self.delta, 10, 0.05))
            sur._chk(lib.psm_init_geometry_cases(sur.h, K, self._ptrs(a), n, self._ptrs(t), (C.c_int64 * K)(*[x.shape[0] for x in t]),
                                                 self._ptrs(o), (C.c_int64 * K)(*[x.shape[0] for x in o])))
        else:
            keep = [[np.ascontiguousarray(getattr(g, f), dt) for g in tables]
                    for f, dt in (("vtx_m2g", np.int32), ("wts_m2g", np.float64), ("indices", np.int32), ("sdfunct", np.float64),
                                  ("vtx_g2m", np.int32), ("wts_g2m", np.float64))]
            sur._chk(lib.psm_set_geometry_cases(sur.h, K, n, ny, nx, *[self._ptrs(col) for col in keep], _p(mx, C.c_double), smd, smd, 0.05))
        off = (C.c_int64 * (K + 1))()
        sur._chk(lib.psm_mesh_cases(sur.h, None, off))
        self.cell_off = [int(v) for v in off]
        self.tables = tables
        if self.step == "poisson":               # everything a step stands on, in the order the library asks for it (keep[3]: the K sdfuncts)
            sur.bind_features(np.stack([np.asarray(sd, np.float64).reshape(ny, nx) for sd in keep[3]]), self.k, self.maxs[:4])
            sur.bind_poststeps(self.sigma_field, self.sigma_weight)
            sur.bind_poisson_solve_cases(self.phi, self.maxs[4], self.weighting, self.apply_filter)
        if self.step == "gradp":                 # the grid is case 0's (all cases share its shape and bounds); keep[3]: the K sdfuncts
            dx, dy, extents, _ = gradp_grid_metrics(a[0], ny, nx)
            sdfs = [np.asarray(sd, np.float64).reshape(ny, nx) for sd in keep[3]]
            self.cuts_used = ([tuple(int(v) for v in c) for c in self.cut] if self.cut is not None
                              else [gradp_default_cut(sdfs[k], a[k], self.delta) for k in range(K)])
            if self.apply_filter:
                sur.bind_poststeps(self.sigma_field, self.sigma_weight)
            sur.bind_gradp_solve_cases(self.cuts_used, dx, dy, extents, self.maxs[3:5], self.apply_filter, self.reference)
        elif smd:
            self.prime(a)
        return 0

    # -- the state of step='delta' (psm_delta_prime_cases / psm_delta_reset / psm_delta_state) and of step='poisson'
    # (psm_poisson_solve_push_cases / psm_poisson_solve_reset / psm_poisson_solve_state)
    def _need_delta(self, what="state"):
        if self.step == "absolute":
            raise RuntimeError("this ensemble was built with step='absolute': the state belongs to step='delta'")
        if self.step == "gradp":
            _no_gradp_state(what)

    def prime(self, arrays):
        """U(t-1) := arrays[k][:,0:2] for every case.  ``init_func`` does this with the start fields.  step='poisson': one frame
        (U and p) of every case is pushed into the two-frame state; a restart primes with two."""
        self._need_delta()
        cells, _ = self._pack(arrays)
        if self.step == "poisson":
            self._sur._chk(self._sur.lib.psm_poisson_solve_push_cases(self._sur.h, _p(cells, C.c_double)))
            return
        self._sur._chk(self._sur.lib.psm_delta_prime_cases(self._sur.h, _p(cells, C.c_double)))

    def reset_state(self):
        self._need_delta()
        if self.tables is None:
            raise RuntimeError("init_func has not been called")
        if self.step == "poisson":
            self._sur._chk(self._sur.lib.psm_poisson_solve_reset(self._sur.h))
            return
        self._sur._chk(self._sur.lib.psm_delta_reset(self._sur.h))

    @property
    def state(self):
        """(primed, steps) of psm_delta_state; step='poisson': (frames held, steps) of psm_poisson_solve_state."""
        self._need_delta()
        if self.tables is None:
            raise RuntimeError("init_func has not been called")
        return _poisson_state(self._sur) if self.step == "poisson" else _delta_state(self._sur)

    def _entry(self, name):
        return getattr(self._sur.lib, name.replace("psm_solve_cases", "psm_solve_cases_delta") if self.step == "delta" else name)

    def _pack(self, arrays):
        if self.tables is None:
            raise RuntimeError("init_func has not been called")
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

    def _split(self, p):
        return [p[self.cell_off[k]:self.cell_off[k + 1]] for k in range(len(self.cell_off) - 1)]

    def py_func_begin(self, arrays):
        """First half of :meth:`py_func` (psm_solve_cases_begin): enqueue the step of all cases and return."""
        if self.step == "poisson":
            raise RuntimeError("step='poisson' has no begin / end halves: use py_func")
        if self.step == "gradp":
            _no_gradp_state("begin / end halves")
        cells, p = self._pack(arrays)
        self._sur._chk(self._entry("psm_solve_cases_begin")(self._sur.h, _p(cells, C.c_double), _p(p, C.c_double)))
        self._inflight = (cells, p)                     # keeps both arrays alive until the end call

    def py_func_end(self):
        if self.step == "gradp":
            _no_gradp_state("begin / end halves")
        self._sur._chk(self._entry("psm_solve_cases_end")(self._sur.h))
        cells, p = self._inflight
        self._inflight = None
        return self._split(p)

    def py_func(self, arrays):
        """One step of every case: list of cells [N_i,5] float64 -> list of p_i [N_i] float64."""
        cells, p = self._pack(arrays)
        if self.step == "poisson":
            self._sur._chk(self._sur.lib.psm_solve_cases_poisson(self._sur.h, _p(cells, C.c_double), _p(p, C.c_double)))
            return self._split(p)
        if self.step == "gradp":
            self._sur._chk(self._sur.lib.psm_solve_cases_gradp(self._sur.h, _p(cells, C.c_double), _p(p, C.c_double)))
            return self._split(p)
        self._sur._chk(self._entry("psm_solve_cases")(self._sur.h, _p(cells, C.c_double), _p(p, C.c_double)))
        return self._split(p)
