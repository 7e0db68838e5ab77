"""The solver boundary of the convolutional path (include/psm_unet.h, ``psm_unet_mesh_*`` / ``psm_unet_solve*``):
``UNetSolverModule`` (one mesh: ``init_func`` / ``py_func`` with the reference's signatures, python_module.py:172, :249) and
``UNetSolverEnsemble`` (K meshes on one grid shape advanced by one call), the U-Net in the place ``SolverModule`` and
``SolverEnsemble`` (solver.py) give the PCA model.  cells [N,5] float64 -> p [N] float64, mesh -> canvas -> network -> mesh on the
device; the grid shape is the geometry's own and may be any shape: the network runs on the canvas of ``psm_unet_canvas_shape``
(both axes rounded up to multiples of 2^(levels-1), zero padding -- a build-defined rule, the conv path has no reference network).
Everything numeric runs in the HIP library; there is no CPU fallback."""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np

from . import _lib, geometry as _geometry
from .solver import _F64P, _TABLES, _check_cells, _check_step
from .unet import WIDTHS_S, UNetSurrogate


def canvas_shape(n_levels: int, ny: int, nx: int):
    """(ny_c, nx_c) of psm_unet_canvas_shape."""
    a, b = C.c_int32(), C.c_int32()
    if _lib.load().psm_unet_canvas_shape(n_levels, ny, nx, C.byref(a), C.byref(b)):
        raise ValueError("bad network depth or grid shape")
    return a.value, b.value


class _UNetSolverBase:
    """What the module (CASES = 0) and the ensemble (CASES = 1) share: the constructor's checks, ``init_func``'s body, the state of
    step='delta' and the introspection of the last step.  A class keeps its own signatures and the packing of its cells."""
    CASES = 0

    def __init__(self, weights, maxs, widths, precision, step, geometry, delta, device, max_cases):
        if geometry not in ("scipy", "native"):
            raise ValueError("geometry must be 'scipy' or 'native'")
        self.step = _check_step(step)
        if precision not in _lib.PRECISIONS:
            raise ValueError("precision must be 'f32' or 'bf16'")
        self.maxs = tuple(float(v) for v in maxs)
        if len(self.maxs) != 4:
            raise ValueError("maxs must be (max_abs_Ux, max_abs_Uy, max_abs_dist, max_abs_p); step='delta': (max_abs_dUx, max_abs_dUy, max_abs_dist, max_abs_dp)")
        if int(max_cases) < 1:
            raise ValueError("max_cases must be at least 1")
        self.weights, self.widths, self.precision = weights, tuple(int(w) for w in widths), precision
        self.geometry, self.delta, self.device, self.max_cases = geometry, float(delta), int(device), int(max_cases)
        self.net = self.h = self.tables = self.cell_off = None
        self.lib = None

    def _chk(self, rc):
        if rc:
            raise _lib.PsmError(rc, (self.lib.psm_unet_mesh_last_error(self.h) or b"").decode())

    def _need_init(self):
        if self.tables is None:
            raise RuntimeError("init_func has not been called")

    def close(self):
        if self.h is not None and self.h:
            self.lib.psm_unet_mesh_destroy(self.h)             # the binding first: it runs on the network
        self.h = None
        if self.net is not None:
            self.net.close()
        self.net = self.tables = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _init(self, arrays, tops, obsts):
        """The six tables per case (psm_geometry_build or geometry.build_geometry), the network planned for their canvas, the
        binding, psm_unet_mesh_set_geometry with the step's two flags (the deltas model's convention is SDF / max_abs_dist and
        interpolate_fill, SM_call.py:441-443); step='delta' primes U(t-1) with the start fields."""
        K = len(arrays)
        a = [np.ascontiguousarray(x, np.float64) for x in arrays]
        build = _geometry.build_geometry_native if self.geometry == "native" else _geometry.build_geometry
        tables = [build(a[k], np.ascontiguousarray(tops[k], np.float64), np.ascontiguousarray(obsts[k], np.float64), self.delta) for k in range(K)]
        ny, nx = tables[0].ny, tables[0].nx
        if any((g.ny, g.nx) != (ny, nx) for g in tables):
            raise ValueError("the cases of an ensemble must share one grid shape")
        self.close()
        self.lib = _lib.load()
        self.ny, self.nx = ny, nx
        self.ny_c, self.nx_c = canvas_shape(len(self.widths), ny, nx)
        self.net = UNetSurrogate(self.weights, self.ny_c, self.nx_c, widths=self.widths, max_cases=self.max_cases, device=self.device,
                                 precision=self.precision)
        h = C.c_void_p()
        rc = self.lib.psm_unet_mesh_create(self.net.h, self.device, self.ny_c, self.nx_c, self.max_cases, _lib.UNET_STEPS[self.step], C.byref(h))
        if rc:
            msg = (self.lib.psm_unet_mesh_last_error(None) or b"").decode()
            self.close()
            raise _lib.PsmError(rc, msg)
        self.h = h
        cols = [[np.ascontiguousarray(getattr(g, f), dt) for g in tables] for f, _, _, dt, _ in _TABLES]
        ptrs = [(C.c_void_p * K)(*[x.ctypes.data for x in col]) for col in cols]
        mx = np.asarray(self.maxs, np.float64)
        flag = 1 if self.step == "delta" else 0
        self._chk(self.lib.psm_unet_mesh_set_geometry(self.h, K, (C.c_int64 * K)(*[x.shape[0] for x in a]), ny, nx, *ptrs,
                                                      mx.ctypes.data_as(_F64P), flag, flag, 0.05))
        self.cell_off = [0] + [int(v) for v in np.cumsum([x.shape[0] for x in a])]
        self.tables = tables if self.CASES else tables[0]
        if self.step == "delta":
            self.prime(arrays if self.CASES else arrays[0])
        return 0

    # -- one library call on the packed cells
    def _solve(self, cells, p):
        self._chk(self.lib.psm_unet_solve(self.h, cells.ctypes.data_as(_F64P), p.ctypes.data_as(_F64P)))
        return p

    # -- the state of step='delta'
    def _need_state(self):
        if self.step != "delta":
            raise RuntimeError("this object was built with step='absolute': the state belongs to step='delta'")
        self._need_init()

    def prime(self, arrays):
        """U(t-1) := array[:,0:2] (of every case).  ``init_func`` does this with the start fields; a restart primes again."""
        self._need_state()
        cells = self._pack(arrays)[0]
        self._chk(self.lib.psm_unet_mesh_prime(self.h, cells.ctypes.data_as(_F64P)))

    def reset_state(self):
        """Forget U(t-1): the next ``py_func`` is the priming step and returns ``array[:,4]``."""
        self._need_state()
        self._chk(self.lib.psm_unet_mesh_reset(self.h))

    @property
    def state(self):
        """(primed, steps) of psm_unet_mesh_state."""
        self._need_state()
        primed, steps = C.c_int32(), C.c_int64()
        self._chk(self.lib.psm_unet_mesh_state(self.h, C.byref(primed), C.byref(steps)))
        return bool(primed.value), int(steps.value)

    # -- the last step's image, field and U_max (psm_unet_mesh_read)
    def read(self, what: str) -> np.ndarray:
        """'canvas' [K,ny_c,nx_c,3] float32, 'field' [K,ny_c,nx_c] float32 or 'umax' [K] float64 of the last step."""
        self._need_init()
        K = len(self.cell_off) - 1
        out = {"canvas": lambda: np.empty((K, self.ny_c, self.nx_c, 3), np.float32), "field": lambda: np.empty((K, self.ny_c, self.nx_c), np.float32),
               "umax": lambda: np.empty(K, np.float64)}[what]()
        self._chk(self.lib.psm_unet_mesh_read(self.h, _lib.UNET_READ[what], out.ctypes.data, out.nbytes))
        return out


class UNetSolverModule(_UNetSolverBase):
    """``init_func`` / ``py_func`` of the reference's python_module.py on one mesh, the U-Net behind them.  ``weights``: the
    convolutions of :class:`UNetSurrogate` (stem c_in 3, head c_out 1) for ``widths``; ``maxs`` = (max_abs_Ux, max_abs_Uy,
    max_abs_dist, max_abs_p); ``step``: 'absolute' (U -> p) or 'delta' ([U(t) - U(t-1)], SDF -> p(t) - p(t-1): ``maxs`` are the
    deltas model's, ``init_func`` primes U(t-1) with its own ``array`` and ``py_func`` returns ``array[:,4] + dp``); ``geometry``:
    who builds ``init_func``'s tables, 'scipy' (geometry.build_geometry) or 'native' (psm_geometry_build) -- see
    :class:`SolverModule`; ``delta``: the grid spacing."""

    def __init__(self, weights, maxs=(1.0, 1.0, 1.0, 1.0), widths: Sequence[int] = WIDTHS_S, precision: str = "f32", step: str = "absolute",
                 geometry: str = "scipy", delta: float = 5e-3, device: int = 0):
        super().__init__(weights, maxs, widths, precision, step, geometry, delta, device, 1)

    def init_func(self, array, top_boundary, obst_boundary, placeholder=0):
        return self._init([array], [top_boundary], [obst_boundary])

    def _pack(self, array, out=None):
        a, out = _check_cells(array, out)
        if a.shape[0] != self.cell_off[-1]:
            raise ValueError("array must be [N,5] = (Ux, Uy, Cx, Cy, p) with the cell count of init_func")
        return a, out

    def py_func(self, array_in, placeholder=0, out: np.ndarray = None) -> np.ndarray:
        """python_module.py:249: cells [N,5] float64 -> p [N] float64 (psm_unet_solve)."""
        self._need_init()
        return self._solve(*self._pack(array_in, out))


class UNetSolverEnsemble(_UNetSolverBase):
    """:class:`UNetSolverModule` for K <= ``max_cases`` meshes that share one grid shape, all advanced by one call: ``init_func``
    takes one (array, top, obst) per case, ``py_func`` one [N_i,5] array per case and returns the list of p_i.  step='delta': one
    state for the set."""
    CASES = 1

    def __init__(self, weights, maxs=(1.0, 1.0, 1.0, 1.0), widths: Sequence[int] = WIDTHS_S, precision: str = "f32", step: str = "absolute",
                 geometry: str = "native", delta: float = 5e-3, device: int = 0, max_cases: int = 8):
        super().__init__(weights, maxs, widths, precision, step, geometry, delta, device, max_cases)

    def init_func(self, arrays, tops, obsts):
        if not (len(arrays) == len(tops) == len(obsts)) or not 1 <= len(arrays) <= self.max_cases:
            raise ValueError("one (array, top, obst) per case, 1..max_cases cases")
        return self._init(arrays, tops, obsts)

    def _pack(self, arrays, out=None):
        K, off = len(self.cell_off) - 1, self.cell_off
        if len(arrays) != K:
            raise ValueError(f"{K} cases were initialised")
        cells = np.empty((off[-1], 5), np.float64)
        for k, x in enumerate(arrays):
            x = np.asarray(x)
            if x.shape != (off[k + 1] - off[k], 5):
                raise ValueError("array must be [N,5] = (Ux, Uy, Cx, Cy, p) with the cell count of init_func")
            cells[off[k]:off[k + 1]] = x
        return cells, np.empty(off[-1], np.float64)

    def py_func(self, arrays):
        """One step of every case: list of cells [N_i,5] float64 -> list of p_i [N_i] float64."""
        self._need_init()
        p = self._solve(*self._pack(arrays))
        return [p[self.cell_off[k]:self.cell_off[k + 1]] for k in range(len(self.cell_off) - 1)]
