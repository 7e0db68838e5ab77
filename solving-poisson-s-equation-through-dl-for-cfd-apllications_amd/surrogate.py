"""Host-side mirror of the reference's surrogate interface on top of the C-ABI.

``GridSurrogate`` owns one ``psm_handle`` (include/psm.h).  The two
``Evaluation*`` classes keep the names, argument order and meaning of the
reference operators for the part of the path that is built so far
(SURVEY.md §8 a7-a12):

* ``pressureSM_deltas.SM_call.Evaluation`` -- ``assemble_prediction`` (SM_call.py:182)
  and the grid-native body of ``timeStep`` (SM_call.py:452-575),
* ``U_to_gradP`` ``Evaluation`` -- ``assemble_prediction`` (Eval_dual_Dense_onlycil.py:255)
  and the grid-native body of ``timeStep`` (:470-547),
* the Chapter-5 solver module -- the grid-native body of ``py_func``
  (python_module.py:299-473) as ``SolverModule.py_func_grid``.

Everything numeric runs in the HIP library; NumPy is only used to hand buffers
over.  Error behaviour follows the reference where it has one (``ValueError(
"Standardization method not valid")``, SM_call.py:525), otherwise ``PsmError``.
"""
from __future__ import annotations

import ctypes as C
import os
import re
from typing import Optional, Sequence

import numpy as np

from . import _lib
from .synthetic import SurrogateModel


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _fold_switch_on() -> bool:
    """PSM_SDF_FOLD as the library reads it (``atoi(value) == 0`` switches the fold off; unset: on)."""
    e = os.environ.get("PSM_SDF_FOLD")
    if e is None:
        return True
    m = re.match(r"\s*[+-]?\d+", e)
    return (int(m.group(0)) if m else 0) != 0


class GridSurrogate:
    """One surrogate model bound to one uniform grid shape on one GPU."""

    def __init__(self, model: SurrogateModel, ny: int, nx: int, max_cases: int = 1, device: int = 0,
                 strict_degenerate: bool = False, precision: str = "f32"):
        if precision not in _lib.PRECISIONS:
            raise ValueError("precision must be 'f32' or 'bf16'")
        if model.scaler_kind not in _lib.SCALERS:
            raise ValueError("Standardization method not valid")
        self.lib = _lib.load()
        self.model, self.ny, self.nx, self.max_cases = model, int(ny), int(nx), int(max_cases)
        self.precision = precision
        cfg = _lib.psm_config(
            abi_version=_lib.PSM_ABI_VERSION, variant=_lib.VARIANTS[model.variant], block=model.S,
            overlap=0 if model.ov is None else int(model.ov), c_in=model.c_in, c_out=model.c_out,
            p_in=model.p_in, p_out=model.p_out, n_dense=len(model.weights) + (1 if getattr(model, "attention", None) else 0),
            scaler=_lib.SCALERS[model.scaler_kind],
            sdf_channel=model.sdf_ch, device=device, max_cases=max_cases, strict_degenerate=int(strict_degenerate),
            precision=_lib.PRECISIONS[precision])
        h = C.c_void_p()
        _lib.check(self.lib.psm_create(C.byref(cfg), C.byref(h)))
        self.h = h
        self._ticket_cases = {}
        try:
            ci, mi, co, mo = _f64(model.comp_in), _f64(model.mean_in), _f64(model.comp_out), _f64(model.mean_out)
            if ci.shape != (model.p_in, model.S ** 2 * model.c_in) or co.shape != (model.p_out, model.S ** 2 * model.c_out):
                raise ValueError("PCA component matrices have the wrong shape")
            self._chk(self.lib.psm_set_pca(h, _p(ci, C.c_double), _p(mi, C.c_double), _p(co, C.c_double), _p(mo, C.c_double)))
            convs = list(getattr(model, "conv1d", None) or [])
            for l, (K, b) in enumerate(convs):                  # conv1D_PCA head: before the Dense layers
                K, b = _f32(K), _f32(b)
                if K.ndim != 3 or b.shape != (K.shape[2],):
                    raise ValueError("Conv1D kernels must be [kernel_size, c_in, c_out] with bias [c_out]")
                self._chk(self.lib.psm_set_conv1d(h, l, len(convs), K.shape[0], K.shape[1], K.shape[2], _p(K, C.c_float), _p(b, C.c_float)))
            att = getattr(model, "attention", None)
            for l, (W, b) in enumerate(model.weights):
                W, b = _f32(W), _f32(b)
                # densePCA_attention: the attention block takes Dense slot 1, the further layers move up by one
                slot = l + 1 if (att and l > 0) else l
                self._chk(self.lib.psm_set_dense(h, slot, W.shape[0], W.shape[1], _p(W, C.c_float), _p(b, C.c_float)))
            if att:
                self._set_attention(att, len(model.weights) - 1)
            ia = _f64(np.broadcast_to(model.in_a, (model.p_in,)))
            ib = _f64(np.broadcast_to(model.in_b, (model.p_in,)))
            oa = _f64(np.broadcast_to(model.out_a, (model.p_out,)))
            ob = _f64(np.broadcast_to(model.out_b, (model.p_out,)))
            self._chk(self.lib.psm_set_scaler(h, _p(ia, C.c_double), _p(ib, C.c_double), _p(oa, C.c_double), _p(ob, C.c_double)))
            self._chk(self.lib.psm_plan_grid(h, self.ny, self.nx))
            self.B = self.lib.psm_num_blocks(h)
        except Exception:
            self.close()
            raise

    def _set_attention(self, att: dict, n_layers: int):
        """The attention part of densePCA_attention (NNs.py:53-64) -> psm_set_attention (slot 1) + one psm_set_layernorm per
        layer; the query / key projections are not passed on: over a sequence of length 1 they cannot change the result."""
        Wv, bv, Wo, bo = _f32(att["Wv"]), _f32(att["bv"]), _f32(att["Wo"]), _f32(att["bo"])
        d, heads, dim = Wv.shape
        if bv.shape != (heads, dim) or Wo.shape != (heads, dim, d) or bo.shape != (d,):
            raise ValueError("attention weights: Wv [d, heads, dim], bv [heads, dim], Wo [heads, dim, d], bo [d]")
        if len(att["ln"]) != n_layers:
            raise ValueError("densePCA_attention has one LayerNormalization per layer")
        self._chk(self.lib.psm_set_attention(self.h, 1, d, heads, dim, _p(Wv, C.c_float), _p(bv, C.c_float), _p(Wo, C.c_float), _p(bo, C.c_float)))
        for i, (g, b) in enumerate(att["ln"]):
            g, b = _f32(g), _f32(b)
            self._chk(self.lib.psm_set_layernorm(self.h, 1 + i, g.shape[0], _p(g, C.c_float), _p(b, C.c_float),
                                                 float(att.get("eps", 1e-3)), 0 if i == 0 else 1))

    # -- plumbing
    def _chk(self, rc):
        return _lib.check(rc, self.h)

    def close(self):
        if getattr(self, "h", None):
            self.lib.psm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- solves
    def solve(self, grid: np.ndarray, out_scale: Optional[Sequence[float]] = None) -> np.ndarray:
        """grid [Ny,Nx,>=c_in] or [n,Ny,Nx,>=c_in] (normalised, PM:288-297) -> fields [n,Ny,Nx,c_out] f32."""
        g = np.asarray(grid)
        if g.ndim == 3:
            g = g[None]
        if g.ndim != 4 or g.shape[1:3] != (self.ny, self.nx) or g.shape[3] < self.model.c_in:
            raise ValueError(f"grid must be [n,{self.ny},{self.nx},>={self.model.c_in}]")
        g = _f32(g[..., :self.model.c_in])
        n = g.shape[0]
        self._check_bound(g)
        out = np.empty((n, self.ny, self.nx, self.model.c_out), np.float32)
        sc = None
        if out_scale is not None:
            sc = _f32(np.broadcast_to(out_scale, (n,)))
        self._chk(self.lib.psm_solve_grid(self.h, _p(g, C.c_float), n, _p(sc, C.c_float) if sc is not None else None,
                                          _p(out, C.c_float)))
        return out

    def submit(self, grid: np.ndarray, out_scale: Optional[Sequence[float]] = None, out: Optional[np.ndarray] = None) -> int:
        """Asynchronous host-buffer solve (psm_submit_grid_io): returns a ticket; up to PSM_RING_SLOTS (8) in
        flight, each on its own stream (H2D copy, kernels and D2H copy of one ticket are one graph replay).  A pageable
        ``grid`` may be reused on return; a grid / ``out`` array inside a range registered with :meth:`host_register` is
        DMA'd from / into directly and must be left alone until :meth:`wait` returns."""
        g = np.asarray(grid)
        if g.ndim == 3:
            g = g[None]
        if g.ndim != 4 or g.shape[1:3] != (self.ny, self.nx) or g.shape[3] < self.model.c_in:
            raise ValueError(f"grid must be [n,{self.ny},{self.nx},>={self.model.c_in}]")
        g = _f32(g[..., :self.model.c_in])
        n = g.shape[0]
        self._check_bound(g)
        sc = _f32(np.broadcast_to(out_scale, (n,))) if out_scale is not None else None
        if out is not None and (out.dtype != np.float32 or not out.flags.c_contiguous or out.size != n * self.ny * self.nx * self.model.c_out):
            raise ValueError("out must be a contiguous float32 array [n,Ny,Nx,c_out]")
        t = C.c_int64(-1)
        self._chk(self.lib.psm_submit_grid_io(self.h, _p(g, C.c_float), n, _p(sc, C.c_float) if sc is not None else None,
                                              _p(out, C.c_float) if out is not None else None, C.byref(t)))
        self._ticket_cases[t.value] = (n, out, g)               # keeps the arrays alive while the DMA may touch them
        return t.value

    def wait(self, ticket: int) -> np.ndarray:
        """Field(s) of a ticket returned by :meth:`submit` -> [n,Ny,Nx,c_out] f32 (blocks until it has arrived)."""
        rec = self._ticket_cases.get(ticket)
        if rec is None:
            raise ValueError("unknown ticket")
        n, out, _ = rec
        if out is None:
            out = np.empty((n, self.ny, self.nx, self.model.c_out), np.float32)
            self._chk(self.lib.psm_wait_grid(self.h, ticket, _p(out, C.c_float)))
        else:
            self._chk(self.lib.psm_wait_grid(self.h, ticket, None))
            out = out.reshape(n, self.ny, self.nx, self.model.c_out)
        del self._ticket_cases[ticket]
        return out

    # -- zero-copy ring: the caller packs straight into the slot's pinned memory
    def ring_acquire(self):
        """-> (ticket, grid_in [max_cases,Ny,Nx,c_in], fields_out [max_cases,Ny,Nx,c_out]): NumPy views of the next
        slot's pinned buffers (psm_ring_acquire)."""
        t, gi, fo = C.c_int64(-1), C.POINTER(C.c_float)(), C.POINTER(C.c_float)()
        self._chk(self.lib.psm_ring_acquire(self.h, C.byref(t), C.byref(gi), C.byref(fo)))
        gin = np.ctypeslib.as_array(gi, shape=(self.max_cases, self.ny, self.nx, self.model.c_in))
        fout = np.ctypeslib.as_array(fo, shape=(self.max_cases, self.ny, self.nx, self.model.c_out))
        return t.value, gin, fout

    def ring_submit(self, ticket: int, n_cases: int = 1, out_scale: Optional[Sequence[float]] = None):
        sc = _f32(np.broadcast_to(out_scale, (n_cases,))) if out_scale is not None else None
        self._chk(self.lib.psm_ring_submit(self.h, ticket, n_cases, _p(sc, C.c_float) if sc is not None else None))

    def ring_wait(self, ticket: int):
        self._chk(self.lib.psm_ring_wait(self.h, ticket))

    def ring_release(self, ticket: int):
        """Give an acquired, not yet submitted ticket back (psm_ring_release)."""
        self._chk(self.lib.psm_ring_release(self.h, ticket))

    def host_register(self, arr: np.ndarray):
        """Register a caller-owned contiguous array for direct DMA (psm_host_register); keep it alive until
        :meth:`host_unregister` / close."""
        if not arr.flags.c_contiguous:
            raise ValueError("contiguous array expected")
        self._chk(self.lib.psm_host_register(self.h, arr.ctypes.data_as(C.c_void_p), arr.nbytes))

    def host_unregister(self, arr: np.ndarray):
        self._chk(self.lib.psm_host_unregister(self.h, arr.ctypes.data_as(C.c_void_p)))

    def bind_geometry(self, grid, on_device: bool = False, n_cases: int = 1) -> bool:
        """Bind the obstacle geometry (SDF channel of ``grid`` [ny, nx, c_in], or a device pointer with
        ``on_device``; a case batch [n, ny, nx, c_in] binds one geometry per case slot) for the following solves with
        the same number of cases: 6 launches instead of 8 (7 instead of 9 for batches; ``psm_bind_geometry_cases``; the
        reference's computeOnlyOnce / init_func split).  Returns False -- and leaves the solves on the general
        path -- for configurations the fused path does not cover.  CONTRACT (as in psm.h): until unbind_geometry the
        SDF channel of every solved grid keeps the bound flow-cell pattern (``check_bound = True`` verifies it on the
        host-grid entries)."""
        if on_device:
            rc = self.lib.psm_bind_geometry_cases(self.h, C.c_void_p(int(grid)), int(n_cases), 1)
        else:
            g = np.ascontiguousarray(np.asarray(grid)[..., :self.model.c_in], np.float32)
            if g.ndim == 3:
                g = g[None]
            if g.ndim != 4 or g.shape[1:] != (self.ny, self.nx, self.model.c_in):
                raise ValueError(f"grid must be [{self.ny},{self.nx},{self.model.c_in}] or [n,{self.ny},{self.nx},{self.model.c_in}]")
            rc = self.lib.psm_bind_geometry_cases(self.h, g.ctypes.data_as(C.c_void_p), g.shape[0], 0)
        self._bound_mask = None
        self._bound_sdf = None
        if rc == -5:                    # PSM_ERR_UNSUPPORTED: configuration outside the fused path
            return False
        self._chk(rc)
        n = int(n_cases) if on_device else g.shape[0]
        m = np.empty((n, self.ny, self.nx), np.uint8)          # the pattern the library bound (also for device grids)
        self._chk(self.lib.psm_bound_mask(self.h, m.ctypes.data_as(C.POINTER(C.c_uint8)), m.size))
        self._bound_mask = m.astype(bool)
        # SDF fold of the bound single-case encode: the contract is then the SDF channel's VALUES.  The
        # conditions mirror fold_applies (psm_api_solve.cpp); a grid bound from a device pointer leaves the host check at the pattern
        # (the guard riders on the device compare the values in every case).
        if (not on_device and n == 1 and self.precision == "f32" and self.model.c_in >= 2
                and self.model.sdf_ch == self.model.c_in - 1):
            self._bound_sdf = g[..., self.model.sdf_ch].copy()
        return True

    def unbind_geometry(self):
        self._bound_mask = None
        self._bound_sdf = None
        self._chk(self.lib.psm_unbind_geometry(self.h))

    # Host-grid entries can verify the contract of psm_bind_geometry: with ``check_bound = True`` a grid whose flow-cell
    # pattern differs from the bound one drops the binding.  Off by default (the comparison costs ~30 us per call, more
    # than the binding saves); the evaluators, whose timeStep_grid takes arbitrary grids, switch it on.
    check_bound = False

    def _check_bound(self, g: np.ndarray):
        if not self.check_bound:
            return
        m = getattr(self, "_bound_mask", None)
        if m is not None and g.shape[0] == m.shape[0] and not np.array_equal(g[..., self.model.sdf_ch] != 0, m):
            self.unbind_geometry()
            return
        v = getattr(self, "_bound_sdf", None)           # folded encode: values (a NaN on either side is a mismatch, as on the device)
        if v is not None and g.shape[0] == v.shape[0] and _fold_switch_on() and not bool(np.all(g[..., self.model.sdf_ch] == v)):
            self.unbind_geometry()

    @property
    def geometry_bound(self) -> bool:
        return bool(self.lib.psm_geometry_bound(self.h))

    @property
    def guard_trips(self) -> int:
        """Solves so far whose grid was not the bound geometry (detected on the device; each dropped the binding)."""
        return int(self.lib.psm_guard_trips(self.h))

    def solve_device(self, d_grid: int, n_cases: int, d_fields: int, stream: int = 0,
                     out_scale: Optional[Sequence[float]] = None):
        """Asynchronous solve on raw device pointers (e.g. ``torch.Tensor.data_ptr()``)."""
        sc = None
        if out_scale is not None:
            sc = _f32(np.broadcast_to(out_scale, (n_cases,)))
        self._chk(self.lib.psm_solve_grid_device(self.h, C.c_void_p(d_grid), n_cases,
                                                 _p(sc, C.c_float) if sc is not None else None,
                                                 C.c_void_p(d_fields), C.c_void_p(stream)))

    def synchronize(self):
        self._chk(self.lib.psm_synchronize(self.h))

    def reassemble(self, grid: np.ndarray, block_pred: np.ndarray) -> np.ndarray:
        """Reassembly alone: block_pred [B,S,S,c_out] (or [B,S,S] when c_out==1) -> [Ny,Nx,c_out]."""
        g = _f32(np.asarray(grid)[..., :self.model.c_in])
        bp = _f32(np.asarray(block_pred).reshape(self.B, -1))
        if bp.shape[1] != self.model.S ** 2 * self.model.c_out:
            raise ValueError("block_pred has the wrong shape")
        out = np.empty((self.ny, self.nx, self.model.c_out), np.float32)
        self._chk(self.lib.psm_reassemble(self.h, _p(g, C.c_float), _p(bp, C.c_float), _p(out, C.c_float)))
        return out

    def label_blocks(self, grid: np.ndarray, labels: np.ndarray) -> np.ndarray:
        """Label blocks of the planned layout with the per-block flow-cell mean removed (SM_call.py:487-488;
        Eval_dual_Dense_onlycil.py:509-511): labels [Ny,Nx,c_out] (or [Ny,Nx]) -> [B,S,S,c_out] float32."""
        g = _f32(np.asarray(grid)[..., :self.model.c_in])
        lab = _f32(np.asarray(labels).reshape(self.ny, self.nx, self.model.c_out))
        if g.shape != (self.ny, self.nx, self.model.c_in):
            raise ValueError("grid has the wrong shape")
        out = np.empty((self.B, self.model.S, self.model.S, self.model.c_out), np.float32)
        self._chk(self.lib.psm_label_blocks(self.h, _p(g, C.c_float), _p(lab, C.c_float), _p(out, C.c_float)))
        return out

    def block_error(self, grid: np.ndarray, labels: np.ndarray) -> dict:
        """``utils.compute_in_block_error`` (pressureSM_deltas/utils.py:210-243) for the LAST solve: decoded blocks against the
        de-meaned label blocks over the flow cells, before the reassembly.  ``labels`` [Ny,Nx,c_out] (or [Ny,Nx]) in the
        network's normalised output units (scaled by the solve's out_scale like SM_call.py:555).  -> the two values the
        reference appends (``mean_err``, ``mean_sq_err``) and the printed normVal / biasNorm / stdeNorm / rmseNorm."""
        g = _f32(np.asarray(grid)[..., :self.model.c_in])
        lab = _f32(np.asarray(labels).reshape(self.ny, self.nx, self.model.c_out))
        if g.shape != (self.ny, self.nx, self.model.c_in):
            raise ValueError("grid has the wrong shape")
        out = (C.c_double * 5)()
        self._chk(self.lib.psm_block_error(self.h, _p(g, C.c_float), _p(lab, C.c_float), out))
        bias, rmse = out[0] * 100, np.sqrt(out[1]) * 100
        with np.errstate(invalid="ignore"):
            stde = np.sqrt(rmse ** 2 - bias ** 2)
        return {"mean_err": float(out[0]), "mean_sq_err": float(out[1]), "normVal": float(out[2]), "norm_pred": float(out[3]),
                "n": int(out[4]), "biasNorm": float(bias), "rmseNorm": float(rmse), "stdeNorm": float(stde)}

    def gaussian_filter(self, field: np.ndarray, sigma=(10.0, 10.0)) -> np.ndarray:
        """scipy.ndimage.gaussian_filter(field, sigma, order=0) on the GPU (SM_call.py:353-363)."""
        f = _f32(field)
        if f.ndim != 2:
            raise ValueError("field must be 2-D")
        out = np.empty_like(f)
        self._chk(self.lib.psm_gaussian_filter(self.h, _p(f, C.c_float), f.shape[0], f.shape[1], float(sigma[0]),
                                                float(sigma[1]), _p(out, C.c_float)))
        return out

    def poisson_features(self, ux, uy, dux, duy, sdfunct, L, U, k, max_abs) -> np.ndarray:
        """pressureSM_Poisson input image (SM_call.py:588-711): float64 grids [Ny,Nx] -> grid [Ny,Nx,4] float32."""
        arrs = [_f64(np.asarray(a)) for a in (ux, uy, dux, duy, sdfunct)]
        ny, nx = arrs[0].shape
        if any(a.shape != (ny, nx) for a in arrs):
            raise ValueError("ux, uy, dux, duy, sdfunct must share one [Ny,Nx] shape")
        params = _f64(np.array([L, U, k, *max_abs], np.float64))
        if params.shape != (7,):
            raise ValueError("max_abs must hold 4 scales")
        out = np.empty((ny, nx, 4), np.float32)
        self._chk(self.lib.psm_poisson_features(self.h, *[_p(a, C.c_double) for a in arrs], ny, nx,
                                                _p(params, C.c_double), _p(out, C.c_float)))
        return out

    def set_integration(self, sdfunct: np.ndarray, center_y: int, center_x: int, dx: float, dy: float):
        """Geometry of the gradP -> p integration (Eval_dual_Dense_onlycil.py:592-628)."""
        sd = _f64(sdfunct)
        self._integ_shape = sd.shape
        self._chk(self.lib.psm_set_integration(self.h, sd.shape[0], sd.shape[1], _p(sd, C.c_double), int(center_y),
                                                int(center_x), float(dx), float(dy)))

    def integrate_gradp(self, gradp: np.ndarray) -> np.ndarray:
        """(dp/dx, dp/dy) [Ny,Nx,2] -> p [Ny,Nx] (integrate_field + four-quadrant stitching)."""
        g = _f32(gradp)
        if g.shape != tuple(self._integ_shape) + (2,):
            raise ValueError("gradp must be [Ny,Nx,2] of the integration geometry")
        out = np.empty(self._integ_shape, np.float32)
        self._chk(self.lib.psm_integrate_gradp(self.h, _p(g, C.c_float), _p(out, C.c_float)))
        return out

    # -- U -> p on the device (gradP variant): psm_bind_integration once, then one call per step
    def bind_integration(self, sdfunct, center_y, center_x, dx: float, dy: float) -> bool:
        """One integration geometry per case slot of the planned grid: ``sdfunct`` [Ny,Nx] with scalar cuts, or [n,Ny,Nx]
        with length-n ``center_y`` / ``center_x``.  Returns False -- nothing bound -- where the reference itself raises for
        any case (unequal flow-cell counts on the cut columns, ``int(sdfunct)`` outside a quadrant row)."""
        sd = _f64(np.asarray(sdfunct))
        if sd.ndim == 2:
            sd = sd[None]
        if sd.ndim != 3 or sd.shape[1:] != (self.ny, self.nx):
            raise ValueError(f"sdfunct must be [{self.ny},{self.nx}] or [n,{self.ny},{self.nx}]")
        n = sd.shape[0]
        cy = np.ascontiguousarray(np.broadcast_to(np.asarray(center_y, np.int32).reshape(-1), (n,)))
        cx = np.ascontiguousarray(np.broadcast_to(np.asarray(center_x, np.int32).reshape(-1), (n,)))
        rc = self.lib.psm_bind_integration(self.h, _p(sd, C.c_double), n, _p(cy, C.c_int32), _p(cx, C.c_int32), float(dx), float(dy))
        if rc == -5:                    # PSM_ERR_UNSUPPORTED
            return False
        self._chk(rc)
        return True

    def unbind_integration(self):
        self._chk(self.lib.psm_unbind_integration(self.h))

    def integrate_device(self, d_gradp: int, n_cases: int, d_p: int, stream: int = 0):
        """(dp/dx, dp/dy) [n,Ny,Nx,2] -> p [n,Ny,Nx] on raw device pointers, asynchronous on ``stream``."""
        self._chk(self.lib.psm_integrate_gradp_device(self.h, C.c_void_p(d_gradp), n_cases, C.c_void_p(d_p), C.c_void_p(stream)))

    def solve_pressure_device(self, d_grid: int, n_cases: int, d_p: int, d_gradp: int = 0, stream: int = 0,
                              out_scale: Optional[Sequence[float]] = None):
        """Solve + integration in one stream on raw device pointers: grid [n,Ny,Nx,c_in] -> p [n,Ny,Nx]; ``d_gradp``
        (optional) receives the assembled gradient [n,Ny,Nx,2]."""
        sc = _f32(np.broadcast_to(out_scale, (n_cases,))) if out_scale is not None else None
        self._chk(self.lib.psm_solve_pressure_device(self.h, C.c_void_p(d_grid), n_cases,
                                                     _p(sc, C.c_float) if sc is not None else None,
                                                     C.c_void_p(d_gradp or None), C.c_void_p(d_p), C.c_void_p(stream)))

    def solve_pressure(self, grid: np.ndarray, out_scale: Optional[Sequence[float]] = None) -> np.ndarray:
        """grid [Ny,Nx,>=c_in] or [n,Ny,Nx,>=c_in] -> p [n,Ny,Nx] f32 (host buffers, synchronous)."""
        g = np.asarray(grid)
        if g.ndim == 3:
            g = g[None]
        if g.ndim != 4 or g.shape[1:3] != (self.ny, self.nx) or g.shape[3] < self.model.c_in:
            raise ValueError(f"grid must be [n,{self.ny},{self.nx},>={self.model.c_in}]")
        g = _f32(g[..., :self.model.c_in])
        n = g.shape[0]
        self._check_bound(g)
        out = np.empty((n, self.ny, self.nx), np.float32)
        sc = _f32(np.broadcast_to(out_scale, (n,))) if out_scale is not None else None
        self._chk(self.lib.psm_solve_pressure(self.h, _p(g, C.c_float), n, _p(sc, C.c_float) if sc is not None else None,
                                              _p(out, C.c_float)))
        return out

    # -- Gaussian post-steps on the device (SM_call.py:352-363): psm_bind_poststeps once, then one call per step
    _post_bound = False

    def bind_poststeps(self, sigma_field=(10.0, 10.0), sigma_weight=(50.0, 50.0)):
        """Tap tables of the field filter and of the deltaU-change weight filter ((sigma_y, sigma_x) each; the reference's
        (10,10) and (50,50)) and per-case scratch on the planned grid: after it a step allocates and copies nothing."""
        sf, sw = _f64(np.asarray(sigma_field, np.float64).reshape(2)), _f64(np.asarray(sigma_weight, np.float64).reshape(2))
        self._post_bound = False
        self._chk(self.lib.psm_bind_poststeps(self.h, _p(sf, C.c_double), _p(sw, C.c_double)))
        self._post_bound = True

    def unbind_poststeps(self):
        self._post_bound = False
        self._chk(self.lib.psm_unbind_poststeps(self.h))

    def filter_device(self, d_in: int, n_cases: int, d_out: int, stream: int = 0):
        """gaussian_filter(sigma_field) of every channel of [n,Ny,Nx,c_out] on raw device pointers (``d_out`` may be
        ``d_in``), asynchronous on ``stream``: two launches for the batch."""
        self._chk(self.lib.psm_filter_fields_device(self.h, C.c_void_p(d_in), n_cases, C.c_void_p(d_out), C.c_void_p(stream)))

    def poststeps_device(self, d_fields: int, n_cases: int, d_result: int, apply_filter: bool = True, d_dU: int = 0,
                         d_prev: int = 0, d_change: int = 0, d_next: int = 0, stream: int = 0):
        """Tail of ``assemble_prediction`` on raw device pointers [n,Ny,Nx]: result = filter(fields) if ``apply_filter``;
        with ``d_dU`` / ``d_prev`` also change = filter((result - prev) * filter(dU, sigma_weight)) and next = prev + change
        (either may be 0).  At most four launches for the batch; ``d_result`` may be ``d_fields``."""
        self._chk(self.lib.psm_poststeps_device(self.h, C.c_void_p(d_fields), n_cases, int(bool(apply_filter)),
                                                C.c_void_p(d_dU or None), C.c_void_p(d_prev or None), C.c_void_p(d_result),
                                                C.c_void_p(d_change or None), C.c_void_p(d_next or None), C.c_void_p(stream)))

    def solve_poststeps_device(self, d_grid: int, n_cases: int, d_result: int, apply_filter: bool = True, d_dU: int = 0,
                               d_prev: int = 0, d_change: int = 0, d_next: int = 0, stream: int = 0,
                               out_scale: Optional[Sequence[float]] = None):
        """Solve + post-steps in one stream (one graph replay) on raw device pointers: grid [n,Ny,Nx,c_in] -> result (and
        change / next) [n,Ny,Nx]."""
        sc = _f32(np.broadcast_to(out_scale, (n_cases,))) if out_scale is not None else None
        self._chk(self.lib.psm_solve_poststeps_device(self.h, C.c_void_p(d_grid), n_cases,
                                                      _p(sc, C.c_float) if sc is not None else None, int(bool(apply_filter)),
                                                      C.c_void_p(d_dU or None), C.c_void_p(d_prev or None), C.c_void_p(d_result),
                                                      C.c_void_p(d_change or None), C.c_void_p(d_next or None), C.c_void_p(stream)))

    def solve_poststeps(self, grid: np.ndarray, apply_filter: bool = False, dU=None, prev=None,
                        out_scale: Optional[Sequence[float]] = None):
        """Host buffers, synchronous: grid [Ny,Nx,>=c_in] or [n,Ny,Nx,>=c_in] -> (result [n,Ny,Nx,c_out], change, next); change
        and next [n,Ny,Nx] are None without ``dU`` / ``prev`` [n,Ny,Nx] (filter only)."""
        g = np.asarray(grid)
        if g.ndim == 3:
            g = g[None]
        if g.ndim != 4 or g.shape[1:3] != (self.ny, self.nx) or g.shape[3] < self.model.c_in:
            raise ValueError(f"grid must be [n,{self.ny},{self.nx},>={self.model.c_in}]")
        g = _f32(g[..., :self.model.c_in])
        n = g.shape[0]
        self._check_bound(g)
        if (dU is None) != (prev is None):
            raise ValueError("dU and prev go together")
        result = np.empty((n, self.ny, self.nx, self.model.c_out), np.float32)
        change = nxt = None
        if dU is not None:
            dU, prev = (_f32(np.asarray(a, np.float32).reshape(n, self.ny, self.nx)) for a in (dU, prev))
            change, nxt = np.empty((n, self.ny, self.nx), np.float32), np.empty((n, self.ny, self.nx), np.float32)
        sc = _f32(np.broadcast_to(out_scale, (n,))) if out_scale is not None else None
        opt = lambda a: _p(a, C.c_float) if a is not None else None
        self._chk(self.lib.psm_solve_poststeps(self.h, _p(g, C.c_float), n, opt(sc), int(bool(apply_filter)), opt(dU), opt(prev),
                                               _p(result, C.c_float), opt(change), opt(nxt)))
        return result, change, nxt

    # -- pressureSM_Poisson input features on the device (SM_call.py:588-711): psm_bind_features once, then one call per step
    _feat_bound = False

    def bind_features(self, sdfunct, k: float, max_abs):
        """SDF planes of the case slots (``sdfunct`` [Ny,Nx] or [n,Ny,Nx] float64, raw, 0 in solids), ``k`` and the four
        ``max_abs`` scales of ``poisson_features``, and every buffer a step touches: after it a step allocates nothing.  Needs
        a four-channel model with the SDF last."""
        sd = _f64(np.asarray(sdfunct))
        if sd.ndim == 2:
            sd = sd[None]
        if sd.ndim != 3 or sd.shape[1:] != (self.ny, self.nx):
            raise ValueError(f"sdfunct must be [{self.ny},{self.nx}] or [n,{self.ny},{self.nx}]")
        ma = _f64(np.asarray(max_abs, np.float64).reshape(-1))
        if ma.shape != (4,):
            raise ValueError("max_abs must hold 4 scales")
        self._feat_bound = False
        self._chk(self.lib.psm_bind_features(self.h, _p(sd, C.c_double), sd.shape[0], float(k), _p(ma, C.c_double)))
        self._feat_bound = True

    def unbind_features(self):
        self._feat_bound = False
        self._chk(self.lib.psm_unbind_features(self.h))

    def _lu(self, LU, n_cases: int) -> np.ndarray:
        lu = _f64(np.asarray(LU, np.float64).reshape(-1, 2))
        if lu.shape != (n_cases, 2):
            raise ValueError("LU must be [n_cases][2] = (L, U) per case")
        return lu

    def features_device(self, d_vel: int, n_cases: int, LU, d_grid: int, stream: int = 0):
        """Velocity planes [n,4,Ny*Nx] float64 (ux, uy, dux, duy) -> image [n,Ny,Nx,4] float32 on raw device pointers,
        asynchronous on ``stream``: two launches for the batch.  ``LU`` [n][2] = (L, U) per case, a host array."""
        lu = self._lu(LU, n_cases)
        self._chk(self.lib.psm_features_device(self.h, C.c_void_p(d_vel), n_cases, _p(lu, C.c_double), C.c_void_p(d_grid),
                                               C.c_void_p(stream)))

    def poisson_step_device(self, d_vel: int, n_cases: int, LU, d_result: int, apply_filter: bool = True, d_dU: int = 0,
                            d_prev: int = 0, d_change: int = 0, d_next: int = 0, stream: int = 0,
                            out_scale: Optional[Sequence[float]] = None):
        """A whole Poisson time step as one graph replay on raw device pointers: velocity planes [n,4,Ny*Nx] float64 ->
        features -> solve -> post-steps -> result (and change / next) [n,Ny,Nx]."""
        lu = self._lu(LU, n_cases)
        sc = _f32(np.broadcast_to(out_scale, (n_cases,))) if out_scale is not None else None
        self._chk(self.lib.psm_poisson_step_device(self.h, C.c_void_p(d_vel), n_cases, _p(lu, C.c_double),
                                                   _p(sc, C.c_float) if sc is not None else None, int(bool(apply_filter)),
                                                   C.c_void_p(d_dU or None), C.c_void_p(d_prev or None), C.c_void_p(d_result),
                                                   C.c_void_p(d_change or None), C.c_void_p(d_next or None), C.c_void_p(stream)))

    def poisson_step(self, vel: np.ndarray, LU, out_scale: Optional[Sequence[float]] = None, apply_filter: bool = False,
                     dU=None, prev=None):
        """Host buffers, synchronous: vel [n,4,Ny,Nx] (or [4,Ny,Nx]) float64 -> (result [n,Ny,Nx,c_out], change, next); change
        and next [n,Ny,Nx] are None without ``dU`` / ``prev`` [n,Ny,Nx]."""
        v = np.asarray(vel)
        if v.ndim == 3:
            v = v[None]
        if v.ndim != 4 or v.shape[1:] != (4, self.ny, self.nx):
            raise ValueError(f"vel must be [n,4,{self.ny},{self.nx}]")
        v = _f64(v)
        n = v.shape[0]
        lu = self._lu(LU, n)
        if (dU is None) != (prev is None):
            raise ValueError("dU and prev go together")
        result = np.empty((n, self.ny, self.nx, self.model.c_out), np.float32)
        change = nxt = None
        if dU is not None:
            dU, prev = (_f32(np.asarray(a, np.float32).reshape(n, self.ny, self.nx)) for a in (dU, prev))
            change, nxt = np.empty((n, self.ny, self.nx), np.float32), np.empty((n, self.ny, self.nx), np.float32)
        sc = _f32(np.broadcast_to(out_scale, (n,))) if out_scale is not None else None
        opt = lambda a: _p(a, C.c_float) if a is not None else None
        self._chk(self.lib.psm_poisson_step(self.h, _p(v, C.c_double), n, _p(lu, C.c_double), opt(sc), int(bool(apply_filter)),
                                            opt(dU), opt(prev), _p(result, C.c_float), opt(change), opt(nxt)))
        return result, change, nxt

    # -- frames of cell columns on the single mesh (psm_set_geometry), on the device: psm_bind_frames once, then one call per batch
    _frames_bound = False
    mesh_cells = None               # cells of the mesh the handle holds (set_mesh / Evaluation.computeOnlyOnce)

    def set_mesh(self, vtx_m2g, wts_m2g, indices, sdfunct, n_cells: int, maxs=(1.0, 1.0, 1.0, 1.0)):
        """The mesh -> grid tables of one mesh on the planned grid (psm_set_geometry without the grid -> mesh side): what
        ``psm_mesh_to_grid`` and the frame entries read.  ``vtx_m2g`` / ``wts_m2g`` [Ny*Nx,3], ``indices`` [Ny*Nx,2] (row, column),
        ``sdfunct`` [Ny,Nx].  Re-plans the grid, so every binding made before it is dropped."""
        v, w = np.ascontiguousarray(vtx_m2g, np.int32), _f64(wts_m2g)
        idx, sdf = np.ascontiguousarray(indices, np.int32), _f64(sdfunct)
        npix = self.ny * self.nx
        if v.shape != (npix, 3) or w.shape != (npix, 3) or idx.shape != (npix, 2) or sdf.size != npix:
            raise ValueError(f"tables must be [{npix},3], [{npix},3], [{npix},2] and sdfunct [{self.ny},{self.nx}]")
        mx = _f64(np.asarray(maxs, np.float64).reshape(-1)[:4])
        self.mesh_cells = None
        self._frames_bound = self._feat_bound = self._post_bound = self._deltas_bound = self._gradp_bound = False; self._rows_bound = 0
        self._bound_mask = self._bound_sdf = None
        self._chk(self.lib.psm_set_geometry(self.h, int(n_cells), self.ny, self.nx, _p(v, C.c_int32), _p(w, C.c_double),
                                            _p(idx, C.c_int32), _p(sdf, C.c_double), None, None, _p(mx, C.c_double), 1, 1, 0.05))
        self.mesh_cells = int(n_cells)

    def bind_frames(self, n_frames: int, k: int):
        """Staging for ``n_frames`` (<= max_cases) frames of ``k`` (<= 16) cell columns on the handle's mesh: after it a batch
        allocates nothing."""
        self._frames_bound = self._deltas_bound = self._gradp_bound = False; self._rows_bound = 0
        self._chk(self.lib.psm_bind_frames(self.h, int(n_frames), int(k)))
        self._frames_bound = True

    def unbind_frames(self):
        self._frames_bound = self._deltas_bound = self._gradp_bound = False; self._rows_bound = 0
        self._chk(self.lib.psm_unbind_frames(self.h))

    def frames_to_grid_device(self, d_cols: int, n_frames: int, k: int, outs, fill: bool = True, stream: int = 0):
        """interpolate_fill + last-writer scatter of ``k`` cell columns of ``n_frames`` frames in one launch, on raw device
        pointers: ``d_cols`` [n,n_cells,k] float64; ``outs`` = one ``(device pointer or 0, frame_stride, as_f32)`` per column --
        column c of frame f goes to plane ``pointer + f * frame_stride`` (elements) as float64, or float32 with ``as_f32``; 0: the
        column is not stored.  Asynchronous on ``stream``."""
        outs = list(outs)
        if len(outs) != k:
            raise ValueError("outs must hold one (pointer, frame_stride, as_f32) per column")
        desc = (_lib.psm_frame_col * max(k, 1))()
        for c, (ptr, stride, as_f32) in enumerate(outs):
            desc[c].dst, desc[c].frame_stride, desc[c].as_f32 = (ptr or None), int(stride), int(bool(as_f32))
        self._chk(self.lib.psm_frames_to_grid_device(self.h, C.c_void_p(d_cols), n_frames, k, int(bool(fill)), desc, C.c_void_p(stream)))

    @staticmethod
    def _frame_columns(k: int, weighting: bool) -> int:
        """Number of extra columns of the evaluator's convention: (Ux, Uy, dUx, dUy), extra..., [dU-change weight, delta_p_prev]."""
        if k < 4:
            raise ValueError("frames need at least the 4 columns (Ux, Uy, dUx, dUy)")
        if weighting and k < 6:
            raise ValueError("with the weighting the last two of at least 6 columns are (dU-change weight, delta_p_prev)")
        if k > 16:
            raise ValueError("at most 16 columns")
        return k - (6 if weighting else 4)

    def poisson_frames_device(self, d_cols: int, n_frames: int, k: int, LU, d_result: int, apply_filter: bool = True,
                              weighting: bool = True, d_extra: int = 0, d_change: int = 0, d_next: int = 0, stream: int = 0,
                              out_scale: Optional[Sequence[float]] = None):
        """The Poisson evaluator's frames as one graph replay on raw device pointers: ``d_cols`` [n,n_cells,k] float64 with columns
        (Ux, Uy, dUx, dUy, extra..., [dU-change weight, delta_p_prev]) -> planes -> features -> solve -> post-steps -> result (and
        change / next) [n,Ny,Nx]; the extra columns' float64 planes go to ``d_extra`` [n,n_extra,Ny*Nx] (0: not stored)."""
        self._frame_columns(k, weighting)
        lu = self._lu(LU, n_frames)
        sc = _f32(np.broadcast_to(out_scale, (n_frames,))) if out_scale is not None else None
        self._chk(self.lib.psm_poisson_frames_device(self.h, C.c_void_p(d_cols), n_frames, k, _p(lu, C.c_double),
                                                     _p(sc, C.c_float) if sc is not None else None, int(bool(apply_filter)),
                                                     int(bool(weighting)), C.c_void_p(d_extra or None), C.c_void_p(d_result),
                                                     C.c_void_p(d_change or None), C.c_void_p(d_next or None), C.c_void_p(stream)))

    def poisson_frames(self, cols: np.ndarray, LU, out_scale: Optional[Sequence[float]] = None, apply_filter: bool = False,
                       weighting: bool = True, want_extra: bool = True):
        """Host buffers, synchronous: ``cols`` [n,n_cells,k] (or [n_cells,k]) float64 -> (result [n,Ny,Nx,c_out], change, next,
        extra); change and next [n,Ny,Nx] are None without the weighting, extra [n,n_extra,Ny,Nx] float64 (NaNs of
        interpolate_fill kept) is None without ``want_extra`` or without extra columns."""
        v = np.asarray(cols)
        if v.ndim == 2:
            v = v[None]
        if v.ndim != 3:
            raise ValueError("cols must be [n,n_cells,k]")
        n, n_cells, k = v.shape
        n_extra = self._frame_columns(k, weighting)
        if self.mesh_cells is None:
            raise RuntimeError("the handle holds no mesh (set_mesh / computeOnlyOnce)")
        if n < 1 or n_cells != self.mesh_cells:
            raise ValueError(f"cols must be [n >= 1, {self.mesh_cells} cells, k]")
        lu = self._lu(LU, n)
        if out_scale is not None and np.size(out_scale) not in (1, n):
            raise ValueError("out_scale must hold one value per frame")
        v = _f64(v)
        result = np.empty((n, self.ny, self.nx, self.model.c_out), np.float32)
        change = nxt = extra = None
        if weighting:
            change, nxt = np.empty((n, self.ny, self.nx), np.float32), np.empty((n, self.ny, self.nx), np.float32)
        if want_extra and n_extra:
            extra = np.empty((n, n_extra, self.ny, self.nx), np.float64)
        sc = _f32(np.broadcast_to(np.asarray(out_scale, np.float32).reshape(-1), (n,))) if out_scale is not None else None
        opt = lambda a, t=C.c_float: _p(a, t) if a is not None else None
        self._chk(self.lib.psm_poisson_frames(self.h, _p(v, C.c_double), n, k, _p(lu, C.c_double), opt(sc), int(bool(apply_filter)),
                                              int(bool(weighting)), opt(extra, C.c_double), _p(result, C.c_float), opt(change), opt(nxt)))
        return result, change, nxt, extra

    # -- the per-frame error blocks of assembled fields on the device: eight float64 sums per (frame, pair) instead of the fields
    RAW_SUMS = ("n", "s1", "s2", "tmin", "tmax", "pmin", "pmax", "tnan")
    METRICS = ("normVal", "biasNorm", "stdeNorm", "rmseNorm", "mean_err", "mean_sq_err")

    @staticmethod
    def _err_plane(desc, what: str, optional: bool = False):
        """``(device pointer, frame_stride, elem_stride, as_f32)`` -> psm_err_plane; None (or pointer 0) where ``optional``: absent."""
        out = _lib.psm_err_plane()
        if desc is None or not desc[0]:
            if not optional:
                raise ValueError(f"{what}: a plane (pointer, frame_stride, elem_stride, as_f32) is needed")
            return out
        ptr, frame_stride, elem_stride, as_f32 = desc
        if int(frame_stride) < 0 or int(elem_stride) < 0:
            raise ValueError(f"{what}: strides must not be negative")
        if int(ptr) % (4 if as_f32 else 8):
            raise ValueError(f"{what}: the plane is not aligned to its element")
        out.ptr, out.frame_stride, out.elem_stride, out.as_f32 = int(ptr), int(frame_stride), int(elem_stride), int(bool(as_f32))
        return out

    def field_errors_device(self, mask, pairs, n_frames: int, d_raw: int, stream: int = 0):
        """The error sums of up to four (prediction, truth) pairs over ``n_frames`` frames of planes on the planned grid, on raw
        device pointers, asynchronous on ``stream``: ``d_raw`` [n_frames][len(pairs)][8] float64 = ``RAW_SUMS``.  A plane is
        ``(pointer, frame_stride, elem_stride, as_f32)`` with strides in elements; ``mask``: flow cell iff != 0 and not NaN;
        a pair is ``(pred, truth, add, sub, truth_nan_to_zero)``, ``add`` / ``sub`` may be None:
        d = ((nan0(add) - nan0(sub)) + pred) - truth over the flow cells, NaN d left out."""
        pairs = list(pairs)
        if not 1 <= len(pairs) <= _lib.PSM_ERR_MAX_PAIRS:
            raise ValueError(f"1..{_lib.PSM_ERR_MAX_PAIRS} pairs")
        if not 1 <= int(n_frames) <= self.max_cases:
            raise ValueError("n_frames outside [1, max_cases]")
        if not d_raw or int(d_raw) % 8:
            raise ValueError("d_raw must be an 8-byte aligned device pointer")
        m = self._err_plane(mask, "mask")
        desc = (_lib.psm_err_pair * len(pairs))()
        for i, pair in enumerate(pairs):
            if len(pair) != 5:
                raise ValueError("a pair is (pred, truth, add, sub, truth_nan_to_zero)")
            desc[i].pred, desc[i].truth = self._err_plane(pair[0], f"pair {i} pred"), self._err_plane(pair[1], f"pair {i} truth")
            desc[i].add, desc[i].sub = self._err_plane(pair[2], f"pair {i} add", True), self._err_plane(pair[3], f"pair {i} sub", True)
            desc[i].truth_nan_to_zero = int(bool(pair[4]))
        self._chk(self.lib.psm_field_errors_device(self.h, C.byref(m), desc, len(pairs), int(n_frames), C.c_void_p(d_raw), C.c_void_p(stream)))

    def poisson_frames_errors_device(self, d_cols: int, n_frames: int, k: int, LU, d_extra: int, d_result: int, d_next: int, d_raw: int,
                                     apply_filter: bool = True, d_change: int = 0, stream: int = 0,
                                     out_scale: Optional[Sequence[float]] = None):
        """``poisson_frames_device`` with the weighting (the same graph replay) and, behind it on the same stream, the evaluator's
        three error blocks of every frame: ``d_raw`` [n][3][8] float64 -- delta-p with the weighting, delta-p without it, p -- from
        next, result and the two label planes (columns 4 and 5) in ``d_extra``; the mask is the bound SDF plane."""
        if self._frame_columns(k, True) < 2:
            raise ValueError("the error blocks need the two label columns (delta_p, p): at least 8 columns")
        if not (d_extra and d_result and d_next):
            raise ValueError("the error blocks read d_extra, d_result and d_next: none of them may be 0")
        if not d_raw or int(d_raw) % 8:
            raise ValueError("d_raw must be an 8-byte aligned device pointer")
        lu = self._lu(LU, n_frames)
        sc = _f32(np.broadcast_to(out_scale, (n_frames,))) if out_scale is not None else None
        self._chk(self.lib.psm_poisson_frames_errors_device(self.h, C.c_void_p(d_cols), n_frames, k, _p(lu, C.c_double),
                                                            _p(sc, C.c_float) if sc is not None else None, int(bool(apply_filter)), 1,
                                                            C.c_void_p(d_extra), C.c_void_p(d_result), C.c_void_p(d_change or None),
                                                            C.c_void_p(d_next), C.c_void_p(d_raw), C.c_void_p(stream)))

    def poisson_frames_errors(self, cols: np.ndarray, LU, out_scale: Optional[Sequence[float]] = None,
                              apply_filter: bool = False) -> np.ndarray:
        """Host buffers, synchronous: ``cols`` [n,n_cells,k >= 8] (or [n_cells,k]) float64 -> raw [n,3,8] float64, the sums of
        the three error blocks per frame (``metrics_from_sums`` turns a row into the metrics).  Nothing else comes back: the
        fields and label planes stay on the device."""
        v = np.asarray(cols)
        if v.ndim == 2:
            v = v[None]
        if v.ndim != 3:
            raise ValueError("cols must be [n,n_cells,k]")
        n, n_cells, k = v.shape
        if self._frame_columns(k, True) < 2:
            raise ValueError("the error blocks need the two label columns (delta_p, p): at least 8 columns")
        if self.mesh_cells is None:
            raise RuntimeError("the handle holds no mesh (set_mesh / computeOnlyOnce)")
        if n < 1 or n_cells != self.mesh_cells:
            raise ValueError(f"cols must be [n >= 1, {self.mesh_cells} cells, k]")
        lu = self._lu(LU, n)
        if out_scale is not None and np.size(out_scale) not in (1, n):
            raise ValueError("out_scale must hold one value per frame")
        v = _f64(v)
        raw = np.empty((n, 3, len(self.RAW_SUMS)), np.float64)
        sc = _f32(np.broadcast_to(np.asarray(out_scale, np.float32).reshape(-1), (n,))) if out_scale is not None else None
        self._chk(self.lib.psm_poisson_frames_errors(self.h, _p(v, C.c_double), n, k, _p(lu, C.c_double),
                                                     _p(sc, C.c_float) if sc is not None else None, int(bool(apply_filter)), 1,
                                                     _p(raw, C.c_double)))
        return raw

    # -- the frame batch of the pressureSM_deltas evaluator on the device: columns -> image, label, truth -> solve -> two error blocks
    _deltas_bound = False

    def bind_deltas_frames(self, sdfunct, max_abs):
        """After ``bind_frames``, on a three-channel model with the SDF last and a one-channel field: the simulation's raw SDF plane
        ``sdfunct`` [Ny,Nx] float64 (NaNs allowed) and ``max_abs`` = (max_abs_Ux, max_abs_Uy, max_abs_dist, max_abs_p), each finite
        and non-zero.  Reserves everything a step touches for the frame count bound with ``bind_frames``."""
        m = self.model
        if m.c_in != 3 or m.sdf_ch != 2 or m.c_out != 1:
            raise ValueError("the deltas frames take a model with 3 input channels, the SDF in channel 2, and 1 output channel")
        if not getattr(self, "_frames_bound", False):
            raise RuntimeError("bind_frames has not been called")
        sdf = _f64(sdfunct)
        if sdf.size != self.ny * self.nx:
            raise ValueError(f"sdfunct must be [{self.ny},{self.nx}]")
        mx = _f64(np.asarray(max_abs, np.float64).reshape(-1))
        if mx.size != 4 or not np.all(np.isfinite(mx)) or np.any(mx == 0):
            raise ValueError("max_abs must hold four finite non-zero scales: (max_abs_Ux, max_abs_Uy, max_abs_dist, max_abs_p)")
        self._deltas_bound = False
        self._chk(self.lib.psm_bind_deltas_frames(self.h, _p(sdf, C.c_double), _p(mx, C.c_double)))
        self._deltas_bound = True

    def unbind_deltas_frames(self):
        self._deltas_bound = False
        self._chk(self.lib.psm_unbind_deltas_frames(self.h))

    def _deltas_call(self, n_frames, k, U2, need_u2: bool = True):
        """The argument checks the deltas frame entries share -> U2 as a float64 array (None where it is optional and absent)."""
        if not self._deltas_bound:
            raise RuntimeError("bind_deltas_frames has not been called (bind_frames and a new mesh drop the binding)")
        if not 3 <= int(k) <= 16:
            raise ValueError("frames take 3..16 columns: (dUx / U, dUy / U, dp / U^2), further columns are not stored")
        if not 1 <= int(n_frames) <= self.max_cases:
            raise ValueError("n_frames outside [1, max_cases]")
        if U2 is None:
            if need_u2:
                raise ValueError("U2 must hold one value per frame")
            return None
        u2 = _f64(np.asarray(U2, np.float64).reshape(-1))
        if u2.size != int(n_frames) or not np.all(np.isfinite(u2)):
            raise ValueError("U2 must hold one finite value per frame")
        return u2

    @staticmethod
    def _dev_ptr(ptr, align: int, what: str, optional: bool = False) -> int:
        if not ptr:
            if not optional:
                raise ValueError(f"{what} must be a device pointer")
            return 0
        if int(ptr) % align:
            raise ValueError(f"{what} must be {align}-byte aligned")
        return int(ptr)

    def _frame_scale(self, out_scale, n: int):
        if out_scale is None:
            return None
        if np.size(out_scale) not in (1, n):
            raise ValueError("out_scale must hold one value per frame")
        return _f32(np.broadcast_to(np.asarray(out_scale, np.float32).reshape(-1), (n,)))

    def deltas_image_device(self, d_cols: int, n_frames: int, k: int, U2, d_grid: int, d_label: int = 0, d_truth: int = 0, stream: int = 0):
        """The image stage alone on raw device pointers, asynchronous on ``stream``: ``d_cols`` [n,n_cells,k] float64 -> ``d_grid``
        [n,Ny,Nx,3] float32, ``d_label`` [n,Ny*Nx] float32 and ``d_truth`` [n,Ny*Nx] float64 (0: not stored), bit for bit the host
        statements of ``Evaluation.timeStep``.  ``U2`` [n]: U_max_norm^2 per frame (None without ``d_truth``)."""
        u2 = self._deltas_call(n_frames, k, U2, need_u2=bool(d_truth))
        d_cols = self._dev_ptr(d_cols, 8, "d_cols")
        d_grid, d_label = self._dev_ptr(d_grid, 4, "d_grid"), self._dev_ptr(d_label, 4, "d_label", True)
        d_truth = self._dev_ptr(d_truth, 8, "d_truth", True)
        self._chk(self.lib.psm_deltas_image_device(self.h, C.c_void_p(d_cols), int(n_frames), int(k), _p(u2, C.c_double) if u2 is not None else None,
                                                   C.c_void_p(d_grid), C.c_void_p(d_label or None), C.c_void_p(d_truth or None), C.c_void_p(stream)))

    def block_errors_device(self, d_grid: int, d_label: int, n_frames: int, d_raw: int, stream: int = 0):
        """``utils.compute_in_block_error`` for the first ``n_frames`` cases of the LAST synchronous or device solve, on raw device
        pointers, asynchronous on ``stream``: the decoded blocks against the de-meaned label blocks of ``d_label`` [n,Ny*Nx] float32
        times the solve's row scale, over the flow cells of ``d_grid`` [n,Ny,Nx,3].  ``d_raw`` [n,8] float64 = ``RAW_SUMS``."""
        if not self._deltas_bound:
            raise RuntimeError("bind_deltas_frames has not been called (bind_frames and a new mesh drop the binding)")
        if not 1 <= int(n_frames) <= self.max_cases:
            raise ValueError("n_frames outside [1, max_cases]")
        d_grid, d_label = self._dev_ptr(d_grid, 4, "d_grid"), self._dev_ptr(d_label, 4, "d_label")
        d_raw = self._dev_ptr(d_raw, 8, "d_raw")
        self._chk(self.lib.psm_block_errors_device(self.h, C.c_void_p(d_grid), C.c_void_p(d_label), int(n_frames), C.c_void_p(d_raw), C.c_void_p(stream)))

    def deltas_frames_device(self, d_cols: int, n_frames: int, k: int, U2, d_result: int = 0, d_truth: int = 0, d_raw: int = 0,
                             apply_filter: bool = False, stream: int = 0, out_scale: Optional[Sequence[float]] = None):
        """The deltas evaluator's frames as one graph replay on raw device pointers: ``d_cols`` [n,n_cells,k] float64 -> planes ->
        image -> one single-case solve per frame (-> the ``sigma_field`` filter of ``bind_poststeps`` with ``apply_filter``) -> ``d_result`` [n,Ny*Nx] float32,
        ``d_truth`` [n,Ny*Nx] float64 (0: the binding's buffers); with ``d_raw`` [n,2,8] float64 the two error blocks behind it:
        row 0 the field against the truth, row 1 the decoded blocks against the de-meaned label blocks."""
        u2 = self._deltas_call(n_frames, k, U2)
        if apply_filter and not getattr(self, "_post_bound", False):
            raise RuntimeError("apply_filter needs bind_poststeps")
        d_cols = self._dev_ptr(d_cols, 8, "d_cols")
        d_result, d_truth = self._dev_ptr(d_result, 4, "d_result", True), self._dev_ptr(d_truth, 8, "d_truth", True)
        d_raw = self._dev_ptr(d_raw, 8, "d_raw", True)
        sc = self._frame_scale(out_scale, int(n_frames))
        self._chk(self.lib.psm_deltas_frames_device(self.h, C.c_void_p(d_cols), int(n_frames), int(k), _p(u2, C.c_double),
                                                    _p(sc, C.c_float) if sc is not None else None, int(bool(apply_filter)),
                                                    C.c_void_p(d_result or None), C.c_void_p(d_truth or None), C.c_void_p(d_raw or None),
                                                    C.c_void_p(stream)))

    def deltas_frames(self, cols: np.ndarray, U2, out_scale: Optional[Sequence[float]] = None, apply_filter: bool = False,
                      want_result: bool = True, want_truth: bool = True, want_raw: bool = True):
        """Host buffers, synchronous: ``cols`` [n,n_cells,k] (or [n_cells,k]) float64 -> (result [n,Ny,Nx] float32, truth [n,Ny,Nx]
        float64, raw [n,2,8] float64); what is not wanted is None and is not copied back -- a metrics-only sweep
        (``want_result = want_truth = False``) brings back 16 doubles per frame."""
        v = np.asarray(cols)
        if v.ndim == 2:
            v = v[None]
        if v.ndim != 3:
            raise ValueError("cols must be [n,n_cells,k]")
        n, n_cells, k = v.shape
        u2 = self._deltas_call(n, k, U2)
        if self.mesh_cells is None:
            raise RuntimeError("the handle holds no mesh (set_mesh / computeOnlyOnce)")
        if n_cells != self.mesh_cells:
            raise ValueError(f"cols must be [n >= 1, {self.mesh_cells} cells, k]")
        if not (want_result or want_truth or want_raw):
            raise ValueError("nothing to return")
        if apply_filter and not getattr(self, "_post_bound", False):
            raise RuntimeError("apply_filter needs bind_poststeps")
        sc = self._frame_scale(out_scale, n)
        v = _f64(v)
        result = np.empty((n, self.ny, self.nx), np.float32) if want_result else None
        truth = np.empty((n, self.ny, self.nx), np.float64) if want_truth else None
        raw = np.empty((n, 2, len(self.RAW_SUMS)), np.float64) if want_raw else None
        opt = lambda a, t: _p(a, t) if a is not None else None
        self._chk(self.lib.psm_deltas_frames(self.h, _p(v, C.c_double), n, k, _p(u2, C.c_double), opt(sc, C.c_float), int(bool(apply_filter)),
                                             opt(result, C.c_float), opt(truth, C.c_double), opt(raw, C.c_double)))
        return result, truth, raw

    # -- the frame batch of the U_to_gradP evaluator on the device: columns -> image, labels -> solve -> p -> four error blocks
    _gradp_bound = False

    def bind_gradp_frames(self, sdfunct, max_abs, center_y: int, center_x: int, dx: float, dy: float) -> bool:
        """After ``bind_frames``, on a three-channel model with the SDF last and a two-channel field: the simulation's raw SDF plane
        ``sdfunct`` [Ny,Nx] float64 (NaNs allowed), ``max_abs`` = the scales of grid channels 0-4, each finite and non-zero, and the
        cut and spacings of ``set_integration``, fixed for the simulation.  The integration tables go into a set of the binding's
        own (``bind_integration`` / ``set_integration`` are not touched).  Reserves everything a step touches for the frame count
        bound with ``bind_frames``.  Returns False -- nothing bound -- where the reference itself raises on the geometry."""
        m = self.model
        if m.c_in != 3 or m.sdf_ch != 2 or m.c_out != 2:
            raise ValueError("the gradP frames take a model with 3 input channels, the SDF in channel 2, and 2 output channels")
        if not getattr(self, "_frames_bound", False):
            raise RuntimeError("bind_frames has not been called")
        sdf = _f64(sdfunct)
        if sdf.size != self.ny * self.nx:
            raise ValueError(f"sdfunct must be [{self.ny},{self.nx}]")
        mx = _f64(np.asarray(max_abs, np.float64).reshape(-1))
        if mx.size != 5 or not np.all(np.isfinite(mx)) or np.any(mx == 0):
            raise ValueError("max_abs must hold five finite non-zero scales: those of grid channels 0-4")
        if not (1 <= int(center_y) < self.ny and 1 <= int(center_x) < self.nx):
            raise ValueError("the cut (center_y, center_x) lies outside the grid")
        self._gradp_bound = False
        rc = self.lib.psm_bind_gradp_frames(self.h, _p(sdf, C.c_double), _p(mx, C.c_double), int(center_y), int(center_x), float(dx), float(dy))
        if rc == -5:                    # PSM_ERR_UNSUPPORTED
            return False
        self._chk(rc)
        self._gradp_bound = True
        return True

    def unbind_gradp_frames(self):
        self._gradp_bound = False
        self._chk(self.lib.psm_unbind_gradp_frames(self.h))

    def _gradp_call(self, n_frames, k):
        """The argument checks the gradP frame entries share."""
        if not self._gradp_bound:
            raise RuntimeError("bind_gradp_frames has not been called (bind_frames and a new mesh drop the binding)")
        if not 5 <= int(k) <= 16:
            raise ValueError("frames take 5..16 columns: (Ux / U, Uy / U, dPdx / U^2, dPdy / U^2, p / U^2), further columns are not stored")
        if not 1 <= int(n_frames) <= self.max_cases:
            raise ValueError("n_frames outside [1, max_cases]")

    def gradp_image_device(self, d_cols: int, n_frames: int, k: int, d_grid: int, d_truth: int = 0, stream: int = 0):
        """The image stage alone on raw device pointers, asynchronous on ``stream``: ``d_cols`` [n,n_cells,k] float64 -> ``d_grid``
        [n,Ny,Nx,3] float32 and ``d_truth`` [n,3,Ny*Nx] float64 (grid channels 3-5; 0: not stored), bit for bit the host statements
        of ``EvaluationGradP.timeStep``."""
        self._gradp_call(n_frames, k)
        d_cols = self._dev_ptr(d_cols, 8, "d_cols")
        d_grid, d_truth = self._dev_ptr(d_grid, 4, "d_grid"), self._dev_ptr(d_truth, 8, "d_truth", True)
        self._chk(self.lib.psm_gradp_image_device(self.h, C.c_void_p(d_cols), int(n_frames), int(k), C.c_void_p(d_grid),
                                                  C.c_void_p(d_truth or None), C.c_void_p(stream)))

    def gradp_frames_device(self, d_cols: int, n_frames: int, k: int, d_gradp: int = 0, d_p: int = 0, d_truth: int = 0, d_raw: int = 0,
                            apply_filter: bool = False, stream: int = 0, out_scale: Optional[Sequence[float]] = None):
        """The U_to_gradP evaluator's frames as one graph replay on raw device pointers: ``d_cols`` [n,n_cells,k] float64 -> planes
        -> image, labels -> one single-case solve per frame (-> the ``sigma_field`` filter of ``bind_poststeps`` with
        ``apply_filter``) -> integration with the binding's tables -> ``d_gradp`` [n,Ny*Nx,2] float32, ``d_p`` [n,Ny*Nx] float32,
        ``d_truth`` [n,3,Ny*Nx] float64 (0: the binding's buffers); with ``d_raw`` [n,4,8] float64 the four error blocks behind it:
        p against label 0 (the reference's metric), p against the pressure label, the two gradient components against theirs."""
        self._gradp_call(n_frames, k)
        if apply_filter and not getattr(self, "_post_bound", False):
            raise RuntimeError("apply_filter needs bind_poststeps")
        d_cols = self._dev_ptr(d_cols, 8, "d_cols")
        d_gradp, d_p = self._dev_ptr(d_gradp, 8, "d_gradp", True), self._dev_ptr(d_p, 4, "d_p", True)
        d_truth, d_raw = self._dev_ptr(d_truth, 8, "d_truth", True), self._dev_ptr(d_raw, 8, "d_raw", True)
        sc = self._frame_scale(out_scale, int(n_frames))
        self._chk(self.lib.psm_gradp_frames_device(self.h, C.c_void_p(d_cols), int(n_frames), int(k),
                                                   _p(sc, C.c_float) if sc is not None else None, int(bool(apply_filter)),
                                                   C.c_void_p(d_gradp or None), C.c_void_p(d_p or None), C.c_void_p(d_truth or None),
                                                   C.c_void_p(d_raw or None), C.c_void_p(stream)))

    def gradp_frames(self, cols: np.ndarray, out_scale: Optional[Sequence[float]] = None, apply_filter: bool = False,
                     want_gradp: bool = True, want_p: bool = True, want_truth: bool = True):
        """Host buffers, synchronous: ``cols`` [n,n_cells,k] (or [n_cells,k]) float64 -> (gradp [n,Ny,Nx,2] float32, p [n,Ny,Nx]
        float32, truth [n,3,Ny,Nx] float64, raw [n,4,8] float64); what is not wanted is None and is not copied back -- a
        metrics-only sweep (``want_gradp = want_p = want_truth = False``) brings back 32 doubles per frame."""
        v = np.asarray(cols)
        if v.ndim == 2:
            v = v[None]
        if v.ndim != 3:
            raise ValueError("cols must be [n,n_cells,k]")
        n, n_cells, k = v.shape
        self._gradp_call(n, k)
        if self.mesh_cells is None:
            raise RuntimeError("the handle holds no mesh (set_mesh / computeOnlyOnce)")
        if n_cells != self.mesh_cells:
            raise ValueError(f"cols must be [n >= 1, {self.mesh_cells} cells, k]")
        if apply_filter and not getattr(self, "_post_bound", False):
            raise RuntimeError("apply_filter needs bind_poststeps")
        sc = self._frame_scale(out_scale, n)
        v = _f64(v)
        gradp = np.empty((n, self.ny, self.nx, 2), np.float32) if want_gradp else None
        p = np.empty((n, self.ny, self.nx), np.float32) if want_p else None
        truth = np.empty((n, 3, self.ny, self.nx), np.float64) if want_truth else None
        raw = np.empty((n, 4, len(self.RAW_SUMS)), np.float64)
        opt = lambda a, t: _p(a, t) if a is not None else None
        self._chk(self.lib.psm_gradp_frames(self.h, _p(v, C.c_double), n, k, opt(sc, C.c_float), int(bool(apply_filter)),
                                            opt(gradp, C.c_float), opt(p, C.c_float), opt(truth, C.c_double), _p(raw, C.c_double)))
        return gradp, p, truth, raw

    # -- a frame's dataset rows (float32, as stored) -> scalars + columns on the device, and the evaluators' steps behind that stage
    _rows_bound = 0                 # the width bound with bind_rows (0: none)
    ROWS_KINDS = {"deltas": (0, 3, 11), "poisson": (1, 8, 11), "gradp": (2, 5, 8)}    # kind -> (PSM_ROWS_*, columns, least width)
    ROW_SCALARS = ("U", "dU", "c", "relevant", "U2", "out_scale", "reserved0", "reserved1")

    def bind_rows(self, width: int):
        """After ``bind_frames``: staging for the bound frame count x mesh cells x ``width`` (8..16) float32 rows, the partial maxima
        and the scalar slots: after it a rows step allocates nothing.  Dropped with the frame binding."""
        if not getattr(self, "_frames_bound", False):
            raise RuntimeError("bind_frames has not been called")
        if not 8 <= int(width) <= 16:
            raise ValueError("rows are 8..16 float32 columns wide")
        self._rows_bound = 0
        self._chk(self.lib.psm_bind_rows(self.h, int(width)))
        self._rows_bound = int(width)

    def unbind_rows(self):
        self._rows_bound = 0
        self._chk(self.lib.psm_unbind_rows(self.h))

    def _rows_live(self) -> bool:
        return bool(self._rows_bound) and getattr(self, "_frames_bound", False)

    def _rows_call(self, kind: str, n_frames, width, base=1.0):
        """The argument checks the rows entries share -> (PSM_ROWS_* value, columns)."""
        if kind not in self.ROWS_KINDS:
            raise ValueError(f"kind must be one of {sorted(self.ROWS_KINDS)}")
        code, k, least = self.ROWS_KINDS[kind]
        if not self._rows_live():
            raise RuntimeError("bind_rows has not been called (bind_frames and a new mesh drop the binding)")
        if not least <= int(width) <= 16:
            raise ValueError(f"{kind} rows are {least}..16 float32 columns wide")
        if not 1 <= int(n_frames) <= self.max_cases:
            raise ValueError("n_frames outside [1, max_cases]")
        if kind != "gradp" and not (np.isfinite(base) and base != 0):
            raise ValueError("base must be finite and non-zero")
        return code, k

    def _host_rows(self, kind: str, rows, base=1.0):
        """A host entry's rows [n,n_cells,width] (or [n_cells,width]) -> (float32 C-contiguous array, n, width)."""
        v = np.asarray(rows)
        if v.ndim == 2:
            v = v[None]
        if v.ndim != 3:
            raise ValueError("rows must be [n,n_cells,width]")
        n, n_cells, width = v.shape
        self._rows_call(kind, n, width, base)
        if self.mesh_cells is None:
            raise RuntimeError("the handle holds no mesh (set_mesh / computeOnlyOnce)")
        if n_cells != self.mesh_cells:
            raise ValueError(f"rows must be [n >= 1, {self.mesh_cells} cells, width]")
        if width > self._rows_bound:
            raise ValueError("wider rows than bind_rows reserved staging for")
        return _f32(v), n, width

    def rows_prepare_device(self, kind: str, d_rows: int, n_frames: int, n_cells: int, width: int, d_cols: int = 0, d_scalars: int = 0,
                            base: float = 1.0, phi: float = 1.0, ex: float = 1.0, ey: float = 1.0, stream: int = 0):
        """The stage alone on raw device pointers, two plain launches, asynchronous on ``stream``: ``d_rows`` [n,n_cells,width]
        float32 (the dataset frame cut at ``indice``) -> ``d_cols`` [n,n_cells,k] float64 (0: the frame binding's buffer) and
        ``d_scalars`` [n,8] float64 = ``ROW_SCALARS`` (0: the binding's slots), bit for bit the host statements at the head of the
        ``kind`` evaluator's ``timeSteps`` ('deltas' k = 3, 'poisson' k = 8, 'gradp' k = 5).  ``base``: max_abs_p / max_abs_delta_p
        of the out-scale; ``ex``, ``ey``: max_x - min_x, max_y - min_y of the gradP dataset."""
        code, _ = self._rows_call(kind, n_frames, width, base)
        if self.mesh_cells is None or not 1 <= int(n_cells) <= self.mesh_cells:
            raise ValueError("n_cells outside [1, cells of the mesh]")
        d_rows = self._dev_ptr(d_rows, 4, "d_rows")
        d_cols, d_scalars = self._dev_ptr(d_cols, 8, "d_cols", True), self._dev_ptr(d_scalars, 8, "d_scalars", True)
        params = _f64(np.array([base, phi, ex, ey], np.float64))
        self._chk(self.lib.psm_rows_prepare_device(self.h, code, C.c_void_p(d_rows), int(n_frames), int(n_cells), int(width),
                                                   _p(params, C.c_double), C.c_void_p(d_cols or None), C.c_void_p(d_scalars or None),
                                                   C.c_void_p(stream)))

    def deltas_rows(self, rows: np.ndarray, base: float, apply_filter: bool = False, want_result: bool = True, want_truth: bool = True,
                    want_raw: bool = True):
        """``deltas_frames`` on the dataset rows themselves: ``rows`` [n,n_cells,width >= 11] float32 -> (result, truth, raw,
        scalars [n,8] = ``ROW_SCALARS``); columns, U^2 and the out-scale ``base`` * U^2 are made on the device at the head of the one
        graph replay.  An irrelevant frame (``scalars[:, 3] == 0``) keeps its slot: its result and sums are unspecified."""
        if not self._deltas_bound:
            raise RuntimeError("bind_deltas_frames has not been called (bind_frames and a new mesh drop the binding)")
        v, n, width = self._host_rows("deltas", rows, base)
        if apply_filter and not getattr(self, "_post_bound", False):
            raise RuntimeError("apply_filter needs bind_poststeps")
        result = np.empty((n, self.ny, self.nx), np.float32) if want_result else None
        truth = np.empty((n, self.ny, self.nx), np.float64) if want_truth else None
        raw = np.empty((n, 2, len(self.RAW_SUMS)), np.float64) if want_raw else None
        scalars = np.empty((n, len(self.ROW_SCALARS)), np.float64)
        opt = lambda a, t: _p(a, t) if a is not None else None
        self._chk(self.lib.psm_deltas_rows(self.h, _p(v, C.c_float), n, width, float(base), int(bool(apply_filter)), opt(result, C.c_float),
                                           opt(truth, C.c_double), opt(raw, C.c_double), _p(scalars, C.c_double)))
        return result, truth, raw, scalars

    def poisson_rows(self, rows: np.ndarray, base: float, phi: float = 1.0, apply_filter: bool = False, weighting: bool = True,
                     want_extra: bool = True):
        """``poisson_frames`` on the dataset rows themselves: ``rows`` [n,n_cells,width >= 11] float32 -> (result, change, next,
        extra, scalars [n,8]); the eight columns, (L, U) = (``phi``, U) and the out-scale ``base`` * U^2 are made on the device."""
        v, n, width = self._host_rows("poisson", rows, base)
        n_extra = 2 if weighting else 4
        result = np.empty((n, self.ny, self.nx, self.model.c_out), np.float32)
        change = nxt = None
        if weighting:
            change, nxt = np.empty((n, self.ny, self.nx), np.float32), np.empty((n, self.ny, self.nx), np.float32)
        extra = np.empty((n, n_extra, self.ny, self.nx), np.float64) if want_extra else None
        scalars = np.empty((n, len(self.ROW_SCALARS)), np.float64)
        opt = lambda a, t: _p(a, t) if a is not None else None
        self._chk(self.lib.psm_poisson_rows(self.h, _p(v, C.c_float), n, width, float(base), float(phi), int(bool(apply_filter)),
                                            int(bool(weighting)), opt(extra, C.c_double), _p(result, C.c_float), opt(change, C.c_float),
                                            opt(nxt, C.c_float), _p(scalars, C.c_double)))
        return result, change, nxt, extra, scalars

    def poisson_rows_errors(self, rows: np.ndarray, base: float, phi: float = 1.0, apply_filter: bool = False):
        """``poisson_frames_errors`` on the dataset rows themselves -> (raw [n,3,8], scalars [n,8]): nothing else comes back."""
        v, n, width = self._host_rows("poisson", rows, base)
        raw = np.empty((n, 3, len(self.RAW_SUMS)), np.float64)
        scalars = np.empty((n, len(self.ROW_SCALARS)), np.float64)
        self._chk(self.lib.psm_poisson_rows_errors(self.h, _p(v, C.c_float), n, width, float(base), float(phi), int(bool(apply_filter)), 1,
                                                   _p(raw, C.c_double), _p(scalars, C.c_double)))
        return raw, scalars

    def gradp_rows(self, rows: np.ndarray, ex: float, ey: float, apply_filter: bool = False, want_gradp: bool = True, want_p: bool = True,
                   want_truth: bool = True):
        """``gradp_frames`` on the dataset rows themselves: ``rows`` [n,n_cells,width >= 8] float32 -> (gradp, p, truth, raw,
        scalars [n,8]); ``ex`` = max_x - min_x and ``ey`` = max_y - min_y are taken in float32, as ``EvaluationGradP`` holds them."""
        if not self._gradp_bound:
            raise RuntimeError("bind_gradp_frames has not been called (bind_frames and a new mesh drop the binding)")
        v, n, width = self._host_rows("gradp", rows)
        if not (np.isfinite(ex) and np.isfinite(ey)):
            raise ValueError("ex and ey must be finite")
        if apply_filter and not getattr(self, "_post_bound", False):
            raise RuntimeError("apply_filter needs bind_poststeps")
        gradp = np.empty((n, self.ny, self.nx, 2), np.float32) if want_gradp else None
        p = np.empty((n, self.ny, self.nx), np.float32) if want_p else None
        truth = np.empty((n, 3, self.ny, self.nx), np.float64) if want_truth else None
        raw = np.empty((n, 4, len(self.RAW_SUMS)), np.float64)
        scalars = np.empty((n, len(self.ROW_SCALARS)), np.float64)
        opt = lambda a, t: _p(a, t) if a is not None else None
        self._chk(self.lib.psm_gradp_rows(self.h, _p(v, C.c_float), n, width, float(ex), float(ey), int(bool(apply_filter)),
                                          opt(gradp, C.c_float), opt(p, C.c_float), opt(truth, C.c_double), _p(raw, C.c_double),
                                          _p(scalars, C.c_double)))
        return gradp, p, truth, raw, scalars

    @classmethod
    def metrics_from_sums(cls, raw) -> dict:
        """One row of raw sums -> the dict of ``error_metrics`` (psm_error_metrics_from_sums: host arithmetic, no GPU).  ValueError
        when no finite difference was counted (n == 0), where NumPy raises on the empty selection."""
        r = _f64(np.asarray(raw, np.float64).reshape(-1))
        if r.size != len(cls.RAW_SUMS):
            raise ValueError(f"a raw row holds {len(cls.RAW_SUMS)} sums: {', '.join(cls.RAW_SUMS)}")
        if not r[0] > 0:
            raise ValueError("no finite difference over the flow cells (n == 0): the metrics are undefined")
        out = np.empty(len(cls.METRICS), np.float64)
        _lib.check(_lib.load().psm_error_metrics_from_sums(_p(r, C.c_double), _p(out, C.c_double)))
        return {key: float(v) for key, v in zip(cls.METRICS, out)}

    # -- introspection
    def stage(self, name: str, n_cases: int = 1, layer: int = 0) -> np.ndarray:
        """An intermediate of the last solve; ``name='hidden'``: the output of hidden Dense layer ``layer`` (the handle must have
        been created with PSM_KEEP_HIDDEN=1 in the environment)."""
        m = self.model
        rows = n_cases * self.B
        if name == "hidden":
            if not 0 <= layer < len(m.weights) - 1:
                raise ValueError("layer must name a hidden Dense layer")
            out = np.empty((rows, np.shape(m.weights[layer][0])[1]), np.float32)
            self._chk(self.lib.psm_read_stage(self.h, _lib.STAGE_HIDDEN + layer, _p(out, C.c_float), out.size))
            return out
        shape = {"x_input": (rows, m.p_in), "res": (rows, m.p_out), "block_pred": (rows, m.S, m.S, m.c_out),
                 "offsets": (n_cases, m.c_out, self.B), "shift": (n_cases, m.c_out)}[name]
        out = np.empty(shape, np.float32)
        self._chk(self.lib.psm_read_stage(self.h, _lib.STAGES[name], _p(out, C.c_float), out.size))
        return out

    def profile(self, d_grid: int, n_cases: int, d_fields: int) -> dict:
        ms = (C.c_float * len(_lib.KERNELS))()
        self._chk(self.lib.psm_profile_solve(self.h, C.c_void_p(d_grid), n_cases, C.c_void_p(d_fields), ms))
        return dict(zip(_lib.KERNELS, [float(v) for v in ms]))

    def enable_kernel_timing(self, kernel: str, on=True, repeat: int = 1):
        """Event-time one kernel group; ``repeat`` launches per event pair (see psm.h)."""
        self._chk(self.lib.psm_enable_kernel_timing(self.h, _lib.KERNELS.index(kernel), int(repeat) if on else 0))

    def event_pair_overhead_ms(self, n: int = 200) -> float:
        t = C.c_double()
        self._chk(self.lib.psm_event_pair_overhead(self.h, n, C.byref(t)))
        return t.value

    def kernel_timing(self, kernel: str):
        t, n = C.c_double(), C.c_int64()
        self._chk(self.lib.psm_get_kernel_timing(self.h, _lib.KERNELS.index(kernel), C.byref(t), C.byref(n)))
        return t.value, n.value


# ---------------------------------------------------------------------------
# host-only helpers (no GPU): layout / owner map / host replay of the reassembly
# ---------------------------------------------------------------------------
def layout(variant: str, ny: int, nx: int, S: int = 128, ov: int = 0):
    """-> (blocks[B,4] = (y0, x0, idx_i, idx_j), n_x, n_y) as enumerated at
    PM:306-329 / SMD:461-479 / UGP:479-500."""
    lib = _lib.load()
    nxv, nyv = C.c_int32(), C.c_int32()
    n = lib.psm_layout(_lib.VARIANTS[variant], ny, nx, S, ov, None, 0, C.byref(nxv), C.byref(nyv))
    if n < 0:
        raise _lib.PsmError(n, _lib.last_error())
    blocks = np.zeros((n, 4), np.int32)
    lib.psm_layout(_lib.VARIANTS[variant], ny, nx, S, ov, _p(blocks, C.c_int32), n, None, None)
    return blocks, nxv.value, nyv.value


def owner_map(variant: str, ny: int, nx: int, S: int = 128, ov: int = 0, strict: bool = False) -> np.ndarray:
    out = np.empty((ny, nx), np.int32)
    _lib.check(_lib.load().psm_owner_map(_lib.VARIANTS[variant], ny, nx, S, ov, int(strict), _p(out, C.c_int32)))
    return out


def debug_reassemble_host(variant: str, grid: np.ndarray, block_pred: np.ndarray, c_out: int, S: int = 128,
                          ov: int = 0, strict: bool = False, sdf_ch: int = 2):
    """Host replay of the device reassembly tables (verification helper)."""
    g = _f32(grid)
    ny, nx, c_in = g.shape
    B = block_pred.shape[0]
    bp = _f32(np.asarray(block_pred).reshape(B, -1))
    fields = np.empty((ny, nx, c_out), np.float32)
    offs = np.empty((c_out, B), np.float32)
    sh = np.empty((c_out,), np.float32)
    _lib.check(_lib.load().psm_debug_reassemble_host(
        _lib.VARIANTS[variant], ny, nx, S, ov, int(strict), c_in, c_out, sdf_ch, _p(g, C.c_float), _p(bp, C.c_float),
        _p(fields, C.c_float), _p(offs, C.c_float), _p(sh, C.c_float)))
    return fields, offs, sh


# ---------------------------------------------------------------------------
# reference-shaped operators
# ---------------------------------------------------------------------------
def _grid_from_blocks(x_array: np.ndarray, blocks: np.ndarray, ny: int, nx: int) -> np.ndarray:
    """Rebuild the grid image from the overlapping input blocks (the reference keeps
    only ``self.x_array`` around when it calls ``assemble_prediction``)."""
    S = x_array.shape[1]
    g = np.zeros((ny, nx, x_array.shape[3]), np.float32)
    for b, (y0, x0, _, _) in enumerate(blocks):
        g[y0:y0 + S, x0:x0 + S] = x_array[b]
    return g


def load_artifacts(variant, model_path, directory, var_p, var_in, max_num_PC, standardization_method, shape, overlap,
                   c_in: int = 3, sdf_ch: int = 2):
    """What the reference's ``Evaluation.__init__`` loads (SM_call.py:70-87; Eval_dual_Dense_onlycil.py:51-66):
    ``maxs`` (+ ``maxs_PCA`` for 'max_abs'), the Keras network of ``model_path`` (Dense stack, HDF5), the two
    pickled PCA objects (``ipca_input``, ``ipca_p``: ``.pkl`` like the reference or the ``.npz`` export) with the
    component-count rule of :86-87, and the scaler file of the chosen standardisation (:507-519).
    -> (SurrogateModel, maxs)."""
    from . import formats
    maxs = formats.read_maxs(os.path.join(directory, "maxs"))
    convs, weights = formats.read_keras_conv1d_head(model_path)     # Dense stack, or the conv1D_PCA head (NNs.py:75-124)
    attention = formats.read_keras_attention(model_path)            # densePCA_attention (NNs.py:40-72), else None
    pin = formats.load_pca(formats.find_pca(directory, "ipca_input"))
    pout = formats.load_pca(formats.find_pca(directory, "ipca_p"))
    pc_p = formats.select_num_pc(pout.explained_variance_ratio_, var_p, max_num_PC)
    pc_in = formats.select_num_pc(pin.explained_variance_ratio_, var_in, max_num_PC)
    c_out = 2 if variant == "gradp" else 1
    if pin.components_.shape[1] != shape * shape * c_in or pout.components_.shape[1] != shape * shape * c_out:
        raise ValueError("PCA artefacts do not match the block shape / channel count")
    first_in = weights[0][0].shape[0] // (convs[-1][0].shape[2] if convs else 1)
    if first_in != pc_in or weights[-1][0].shape[1] != pc_p:
        raise ValueError(f"network is {first_in} -> {weights[-1][0].shape[1]} but the PCA rule gives "
                         f"{pc_in} -> {pc_p} components")
    m = SurrogateModel(variant, c_in, c_out, pin.components_[:pc_in], pin.mean_, pout.components_[:pc_p], pout.mean_,
                       list(weights), scaler_kind=standardization_method, S=shape)
    m.conv1d = list(convs)
    m.attention = attention
    m.ov = int(overlap) if overlap else None                 # deltas: overlap in cells; gradp: `avance`
    m.sdf_ch = sdf_ch
    if standardization_method == "max_abs":
        mp = formats.read_maxs(os.path.join(directory, "maxs_PCA"))      # Eval_dual_Dense_onlycil.py:52-55
        m.in_a, m.out_a = float(mp[0]), float(mp[1])
    else:
        fn = "mean_std.npz" if standardization_method == "std" else "min_max_values.npz"
        a, b, c, d = formats.read_scaler_npz(os.path.join(directory, fn), standardization_method)
        m.in_a, m.in_b, m.out_a, m.out_b = (np.asarray(a, np.float64)[:pc_in], np.asarray(b, np.float64)[:pc_in],
                                            np.asarray(c, np.float64)[:pc_p], np.asarray(d, np.float64)[:pc_p])
    return m, maxs


def error_metrics(pred, truth, no_flow_bool) -> dict:
    """The error summary every evaluator of the reference prints per frame (SM_call.py:696-724;
    pressureSM_Poisson/SM_call.py:962-994; Eval_dual_Dense_onlycil.py:667-687): over the flow cells, with
    norm = max - min of the truth there and NaN differences left out,
    BIAS = mean(pred - true) / norm, RMSE = sqrt(mean((pred - true)^2)) / norm, STDE = sqrt(RMSE^2 - BIAS^2), in percent;
    ``mean_err`` / ``mean_sq_err`` are the two values the reference appends to ``pred_minus_true`` / ``pred_minus_true_squared``."""
    true_masked, pred_masked = np.asarray(truth)[~no_flow_bool], np.asarray(pred)[~no_flow_bool]
    norm = np.max(true_masked) - np.min(true_masked)
    diff = pred_masked - true_masked
    diff = diff[~np.isnan(diff)]
    bias = np.mean(diff) / norm * 100
    rmse = np.sqrt(np.mean(diff ** 2)) / norm * 100
    with np.errstate(invalid="ignore"):
        stde = np.sqrt(rmse ** 2 - bias ** 2)
    return {"normVal": float(norm), "biasNorm": float(bias), "stdeNorm": float(stde), "rmseNorm": float(rmse),
            "mean_err": float(np.mean(diff) / norm), "mean_sq_err": float(np.mean(diff ** 2) / norm ** 2)}


def _summary(b, s) -> dict:
    """BIAS / RMSE / STDE [%] of a list of frames as the reference's mains print them (SM_call.py:887-895)."""
    bias, rmse = np.mean(b) * 100, np.sqrt(np.mean(s)) * 100
    return {"BIAS": float(bias), "RMSE": float(rmse), "STDE": float(np.sqrt(max(rmse ** 2 - bias ** 2, 0.0)))}


class Evaluation:
    """``pressureSM_deltas.SM_call.Evaluation`` (SM_call.py:26-87) on the GPU path.

    ``model`` carries the artefacts the reference loads from the working
    directory (``maxs``, the Keras model, ``ipca_*.pkl``, ``mean_std.npz``)."""
    variant = "deltas"

    c_in_expected, sdf_ch_expected = 3, 2
    max_frames = 1                  # case slots of the surrogate (EvaluationPoisson: frames one timeSteps call sends at once)

    def __init__(self, delta, shape, overlap, var_p, var_in, dataset_path, model_path, max_num_PC,
                 standardization_method, model: SurrogateModel = None, device: int = 0, artifact_dir: str = None,
                 max_frames: int = None):
        if standardization_method not in ("std", "min_max", "max_abs"):
            raise ValueError("Standardization method not valid")
        if max_frames is not None:
            if int(max_frames) < 1:
                raise ValueError("max_frames must be at least 1")
            self.max_frames = int(max_frames)                    # the surrogate's max_cases: frames one timeSteps call sends at once
        self.maxs = None
        if model is None:
            # like the reference: `maxs`, `ipca_input.pkl`, `ipca_p.pkl` and the scaler files are read from
            # the working directory (SM_call.py:70-87, 507-519), the network from model_path (:74-79)
            model, self.maxs = load_artifacts(self.variant, model_path, artifact_dir or os.getcwd(), var_p, var_in,
                                              max_num_PC, standardization_method, shape, overlap, self.c_in_expected,
                                              self.sdf_ch_expected)
        self.delta, self.shape, self.overlap = delta, shape, overlap
        self.var_p, self.var_in, self.dataset_path, self.max_num_PC = var_p, var_in, dataset_path, max_num_PC
        self.standardization_method = standardization_method
        self.artifacts = model
        self.pc_in, self.pc_p = model.p_in, model.p_out
        self.device = device
        self.Ref_BC = 0
        self._sur = None
        self.x_array = None

    def _surrogate(self, ny, nx):
        if self._sur is None or (self._sur.ny, self._sur.nx) != (ny, nx):
            if self._sur is not None:
                self._sur.close()
            self._sur = GridSurrogate(self.artifacts, ny, nx, self.max_frames, self.device)
            self._sur.check_bound = True          # timeStep_grid takes arbitrary grids: a foreign geometry drops the binding
        return self._sur

    # ---- dataset-driven entry points (same names and arguments as the reference) -------------------
    def computeOnlyOnce(self, sim):
        """SM_call.py:89-180: geometry of simulation ``sim`` (frame 0 of the dataset) -> interpolation tables,
        SDF image, index map; handed to the GPU library (psm_set_geometry).  Returns 0."""
        from . import formats
        from .geometry import build_geometry_evaluator
        data, top_b, obst_b = formats.read_dataset(self.dataset_path, sim, 0)
        self.indice = formats.first_index(data[0, 0, :, 0], formats.PAD_VALUE)
        cells = np.asarray(data[0, 0, :self.indice], np.float64)
        top = np.asarray(top_b[0, 0, :formats.first_index(top_b[0, 0, :, 0], formats.PAD_VALUE)], np.float64)
        obst = np.asarray(obst_b[0, 0, :formats.first_index(obst_b[0, 0, :, 0], formats.PAD_VALUE)], np.float64)
        t = build_geometry_evaluator(cells[:, 3:5], cells[:, 2], top, obst, self.delta, idw_fallback=True)   # utils.interp_weights
        self.grid_shape_y, self.grid_shape_x = t.ny, t.nx
        self.vert, self.weights, self.indices, self.sdfunct = t.vtx_m2g, t.wts_m2g, t.indices, t.sdfunct[:, :, None]
        sur = self._surrogate(t.ny, t.nx)
        v1, w1 = np.ascontiguousarray(t.vtx_m2g, np.int32), _f64(t.wts_m2g)
        idx, sdf = np.ascontiguousarray(t.indices, np.int32), _f64(t.sdfunct)
        mx = _f64(np.asarray(self.maxs if self.maxs is not None else (1.0, 1.0, 1.0, 1.0), np.float64)[:4])
        sur._chk(sur.lib.psm_set_geometry(sur.h, int(self.indice), t.ny, t.nx, _p(v1, C.c_int32), _p(w1, C.c_double),
                                          _p(idx, C.c_int32), _p(sdf, C.c_double), None, None, _p(mx, C.c_double), 1, 1, 0.05))
        sur.mesh_cells = int(self.indice)
        sur._frames_bound = sur._feat_bound = sur._post_bound = sur._deltas_bound = sur._gradp_bound = False; sur._rows_bound = 0      # the new plan dropped them
        self.tables = t
        self._bind_simulation_geometry(sur, t.sdfunct, float(mx[2]))
        return 0

    def _bind_simulation_geometry(self, sur, sdfunct: np.ndarray, max_abs_dist: float):
        """computeOnlyOnce fixes the obstacle for every timeStep of the simulation: bind its flow-cell pattern (the SDF
        channel exactly as timeStep normalises it) so that the steps take the 6-launch path.  Grids of another
        geometry passed to timeStep_grid drop the binding again (GridSurrogate._check_bound).  The frames of ``timeSteps`` are solved one by
        one inside their call, so they take this single-case binding too."""
        g = np.zeros((sur.ny, sur.nx, self.artifacts.c_in), np.float32)
        sd = np.asarray(sdfunct, np.float64) / max_abs_dist
        g[..., self.artifacts.sdf_ch] = np.where(np.isnan(sd), 0.0, sd).astype(np.float32)
        sur.bind_geometry(g)

    def _mesh_to_grid(self, columns: np.ndarray) -> np.ndarray:
        """interpolate_fill + scatter of k cell columns on the GPU (psm_mesh_to_grid) -> [Ny,Nx,k] float64."""
        sur = self._surrogate(self.grid_shape_y, self.grid_shape_x)
        v = _f64(columns)
        out = np.empty((self.grid_shape_y, self.grid_shape_x, v.shape[1]), np.float64)
        sur._chk(sur.lib.psm_mesh_to_grid(sur.h, _p(v, C.c_double), v.shape[0], v.shape[1], 1, _p(out, C.c_double)))
        return out

    def timeStep(self, sim, time, plot_intermediate_fields=False, save_plots=False, show_plots=False, apply_filter=False):
        """SM_call.py:367-575 without the plots and error prints: frame (sim, time) of the dataset -> assembled
        delta-p image [Ny,Nx] (dimensional, like ``deltap_res``), or 0 for an irrelevant time step (:417-421).
        Also kept: ``self.cfd_results`` (the frame's own delta-p image) and ``self.no_flow_bool``."""
        from . import formats
        if getattr(self, "tables", None) is None:
            raise RuntimeError("computeOnlyOnce has not been called")
        data, _, _ = formats.read_dataset(self.dataset_path, sim, time)
        d = data[0, 0, :self.indice]                  # float32 like the file: the reference normalises in float32
        Ux, Uy, p = d[:, 0:1], d[:, 1:2], d[:, 2:3]
        delta_U, delta_p = d[:, 5:7], d[:, 7:8]
        delta_U_prev, delta_p_prev = d[:, 8:10], d[:, 10:11]
        deltaU_changed = np.abs(delta_U - delta_U_prev).sum(axis=-1)                     # :400-401
        deltaU_changed = deltaU_changed / deltaU_changed.max()
        U_max_norm = np.max(np.sqrt(np.square(Ux) + np.square(Uy)))                      # :407
        deltaU_max_norm = np.max(np.sqrt(np.square(delta_U[:, 0:1]) + np.square(delta_U[:, 1:2])))
        if (deltaU_max_norm / U_max_norm) < 1e-4:                                       # :413-421
            return 0
        cols = np.concatenate([delta_U / U_max_norm, delta_p / pow(U_max_norm, 2.0), p, deltaU_changed[:, None], delta_p_prev],
                              axis=1).astype(np.float64)
        g = self._mesh_to_grid(cols)                                                    # :423-431
        max_abs_Ux, max_abs_Uy, max_abs_dist, max_abs_p = [float(v) for v in self.maxs[:4]]
        grid = np.zeros((self.grid_shape_y, self.grid_shape_x, 5))
        grid[..., 0:2] = g[..., 0:2]
        grid[..., 2] = self.sdfunct[..., 0]
        grid[..., 3:5] = g[..., 2:4]
        grid[np.isnan(grid)] = 0                                                        # :439
        grid[..., 0] /= max_abs_Ux; grid[..., 1] /= max_abs_Uy                          # :442-445
        grid[..., 2] /= max_abs_dist; grid[..., 3] /= max_abs_p
        self.grid = grid
        self.deltaU_change_grid, self.deltaP_prev_grid = g[..., 4], g[..., 5]            # :448-451 (NaNs kept)
        self.max_abs_p = max_abs_p
        res = self.timeStep_grid(grid[..., :3], U_max_norm, max_abs_p)                   # :452-572
        # :553-557 the error of the decoded blocks against the de-meaned label blocks, before the assembly
        mb = self._surrogate(*grid.shape[:2]).block_error(grid[..., :3], grid[..., 3])
        for name, key in (("pred_minus_true_block", "mean_err"), ("pred_minus_true_squared_block", "mean_sq_err")):
            if not hasattr(self, name):
                setattr(self, name, [])
            getattr(self, name).append(mb[key])
        if not isinstance(getattr(self, "last_metrics", None), dict):
            self.last_metrics = {}
        self.last_metrics["blocks"] = mb
        if apply_filter:
            res = self._surrogate(*grid.shape[:2]).gaussian_filter(res, (10, 10))
        self.cfd_results = grid[..., 3] * max_abs_p * pow(U_max_norm, 2.0)               # :580 (float32 square, like the reference)
        self.no_flow_bool = grid[..., 2] == 0
        self.U_max_norm = float(U_max_norm)
        self._record_errors(res, self.cfd_results, self.no_flow_bool)
        return res

    FRAME_COLUMNS = 3               # dUx / U, dUy / U, dp / U^2 (the label column)

    def _bind_frames(self, sur, apply_filter: bool):
        """What timeSteps needs on the handle, once per computeOnlyOnce (whose new plan drops them): the frame staging, the deltas
        binding with the simulation's SDF plane, and the post-steps (SM_call.py:353) when a filtered field is asked for."""
        if apply_filter and not sur._post_bound:
            sur.bind_poststeps((10, 10), (50, 50))
        if getattr(self, "_frames_tables", None) is self.tables and sur._frames_bound and sur._deltas_bound:
            return
        sur.bind_frames(self.max_frames, self.FRAME_COLUMNS)
        sur.bind_deltas_frames(self.sdfunct[..., 0], [float(v) for v in self.maxs[:4]])
        self._frames_tables = self.tables

    def timeSteps(self, sim, times, apply_filter=False, fields=True, device_prep=False):
        """``timeStep`` for several frames of one simulation, the relevant ones sent ``max_frames`` at a time as ONE call each
        (``deltas_frames``: cell columns -> planes -> image -> solve -> filter -> both error blocks on the device).  The per-frame
        host scalars and the skip rule are those of ``timeStep``; ``pred_minus_true*``, ``pred_minus_true*_block`` and
        ``last_metrics`` are filled in frame order.  Returns the list of delta-p images with 0 for an irrelevant frame; afterwards
        ``cfd_results``, ``no_flow_bool`` and ``U_max_norm`` hold what ``timeStep`` leaves on the last relevant frame (``grid`` and
        the weighting planes are not produced).  The block errors come from the device sums in either mode.
        ``fields=False``: a metrics-only sweep -- nothing but the sums comes back, the field's metrics are taken from them too, the
        return is one ``{'delta_p': metrics, 'blocks': metrics}`` dict per frame (0 for an irrelevant frame) and ``cfd_results`` is
        None.
        ``device_prep=True``: the loop over ``times`` only slices the float32 rows; ``deltas_rows`` derives U_max_norm, the skip rule,
        the columns and the scales on the device (every frame keeps its slot in its call, an irrelevant one is read off the
        returned scalars), and everything returned and recorded holds the bits of the default mode."""
        from . import formats
        if getattr(self, "tables", None) is None:
            raise RuntimeError("computeOnlyOnce has not been called")
        times = [int(t) for t in times]
        if device_prep:
            return self._time_steps_rows(sim, times, apply_filter, fields)
        out, cols, Us, slot = [0] * len(times), [], [], []
        for i, time in enumerate(times):
            data, _, _ = formats.read_dataset(self.dataset_path, sim, time)
            d = data[0, 0, :self.indice]                  # float32 like the file: the reference normalises in float32
            Ux, Uy = d[:, 0:1], d[:, 1:2]
            delta_U, delta_p = d[:, 5:7], d[:, 7:8]
            U_max_norm = np.max(np.sqrt(np.square(Ux) + np.square(Uy)))                      # :407
            deltaU_max_norm = np.max(np.sqrt(np.square(delta_U[:, 0:1]) + np.square(delta_U[:, 1:2])))
            if (deltaU_max_norm / U_max_norm) < 1e-4:                                       # :413-421
                continue
            cols.append(np.concatenate([delta_U / U_max_norm, delta_p / pow(U_max_norm, 2.0)], axis=1).astype(np.float64))
            Us.append(U_max_norm)
            slot.append(i)
        if not cols:
            return out
        sur = self._surrogate(self.grid_shape_y, self.grid_shape_x)
        self._bind_frames(sur, apply_filter)
        max_abs_dist, max_abs_p = float(self.maxs[2]), float(self.maxs[3])
        self.max_abs_p = max_abs_p
        sd = np.nan_to_num(np.asarray(self.sdfunct[..., 0], np.float64), nan=0.0) / max_abs_dist
        self.no_flow_bool = sd == 0
        if not isinstance(getattr(self, "last_metrics", None), dict):
            self.last_metrics = {}
        for name in ("pred_minus_true_block", "pred_minus_true_squared_block"):
            if not hasattr(self, name):
                setattr(self, name, [])
        for c0 in range(0, len(cols), self.max_frames):
            chunk, U_chunk = np.stack(cols[c0:c0 + self.max_frames]), Us[c0:c0 + self.max_frames]
            res, truth, raw = sur.deltas_frames(chunk, [float(pow(U, 2.0)) for U in U_chunk],       # :580 (float32 square, like the reference)
                                                out_scale=[max_abs_p * U ** 2 for U in U_chunk], apply_filter=apply_filter,
                                                want_result=fields, want_truth=fields)
            for j, U in enumerate(U_chunk):
                self.U_max_norm = float(U)
                mb = sur.metrics_from_sums(raw[j, 1])                                          # :553-557, before the assembly
                mb.update(norm_pred=float(raw[j, 1, 6] - raw[j, 1, 5]), n=int(raw[j, 1, 0]))
                self.pred_minus_true_block.append(mb["mean_err"])
                self.pred_minus_true_squared_block.append(mb["mean_sq_err"])
                self.last_metrics["blocks"] = mb
                if fields:
                    self.cfd_results = truth[j]
                    m = self._record_errors(res[j], self.cfd_results, self.no_flow_bool)
                    out[slot[c0 + j]] = res[j]
                else:
                    m = self._record_metrics(sur.metrics_from_sums(raw[j, 0]))
                    out[slot[c0 + j]] = {"delta_p": m, "blocks": mb}
        if not fields:
            self.cfd_results = None
        return out

    def _time_steps_rows(self, sim, times, apply_filter, fields):
        """``timeSteps(device_prep=True)``: the dataset rows as stored go up, the device makes scalars and columns."""
        from . import formats
        out = [0] * len(times)
        rows = [formats.read_dataset(self.dataset_path, sim, time)[0][0, 0, :self.indice] for time in times]
        if not rows:
            return out
        sur = self._surrogate(self.grid_shape_y, self.grid_shape_x)
        self._bind_frames(sur, apply_filter)
        if sur._rows_bound < rows[0].shape[1]:
            sur.bind_rows(rows[0].shape[1])
        max_abs_dist, max_abs_p = float(self.maxs[2]), float(self.maxs[3])
        calls = [sur.deltas_rows(np.stack(rows[c0:c0 + self.max_frames]), max_abs_p, apply_filter=apply_filter, want_result=fields,
                                 want_truth=fields) for c0 in range(0, len(rows), self.max_frames)]
        if not any(sc[:, 3].any() for _, _, _, sc in calls):
            return out
        self.max_abs_p = max_abs_p
        sd = np.nan_to_num(np.asarray(self.sdfunct[..., 0], np.float64), nan=0.0) / max_abs_dist
        self.no_flow_bool = sd == 0
        if not isinstance(getattr(self, "last_metrics", None), dict):
            self.last_metrics = {}
        for name in ("pred_minus_true_block", "pred_minus_true_squared_block"):
            if not hasattr(self, name):
                setattr(self, name, [])
        for c, (res, truth, raw, sc) in enumerate(calls):
            for j in range(sc.shape[0]):
                if sc[j, 3] == 0:                                                              # :413-421, decided on the device
                    continue
                self.U_max_norm = float(sc[j, 0])
                mb = sur.metrics_from_sums(raw[j, 1])
                mb.update(norm_pred=float(raw[j, 1, 6] - raw[j, 1, 5]), n=int(raw[j, 1, 0]))
                self.pred_minus_true_block.append(mb["mean_err"])
                self.pred_minus_true_squared_block.append(mb["mean_sq_err"])
                self.last_metrics["blocks"] = mb
                if fields:
                    self.cfd_results = truth[j]
                    m = self._record_errors(res[j], self.cfd_results, self.no_flow_bool)
                    out[c * self.max_frames + j] = res[j]
                else:
                    m = self._record_metrics(sur.metrics_from_sums(raw[j, 0]))
                    out[c * self.max_frames + j] = {"delta_p": m, "blocks": mb}
        if not fields:
            self.cfd_results = None
        return out

    print_metrics = False           # True: print the per-frame error block like the reference's timeStep does

    def _record_errors(self, field, truth, no_flow_bool, suffix: str = "", title: str = None):
        """SM_call.py:696-724: normalised bias / squared error of the assembled field over the flow cells, appended to
        ``pred_minus_true<suffix>`` / ``pred_minus_true_squared<suffix>`` (what the mains average); the frame's
        normVal / biasNorm / stdeNorm / rmseNorm are kept in ``self.last_metrics[suffix or 'delta_p']``."""
        return self._record_metrics(error_metrics(field, truth, no_flow_bool), suffix, title)

    def _record_metrics(self, m: dict, suffix: str = "", title: str = None):
        """The bookkeeping of ``_record_errors`` for metrics that exist already (``timeSteps(fields=False)``: from device sums)."""
        for name in ("pred_minus_true" + suffix, "pred_minus_true_squared" + suffix):
            if not hasattr(self, name):
                setattr(self, name, [])
        getattr(self, "pred_minus_true" + suffix).append(m["mean_err"])
        getattr(self, "pred_minus_true_squared" + suffix).append(m["mean_sq_err"])
        if not isinstance(getattr(self, "last_metrics", None), dict):
            self.last_metrics = {}
        self.last_metrics[suffix.lstrip("_") or "delta_p"] = m
        if self.print_metrics:
            print(f"""
		{'** ' + title + ' **' if title else ''}
		normVal  = {m['normVal']} Pa
		biasNorm = {m['biasNorm']:.3f}%
		stdeNorm = {m['stdeNorm']:.3f}%
		rmseNorm = {m['rmseNorm']:.3f}%
		""", flush=True)
        return m

    def timeStep_grid(self, grid: np.ndarray, U_max_norm: float = 1.0, max_abs_p: float = 1.0) -> np.ndarray:
        """Grid-native body of ``timeStep`` (SM_call.py:452-575): -> deltap_res [Ny,Nx]."""
        sur = self._surrogate(grid.shape[0], grid.shape[1])
        return sur.solve(grid, out_scale=[max_abs_p * U_max_norm ** 2])[0, :, :, 0]

    def label_self_check(self, grid: np.ndarray, labels: np.ndarray) -> np.ndarray:
        """The reference's own check of the assembly algorithm: the CFD labels, de-meaned per block over the flow cells
        (SM_call.py:487-488; Eval_dual_Dense_onlycil.py:509-511), pushed through the same reassembly as the prediction
        ("it should be almost perfect in that case", SM_call.py:577-580; live as test_dPdx / test_dPdy at
        Eval_dual_Dense_onlycil.py:546-547).  ``grid`` [Ny,Nx,>=c_in] normalised input image (flow mask = its SDF
        channel), ``labels`` [Ny,Nx,c_out] -> assembled label field(s) [Ny,Nx,c_out]; also keeps ``self.y_array``."""
        sur = self._surrogate(grid.shape[0], grid.shape[1])
        self.y_array = sur.label_blocks(grid, labels)
        return sur.reassemble(grid, self.y_array)

    def assemble_prediction(self, array, indices_list, n_x, n_y, apply_filter, shape_x, shape_y,
                            deltaU_change_grid=None, deltaP_prev_grid=None, apply_deltaU_change_wgt=False):
        """SM_call.py:182: ``array`` [B,S,S] corrected and pasted into [shape_y, shape_x].
        The flow mask comes from ``self.x_array`` like in the reference."""
        if self.x_array is None:
            raise ValueError("self.x_array must hold the input blocks")
        blocks, nx_, ny_ = layout(self.variant, shape_y, shape_x, self.shape, self.overlap)
        if (nx_, ny_) != (n_x, n_y) or len(indices_list) != len(blocks):
            raise ValueError("n_x / n_y / indices_list do not match this grid")
        sur = self._surrogate(shape_y, shape_x)
        grid = _grid_from_blocks(np.asarray(self.x_array, np.float32), blocks, shape_y, shape_x)
        result = sur.reassemble(grid, np.asarray(array))[..., 0]
        return self._post_steps(sur, result, apply_filter, deltaU_change_grid, deltaP_prev_grid, apply_deltaU_change_wgt)

    @staticmethod
    def _post_steps(sur, result, apply_filter, deltaU_change_grid, deltaP_prev_grid, apply_deltaU_change_wgt):
        """Tail of ``assemble_prediction`` (SM_call.py:352-363): optional Gaussian filter and deltaU-change weighting."""
        filter_tuple = (10, 10)                                   # SM_call.py:353
        if apply_filter:
            result = sur.gaussian_filter(result, filter_tuple)
        change_in_deltap = None
        if apply_deltaU_change_wgt:                               # SM_call.py:359-363
            w = sur.gaussian_filter(np.asarray(deltaU_change_grid, np.float32), (50, 50))
            change_in_deltap = (result - np.asarray(deltaP_prev_grid, np.float32)) * w
            change_in_deltap = sur.gaussian_filter(change_in_deltap, filter_tuple)
        return result, change_in_deltap


def call_SM_main(delta, model_name, shape, overlap_ratio, var_p, var_in, max_num_PC, dataset_path,
                 plot_intermediate_fields=False, standardization_method="std", save_plots=False, show_plots=False,
                 apply_filter=False, create_GIF=False, n_sims=1, n_ts=1, device: int = 0, artifact_dir: str = None,
                 frames_per_call: int = 1, fields: bool = True, device_prep: bool = False):
    """``pressureSM_deltas.SM_call.call_SM_main`` (SM_call.py:778-900): evaluate ``n_ts`` frames of ``n_sims``
    simulations of the dataset and return the error summary the reference prints -- per simulation and overall
    BIAS / STDE / RMSE [%] of delta-p over the flow cells, and BIAS_block / RSME_block / STDE_block [%] of the decoded blocks
    before the assembly (SM_call.py:824-826, from ``utils.compute_in_block_error``); plots and GIFs are not produced.
    ``frames_per_call`` > 1: the frames of a simulation go through ``Evaluation.timeSteps``, that many per call, instead of one
    ``timeStep`` each.  ``fields=False``: the same summary from ``timeSteps(..., fields=False)``, whose error sums are taken on the
    device: no field is copied back.  ``device_prep=True`` (implies ``timeSteps``): the per-frame scalars and columns are made on the
    device from the dataset rows (``timeSteps(..., device_prep=True)``)."""
    overlap = int(overlap_ratio * shape)
    batched = frames_per_call > 1 or not fields or device_prep
    ev = Evaluation(delta, shape, overlap, var_p, var_in, dataset_path, model_name, max_num_PC, standardization_method,
                    device=device, artifact_dir=artifact_dir, max_frames=frames_per_call)
    ev.pred_minus_true, ev.pred_minus_true_squared = [], []
    ev.pred_minus_true_block, ev.pred_minus_true_squared_block = [], []

    summary = _summary
    out = {"sims": []}
    for sim in range(n_sims):
        n0 = len(ev.pred_minus_true)
        ev.computeOnlyOnce(sim)
        if batched:
            ev.timeSteps(sim, range(n_ts), apply_filter, fields=fields, device_prep=device_prep)
        for time in range(0 if batched else n_ts):
            ev.timeStep(sim, time, plot_intermediate_fields, save_plots, show_plots, apply_filter)
        if len(ev.pred_minus_true) > n0:
            s = summary(ev.pred_minus_true[n0:], ev.pred_minus_true_squared[n0:])
            # SM_call.py:824-826 BIAS_block / RSME_block / STDE_block: the same summary over the per-frame block errors
            blk = summary(ev.pred_minus_true_block[n0:], ev.pred_minus_true_squared_block[n0:])
            s.update(BIAS_block=blk["BIAS"], RSME_block=blk["RMSE"], STDE_block=blk["STDE"])
            out["sims"].append(s)
        else:
            out["sims"].append(None)                       # every frame of this simulation was irrelevant
    if ev.pred_minus_true:
        out["overall"] = summary(ev.pred_minus_true, ev.pred_minus_true_squared)
        blk = summary(ev.pred_minus_true_block, ev.pred_minus_true_squared_block)
        out["overall"].update(BIAS_block=blk["BIAS"], RSME_block=blk["RMSE"], STDE_block=blk["STDE"])
    return out


def call_SM_main_Poisson(delta, model_name, shape, overlap_ratio, var_p, var_in, max_num_PC, dataset_path,
                         plot_intermediate_fields, standardization_method, k, save_plots, show_plots, apply_filter, create_GIF,
                         n_sims, n_ts, phis_fn, device: int = 0, artifact_dir: str = None, sim_offset: int = 1, time_offset: int = 16,
                         frames_per_call: int = 1, fields: bool = True, device_prep: bool = False):
    """``pressureSM_Poisson.SM_call.call_SM_main`` (pressureSM_Poisson/SM_call.py:1069-1170), same argument list: evaluates
    frames ``time_offset .. time_offset + n_ts`` of simulations ``sim_offset .. sim_offset + n_sims`` (the reference's
    ``sim += 1`` / ``time += 16``, :1095, :1104) with ``phi = phi_list[sim]`` from ``phis_fn`` and returns the three error
    summaries it prints -- delta-p with the deltaU-change weighting, delta-p without it, and p -- per simulation (last
    ``n_ts`` frames, :1110-1116) and overall.  Plots and GIFs are not produced.  ``frames_per_call`` > 1: the frames of a
    simulation go through ``EvaluationPoisson.timeSteps``, that many per call, instead of one ``timeStep`` each.  ``fields=False``:
    the same summaries from ``timeSteps(..., fields=False)``, whose error sums are taken on the device: no field is copied back.
    ``device_prep=True`` (implies ``timeSteps``): the per-frame scalars and columns are made on the device from the dataset rows."""
    overlap = int(overlap_ratio * shape)
    ev = EvaluationPoisson(delta, shape, overlap, var_p, var_in, dataset_path, model_name, max_num_PC, standardization_method,
                           k, phis_fn, device=device, artifact_dir=artifact_dir, max_frames=frames_per_call)
    for sfx in ("", "_deltap_crude", "_p"):
        setattr(ev, "pred_minus_true" + sfx, [])
        setattr(ev, "pred_minus_true_squared" + sfx, [])
    phi_list = np.atleast_1d(np.loadtxt(phis_fn, dtype=float))
    out = {"sims": []}
    for sim in range(n_sims):
        sim += sim_offset
        ev.computeOnlyOnce(sim)
        phi = phi_list[sim]
        n0 = len(ev.pred_minus_true)
        batched = frames_per_call > 1 or not fields or device_prep
        if batched:
            ev.timeSteps(sim, [time + time_offset for time in range(n_ts)], apply_filter, phi, fields=fields, device_prep=device_prep)
        for time in range(0 if batched else n_ts):
            ev.timeStep(sim, time + time_offset, plot_intermediate_fields, save_plots, show_plots, apply_filter, phi)
        if len(ev.pred_minus_true) > n0:
            out["sims"].append({"sim": sim, "phi": float(phi),
                                "delta_p": _summary(ev.pred_minus_true[-n_ts:], ev.pred_minus_true_squared[-n_ts:]),
                                "delta_p_no_weighting": _summary(ev.pred_minus_true_deltap_crude[-n_ts:], ev.pred_minus_true_squared_deltap_crude[-n_ts:])})
        else:
            out["sims"].append(None)
    if ev.pred_minus_true:
        out["overall"] = {"delta_p": _summary(ev.pred_minus_true, ev.pred_minus_true_squared),
                          "delta_p_no_weighting": _summary(ev.pred_minus_true_deltap_crude, ev.pred_minus_true_squared_deltap_crude),
                          "p": _summary(ev.pred_minus_true_p, ev.pred_minus_true_squared_p)}
    return out


def main_gradP(delta=5e-3, model_directory="model_1.h5", shape=128, avance=None, var_p=0.95, var_in=0.95, max_number_PC=512,
               hdf5_path="dataset_gradP_cil.hdf5", plot_intermediate_fields=True, save_plots=True, show_plots=False,
               apply_filter=False, sims=(0,), n_ts=5, device: int = 0, artifact_dir: str = None, frames_per_call: int = 1,
               fields: bool = True, device_prep: bool = False):
    """``main`` of the U_to_gradP evaluator (Eval_dual_Dense_onlycil.py:692-744) with its hard-coded inputs as defaults
    (``avance = int(0.75 * shape)``, simulations ``[0]``, five time steps): computeOnlyOnce + timeStep per frame, then
    BIAS / RMSE / STDE [%] "for the sim" from the accumulated per-frame values (:735-742) -- printed like the reference and
    returned.  Plots are not produced.
    ``frames_per_call`` > 1: the frames of a simulation go through ``EvaluationGradP.timeSteps``, that many per call, instead of one
    ``timeStep`` each.  ``fields=False``: the same summary from ``timeSteps(..., fields=False)``, whose error sums are taken on the
    device: no field is copied back.  ``device_prep=True`` (implies ``timeSteps``): the per-frame scalar and columns are made on the
    device from the dataset rows.  With the defaults the loop is the per-frame one."""
    if avance is None:
        avance = int(0.75 * shape)
    ev = EvaluationGradP(delta, shape, avance, var_p, var_in, hdf5_path, model_directory, max_number_PC, device=device,
                         artifact_dir=artifact_dir, max_frames=frames_per_call)
    ev.pred_minus_true, ev.pred_minus_true_squared = [], []
    out = {"sims": [], "frames": []}
    batched = frames_per_call > 1 or not fields or device_prep
    for sim in sims:
        ev.computeOnlyOnce(sim)
        for t0 in range(0, n_ts if batched else 0, frames_per_call):
            chunk = range(t0, min(t0 + frames_per_call, n_ts))
            ev.timeSteps(sim, chunk, apply_filter, fields=fields, device_prep=device_prep)
            for time, m in zip(chunk, ev.frame_metrics):
                out["frames"].append(dict(sim=sim, time=time, **{k: dict(v) for k, v in m.items()}))
        for time in range(0 if batched else n_ts):
            ev.timeStep(sim, time, plot_intermediate_fields, save_plots, show_plots, apply_filter)
            out["frames"].append(dict(sim=sim, time=time, **{k: dict(v) for k, v in ev.last_metrics.items()}))
        # like the reference: over everything accumulated so far, not only this simulation (:735-737)
        s = _summary(ev.pred_minus_true, ev.pred_minus_true_squared)
        print("Metrics for the whole simulation:")
        print("BIAS for the sim: " + str(s["BIAS"]))
        print("RMSE for the sim: " + str(s["RMSE"]))
        print("STDE for the sim: " + str(s["STDE"]))
        out["sims"].append(s)
    return out


class EvaluationPoisson(Evaluation):
    """``pressureSM_Poisson.SM_call.Evaluation`` (pressureSM_Poisson/SM_call.py:71-118): the deltas layout fed with
    four channels (arcsinh-smoothed Poisson source term, dUx, dUy, SDF; mask = channel 3).

    ``max_abs`` = (max_abs_Poisson_term_1, max_abs_delta_Ux, max_abs_delta_Uy, max_abs_dist, max_abs_delta_p),
    the constants the reference reads from its ``maxs`` file."""
    variant = "deltas"
    c_in_expected, sdf_ch_expected = 4, 3

    def __init__(self, delta, shape, overlap, var_p, var_in, dataset_path, model_path, max_num_PC,
                 standardization_method, k, phis_fn, model: SurrogateModel = None, device: int = 0,
                 max_abs=None, artifact_dir: str = None, max_frames: int = 1):
        super().__init__(delta, shape, overlap, var_p, var_in, dataset_path, model_path, max_num_PC,
                         standardization_method, model, device, artifact_dir)
        if int(max_frames) < 1:
            raise ValueError("max_frames must be at least 1")
        self.max_frames = int(max_frames)                        # the surrogate's max_cases: frames one timeSteps call sends at once
        model = self.artifacts
        if model.c_in != 4 or model.sdf_ch != 3:
            raise ValueError("the Poisson surrogate takes 4 input channels with the SDF in channel 3")
        self.k, self.phis_fn = k, phis_fn
        if max_abs is None:                                     # the five values of the `maxs` file (SM_call.py:124)
            max_abs = self.maxs if self.maxs is not None else (1.0, 1.0, 1.0, 1.0, 1.0)
        (self.max_abs_Poisson_term_1, self.max_abs_delta_Ux, self.max_abs_delta_Uy, self.max_abs_dist,
         self.max_abs_delta_p) = [float(v) for v in max_abs]

    def timeStep(self, sim, time, plot_intermediate_fields=False, save_plots=False, show_plots=False, apply_filter=False,
                 phi=1.0):
        """pressureSM_Poisson/SM_call.py:519-848 without plots and error prints: frame (sim, time) of the dataset ->
        ``field_deltap`` [Ny,Nx] = previous delta-p image + weighted change (:843-848), or 0 for an irrelevant step."""
        from . import formats
        if getattr(self, "tables", None) is None:
            raise RuntimeError("computeOnlyOnce has not been called")
        data, _, _ = formats.read_dataset(self.dataset_path, sim, time)
        d = data[0, 0, :self.indice]
        Ux, Uy, p = d[:, 0:1], d[:, 1:2], d[:, 2:3]
        delta_U, delta_p = d[:, 5:7], d[:, 7:8]
        delta_U_prev, delta_p_prev = d[:, 8:10], d[:, 10:11]
        deltaU_changed = np.abs(delta_U - delta_U_prev).sum(axis=-1)
        deltaU_changed = deltaU_changed / deltaU_changed.max()
        U_max_norm = np.max(np.sqrt(np.square(Ux) + np.square(Uy)))
        deltaU_max_norm = np.max(np.sqrt(np.square(delta_U[:, 0:1]) + np.square(delta_U[:, 1:2])))
        if (deltaU_max_norm / U_max_norm) < 1e-4 or deltaU_max_norm < 1e-6 or U_max_norm < 1e-6:      # :562-567
            return 0
        cols = np.concatenate([Ux, Uy, delta_U, delta_p, p, deltaU_changed[:, None], delta_p_prev], axis=1).astype(np.float64)
        g = self._mesh_to_grid(cols)                                                                 # :577-600, NaNs kept
        U = float(U_max_norm)
        self.U_max_norm = U
        field_deltap = self.timeStep_grid(g[..., 0], g[..., 1], g[..., 2], g[..., 3], self.sdfunct[..., 0], phi, U,
                                          deltaU_change_grid=g[..., 6], deltaP_prev_grid=g[..., 7], apply_filter=apply_filter,
                                          apply_deltaU_change_wgt=True)                               # :831
        # ---- the three error blocks of :962-1043: delta-p (weighted), delta-p without the weighting, and p
        delta_p_grid = np.nan_to_num(g[..., 4] / pow(U, 2.0), nan=0.0) / self.max_abs_delta_p         # :687-711 (channel 4)
        p_grid = np.nan_to_num(g[..., 5], nan=0.0)                                                    # :692-702 (channel 5)
        self.cfd_results = delta_p_grid * self.max_abs_delta_p * pow(U, 2.0)                          # :849
        sd = np.nan_to_num(self.sdfunct[..., 0], nan=0.0) / self.max_abs_dist
        self.no_flow_bool = sd == 0                                                                   # :850
        self.p_pred = (p_grid - self.cfd_results) + field_deltap                                      # :907-908
        self._record_errors(field_deltap, self.cfd_results, self.no_flow_bool, "", "Error in delta_p")
        self._record_errors(self.deltap_res, self.cfd_results, self.no_flow_bool, "_deltap_crude", "Error in delta_p - no weighting")
        self._record_errors(self.p_pred, p_grid, self.no_flow_bool, "_p", "Error in p")
        return field_deltap

    def _bind_simulation_geometry(self, sur, sdfunct: np.ndarray, max_abs_dist: float):
        """One frame at a time: as the base class.  ``max_frames`` > 1: the simulation's obstacle in every one of the slots, with
        the SDF channel as the features write it (float32 of sdfunct / max_abs_dist), so that a full batch takes the bound route."""
        if self.max_frames == 1:
            return super()._bind_simulation_geometry(sur, sdfunct, max_abs_dist)
        g = np.zeros((self.max_frames, sur.ny, sur.nx, self.artifacts.c_in), np.float32)
        sd = np.asarray(sdfunct, np.float64) / self.max_abs_dist
        g[..., self.artifacts.sdf_ch] = np.where(np.isnan(sd), 0.0, sd).astype(np.float32)[None]
        sur.bind_geometry(g)

    FRAME_COLUMNS = 8               # Ux, Uy, dUx, dUy | delta_p, p (the label planes) | dU-change weight, delta_p_prev

    def _bind_frames(self, sur):
        """What timeSteps needs on the handle, once per computeOnlyOnce (whose new plan drops all three): the features with the
        simulation's SDF plane in every slot, the post-steps (SM_call.py:353, :360) and the frame staging."""
        if getattr(self, "_frames_tables", None) is self.tables and sur._frames_bound and sur._feat_bound and sur._post_bound:
            return
        sur.bind_features(np.repeat(np.asarray(self.sdfunct[..., 0], np.float64)[None], self.max_frames, axis=0), self.k,
                          (self.max_abs_Poisson_term_1, self.max_abs_delta_Ux, self.max_abs_delta_Uy, self.max_abs_dist))
        sur.bind_poststeps((10, 10), (50, 50))
        sur.bind_frames(self.max_frames, self.FRAME_COLUMNS)
        self._frames_tables = self.tables

    ERROR_BLOCKS = (("", "Error in delta_p"), ("_deltap_crude", "Error in delta_p - no weighting"), ("_p", "Error in p"))

    def timeSteps(self, sim, times, apply_filter=False, phi=1.0, fields=True, device_prep=False):
        """``timeStep`` for several frames of one simulation, the relevant ones sent ``max_frames`` at a time as ONE call each
        (``poisson_frames``: cell columns -> planes -> features -> solve -> post-steps on the device).  The per-frame host scalars
        and the three error blocks are those of ``timeStep``, in frame order; returns the list of ``field_deltap`` with 0 for an
        irrelevant frame.  Afterwards the attributes hold what ``timeStep`` leaves on the last relevant frame, and
        ``self.label_planes`` the interpolated (delta_p, p) planes [2,Ny,Nx] float64 of every frame (None: irrelevant).
        ``fields=False``: a metrics-only sweep -- the chunks go through ``poisson_frames_errors``, which brings back the sums of the
        three error blocks and no field; the six lists and ``last_metrics`` are filled as above, the return is one
        ``{suffix: metrics}`` dict per frame ('' / '_deltap_crude' / '_p'; 0 for an irrelevant frame), and ``deltap_res``,
        ``cfd_results``, ``p_pred`` and ``label_planes`` are None.  The device takes nan0(label plane) as the delta-p truth where the
        host chain writes nan_to_num(x / U^2) / m * m * U^2: at most 4 ulp per element apart.
        ``device_prep=True``: the loop over ``times`` only slices the float32 rows; ``poisson_rows`` / ``poisson_rows_errors`` derive
        U_max_norm, the skip rule, the eight columns, (L, U) and the scale on the device (every frame keeps its slot in its call, an
        irrelevant one is read off the returned scalars), and everything returned and recorded holds the bits of the default mode."""
        from . import formats
        if getattr(self, "tables", None) is None:
            raise RuntimeError("computeOnlyOnce has not been called")
        times = [int(t) for t in times]
        if device_prep:
            return self._time_steps_rows(sim, times, apply_filter, phi, fields)
        out, cols, Us, slot = [0] * len(times), [], [], []
        self.label_planes = [None] * len(times)
        for i, time in enumerate(times):
            data, _, _ = formats.read_dataset(self.dataset_path, sim, time)
            d = data[0, 0, :self.indice]
            Ux, Uy, p = d[:, 0:1], d[:, 1:2], d[:, 2:3]
            delta_U, delta_p = d[:, 5:7], d[:, 7:8]
            delta_U_prev, delta_p_prev = d[:, 8:10], d[:, 10:11]
            deltaU_changed = np.abs(delta_U - delta_U_prev).sum(axis=-1)
            deltaU_changed = deltaU_changed / deltaU_changed.max()
            U_max_norm = np.max(np.sqrt(np.square(Ux) + np.square(Uy)))
            deltaU_max_norm = np.max(np.sqrt(np.square(delta_U[:, 0:1]) + np.square(delta_U[:, 1:2])))
            if (deltaU_max_norm / U_max_norm) < 1e-4 or deltaU_max_norm < 1e-6 or U_max_norm < 1e-6:      # :562-567
                continue
            cols.append(np.concatenate([Ux, Uy, delta_U, delta_p, p, deltaU_changed[:, None], delta_p_prev], axis=1).astype(np.float64))
            Us.append(float(U_max_norm))
            slot.append(i)
        if not cols:
            return out
        sur = self._surrogate(self.grid_shape_y, self.grid_shape_x)
        self._bind_frames(sur)
        sd = np.nan_to_num(self.sdfunct[..., 0], nan=0.0) / self.max_abs_dist
        for c0 in range(0, len(cols), self.max_frames):
            chunk, U_chunk = np.stack(cols[c0:c0 + self.max_frames]), Us[c0:c0 + self.max_frames]
            if not fields:
                raw = sur.poisson_frames_errors(chunk, [[phi, U] for U in U_chunk],
                                                out_scale=[self.max_abs_delta_p * U ** 2 for U in U_chunk], apply_filter=apply_filter)
                for j, U in enumerate(U_chunk):
                    self.U_max_norm = U
                    out[slot[c0 + j]] = {sfx: self._record_metrics(sur.metrics_from_sums(raw[j, q]), sfx, title)
                                         for q, (sfx, title) in enumerate(self.ERROR_BLOCKS)}
                continue
            res, _, nxt, extra = sur.poisson_frames(chunk, [[phi, U] for U in U_chunk],
                                                    out_scale=[self.max_abs_delta_p * U ** 2 for U in U_chunk],    # :816
                                                    apply_filter=apply_filter, weighting=True, want_extra=True)
            for j, U in enumerate(U_chunk):
                field_deltap = nxt[j]
                self.U_max_norm = U
                self.deltap_res = res[j, :, :, 0]
                delta_p_grid = np.nan_to_num(extra[j, 0] / pow(U, 2.0), nan=0.0) / self.max_abs_delta_p
                p_grid = np.nan_to_num(extra[j, 1], nan=0.0)
                self.cfd_results = delta_p_grid * self.max_abs_delta_p * pow(U, 2.0)
                self.no_flow_bool = sd == 0
                self.p_pred = (p_grid - self.cfd_results) + field_deltap
                self._record_errors(field_deltap, self.cfd_results, self.no_flow_bool, "", "Error in delta_p")
                self._record_errors(self.deltap_res, self.cfd_results, self.no_flow_bool, "_deltap_crude", "Error in delta_p - no weighting")
                self._record_errors(self.p_pred, p_grid, self.no_flow_bool, "_p", "Error in p")
                out[slot[c0 + j]], self.label_planes[slot[c0 + j]] = field_deltap, extra[j]
        if not fields:
            self.no_flow_bool = sd == 0
            self.deltap_res = self.cfd_results = self.p_pred = self.label_planes = None
        return out

    def _time_steps_rows(self, sim, times, apply_filter, phi, fields):
        """``timeSteps(device_prep=True)``: the dataset rows as stored go up, the device makes scalars and columns."""
        from . import formats
        out = [0] * len(times)
        self.label_planes = [None] * len(times)
        rows = [formats.read_dataset(self.dataset_path, sim, time)[0][0, 0, :self.indice] for time in times]
        if not rows:
            return out
        sur = self._surrogate(self.grid_shape_y, self.grid_shape_x)
        self._bind_frames(sur)
        if sur._rows_bound < rows[0].shape[1]:
            sur.bind_rows(rows[0].shape[1])
        chunks = [np.stack(rows[c0:c0 + self.max_frames]) for c0 in range(0, len(rows), self.max_frames)]
        if fields:
            calls = [sur.poisson_rows(chunk, self.max_abs_delta_p, phi, apply_filter=apply_filter, weighting=True, want_extra=True) for chunk in chunks]
        else:
            calls = [sur.poisson_rows_errors(chunk, self.max_abs_delta_p, phi, apply_filter=apply_filter) for chunk in chunks]
        if not any(call[-1][:, 3].any() for call in calls):
            return out
        sd = np.nan_to_num(self.sdfunct[..., 0], nan=0.0) / self.max_abs_dist
        for c, call in enumerate(calls):
            sc = call[-1]
            for j in range(sc.shape[0]):
                if sc[j, 3] == 0:                                                              # :562-567, decided on the device
                    continue
                i, U = c * self.max_frames + j, float(sc[j, 0])
                self.U_max_norm = U
                if not fields:
                    out[i] = {sfx: self._record_metrics(sur.metrics_from_sums(call[0][j, q]), sfx, title)
                              for q, (sfx, title) in enumerate(self.ERROR_BLOCKS)}
                    continue
                res, _, nxt, extra, _ = call
                field_deltap = nxt[j]
                self.deltap_res = res[j, :, :, 0]
                delta_p_grid = np.nan_to_num(extra[j, 0] / pow(U, 2.0), nan=0.0) / self.max_abs_delta_p
                p_grid = np.nan_to_num(extra[j, 1], nan=0.0)
                self.cfd_results = delta_p_grid * self.max_abs_delta_p * pow(U, 2.0)
                self.no_flow_bool = sd == 0
                self.p_pred = (p_grid - self.cfd_results) + field_deltap
                self._record_errors(field_deltap, self.cfd_results, self.no_flow_bool, "", "Error in delta_p")
                self._record_errors(self.deltap_res, self.cfd_results, self.no_flow_bool, "_deltap_crude", "Error in delta_p - no weighting")
                self._record_errors(self.p_pred, p_grid, self.no_flow_bool, "_p", "Error in p")
                out[i], self.label_planes[i] = field_deltap, extra[j]
        if not fields:
            self.no_flow_bool = sd == 0
            self.deltap_res = self.cfd_results = self.p_pred = self.label_planes = None
        return out

    def build_features(self, ux_grid, uy_grid, delta_ux_grid, delta_uy_grid, sdfunct, phi, U_max_norm) -> np.ndarray:
        """SM_call.py:588-711 (after the interpolation to the grid): -> grid [Ny,Nx,4] float32."""
        ny, nx = np.shape(ux_grid)
        sur = self._surrogate(ny, nx)
        return sur.poisson_features(ux_grid, uy_grid, delta_ux_grid, delta_uy_grid, sdfunct, phi, U_max_norm, self.k,
                                    (self.max_abs_Poisson_term_1, self.max_abs_delta_Ux, self.max_abs_delta_Uy,
                                     self.max_abs_dist))

    def timeStep_grid(self, ux_grid, uy_grid, delta_ux_grid, delta_uy_grid, sdfunct, phi, U_max_norm,
                      deltaU_change_grid=None, deltaP_prev_grid=None, apply_filter=False,
                      apply_deltaU_change_wgt=True) -> np.ndarray:
        """Grid-native body of ``timeStep`` (SM_call.py:588-848): features, surrogate, assembly, post-steps
        -> field_deltap [Ny,Nx] (``deltaP_prev_grid + change_in_deltap`` with the weighting, :843-848)."""
        grid = self.build_features(ux_grid, uy_grid, delta_ux_grid, delta_uy_grid, sdfunct, phi, U_max_norm)
        sur = self._surrogate(grid.shape[0], grid.shape[1])
        wgt = apply_deltaU_change_wgt and deltaU_change_grid is not None and deltaP_prev_grid is not None
        scale = [self.max_abs_delta_p * U_max_norm ** 2]                                          # :816
        if not (wgt or apply_filter):
            self.deltap_res = sur.solve(grid, out_scale=scale)[0, :, :, 0]
            return self.deltap_res
        # solve and post-steps (:352-363, :843-848) as one call: the field stays on the device between the stages
        if not sur._post_bound:
            sur.bind_poststeps((10, 10), (50, 50))                # SM_call.py:353, :360
        res, _, nxt = sur.solve_poststeps(grid, apply_filter, deltaU_change_grid if wgt else None,
                                          deltaP_prev_grid if wgt else None, out_scale=scale)
        self.deltap_res = res[0, :, :, 0]                        # the assembled delta-p before the weighting (:833)
        return nxt[0] if wgt else self.deltap_res


class EvaluationGradP(Evaluation):
    """``U_to_gradP`` ``Evaluation`` (Eval_dual_Dense_onlycil.py:30-66)."""
    variant = "gradp"

    def __init__(self, delta, shape, avance, var_p, var_in, hdf5_path, model_path, max_number_PC,
                 model: SurrogateModel = None, device: int = 0, artifact_dir: str = None, max_frames: int = None):
        super().__init__(delta, shape, avance, var_p, var_in, hdf5_path, model_path, max_number_PC,
                         model.scaler_kind if model is not None else "max_abs", model, device, artifact_dir, max_frames)
        self.avance = avance
        self.hdf5_path = hdf5_path

    def computeOnlyOnce(self, sim):
        """Eval_dual_Dense_onlycil.py:160-253: 2-digit bounds, box = the ``top`` patch, every 2nd boundary point,
        column 5 decides interpolability.  Returns 0."""
        from . import formats
        from .geometry import build_geometry_evaluator
        data, top_b, obst_b = formats.read_dataset(self.hdf5_path, sim, 0)
        self.indice = formats.first_index(data[0, 0, :, 0], formats.PAD_VALUE)
        cells = np.asarray(data[0, 0, :self.indice], np.float64)
        top32 = top_b[0, 0, :formats.first_index(top_b[0, 0, :, 0], formats.PAD_VALUE)]
        obst32 = obst_b[0, 0, :formats.first_index(obst_b[0, 0, :, 0], formats.PAD_VALUE)]
        t = build_geometry_evaluator(cells[:, 3:5], cells[:, 5], np.asarray(top32, np.float64), np.asarray(obst32, np.float64),
                                     self.delta, every=2, round_digits=2, box="top")
        # float32 like `np.max(top[:,0])` of the float32 file data (:192): used in float32 arithmetic by timeStep
        self.max_x, self.max_y = np.max(top32[:, 0]), np.max(top32[:, 1])
        self.min_x, self.min_y = np.min(top32[:, 0]), np.min(top32[:, 1])
        self.grid_shape_y, self.grid_shape_x = t.ny, t.nx
        self.vert, self.weights, self.indices, self.sdfunct = t.vtx_m2g, t.wts_m2g, t.indices, t.sdfunct[:, :, None]
        self.X0_min = t.x0
        sur = self._surrogate(t.ny, t.nx)
        v1, w1 = np.ascontiguousarray(t.vtx_m2g, np.int32), _f64(t.wts_m2g)
        idx, sdf = np.ascontiguousarray(t.indices, np.int32), _f64(t.sdfunct)
        mx = _f64(np.asarray(self.maxs, np.float64)[:4])
        sur._chk(sur.lib.psm_set_geometry(sur.h, int(self.indice), t.ny, t.nx, _p(v1, C.c_int32), _p(w1, C.c_double),
                                          _p(idx, C.c_int32), _p(sdf, C.c_double), None, None, _p(mx, C.c_double), 1, 1, 0.05))
        sur.mesh_cells = int(self.indice)
        sur._frames_bound = sur._feat_bound = sur._post_bound = sur._deltas_bound = sur._gradp_bound = False; sur._rows_bound = 0      # the new plan dropped them
        self.tables = t
        self._bind_simulation_geometry(sur, t.sdfunct, float(mx[2]))
        return 0

    def timeStep(self, sim, time, plot_intermediate_fields=False, save_plots=False, show_plots=False, apply_filter=False):
        """Eval_dual_Dense_onlycil.py:418-640 without plots and error prints: frame (sim, time) -> the integrated
        pressure image [Ny,Nx] (``field``).  Kept: ``self.grid`` (6 channels), ``self.gradP`` [Ny,Nx,2]."""
        from . import formats
        if getattr(self, "tables", None) is None:
            raise RuntimeError("computeOnlyOnce has not been called")
        data, _, _ = formats.read_dataset(self.hdf5_path, sim, time)
        d = data[0, 0, :self.indice]                                  # float32, normalised in float32 like the reference
        Ux, Uy, p, dPdx, dPdy = d[:, 0:1], d[:, 1:2], d[:, 2:3], d[:, 6:7], d[:, 7:8]
        U_max_norm = np.max(np.sqrt(np.square(Ux) + np.square(Uy)))                       # :438
        cols = np.concatenate([Ux / U_max_norm, Uy / U_max_norm,                        # :443-444
                               dPdx * (self.max_x - self.min_x) / pow(U_max_norm, 2.0),   # :440
                               dPdy * (self.max_y - self.min_y) / pow(U_max_norm, 2.0),   # :441
                               p / pow(U_max_norm, 2.0)], axis=1).astype(np.float64)      # :442
        g = self._mesh_to_grid(cols)
        mx = [float(v) for v in self.maxs[:5]]
        grid = np.zeros((self.grid_shape_y, self.grid_shape_x, 6))
        grid[..., 0:2] = g[..., 0:2]
        grid[..., 2] = self.sdfunct[..., 0]
        grid[..., 3:6] = g[..., 2:5]
        grid[np.isnan(grid)] = 0                                                          # :461
        for ch in range(5):
            grid[..., ch] /= mx[ch]                                                       # :463-467
        self.grid = grid
        self.U_max_norm = float(U_max_norm)
        sur = self._surrogate(*grid.shape[:2])
        if apply_filter:                                                                 # :470-544 and :366-367 (per field) in one call
            if not sur._post_bound:
                sur.bind_poststeps((10, 10), (50, 50))
            gradP = sur.solve_poststeps(grid[..., :3], apply_filter=True)[0][0]
        else:
            gradP = sur.solve(grid[..., :3])[0]                                           # :470-544
        self.gradP = gradP
        xl = np.linspace(self.min_x, self.max_x, grid.shape[1])                            # :591-592
        yl = np.linspace(self.min_y, self.max_y, grid.shape[0])
        solid = self.sdfunct[200, :, 0] == 0                                              # :594 (row 200 is hard-wired)
        center_p_x = int(((xl[solid].max() + xl[solid].min()) / 2 - self.X0_min) / self.delta)
        center_p_y = 200
        sur.set_integration(self.sdfunct[..., 0], center_p_y, center_p_x, float(np.diff(xl)[0]), float(np.diff(yl)[0]))
        self.center_p_x, self.center_p_y = center_p_x, center_p_y
        field = sur.integrate_gradp(gradP)                                                # :597-628
        # ---- error block of :667-687.  The reference takes its "true" values from grid channel 3 -- the normalised dP/dx
        # label, not the pressure of channel 5 that its plot shows (:644-650) -- and that is what it accumulates in
        # pred_minus_true / pred_minus_true_squared; reproduced as written, with the comparison against the pressure label
        # kept beside it (last_metrics['p']).
        no_flow = grid[..., 2] == 0
        self.no_flow_bool = no_flow
        self._record_errors(field, grid[..., 3], no_flow, "", "reference metric (grid channel 3)")
        self.last_metrics["reference"] = self.last_metrics.pop("delta_p")
        self.last_metrics["p"] = error_metrics(field, grid[..., 5], no_flow)
        return field

    FRAME_COLUMNS = 5               # Ux / U, Uy / U and the three label columns dPdx / U^2, dPdy / U^2, p / U^2

    def _integration_cut(self):
        """The cut and the spacings ``timeStep`` computes (Eval_dual_Dense_onlycil.py:591-600; row 200 is hard-wired): fixed for a
        simulation -> (center_p_y, center_p_x, dx, dy)."""
        xl = np.linspace(self.min_x, self.max_x, self.grid_shape_x)
        yl = np.linspace(self.min_y, self.max_y, self.grid_shape_y)
        solid = self.sdfunct[200, :, 0] == 0
        center_p_x = int(((xl[solid].max() + xl[solid].min()) / 2 - self.X0_min) / self.delta)
        return 200, center_p_x, float(np.diff(xl)[0]), float(np.diff(yl)[0])

    def _bind_frames(self, sur, apply_filter: bool):
        """What timeSteps needs on the handle, once per computeOnlyOnce (whose new plan drops them): the frame staging, the gradP
        binding with the simulation's SDF plane, scales and cut, and the post-steps when a filtered gradient is asked for."""
        if apply_filter and not sur._post_bound:
            sur.bind_poststeps((10, 10), (50, 50))
        if getattr(self, "_frames_tables", None) is self.tables and sur._frames_bound and sur._gradp_bound:
            return
        cy, cx, dx, dy = self._integration_cut()
        sur.bind_frames(self.max_frames, self.FRAME_COLUMNS)
        if not sur.bind_gradp_frames(self.sdfunct[..., 0], [float(v) for v in self.maxs[:5]], cy, cx, dx, dy):
            raise RuntimeError("the integration cannot process this geometry at the cut (the reference raises here too)")
        self._frames_tables = self.tables

    METRIC_ROWS = ("reference", "p", "dp_dx", "dp_dy")    # the rows of gradp_frames' raw sums

    def timeSteps(self, sim, times, apply_filter=False, fields=True, device_prep=False):
        """``timeStep`` for several frames of one simulation, sent ``max_frames`` at a time as ONE call each (``gradp_frames``: cell
        columns -> planes -> image, labels -> solve -> filter -> integration -> four error blocks on the device).  The per-frame
        host scalars and columns are those of ``timeStep``; ``pred_minus_true``, ``pred_minus_true_squared`` (the reference's own
        metric) and ``last_metrics`` -- keys ``reference`` and ``p`` as after ``timeStep``, plus ``dp_dx`` / ``dp_dy``: the assembled
        gradient components against their labels -- are filled in frame order.
        ``fields=True``: returns the list of p images; the first two metric blocks are taken from the images on the host like
        ``timeStep`` takes them, and ``gradP``, ``no_flow_bool``, ``U_max_norm``, ``center_p_x`` and ``center_p_y`` hold what
        ``timeStep`` leaves on the last frame (``grid`` is not produced).
        ``fields=False``: a metrics-only sweep -- nothing but the sums comes back (4 x 8 doubles per frame), the return is one dict
        of the four metric blocks per frame.
        Either way ``frame_metrics`` holds the call's four metric blocks per frame.
        ``device_prep=True``: the loop over ``times`` only slices the float32 rows; ``gradp_rows`` derives U_max_norm and the five
        columns on the device, and everything returned and recorded holds the bits of the default mode."""
        from . import formats
        if getattr(self, "tables", None) is None:
            raise RuntimeError("computeOnlyOnce has not been called")
        times = [int(t) for t in times]
        cols, Us = [], []
        for time in times:
            data, _, _ = formats.read_dataset(self.hdf5_path, sim, time)
            d = data[0, 0, :self.indice]                                  # float32, normalised in float32 like the reference
            if device_prep:
                cols.append(d)
                continue
            Ux, Uy, p, dPdx, dPdy = d[:, 0:1], d[:, 1:2], d[:, 2:3], d[:, 6:7], d[:, 7:8]
            U_max_norm = np.max(np.sqrt(np.square(Ux) + np.square(Uy)))                       # :438
            cols.append(np.concatenate([Ux / U_max_norm, Uy / U_max_norm,                   # :443-444
                                        dPdx * (self.max_x - self.min_x) / pow(U_max_norm, 2.0),   # :440
                                        dPdy * (self.max_y - self.min_y) / pow(U_max_norm, 2.0),   # :441
                                        p / pow(U_max_norm, 2.0)], axis=1).astype(np.float64))      # :442
            Us.append(U_max_norm)
        out, self.frame_metrics = [], []
        if not cols:
            return out
        sur = self._surrogate(self.grid_shape_y, self.grid_shape_x)
        self._bind_frames(sur, apply_filter)
        sd = np.nan_to_num(np.asarray(self.sdfunct[..., 0], np.float64), nan=0.0) / float(self.maxs[2])
        self.no_flow_bool = sd == 0
        self.center_p_y, self.center_p_x = self._integration_cut()[:2]
        if not isinstance(getattr(self, "last_metrics", None), dict):
            self.last_metrics = {}
        for c0 in range(0, len(cols), self.max_frames):
            chunk, U_chunk = np.stack(cols[c0:c0 + self.max_frames]), Us[c0:c0 + self.max_frames]
            if device_prep:
                if sur._rows_bound < chunk.shape[2]:
                    sur.bind_rows(chunk.shape[2])
                gradp, p, truth, raw, sc = sur.gradp_rows(chunk, float(self.max_x - self.min_x), float(self.max_y - self.min_y),
                                                          apply_filter=apply_filter, want_gradp=fields, want_p=fields, want_truth=fields)
                U_chunk = sc[:, 0]
            else:
                gradp, p, truth, raw = sur.gradp_frames(chunk, apply_filter=apply_filter, want_gradp=fields, want_p=fields, want_truth=fields)
            for j, U in enumerate(U_chunk):
                self.U_max_norm = float(U)
                m = {name: sur.metrics_from_sums(raw[j, r]) for r, name in enumerate(self.METRIC_ROWS)}
                if fields:
                    self.gradP = gradp[j]
                    m["reference"] = error_metrics(p[j], truth[j, 0], self.no_flow_bool)
                    m["p"] = error_metrics(p[j], truth[j, 2], self.no_flow_bool)
                self._record_metrics(m["reference"], "", "reference metric (grid channel 3)")
                self.last_metrics.pop("delta_p")
                self.last_metrics.update(m)
                self.frame_metrics.append(m)
                out.append(p[j] if fields else m)
        return out

    def timeStep_grid(self, grid: np.ndarray) -> np.ndarray:
        """Eval_dual_Dense_onlycil.py:470-547: -> [Ny,Nx,2] = (res_dPdx, res_dPdy)."""
        return self._surrogate(grid.shape[0], grid.shape[1]).solve(grid)[0]

    def assemble_prediction(self, field, array, indices_list, n_x, n_y, apply_filter, shape_x, shape_y):
        """Eval_dual_Dense_onlycil.py:255: one channel ('dp_dx' | 'dp_dy') of decoded blocks."""
        if field not in ("dp_dx", "dp_dy"):
            raise ValueError(field)
        blocks, nx_, ny_ = layout(self.variant, shape_y, shape_x, self.shape, self.avance)
        if (nx_, ny_) != (n_x, n_y) or len(indices_list) != len(blocks):
            raise ValueError("n_x / n_y / indices_list do not match this grid")
        sur = self._surrogate(shape_y, shape_x)
        grid = _grid_from_blocks(np.asarray(self.x_array, np.float32), blocks, shape_y, shape_x)
        a = np.asarray(array, np.float32)
        both = np.zeros(a.shape + (2,), np.float32)
        ch = 0 if field == "dp_dx" else 1
        both[..., ch] = a
        res = sur.reassemble(grid, both)[..., ch]
        if apply_filter:                                          # Eval_dual_Dense_onlycil.py:366-367 (returns the 2-D array)
            return sur.gaussian_filter(res, (10, 10))
        return res[None, :, :, None]


class SolverModule:
    """Chapter-5 ``python_module`` (python_module.py): ``init_func`` / ``py_func`` with the
    reference's signatures on one rank (the serial solver, singleCore/test_Case/python_module.py:
    139,199; in the parallel solver the mpi4py gather/scatter of python_module.py:179-185,258,511
    stays around these calls).  ``maxs`` = (max_abs_Ux, max_abs_Uy, max_abs_dist, max_abs_p) of
    the ``maxs`` file (python_module.py:106-109)."""

    def __init__(self, model: SurrogateModel, maxs=(1.0, 1.0, 1.0, 1.0), device: int = 0, delta: float = 5e-3,
                 geometry: str = "scipy"):
        """``geometry``: who builds init_func's tables -- 'scipy' (default in this Python mirror: the routines the reference
        itself calls, qhull Delaunay in both directions, so that the tables -- including qhull's arbitrary choice of diagonal
        in every cocircular lattice square of the grid -> mesh step -- are the reference's) or 'native' (the library's C++
        builder behind ``psm_init_geometry``, csrc/psm_geometry.cpp: what a C++ solver gets; no SciPy).  The two differ only
        where the reference's own result is an accident of qhull (include/psm.h): fixed lattice diagonals -- a second-order
        difference on smooth fields, O(1) per cell on the white-noise fields of randomly initialised test networks
        (tests/measure/mesh_native_vs_scipy.py) -- and the simplex used for lattice points outside the hull."""
        if geometry not in ("scipy", "native"):
            raise ValueError("geometry must be 'scipy' or 'native'")
        self.model, self.maxs, self.device, self.delta = model, tuple(float(v) for v in maxs), device, delta
        self.geometry = geometry
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
        idx, sdf, mx = np.ascontiguousarray(t.indices, np.int32), _f64(t.sdfunct), _f64(self.maxs)
        self._sur._chk(self._sur.lib.psm_set_geometry(
            self._sur.h, int(np.asarray(array).shape[0]), t.ny, t.nx, _p(v1, C.c_int32), _p(w1, C.c_double),
            _p(idx, C.c_int32), _p(sdf, C.c_double), _p(v2, C.c_int32), _p(w2, C.c_double), _p(mx, C.c_double),
            0, 0, 0.05))
        self.tables = t
        return 0

    def _init_func_native(self, array, top_boundary, obst_boundary):
        """psm_set_case + psm_init_geometry: the tables are built inside the library (csrc/psm_geometry.cpp)."""
        a, t, o = _f64(array), _f64(top_boundary), _f64(obst_boundary)
        lib = _lib.load()
        ny, nx = C.c_int32(), C.c_int32()
        if lib.psm_geometry_shape(_p(a, C.c_double), a.shape[0], self.delta, C.byref(ny), C.byref(nx), None):
            raise ValueError(lib.psm_geometry_last_error().decode())
        if self._sur is not None:
            self._sur.close()
        self._sur = GridSurrogate(self.model, ny.value, nx.value, 1, self.device)
        mx = _f64(self.maxs)
        self._sur._chk(lib.psm_set_case(self._sur.h, _p(mx, C.c_double), self.delta, 10, 0.05))
        self._sur._chk(lib.psm_init_geometry(self._sur.h, _p(a, C.c_double), a.shape[0], _p(t, C.c_double), t.shape[0],
                                             _p(o, C.c_double), o.shape[0], 0))
        self.tables = "native"
        return 0

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
        a = _f64(array_in)
        if a.ndim != 2 or a.shape[1] != 5:
            raise ValueError("array must be [N,5] = (Ux, Uy, Cx, Cy, p)")
        if out is None:
            out = np.empty(a.shape[0], np.float64)
        self._sur._chk(self._sur.lib.psm_solve_begin(self._sur.h, _p(a, C.c_double), a.shape[0], 0, _p(out, C.c_double)))
        self._inflight = (a, out)                       # keeps both arrays alive until the end call (set only once the step is in flight)

    def py_func_end(self) -> np.ndarray:
        self._sur._chk(self._sur.lib.psm_solve_end(self._sur.h))
        a, out = self._inflight
        self._inflight = None
        return out

    def py_func(self, array_in, placeholder=0, out: np.ndarray = None) -> np.ndarray:
        """python_module.py:249: cells [N,5] float64 -> p [N] float64."""
        if self.tables is None:
            raise RuntimeError("init_func has not been called")
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
    (``geometry.build_geometry`` per case, handed over with ``psm_set_geometry_cases``) -- see :class:`SolverModule`."""

    def __init__(self, model: SurrogateModel, maxs=(1.0, 1.0, 1.0, 1.0), max_cases: int = 8, geometry: str = "native",
                 device: int = 0, delta: float = 5e-3):
        if geometry not in ("scipy", "native"):
            raise ValueError("geometry must be 'scipy' or 'native'")
        self.model, self.maxs, self.max_cases = model, tuple(float(v) for v in maxs), int(max_cases)
        self.geometry, self.device, self.delta = geometry, device, delta
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
        mx = _f64(self.maxs)
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
        if self.geometry == "native":
            sur._chk(lib.psm_set_case(sur.h, _p(mx, C.c_double), self.delta, 10, 0.05))
            sur._chk(lib.psm_init_geometry_cases(sur.h, K, self._ptrs(a), n, self._ptrs(t), (C.c_int64 * K)(*[x.shape[0] for x in t]),
                                                 self._ptrs(o), (C.c_int64 * K)(*[x.shape[0] for x in o])))
        else:
            keep = [[np.ascontiguousarray(getattr(g, f), dt) for g in tables]
                    for f, dt in (("vtx_m2g", np.int32), ("wts_m2g", np.float64), ("indices", np.int32), ("sdfunct", np.float64),
                                  ("vtx_g2m", np.int32), ("wts_g2m", np.float64))]
            sur._chk(lib.psm_set_geometry_cases(sur.h, K, n, ny, nx, *[self._ptrs(col) for col in keep], _p(mx, C.c_double), 0, 0, 0.05))
        off = (C.c_int64 * (K + 1))()
        sur._chk(lib.psm_mesh_cases(sur.h, None, off))
        self.cell_off = [int(v) for v in off]
        self.tables = tables
        return 0

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
        cells, p = self._pack(arrays)
        self._sur._chk(self._sur.lib.psm_solve_cases_begin(self._sur.h, _p(cells, C.c_double), _p(p, C.c_double)))
        self._inflight = (cells, p)                     # keeps both arrays alive until the end call

    def py_func_end(self):
        self._sur._chk(self._sur.lib.psm_solve_cases_end(self._sur.h))
        cells, p = self._inflight
        self._inflight = None
        return self._split(p)

    def py_func(self, arrays):
        """One step of every case: list of cells [N_i,5] float64 -> list of p_i [N_i] float64."""
        cells, p = self._pack(arrays)
        self._sur._chk(self._sur.lib.psm_solve_cases(self._sur.h, _p(cells, C.c_double), _p(p, C.c_double)))
        return self._split(p)
