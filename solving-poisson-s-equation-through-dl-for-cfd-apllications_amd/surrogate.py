"""Host-side mirror of the C-ABI: ``GridSurrogate`` owns one ``psm_handle`` (include/psm.h) and hands NumPy buffers and device
pointers over to it; behind it the host-only layout helpers (``layout``, ``owner_map``, ``debug_reassemble_host``).

The operators with the reference's names on top of it live in two modules by seam and are re-exported here:

* ``evaluators.py`` -- the three dataset evaluators (``Evaluation``, ``EvaluationPoisson``, ``EvaluationGradP``), what they load
  and summarise (``load_artifacts``, ``error_metrics``, ``_summary``) and their mains,
* ``solver.py`` -- the Chapter-5 solver module (``SolverModule``, ``SolverEnsemble``).

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


def _opt(a, t=C.c_float):
    """``_p`` of an optional array: None stays None (a NULL pointer)."""
    return _p(a, t) if a is not None else None


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
        self._chk(self.lib.psm_solve_grid(self.h, _p(g, C.c_float), n, _opt(sc),
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
        self._chk(self.lib.psm_submit_grid_io(self.h, _p(g, C.c_float), n, _opt(sc),
                                              _opt(out), C.byref(t)))
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
        self._chk(self.lib.psm_ring_submit(self.h, ticket, n_cases, _opt(sc)))

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
                                                 _opt(sc),
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
                                                     _opt(sc),
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
        self._chk(self.lib.psm_solve_pressure(self.h, _p(g, C.c_float), n, _opt(sc),
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
                                                      _opt(sc), int(bool(apply_filter)),
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
        self._chk(self.lib.psm_solve_poststeps(self.h, _p(g, C.c_float), n, _opt(sc), int(bool(apply_filter)), _opt(dU), _opt(prev),
                                               _p(result, C.c_float), _opt(change), _opt(nxt)))
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
                                                   _opt(sc), int(bool(apply_filter)),
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
        self._chk(self.lib.psm_poisson_step(self.h, _p(v, C.c_double), n, _p(lu, C.c_double), _opt(sc), int(bool(apply_filter)),
                                            _opt(dU), _opt(prev), _p(result, C.c_float), _opt(change), _opt(nxt)))
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
        self._drop_mesh_bindings()
        self._chk(self.lib.psm_set_geometry(self.h, int(n_cells), self.ny, self.nx, _p(v, C.c_int32), _p(w, C.c_double),
                                            _p(idx, C.c_int32), _p(sdf, C.c_double), None, None, _p(mx, C.c_double), 1, 1, 0.05))
        self.mesh_cells = int(n_cells)

    # The mirrors of the library's bindings (``_*_bound``) are written by the bind / unbind methods and by these two alone.
    def _drop_frame_bindings(self):
        """What a new frame binding (or none) drops in the library: the frame staging and the four bindings made on top of it."""
        self._frames_bound = self._deltas_bound = self._gradp_bound = self._chapter4_bound = False
        self._rows_bound = 0

    def _drop_mesh_bindings(self):
        """What a new mesh drops: its new plan leaves no binding, the geometry's included."""
        self._drop_frame_bindings()
        self._feat_bound = self._post_bound = False
        self._bound_mask = self._bound_sdf = None

    def bind_frames(self, n_frames: int, k: int):
        """Staging for ``n_frames`` (<= max_cases) frames of ``k`` (<= 16) cell columns on the handle's mesh: after it a batch
        allocates nothing."""
        self._drop_frame_bindings()
        self._chk(self.lib.psm_bind_frames(self.h, int(n_frames), int(k)))
        self._frames_bound = True

    def unbind_frames(self):
        self._drop_frame_bindings()
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

    # -- what the host entries of the frame batches share: one marshaller per kind of argument
    def _host_batch(self, a, what: str, last: str, dtype, check):
        """A host entry's batch [n,n_cells,last] (or [n_cells,last]) on the handle's mesh -> (C-contiguous ``dtype`` array, n, last
        dimension, ``check(n, last dimension)``): the entry's own argument checks, made before the mesh is looked at."""
        v = np.asarray(a)
        if v.ndim == 2:
            v = v[None]
        if v.ndim != 3:
            raise ValueError(f"{what} must be [n,n_cells,{last}]")
        n, n_cells, k = v.shape
        checked = check(n, k)
        if self.mesh_cells is None:
            raise RuntimeError("the handle holds no mesh (set_mesh / computeOnlyOnce)")
        if n < 1 or n_cells != self.mesh_cells:
            raise ValueError(f"{what} must be [n >= 1, {self.mesh_cells} cells, {last}]")
        return np.ascontiguousarray(v, dtype), n, k, checked

    def _host_cols(self, cols, check):
        """``cols`` [n,n_cells,k] (or [n_cells,k]) -> (float64 array, n, k, ``check(n, k)``)."""
        return self._host_batch(cols, "cols", "k", np.float64, check)

    def _needs_post(self, apply_filter):
        if apply_filter and not getattr(self, "_post_bound", False):
            raise RuntimeError("apply_filter needs bind_poststeps")

    def _frame_scale(self, out_scale, n: int):
        if out_scale is None:
            return None
        if np.size(out_scale) not in (1, n):
            raise ValueError("out_scale must hold one value per frame")
        return _f32(np.broadcast_to(np.asarray(out_scale, np.float32).reshape(-1), (n,)))

    # One allocator per evaluator kind, shared by its frames and its rows entry: what is not wanted is None and is not copied back.
    def _poisson_out(self, n: int, weighting: bool, n_extra: int):
        """-> (result [n,Ny,Nx,c_out], change, next [n,Ny,Nx] float32, extra [n,n_extra,Ny,Nx] float64)."""
        result = np.empty((n, self.ny, self.nx, self.model.c_out), np.float32)
        change = nxt = None
        if weighting:
            change, nxt = np.empty((n, self.ny, self.nx), np.float32), np.empty((n, self.ny, self.nx), np.float32)
        return result, change, nxt, np.empty((n, n_extra, self.ny, self.nx), np.float64) if n_extra else None

    def _deltas_out(self, n: int, want_result: bool, want_truth: bool, want_raw: bool):
        """-> (result [n,Ny,Nx] float32, truth [n,Ny,Nx] float64, raw [n,2,8] float64)."""
        return (np.empty((n, self.ny, self.nx), np.float32) if want_result else None,
                np.empty((n, self.ny, self.nx), np.float64) if want_truth else None,
                np.empty((n, 2, len(self.RAW_SUMS)), np.float64) if want_raw else None)

    def _gradp_out(self, n: int, want_gradp: bool, want_p: bool, want_truth: bool):
        """-> (gradp [n,Ny,Nx,2], p [n,Ny,Nx] float32, truth [n,3,Ny,Nx], raw [n,4,8] float64)."""
        return (np.empty((n, self.ny, self.nx, 2), np.float32) if want_gradp else None,
                np.empty((n, self.ny, self.nx), np.float32) if want_p else None,
                np.empty((n, 3, self.ny, self.nx), np.float64) if want_truth else None,
                np.empty((n, 4, len(self.RAW_SUMS)), np.float64))

    def _chapter4_out(self, n: int, want_result: bool, want_truth: bool, want_raw: bool):
        """-> (result [n,Ny,Nx] float32, truth [n,Ny,Nx] float64, raw [n,1,8] float64)."""
        return (np.empty((n, self.ny, self.nx), np.float32) if want_result else None,
                np.empty((n, self.ny, self.nx), np.float64) if want_truth else None,
                np.empty((n, 1, len(self.RAW_SUMS)), np.float64) if want_raw else None)

    def _scalars(self, n: int):
        return np.empty((n, len(self.ROW_SCALARS)), np.float64)

    def poisson_frames_device(self, d_cols: int, n_frames: int, k: int, LU, d_result: int, apply_filter: bool = True,
                              weighting: bool = True, d_extra: int = 0, d_change: int = 0, d_next: int = 0, stream: int = 0,
                              out_scale: Optional[Sequence[float]] = None):
        """The Poisson evaluator's frames as one graph replay on raw device pointers: ``d_cols`` [n,n_cells,k] float64 with columns
        (Ux, Uy, dUx, dUy, extra..., [dU-change weight, delta_p_prev]) -> planes -> features -> solve -> post-steps -> result (and
        change / next) [n,Ny,Nx]; the extra columns' float64 planes go to ``d_extra`` [n,n_extra,Ny*Nx] (0: not stored)."""
        self._frame_columns(k, weighting)
        lu = self._lu(LU, n_frames)
        sc = self._frame_scale(out_scale, n_frames)
        self._chk(self.lib.psm_poisson_frames_device(self.h, C.c_void_p(d_cols), n_frames, k, _p(lu, C.c_double),
                                                     _opt(sc), int(bool(apply_filter)),
                                                     int(bool(weighting)), C.c_void_p(d_extra or None), C.c_void_p(d_result),
                                                     C.c_void_p(d_change or None), C.c_void_p(d_next or None), C.c_void_p(stream)))

    def poisson_frames(self, cols: np.ndarray, LU, out_scale: Optional[Sequence[float]] = None, apply_filter: bool = False,
                       weighting: bool = True, want_extra: bool = True):
        """Host buffers, synchronous: ``cols`` [n,n_cells,k] (or [n_cells,k]) float64 -> (result [n,Ny,Nx,c_out], change, next,
        extra); change and next [n,Ny,Nx] are None without the weighting, extra [n,n_extra,Ny,Nx] float64 (NaNs of
        interpolate_fill kept) is None without ``want_extra`` or without extra columns."""
        v, n, k, n_extra = self._host_cols(cols, lambda n, k: self._frame_columns(k, weighting))
        lu, sc = self._lu(LU, n), self._frame_scale(out_scale, n)
        result, change, nxt, extra = self._poisson_out(n, weighting, n_extra if want_extra else 0)
        self._chk(self.lib.psm_poisson_frames(self.h, _p(v, C.c_double), n, k, _p(lu, C.c_double), _opt(sc), int(bool(apply_filter)),
                                              int(bool(weighting)), _opt(extra, C.c_double), _p(result, C.c_float), _opt(change), _opt(nxt)))
        return result, change, nxt, extra

    # -- the Poisson-model step at the solver boundary (psm_solve_poisson*): cells [N,5] -> p [N], two-frame state on the device
    POISSON_SOLVE_SCALARS = ("U", "c", "U2", "out_scale", "skip", "frames", "_6", "_7")

    def bind_poisson_solve(self, phi: float, max_abs_delta_p: float, weighting: bool = True, apply_filter: bool = True):
        """The state (U, dU and p of the previous call per mesh cell), the partial maxima and the scalar slots of the Poisson solver
        step, behind ``bind_features``, ``bind_poststeps`` and ``bind_frames(n, k >= 6)`` on a mesh with both table sets: after it
        a step allocates nothing.  ``phi`` is the length scale L of the features, ``max_abs_delta_p`` the label scale."""
        self._chk(self.lib.psm_bind_poisson_solve(self.h, float(phi), float(max_abs_delta_p), int(bool(weighting)), int(bool(apply_filter))))

    def unbind_poisson_solve(self):
        self._chk(self.lib.psm_unbind_poisson_solve(self.h))

    def poisson_solve_push(self, cells: np.ndarray):
        """One frame [N,5] = (Ux, Uy, Cx, Cy, p) from the host into the state (a restart primes with two)."""
        a = self._solver_cells(cells)
        self._chk(self.lib.psm_poisson_solve_push(self.h, _p(a, C.c_double), a.shape[0]))

    def poisson_solve_reset(self):
        self._chk(self.lib.psm_poisson_solve_reset(self.h))

    @property
    def poisson_solve_state(self):
        """(frames held, steps taken) of psm_poisson_solve_state."""
        frames, steps = C.c_int32(), C.c_int64()
        self._chk(self.lib.psm_poisson_solve_state(self.h, C.byref(frames), C.byref(steps)))
        return int(frames.value), int(steps.value)

    @staticmethod
    def _solver_cells(cells):
        a = _f64(cells)
        if a.ndim != 2 or a.shape[1] != 5:
            raise ValueError("cells must be [N,5] = (Ux, Uy, Cx, Cy, p)")
        return a

    def _solver_step(self, entry, cells, out, cases: bool):
        """What the four host steps at the solver boundary share: the checks of cells and ``out``, of a case set's cell count, then
        ``entry`` on the single mesh (cells, N, rank 0, p) or on the case set (cells, p)."""
        a = self._solver_cells(cells)
        if out is None:
            out = np.empty(a.shape[0], np.float64)
        elif not isinstance(out, np.ndarray) or out.dtype != np.float64 or not out.flags.c_contiguous or out.shape != (a.shape[0],):
            raise ValueError(f"out must be a contiguous float64 array [{'sum N_i' if cases else 'N'}]")
        if cases:
            self._cases_count(a)
            self._chk(entry(self.h, _p(a, C.c_double), _p(out, C.c_double)))
        else:
            self._chk(entry(self.h, _p(a, C.c_double), a.shape[0], 0, _p(out, C.c_double)))
        return out

    def _solver_step_device(self, entry, d_cells, d_p, optional, stream):
        """The device form: cells and p, the entry's optional outputs (0: a null pointer), the stream."""
        self._chk(entry(self.h, C.c_void_p(d_cells), C.c_void_p(d_p), *[C.c_void_p(d or None) for d in optional], C.c_void_p(stream)))

    def solve_poisson(self, cells: np.ndarray, out: Optional[np.ndarray] = None) -> np.ndarray:
        """Host buffers, synchronous: cells [N,5] float64 = (Ux, Uy, Cx, Cy, p(t-1)) -> p [N] float64 = p(t-1) + dp; p(t-1) itself
        on a priming or skipped step and on the fallback cells."""
        return self._solver_step(self.lib.psm_solve_poisson, cells, out, False)

    def solve_poisson_device(self, d_cells: int, d_p: int, d_fields: int = 0, d_scalars: int = 0, stream: int = 0):
        """The same step on raw device pointers, asynchronous on ``stream``: ``d_cells`` [N,5] and ``d_p`` [N] float64;
        ``d_fields`` [3,Ny*Nx] float32 receives (result, change, next) and ``d_scalars`` [8] float64 ``POISSON_SOLVE_SCALARS``
        (0: the handle's own buffers)."""
        self._solver_step_device(self.lib.psm_solve_poisson_device, d_cells, d_p, (d_fields, d_scalars), stream)

    # -- the same step for the case set of psm_set_geometry_cases (psm_solve_cases_poisson*): cells [sum N_i,5] -> p [sum N_i]
    def bind_poisson_solve_cases(self, phi: float, max_abs_delta_p: float, weighting: bool = True, apply_filter: bool = True):
        """``bind_poisson_solve`` on a case set of K meshes under the four-channel model, behind ``bind_features`` (the K SDF planes
        in case order) and ``bind_poststeps``; no ``bind_frames``.  One state, one frame counter and one step counter for the set."""
        self._chk(self.lib.psm_bind_poisson_solve_cases(self.h, float(phi), float(max_abs_delta_p), int(bool(weighting)), int(bool(apply_filter))))

    def poisson_solve_push_cases(self, cells: np.ndarray):
        """One frame of every case, concatenated in case order [sum N_i,5], from the host into the state."""
        a = self._solver_cells(cells)
        self._cases_count(a)
        self._chk(self.lib.psm_poisson_solve_push_cases(self.h, _p(a, C.c_double)))

    def solve_cases_poisson(self, cells: np.ndarray, out: Optional[np.ndarray] = None) -> np.ndarray:
        """Host buffers, synchronous: the cases' cells concatenated in case order [sum N_i,5] float64 -> p [sum N_i] float64, per case
        what ``solve_poisson`` returns for a single mesh."""
        return self._solver_step(self.lib.psm_solve_cases_poisson, cells, out, True)

    def _cases_count(self, a):
        """The entries of a case set take no cell count, so the mirror checks it; without a case set the entry itself refuses."""
        total = self._cases_total()
        if total is not None and a.shape[0] != total:
            raise ValueError(f"cells must hold the {total} cells of the case set")

    def _cases_total(self):
        """sum N_i of the case set (psm_mesh_cases), None without one."""
        n = C.c_int32()
        if self.lib.psm_mesh_cases(self.h, C.byref(n), None):
            return None
        off = (C.c_int64 * (n.value + 1))()
        self._chk(self.lib.psm_mesh_cases(self.h, None, off))
        return int(off[n.value])

    def solve_cases_poisson_device(self, d_cells: int, d_p: int, d_fields: int = 0, d_scalars: int = 0, stream: int = 0):
        """The same step on raw device pointers, asynchronous on ``stream``: ``d_cells`` [sum N_i,5] and ``d_p`` [sum N_i] float64;
        ``d_fields`` [3,K,Ny*Nx] float32 receives (result, change, next) and ``d_scalars`` [K,8] float64 ``POISSON_SOLVE_SCALARS`` per
        case (0: the handle's own buffers)."""
        self._solver_step_device(self.lib.psm_solve_cases_poisson_device, d_cells, d_p, (d_fields, d_scalars), stream)

    # -- the gradient-model step at the solver boundary (psm_solve_gradp*): cells [N,5] -> p [N] through U -> grad p -> p, no state
    GRADP_SOLVE_SCALARS = ("U", "U2", "s", "sx", "sy", "_5", "_6", "_7")
    GRADP_REFERENCES = {"none": 0, "outlet": 1}

    def _gradp_solve_args(self, dx, dy, extents, max_abs_grad, apply_filter, reference):
        """What the two bind entries take alike behind their cut(s)."""
        if reference not in self.GRADP_REFERENCES:
            raise ValueError("reference must be 'none' or 'outlet'")
        ex, mg = _f64(extents).reshape(-1), _f64(max_abs_grad).reshape(-1)
        if ex.size != 2 or mg.size != 2:
            raise ValueError("extents = (extent_x, extent_y) and max_abs_grad = (max_abs_dPdx, max_abs_dPdy)")
        return float(dx), float(dy), float(ex[0]), float(ex[1]), _p(mg, C.c_double), int(bool(apply_filter)), self.GRADP_REFERENCES[reference]

    def bind_gradp_solve(self, cut, dx: float, dy: float, extents, max_abs_grad, apply_filter: bool = False, reference: str = "outlet"):
        """The integration tables (from the mesh's own sdfunct and ``cut`` = (center_y, center_x)), the planes and the scalar slots
        of the gradient solver step on a gradP handle with a single mesh (both table sets; with ``apply_filter`` behind
        ``bind_poststeps``): after it a step allocates nothing.  The integration's spacings are ``dx * max_abs_dPdx / extent_x`` and
        ``dy * max_abs_dPdy / extent_y``; ``reference``: 'outlet' (p = 0 at the outlet) or 'none'."""
        cy, cx = (int(v) for v in cut)
        self._chk(self.lib.psm_bind_gradp_solve(self.h, cy, cx, *self._gradp_solve_args(dx, dy, extents, max_abs_grad, apply_filter, reference)))

    def bind_gradp_solve_cases(self, cuts, dx: float, dy: float, extents, max_abs_grad, apply_filter: bool = False, reference: str = "outlet"):
        """``bind_gradp_solve`` on a case set of K meshes under the gradP model; ``cuts`` [K,2] = (center_y, center_x) in case order."""
        c = np.ascontiguousarray(cuts, np.int32).reshape(-1, 2)
        cy, cx = np.ascontiguousarray(c[:, 0]), np.ascontiguousarray(c[:, 1])
        total = C.c_int32()
        if self.lib.psm_mesh_cases(self.h, C.byref(total), None) == 0 and total.value != c.shape[0]:
            raise ValueError(f"cuts must hold one (center_y, center_x) for each of the {total.value} cases")
        self._chk(self.lib.psm_bind_gradp_solve_cases(self.h, _p(cy, C.c_int32), _p(cx, C.c_int32),
                                                      *self._gradp_solve_args(dx, dy, extents, max_abs_grad, apply_filter, reference)))

    def unbind_gradp_solve(self):
        self._chk(self.lib.psm_unbind_gradp_solve(self.h))

    def solve_gradp(self, cells: np.ndarray, out: Optional[np.ndarray] = None) -> np.ndarray:
        """Host buffers, synchronous: cells [N,5] float64 = (Ux, Uy, Cx, Cy, p(t-1)) -> p [N] float64; p(t-1) on the fallback cells."""
        return self._solver_step(self.lib.psm_solve_gradp, cells, out, False)

    def solve_gradp_device(self, d_cells: int, d_p: int, d_image: int = 0, d_gradp: int = 0, d_pgrid: int = 0, d_scalars: int = 0, stream: int = 0):
        """The same step on raw device pointers, asynchronous on ``stream``: ``d_cells`` [N,5] and ``d_p`` [N] float64; optional
        ``d_image`` [Ny,Nx,3], ``d_gradp`` [Ny,Nx,2] and ``d_pgrid`` [Ny,Nx] float32 receive the solved image, the gradient behind
        the filter and q = p / U^2 before the shift, ``d_scalars`` [8] float64 ``GRADP_SOLVE_SCALARS`` (0: the handle's own buffers)."""
        self._solver_step_device(self.lib.psm_solve_gradp_device, d_cells, d_p, (d_image, d_gradp, d_pgrid, d_scalars), stream)

    def solve_cases_gradp(self, cells: np.ndarray, out: Optional[np.ndarray] = None) -> np.ndarray:
        """Host buffers, synchronous: the cases' cells concatenated in case order [sum N_i,5] float64 -> p [sum N_i] float64, per case
        what ``solve_gradp`` returns for a single mesh."""
        return self._solver_step(self.lib.psm_solve_cases_gradp, cells, out, True)

    def solve_cases_gradp_device(self, d_cells: int, d_p: int, d_image: int = 0, d_gradp: int = 0, d_pgrid: int = 0, d_scalars: int = 0, stream: int = 0):
        """The same step on raw device pointers: ``d_cells`` [sum N_i,5], ``d_p`` [sum N_i]; the optional outputs per case:
        ``d_image`` [K,Ny,Nx,3], ``d_gradp`` [K,Ny,Nx,2], ``d_pgrid`` [K,Ny,Nx], ``d_scalars`` [K,8]."""
        self._solver_step_device(self.lib.psm_solve_cases_gradp_device, d_cells, d_p, (d_image, d_gradp, d_pgrid, d_scalars), stream)

    # -- the per-frame error blocks of assembled fields on the device: eight float64 sums per (frame, pair) instead of the fields
    RAW_SUMS =("n", "s1", "s2", "tmin", "tmax", "pmin", "pmax", "tnan")
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

    def _label_columns(self, k: int):
        if self._frame_columns(k, True) < 2:
            raise ValueError("the error blocks need the two label columns (delta_p, p): at least 8 columns")

    def poisson_frames_errors_device(self, d_cols: int, n_frames: int, k: int, LU, d_extra: int, d_result: int, d_next: int, d_raw: int,
                                     apply_filter: bool = True, d_change: int = 0, stream: int = 0,
                                     out_scale: Optional[Sequence[float]] = None):
        """``poisson_frames_device`` with the weighting (the same graph replay) and, behind it on the same stream, the evaluator's
        three error blocks of every frame: ``d_raw`` [n][3][8] float64 -- delta-p with the weighting, delta-p without it, p -- from
        next, result and the two label planes (columns 4 and 5) in ``d_extra``; the mask is the bound SDF plane."""
        self._label_columns(k)
        if not (d_extra and d_result and d_next):
            raise ValueError("the error blocks read d_extra, d_result and d_next: none of them may be 0")
        if not d_raw or int(d_raw) % 8:
            raise ValueError("d_raw must be an 8-byte aligned device pointer")
        lu = self._lu(LU, n_frames)
        sc = self._frame_scale(out_scale, n_frames)
        self._chk(self.lib.psm_poisson_frames_errors_device(self.h, C.c_void_p(d_cols), n_frames, k, _p(lu, C.c_double),
                                                            _opt(sc), int(bool(apply_filter)), 1,
                                                            C.c_void_p(d_extra), C.c_void_p(d_result), C.c_void_p(d_change or None),
                                                            C.c_void_p(d_next), C.c_void_p(d_raw), C.c_void_p(stream)))

    def poisson_frames_errors(self, cols: np.ndarray, LU, out_scale: Optional[Sequence[float]] = None,
                              apply_filter: bool = False) -> np.ndarray:
        """Host buffers, synchronous: ``cols`` [n,n_cells,k >= 8] (or [n_cells,k]) float64 -> raw [n,3,8] float64, the sums of
        the three error blocks per frame (``metrics_from_sums`` turns a row into the metrics).  Nothing else comes back: the
        fields and label planes stay on the device."""
        v, n, k, _ = self._host_cols(cols, lambda n, k: self._label_columns(k))
        lu, sc = self._lu(LU, n), self._frame_scale(out_scale, n)
        raw = np.empty((n, 3, len(self.RAW_SUMS)), np.float64)
        self._chk(self.lib.psm_poisson_frames_errors(self.h, _p(v, C.c_double), n, k, _p(lu, C.c_double), _opt(sc), int(bool(apply_filter)), 1,
                                                     _p(raw, C.c_double)))
        return raw

    # -- what the three evaluator frame batches below share: the checks of a bind and of a call, before any library call
    _EVAL_COLUMNS = {   # kind -> (fewest columns (0: the model's c_in), the message of a k outside the range)
        "deltas": (3, "frames take 3..16 columns: (dUx / U, dUy / U, dp / U^2), further columns are not stored"),
        "gradp": (5, "frames take 5..16 columns: (Ux / U, Uy / U, dPdx / U^2, dPdy / U^2, p / U^2), further columns are not stored"),
        "chapter4": (0, "frames take c_in..16 columns: the c_in - 1 input channels, then p / U^2; further columns are not stored")}

    def _bind_eval_frames(self, model_ok: bool, model_msg: str, sdfunct, max_abs, n_scales: int, scales_msg: str):
        """The argument checks the three ``bind_*_frames`` share -> (sdfunct, max_abs) as float64 arrays."""
        if not model_ok:
            raise ValueError(model_msg)
        if not getattr(self, "_frames_bound", False):
            raise RuntimeError("bind_frames has not been called")
        sdf = _f64(sdfunct)
        if sdf.size != self.ny * self.nx:
            raise ValueError(f"sdfunct must be [{self.ny},{self.nx}]")
        mx = _f64(np.asarray(max_abs, np.float64).reshape(-1))
        if mx.size != n_scales or not np.all(np.isfinite(mx)) or np.any(mx == 0):
            raise ValueError(f"max_abs must hold {scales_msg}")
        return sdf, mx

    def _eval_call(self, kind: str, n_frames, k):
        """The argument checks the frame entries of the three evaluators share."""
        k_min, k_msg = self._EVAL_COLUMNS[kind]
        if not getattr(self, f"_{kind}_bound"):
            raise RuntimeError(f"bind_{kind}_frames has not been called (bind_frames and a new mesh drop the binding)")
        if not (k_min or self.model.c_in) <= int(k) <= 16:
            raise ValueError(k_msg)
        if not 1 <= int(n_frames) <= self.max_cases:
            raise ValueError("n_frames outside [1, max_cases]")

    # -- the frame batch of the pressureSM_deltas evaluator on the device: columns -> image, label, truth -> solve -> two error blocks
    _deltas_bound = False

    def bind_deltas_frames(self, sdfunct, max_abs):
        """After ``bind_frames``, on a three-channel model with the SDF last and a one-channel field: the simulation's raw SDF plane
        ``sdfunct`` [Ny,Nx] float64 (NaNs allowed) and ``max_abs`` = (max_abs_Ux, max_abs_Uy, max_abs_dist, max_abs_p), each finite
        and non-zero.  Reserves everything a step touches for the frame count bound with ``bind_frames``."""
        m = self.model
        sdf, mx = self._bind_eval_frames(
            m.c_in == 3 and m.sdf_ch == 2 and m.c_out == 1, "the deltas frames take a model with 3 input channels, the SDF in channel 2, and 1 output channel",
            sdfunct, max_abs, 4, "four finite non-zero scales: (max_abs_Ux, max_abs_Uy, max_abs_dist, max_abs_p)")
        self._deltas_bound = False
        self._chk(self.lib.psm_bind_deltas_frames(self.h, _p(sdf, C.c_double), _p(mx, C.c_double)))
        self._deltas_bound = True

    def unbind_deltas_frames(self):
        self._deltas_bound = False
        self._chk(self.lib.psm_unbind_deltas_frames(self.h))

    def _deltas_call(self, n_frames, k, U2, need_u2: bool = True):
        """The argument checks the deltas frame entries share -> U2 as a float64 array (None where it is optional and absent)."""
        self._eval_call("deltas", n_frames, k)
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

    def deltas_image_device(self, d_cols: int, n_frames: int, k: int, U2, d_grid: int, d_label: int = 0, d_truth: int = 0, stream: int = 0):
        """The image stage alone on raw device pointers, asynchronous on ``stream``: ``d_cols`` [n,n_cells,k] float64 -> ``d_grid``
        [n,Ny,Nx,3] float32, ``d_label`` [n,Ny*Nx] float32 and ``d_truth`` [n,Ny*Nx] float64 (0: not stored), bit for bit the host
        statements of ``Evaluation.timeStep``.  ``U2`` [n]: U_max_norm^2 per frame (None without ``d_truth``)."""
        u2 = self._deltas_call(n_frames, k, U2, need_u2=bool(d_truth))
        d_cols = self._dev_ptr(d_cols, 8, "d_cols")
        d_grid, d_label = self._dev_ptr(d_grid, 4, "d_grid"), self._dev_ptr(d_label, 4, "d_label", True)
        d_truth = self._dev_ptr(d_truth, 8, "d_truth", True)
        self._chk(self.lib.psm_deltas_image_device(self.h, C.c_void_p(d_cols), int(n_frames), int(k), _opt(u2, C.c_double),
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
        self._needs_post(apply_filter)
        d_cols = self._dev_ptr(d_cols, 8, "d_cols")
        d_result, d_truth = self._dev_ptr(d_result, 4, "d_result", True), self._dev_ptr(d_truth, 8, "d_truth", True)
        d_raw = self._dev_ptr(d_raw, 8, "d_raw", True)
        sc = self._frame_scale(out_scale, int(n_frames))
        self._chk(self.lib.psm_deltas_frames_device(self.h, C.c_void_p(d_cols), int(n_frames), int(k), _p(u2, C.c_double),
                                                    _opt(sc), int(bool(apply_filter)),
                                                    C.c_void_p(d_result or None), C.c_void_p(d_truth or None), C.c_void_p(d_raw or None),
                                                    C.c_void_p(stream)))

    def deltas_frames(self, cols: np.ndarray, U2, out_scale: Optional[Sequence[float]] = None, apply_filter: bool = False,
                      want_result: bool = True, want_truth: bool = True, want_raw: bool = True):
        """Host buffers, synchronous: ``cols`` [n,n_cells,k] (or [n_cells,k]) float64 -> (result [n,Ny,Nx] float32, truth [n,Ny,Nx]
        float64, raw [n,2,8] float64); what is not wanted is None and is not copied back -- a metrics-only sweep
        (``want_result = want_truth = False``) brings back 16 doubles per frame."""
        v, n, k, u2 = self._host_cols(cols, lambda n, k: self._deltas_call(n, k, U2))
        if not (want_result or want_truth or want_raw):
            raise ValueError("nothing to return")
        self._needs_post(apply_filter)
        sc = self._frame_scale(out_scale, n)
        result, truth, raw = self._deltas_out(n, want_result, want_truth, want_raw)
        self._chk(self.lib.psm_deltas_frames(self.h, _p(v, C.c_double), n, k, _p(u2, C.c_double), _opt(sc), int(bool(apply_filter)),
                                             _opt(result), _opt(truth, C.c_double), _opt(raw, C.c_double)))
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
        sdf, mx = self._bind_eval_frames(
            m.c_in == 3 and m.sdf_ch == 2 and m.c_out == 2, "the gradP frames take a model with 3 input channels, the SDF in channel 2, and 2 output channels",
            sdfunct, max_abs, 5, "five finite non-zero scales: those of grid channels 0-4")
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

    def gradp_image_device(self, d_cols: int, n_frames: int, k: int, d_grid: int, d_truth: int = 0, stream: int = 0):
        """The image stage alone on raw device pointers, asynchronous on ``stream``: ``d_cols`` [n,n_cells,k] float64 -> ``d_grid``
        [n,Ny,Nx,3] float32 and ``d_truth`` [n,3,Ny*Nx] float64 (grid channels 3-5; 0: not stored), bit for bit the host statements
        of ``EvaluationGradP.timeStep``."""
        self._eval_call("gradp", n_frames, k)
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
        self._eval_call("gradp", n_frames, k)
        self._needs_post(apply_filter)
        d_cols = self._dev_ptr(d_cols, 8, "d_cols")
        d_gradp, d_p = self._dev_ptr(d_gradp, 8, "d_gradp", True), self._dev_ptr(d_p, 4, "d_p", True)
        d_truth, d_raw = self._dev_ptr(d_truth, 8, "d_truth", True), self._dev_ptr(d_raw, 8, "d_raw", True)
        sc = self._frame_scale(out_scale, int(n_frames))
        self._chk(self.lib.psm_gradp_frames_device(self.h, C.c_void_p(d_cols), int(n_frames), int(k),
                                                   _opt(sc), int(bool(apply_filter)),
                                                   C.c_void_p(d_gradp or None), C.c_void_p(d_p or None), C.c_void_p(d_truth or None),
                                                   C.c_void_p(d_raw or None), C.c_void_p(stream)))

    def gradp_frames(self, cols: np.ndarray, out_scale: Optional[Sequence[float]] = None, apply_filter: bool = False,
                     want_gradp: bool = True, want_p: bool = True, want_truth: bool = True):
        """Host buffers, synchronous: ``cols`` [n,n_cells,k] (or [n_cells,k]) float64 -> (gradp [n,Ny,Nx,2] float32, p [n,Ny,Nx]
        float32, truth [n,3,Ny,Nx] float64, raw [n,4,8] float64); what is not wanted is None and is not copied back -- a
        metrics-only sweep (``want_gradp = want_p = want_truth = False``) brings back 32 doubles per frame."""
        v, n, k, _ = self._host_cols(cols, lambda n, k: self._eval_call("gradp", n, k))
        self._needs_post(apply_filter)
        sc = self._frame_scale(out_scale, n)
        gradp, p, truth, raw = self._gradp_out(n, want_gradp, want_p, want_truth)
        self._chk(self.lib.psm_gradp_frames(self.h, _p(v, C.c_double), n, k, _opt(sc), int(bool(apply_filter)),
                                            _opt(gradp), _opt(p), _opt(truth, C.c_double), _p(raw, C.c_double)))
        return gradp, p, truth, raw

    # -- the frame batch of the two Chapter-4 evaluators on the device: columns -> image, truth -> solve -> one error block
    _chapter4_bound = False

    def bind_chapter4_frames(self, sdfunct, max_abs):
        """After ``bind_frames``, on a chapter5-variant model with 2 or 3 input channels, the SDF last, and a one-channel field: the
        simulation's raw SDF plane ``sdfunct`` [Ny,Nx] float64 (0 in solids, NaNs allowed) and ``max_abs`` [c_in + 1] = the scales of
        the c_in - 1 input channels, of the distance and of p, each finite and non-zero (M_u: max_abs_Ux, max_abs_Uy, max_abs_dist,
        max_abs_p; M_fU: max_abs_fU, max_abs_dist, max_abs_p).  Reserves everything a step touches for the frame count bound with
        ``bind_frames``."""
        m = self.model
        sdf, mx = self._bind_eval_frames(
            m.variant == "chapter5" and m.c_in in (2, 3) and m.sdf_ch == m.c_in - 1 and m.c_out == 1,
            "the Chapter-4 frames take a chapter5-variant model with 2 or 3 input channels, the SDF in the last one, and 1 output channel",
            sdfunct, max_abs, m.c_in + 1, "c_in + 1 finite non-zero scales: the c_in - 1 input channels, dist, p")
        self._chapter4_bound = False
        self._chk(self.lib.psm_bind_chapter4_frames(self.h, _p(sdf, C.c_double), _p(mx, C.c_double)))
        self._chapter4_bound = True

    def unbind_chapter4_frames(self):
        self._chapter4_bound = False
        self._chk(self.lib.psm_unbind_chapter4_frames(self.h))

    def chapter4_image_device(self, d_cols: int, n_frames: int, k: int, d_grid: int, d_truth: int = 0, stream: int = 0):
        """The image stage alone on raw device pointers, asynchronous on ``stream``: ``d_cols`` [n,n_cells,k] float64 -> ``d_grid``
        [n,Ny,Nx,c_in] float32 and ``d_truth`` [n,Ny*Nx] float64 (the normalised pressure label; 0: not stored), bit for bit the
        host statements of ``EvaluationChapter4.timeStep``."""
        self._eval_call("chapter4", n_frames, k)
        d_cols = self._dev_ptr(d_cols, 8, "d_cols")
        d_grid, d_truth = self._dev_ptr(d_grid, 4, "d_grid"), self._dev_ptr(d_truth, 8, "d_truth", True)
        self._chk(self.lib.psm_chapter4_image_device(self.h, C.c_void_p(d_cols), int(n_frames), int(k), C.c_void_p(d_grid),
                                                     C.c_void_p(d_truth or None), C.c_void_p(stream)))

    def chapter4_frames_device(self, d_cols: int, n_frames: int, k: int, d_result: int = 0, d_truth: int = 0, d_raw: int = 0,
                               stream: int = 0):
        """The Chapter-4 evaluators' frames as one graph replay on raw device pointers: ``d_cols`` [n,n_cells,k] float64 -> planes
        -> image, truth -> one single-case solve per frame -> ``d_result`` [n,Ny*Nx] float32, ``d_truth`` [n,Ny*Nx] float64 (0: the
        binding's buffers); with ``d_raw`` [n,1,8] float64 the error block behind it: the field against the truth, both normalised."""
        self._eval_call("chapter4", n_frames, k)
        d_cols = self._dev_ptr(d_cols, 8, "d_cols")
        d_result, d_truth = self._dev_ptr(d_result, 4, "d_result", True), self._dev_ptr(d_truth, 8, "d_truth", True)
        d_raw = self._dev_ptr(d_raw, 8, "d_raw", True)
        self._chk(self.lib.psm_chapter4_frames_device(self.h, C.c_void_p(d_cols), int(n_frames), int(k), C.c_void_p(d_result or None),
                                                      C.c_void_p(d_truth or None), C.c_void_p(d_raw or None), C.c_void_p(stream)))

    def chapter4_frames(self, cols: np.ndarray, want_result: bool = True, want_truth: bool = True, want_raw: bool = True):
        """Host buffers, synchronous: ``cols`` [n,n_cells,k] (or [n_cells,k]) float64 -> (result [n,Ny,Nx] float32, truth [n,Ny,Nx]
        float64, raw [n,1,8] float64); what is not wanted is None and is not copied back -- a metrics-only sweep
        (``want_result = want_truth = False``) brings back 8 doubles per frame."""
        v, n, k, _ = self._host_cols(cols, lambda n, k: self._eval_call("chapter4", n, k))
        if not (want_result or want_truth or want_raw):
            raise ValueError("nothing to return")
        result, truth, raw = self._chapter4_out(n, want_result, want_truth, want_raw)
        self._chk(self.lib.psm_chapter4_frames(self.h, _p(v, C.c_double), n, k, _opt(result), _opt(truth, C.c_double), _opt(raw, C.c_double)))
        return result, truth, raw

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
        v, n, width, _ = self._host_batch(rows, "rows", "width", np.float32, lambda n, width: self._rows_call(kind, n, width, base))
        if width > self._rows_bound:
            raise ValueError("wider rows than bind_rows reserved staging for")
        return v, n, width

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
        self._needs_post(apply_filter)
        (result, truth, raw), scalars = self._deltas_out(n, want_result, want_truth, want_raw), self._scalars(n)
        self._chk(self.lib.psm_deltas_rows(self.h, _p(v, C.c_float), n, width, float(base), int(bool(apply_filter)), _opt(result),
                                           _opt(truth, C.c_double), _opt(raw, C.c_double), _p(scalars, C.c_double)))
        return result, truth, raw, scalars

    def poisson_rows(self, rows: np.ndarray, base: float, phi: float = 1.0, apply_filter: bool = False, weighting: bool = True,
                     want_extra: bool = True):
        """``poisson_frames`` on the dataset rows themselves: ``rows`` [n,n_cells,width >= 11] float32 -> (result, change, next,
        extra, scalars [n,8]); the eight columns, (L, U) = (``phi``, U) and the out-scale ``base`` * U^2 are made on the device."""
        v, n, width = self._host_rows("poisson", rows, base)
        result, change, nxt, extra = self._poisson_out(n, weighting, (2 if weighting else 4) if want_extra else 0)
        scalars = self._scalars(n)
        self._chk(self.lib.psm_poisson_rows(self.h, _p(v, C.c_float), n, width, float(base), float(phi), int(bool(apply_filter)),
                                            int(bool(weighting)), _opt(extra, C.c_double), _p(result, C.c_float), _opt(change),
                                            _opt(nxt), _p(scalars, C.c_double)))
        return result, change, nxt, extra, scalars

    def poisson_rows_errors(self, rows: np.ndarray, base: float, phi: float = 1.0, apply_filter: bool = False):
        """``poisson_frames_errors`` on the dataset rows themselves -> (raw [n,3,8], scalars [n,8]): nothing else comes back."""
        v, n, width = self._host_rows("poisson", rows, base)
        raw, scalars = np.empty((n, 3, len(self.RAW_SUMS)), np.float64), self._scalars(n)
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
        self._needs_post(apply_filter)
        (gradp, p, truth, raw), scalars = self._gradp_out(n, want_gradp, want_p, want_truth), self._scalars(n)
        self._chk(self.lib.psm_gradp_rows(self.h, _p(v, C.c_float), n, width, float(ex), float(ey), int(bool(apply_filter)),
                                          _opt(gradp), _opt(p), _opt(truth, C.c_double), _p(raw, C.c_double),
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

    # -- input trust: the per-block PCA reconstruction residual of the last solve (include/psm.h, psm_bind_trust)
    def bind_trust(self):
        """psm_bind_trust with the model's input basis: once per surrogate; after it :meth:`trust_last` allocates nothing."""
        ci = _f64(self.model.comp_in)
        self._chk(self.lib.psm_bind_trust(self.h, _p(ci, C.c_double)))

    def unbind_trust(self):
        self._chk(self.lib.psm_unbind_trust(self.h))

    def trust_last(self) -> dict:
        """The score of the image the last solve ran on: ``n`` = |x - mean|^2 and ``spe`` = |x - mean - C^T z|^2 per block, float64
        ``[n_cases, B]``, and ``explained`` = 1 - spe / n, the share the retained components represent (comparable with the var_in
        the model was trained to; NaN where n == 0).  An evaluator's frame step leaves its last frame: n_cases = 1."""
        out = np.empty((self.max_cases, self.B, 2), np.float64)
        n = C.c_int32()
        self._chk(self.lib.psm_trust_last(self.h, C.byref(n), _p(out, C.c_double), out.size))
        out = out[:n.value]
        nn, spe = out[..., 0].copy(), out[..., 1].copy()
        with np.errstate(invalid="ignore", divide="ignore"):
            explained = 1.0 - spe / nn
        return {"n": nn, "spe": spe, "explained": explained}

    def trust_last_device(self, d_out: int, stream: int = 0):
        """psm_trust_last_device: two asynchronous launches on ``stream`` (0: the handle's); ``d_out`` [n_cases, B, 2] float64 in
        device memory, (n, spe) per block row."""
        self._chk(self.lib.psm_trust_last_device(self.h, C.c_void_p(self._dev_ptr(d_out, 8, "d_out")), C.c_void_p(stream)))

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


# the reference-shaped operators, one module per seam; imported last: both modules take GridSurrogate and the helpers from here
from .evaluators import (Evaluation, EvaluationChapter4, EvaluationGradP, EvaluationPoisson, _summary, call_SM_main,  # noqa: E402,F401
                         call_SM_main_Poisson, error_metrics, load_artifacts, main_chapter4, main_gradP)
from .solver import SolverEnsemble, SolverModule  # noqa: E402,F401
