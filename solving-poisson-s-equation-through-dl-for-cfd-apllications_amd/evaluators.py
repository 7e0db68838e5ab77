"""The three dataset evaluators of the reference on top of ``GridSurrogate``, with the names, argument order and meaning of its
operators, what they load and summarise, and their mains:

* ``Evaluation`` -- ``pressureSM_deltas.SM_call.Evaluation``: ``assemble_prediction`` (SM_call.py:182), ``timeStep`` (:367-575),
* ``EvaluationPoisson`` -- ``pressureSM_Poisson.SM_call.Evaluation`` (pressureSM_Poisson/SM_call.py:71-118, :519-848),
* ``EvaluationGradP`` -- the ``U_to_gradP`` ``Evaluation``: ``assemble_prediction`` (Eval_dual_Dense_onlycil.py:255), ``timeStep`` (:418-640).

``timeSteps`` sends several frames of a simulation per call.  The loop is ``Evaluation._time_steps`` for all three; an evaluator
states its own part once each: the per-frame scalars and columns (``_frame_prepare``, which ``timeStep`` uses too), the device call
on prepared columns (``_host_call``) and on the dataset rows (``_rows_call``), and the bookkeeping of one frame (``_record_frame``),
which every combination of ``fields`` and ``device_prep`` goes through.  ``surrogate.py`` re-exports the names of this module."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .surrogate import GridSurrogate, _f64, _p, layout
from .synthetic import SurrogateModel


def _grid_from_blocks(x_array: np.ndarray, blocks: np.ndarray, ny: int, nx: int) -> np.ndarray:
    """Rebuild the grid image from the overlapping input blocks (the reference keeps
    only ``self.x_array`` around when it calls ``assemble_prediction``)."""
    S = x_array.shape[1]
    g = np.zeros((ny, nx, x_array.shape[3]), np.float32)
    for b, (y0, x0, _, _) in enumerate(blocks):
        g[y0:y0 + S, x0:x0 + S] = x_array[b]
    return g


def load_artifacts(variant, model_path, directory, var_p, var_in, max_num_PC, standardization_method, shape, overlap,
                   c_in: int = 3, sdf_ch: int = 2, pca_stems=("ipca_input", "ipca_p"), pc_rule=None):
    """What the reference's ``Evaluation.__init__`` loads (SM_call.py:70-87; Eval_dual_Dense_onlycil.py:51-66):
    ``maxs`` (+ ``maxs_PCA`` for 'max_abs'), the Keras network of ``model_path`` (Dense stack, HDF5), the two
    pickled PCA objects (``ipca_input``, ``ipca_p``: ``.pkl`` like the reference or the ``.npz`` export) with the
    component-count rule of :86-87, and the scaler file of the chosen standardisation (:507-519).
    ``pca_stems``: the file stems of the input and the output PCA; ``pc_rule(explained_variance_ratio, var, side)`` with side 'in' /
    'p': another component-count rule (the Chapter-4 evaluators: ``ipca_*_more``, ``formats.select_num_pc_chapter4``).
    -> (SurrogateModel, maxs)."""
    from . import formats
    maxs = formats.read_maxs(os.path.join(directory, "maxs"))
    convs, weights = formats.read_keras_conv1d_head(model_path)     # Dense stack, or the conv1D_PCA head (NNs.py:75-124)
    attention = formats.read_keras_attention(model_path)            # densePCA_attention (NNs.py:40-72), else None
    pin = formats.load_pca(formats.find_pca(directory, pca_stems[0]))
    pout = formats.load_pca(formats.find_pca(directory, pca_stems[1]))
    if pc_rule is None:
        pc_rule = lambda evr, var, side: formats.select_num_pc(evr, var, max_num_PC)
    pc_p = pc_rule(pout.explained_variance_ratio_, var_p, "p")
    pc_in = pc_rule(pin.explained_variance_ratio_, var_in, "in")
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
        SDF image, index map; handed to the GPU library (``GridSurrogate.set_mesh``).  Returns 0."""
        from . import formats
        from .geometry import build_geometry_evaluator
        data, top_b, obst_b = formats.read_dataset(self.dataset_path, sim, 0)
        self.indice = formats.first_index(data[0, 0, :, 0], formats.PAD_VALUE)
        cells = np.asarray(data[0, 0, :self.indice], np.float64)
        top = np.asarray(top_b[0, 0, :formats.first_index(top_b[0, 0, :, 0], formats.PAD_VALUE)], np.float64)
        obst = np.asarray(obst_b[0, 0, :formats.first_index(obst_b[0, 0, :, 0], formats.PAD_VALUE)], np.float64)
        return self._set_tables(build_geometry_evaluator(cells[:, 3:5], cells[:, 2], top, obst, self.delta, idw_fallback=True))   # utils.interp_weights

    def _set_tables(self, t):
        """The tail of computeOnlyOnce: the tables of the simulation's mesh go to the handle (a new mesh drops every binding made
        before it) and the simulation's obstacle is bound.  Returns 0."""
        self.grid_shape_y, self.grid_shape_x = t.ny, t.nx
        self.vert, self.weights, self.indices, self.sdfunct = t.vtx_m2g, t.wts_m2g, t.indices, t.sdfunct[:, :, None]
        sur = self._surrogate(t.ny, t.nx)
        mx = self._mesh_maxs()
        sur.set_mesh(t.vtx_m2g, t.wts_m2g, t.indices, t.sdfunct, self.indice, mx)
        self.tables = t
        self._bind_simulation_geometry(sur, t.sdfunct, float(mx[2]))
        return 0

    def _mesh_maxs(self) -> np.ndarray:
        """The four scales the mesh takes: (max_abs_Ux, max_abs_Uy, max_abs_dist, max_abs_p)."""
        return np.asarray(self.maxs if self.maxs is not None else (1.0, 1.0, 1.0, 1.0), np.float64)[:4]

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
        if getattr(self, "tables", None) is None:
            raise RuntimeError("computeOnlyOnce has not been called")
        U_max_norm, cols = self._frame_prepare(self._frame_rows(sim, time))
        if cols is None:                                                                # :413-421
            return 0
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
        self._record_blocks(self._surrogate(*grid.shape[:2]).block_error(grid[..., :3], grid[..., 3]))
        if apply_filter:
            res = self._surrogate(*grid.shape[:2]).gaussian_filter(res, (10, 10))
        self.cfd_results = grid[..., 3] * max_abs_p * pow(U_max_norm, 2.0)               # :580 (float32 square, like the reference)
        self.no_flow_bool = grid[..., 2] == 0
        self.U_max_norm = float(U_max_norm)
        self._record_errors(res, self.cfd_results, self.no_flow_bool)
        return res

    def _record_blocks(self, mb: dict):
        """:553-557 the error of the decoded blocks: appended to ``pred_minus_true_block`` / ``pred_minus_true_squared_block``, kept
        in ``last_metrics['blocks']``."""
        for name, key in (("pred_minus_true_block", "mean_err"), ("pred_minus_true_squared_block", "mean_sq_err")):
            if not hasattr(self, name):
                setattr(self, name, [])
            getattr(self, name).append(mb[key])
        if not isinstance(getattr(self, "last_metrics", None), dict):
            self.last_metrics = {}
        self.last_metrics["blocks"] = mb

    # ---- a frame's scalars and columns: the statements timeStep and timeSteps share (quoted in tests/test_frame_rows.py) ------
    def _frame_rows(self, sim, time) -> np.ndarray:
        """The rows of frame (sim, time) as stored: float32 like the file, the reference normalises in float32."""
        from . import formats
        return formats.read_dataset(self.dataset_path, sim, time)[0][0, 0, :self.indice]

    def _frame_prepare(self, d: np.ndarray, full: bool = True):
        """-> (U_max_norm as the float32 the statements give, cell columns float64; None for an irrelevant time step, :413-421).
        Columns: dUx / U, dUy / U, dp / U^2 (what ``timeSteps`` sends), and with ``full`` p, the dU-change weight and delta_p_prev."""
        Ux, Uy, p = d[:, 0:1], d[:, 1:2], d[:, 2:3]
        delta_U, delta_p = d[:, 5:7], d[:, 7:8]
        U_max_norm = np.max(np.sqrt(np.square(Ux) + np.square(Uy)))                      # :407
        deltaU_max_norm = np.max(np.sqrt(np.square(delta_U[:, 0:1]) + np.square(delta_U[:, 1:2])))
        if (deltaU_max_norm / U_max_norm) < 1e-4:                                       # :413-421
            return U_max_norm, None
        cols = [delta_U / U_max_norm, delta_p / pow(U_max_norm, 2.0)]
        if full:
            delta_U_prev, delta_p_prev = d[:, 8:10], d[:, 10:11]
            deltaU_changed = np.abs(delta_U - delta_U_prev).sum(axis=-1)                 # :400-401
            deltaU_changed = deltaU_changed / deltaU_changed.max()
            cols += [p, deltaU_changed[:, None], delta_p_prev]
        return U_max_norm, np.concatenate(cols, axis=1).astype(np.float64)

    # ---- timeSteps: one loop for the three evaluators and both ways of preparing a frame ------------------------------------
    def _frames(self, sim, times, apply_filter, fields, device_prep, *params):
        """The calls of one ``timeSteps``, ``max_frames`` frames each -> per call (surrogate, the evaluator's outputs of the call,
        [(slot in times, U_max_norm, relevant) per frame of the call]).  Host preparation sends the relevant frames only;
        ``device_prep`` sends the rows of every frame, which keeps its slot in its call and is read off the returned scalars.
        Nothing is bound or sent when no frame is left."""
        rows = [self._frame_rows(sim, time) for time in times]
        if device_prep:
            picked = [(i, None, d) for i, d in enumerate(rows)]
        else:
            picked = [(i, U, cols) for i, (U, cols) in enumerate(self._frame_prepare(d, full=False) for d in rows) if cols is not None]
        if not picked:
            return
        sur = self._surrogate(self.grid_shape_y, self.grid_shape_x)
        self._bind_frames(sur, apply_filter)
        if device_prep and sur._rows_bound < rows[0].shape[1]:
            sur.bind_rows(rows[0].shape[1])
        for c0 in range(0, len(picked), self.max_frames):
            part = picked[c0:c0 + self.max_frames]
            chunk = np.stack([a for _, _, a in part])
            if device_prep:
                *outs, sc = self._rows_call(sur, chunk, apply_filter, fields, *params)
                yield sur, outs, [(i, sc[j, 0], sc[j, 3] != 0) for j, (i, _, _) in enumerate(part)]      # the skip rule, decided on the device
            else:
                outs = self._host_call(sur, chunk, [U for _, U, _ in part], apply_filter, fields, *params)
                yield sur, outs, [(i, U, True) for i, U, _ in part]

    def _time_steps(self, sim, times, apply_filter, fields, device_prep, *params):
        """``timeSteps`` of every evaluator: the frames in order through ``_record_frame``, 0 left in the slot of an irrelevant one.
        What ``timeStep`` leaves once per call (``_frames_start``) is set before the first relevant frame is recorded, the tail of
        a metrics-only sweep (``_frames_end``) after the last: neither happens when every frame was irrelevant."""
        if getattr(self, "tables", None) is None:
            raise RuntimeError("computeOnlyOnce has not been called")
        times = [int(t) for t in times]
        out, started = [0] * len(times), False
        self._frames_reset(len(times))
        for sur, outs, frames in self._frames(sim, times, apply_filter, fields, device_prep, *params):
            for j, (slot, U, relevant) in enumerate(frames):
                if not relevant:
                    continue
                if not started:
                    self._frames_start()
                    started = True
                self.U_max_norm = float(U)
                out[slot] = self._record_frame(sur, outs, j, slot, self.U_max_norm, fields)
        if started:
            self._frames_end(fields)
        return out

    def _frames_reset(self, n_frames: int):
        """What a ``timeSteps`` call resets whatever its frames are."""

    def _frames_start(self):
        self.max_abs_p = float(self.maxs[3])
        sd = np.nan_to_num(np.asarray(self.sdfunct[..., 0], np.float64), nan=0.0) / float(self.maxs[2])
        self.no_flow_bool = sd == 0

    def _frames_end(self, fields: bool):
        if not fields:
            self.cfd_results = None

    def _host_call(self, sur, cols, Us, apply_filter, fields):
        max_abs_p = float(self.maxs[3])
        return sur.deltas_frames(cols, [float(pow(U, 2.0)) for U in Us],                       # :580 (float32 square, like the reference)
                                 out_scale=[max_abs_p * U ** 2 for U in Us], apply_filter=apply_filter,
                                 want_result=fields, want_truth=fields)

    def _rows_call(self, sur, rows, apply_filter, fields):
        return sur.deltas_rows(rows, float(self.maxs[3]), apply_filter=apply_filter, want_result=fields, want_truth=fields)

    def _record_frame(self, sur, outs, j, slot, U, fields):
        """One relevant frame of a call's (result, truth, raw) -> what ``timeSteps`` returns for it."""
        res, truth, raw = outs
        mb = sur.metrics_from_sums(raw[j, 1])                                          # :553-557, before the assembly
        mb.update(norm_pred=float(raw[j, 1, 6] - raw[j, 1, 5]), n=int(raw[j, 1, 0]))
        self._record_blocks(mb)
        if fields:
            self.cfd_results = truth[j]
            self._record_errors(res[j], self.cfd_results, self.no_flow_bool)
            return res[j]
        return {"delta_p": self._record_metrics(sur.metrics_from_sums(raw[j, 0])), "blocks": mb}

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
        return self._time_steps(sim, times, apply_filter, fields, device_prep)

    print_metrics = False          # True: print the per-frame error block like the reference's timeStep does

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
        if getattr(self, "tables", None) is None:
            raise RuntimeError("computeOnlyOnce has not been called")
        U, cols = self._frame_prepare(self._frame_rows(sim, time))
        if cols is None:                                                                             # :562-567
            return 0
        g = self._mesh_to_grid(cols)                                                                 # :577-600, NaNs kept
        self.U_max_norm = U
        field_deltap = self.timeStep_grid(g[..., 0], g[..., 1], g[..., 2], g[..., 3], self.sdfunct[..., 0], phi, U,
                                          deltaU_change_grid=g[..., 6], deltaP_prev_grid=g[..., 7], apply_filter=apply_filter,
                                          apply_deltaU_change_wgt=True)                               # :831
        self._frames_start()                                                                         # :850
        return self._record_fields(field_deltap, g[..., 4], g[..., 5], U)

    def _frame_prepare(self, d: np.ndarray, full: bool = True):
        """-> (float(U_max_norm), the eight cell columns float64; None for an irrelevant time step, :562-567)."""
        Ux, Uy, p = d[:, 0:1], d[:, 1:2], d[:, 2:3]
        delta_U, delta_p = d[:, 5:7], d[:, 7:8]
        delta_U_prev, delta_p_prev = d[:, 8:10], d[:, 10:11]
        deltaU_changed = np.abs(delta_U - delta_U_prev).sum(axis=-1)
        deltaU_changed = deltaU_changed / deltaU_changed.max()
        U_max_norm = np.max(np.sqrt(np.square(Ux) + np.square(Uy)))
        deltaU_max_norm = np.max(np.sqrt(np.square(delta_U[:, 0:1]) + np.square(delta_U[:, 1:2])))
        if (deltaU_max_norm / U_max_norm) < 1e-4 or deltaU_max_norm < 1e-6 or U_max_norm < 1e-6:      # :562-567
            return float(U_max_norm), None
        return float(U_max_norm), np.concatenate([Ux, Uy, delta_U, delta_p, p, deltaU_changed[:, None], delta_p_prev], axis=1).astype(np.float64)

    def _record_fields(self, field_deltap, delta_p_plane, p_plane, U):
        """The three error blocks of :962-1043 -- delta-p (weighted), delta-p without the weighting (``deltap_res``), and p -- from a
        frame's field and its interpolated label planes (NaNs kept); ``no_flow_bool`` is set.  Returns ``field_deltap``."""
        delta_p_grid = np.nan_to_num(delta_p_plane / pow(U, 2.0), nan=0.0) / self.max_abs_delta_p     # :687-711 (channel 4)
        p_grid = np.nan_to_num(p_plane, nan=0.0)                                                      # :692-702 (channel 5)
        self.cfd_results = delta_p_grid * self.max_abs_delta_p * pow(U, 2.0)                          # :849
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

    def _bind_frames(self, sur, apply_filter: bool = False):
        """What timeSteps needs on the handle, once per computeOnlyOnce (whose new plan drops all three): the features with the
        simulation's SDF plane in every slot, the post-steps (SM_call.py:353, :360; with or without ``apply_filter``: the weighting
        needs them) and the frame staging."""
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
        return self._time_steps(sim, times, apply_filter, fields, device_prep, phi)

    def _frames_reset(self, n_frames: int):
        self.label_planes = [None] * n_frames

    def _frames_start(self):
        sd = np.nan_to_num(self.sdfunct[..., 0], nan=0.0) / self.max_abs_dist
        self.no_flow_bool = sd == 0                                                                   # :850

    def _frames_end(self, fields: bool):
        if not fields:
            self.deltap_res = self.cfd_results = self.p_pred = self.label_planes = None

    def _host_call(self, sur, cols, Us, apply_filter, fields, phi):
        """-> (result, next, label planes, raw): the fields, or the sums alone for a metrics-only sweep."""
        LU, scale = [[phi, U] for U in Us], [self.max_abs_delta_p * U ** 2 for U in Us]              # :816
        if not fields:
            return None, None, None, sur.poisson_frames_errors(cols, LU, out_scale=scale, apply_filter=apply_filter)
        res, _, nxt, extra = sur.poisson_frames(cols, LU, out_scale=scale, apply_filter=apply_filter, weighting=True, want_extra=True)
        return res, nxt, extra, None

    def _rows_call(self, sur, rows, apply_filter, fields, phi):
        if not fields:
            return (None, None, None, *sur.poisson_rows_errors(rows, self.max_abs_delta_p, phi, apply_filter=apply_filter))
        res, _, nxt, extra, sc = sur.poisson_rows(rows, self.max_abs_delta_p, phi, apply_filter=apply_filter, weighting=True, want_extra=True)
        return res, nxt, extra, None, sc

    def _record_frame(self, sur, outs, j, slot, U, fields):
        res, nxt, extra, raw = outs
        if not fields:
            return {sfx: self._record_metrics(sur.metrics_from_sums(raw[j, q]), sfx, title) for q, (sfx, title) in enumerate(self.ERROR_BLOCKS)}
        self.deltap_res, self.label_planes[slot] = res[j, :, :, 0], extra[j]
        return self._record_fields(nxt[j], extra[j, 0], extra[j, 1], U)

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
        self.X0_min = t.x0
        return self._set_tables(t)

    def _frame_rows(self, sim, time) -> np.ndarray:
        from . import formats
        return formats.read_dataset(self.hdf5_path, sim, time)[0][0, 0, :self.indice]

    def _frame_prepare(self, d: np.ndarray, full: bool = True):
        """-> (U_max_norm as the float32 the statements give, the five cell columns float64): every frame is relevant."""
        Ux, Uy, p, dPdx, dPdy = d[:, 0:1], d[:, 1:2], d[:, 2:3], d[:, 6:7], d[:, 7:8]
        U_max_norm = np.max(np.sqrt(np.square(Ux) + np.square(Uy)))                       # :438
        return U_max_norm, np.concatenate([Ux / U_max_norm, Uy / U_max_norm,            # :443-444
                                           dPdx * (self.max_x - self.min_x) / pow(U_max_norm, 2.0),   # :440
                                           dPdy * (self.max_y - self.min_y) / pow(U_max_norm, 2.0),   # :441
                                           p / pow(U_max_norm, 2.0)], axis=1).astype(np.float64)      # :442

    def timeStep(self, sim, time, plot_intermediate_fields=False, save_plots=False, show_plots=False, apply_filter=False):
        """Eval_dual_Dense_onlycil.py:418-640 without plots and error prints: frame (sim, time) -> the integrated
        pressure image [Ny,Nx] (``field``).  Kept: ``self.grid`` (6 channels), ``self.gradP`` [Ny,Nx,2]."""
        if getattr(self, "tables", None) is None:
            raise RuntimeError("computeOnlyOnce has not been called")
        U_max_norm, cols = self._frame_prepare(self._frame_rows(sim, time))
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
        center_p_y, center_p_x, dx, dy = self._integration_cut()                          # :591-600
        sur.set_integration(self.sdfunct[..., 0], center_p_y, center_p_x, dx, dy)
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
        return self._time_steps(sim, times, apply_filter, fields, device_prep)

    def _frames_reset(self, n_frames: int):
        self.frame_metrics = []

    def _frames_start(self):
        sd = np.nan_to_num(np.asarray(self.sdfunct[..., 0], np.float64), nan=0.0) / float(self.maxs[2])
        self.no_flow_bool = sd == 0
        self.center_p_y, self.center_p_x = self._integration_cut()[:2]
        if not isinstance(getattr(self, "last_metrics", None), dict):
            self.last_metrics = {}

    def _frames_end(self, fields: bool):
        pass

    def _host_call(self, sur, cols, Us, apply_filter, fields):
        return sur.gradp_frames(cols, apply_filter=apply_filter, want_gradp=fields, want_p=fields, want_truth=fields)

    def _rows_call(self, sur, rows, apply_filter, fields):
        return sur.gradp_rows(rows, float(self.max_x - self.min_x), float(self.max_y - self.min_y), apply_filter=apply_filter,
                              want_gradp=fields, want_p=fields, want_truth=fields)

    def _record_frame(self, sur, outs, j, slot, U, fields):
        """One frame of a call's (gradp, p, truth, raw) -> its p image, or its four metric blocks for a metrics-only sweep."""
        gradp, p, truth, raw = outs
        m = {name: sur.metrics_from_sums(raw[j, r]) for r, name in enumerate(self.METRIC_ROWS)}
        if fields:
            self.gradP = gradp[j]
            m["reference"] = error_metrics(p[j], truth[j, 0], self.no_flow_bool)
            m["p"] = error_metrics(p[j], truth[j, 2], self.no_flow_bool)
        self._record_metrics(m["reference"], "", "reference metric (grid channel 3)")
        self.last_metrics.pop("delta_p")
        self.last_metrics.update(m)
        self.frame_metrics.append(m)
        return p[j] if fields else m

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


class EvaluationChapter4(Evaluation):
    """The ``Evaluation`` of the two Chapter-4 thesis evaluators on the GPU path, chosen by ``inputs``:

    * ``'M_u'``  -- Thesis_Work/Chapter4/MLP/M_u/Evaluation/Eval_dual_Dense_onlycil.py: (Ux, Uy, SDF) -> p; ``maxs`` = (max_abs_Ux,
      max_abs_Uy, max_abs_dist, max_abs_p);
    * ``'M_fU'`` -- Thesis_Work/Chapter4/MLP/M_fU/Evaluation/Eval.py: (f(U), SDF) -> p, f(U) = dataset column 5; ``maxs`` =
      (max_abs_fU, max_abs_dist, max_abs_p).

    Both read ``maxs``, ``maxs_PCA``, ``ipca_input_more.pkl`` and ``ipca_p_more.pkl`` from the working directory (``artifact_dir``),
    scale the PCA coefficients by the two ``maxs_PCA`` values, and count components by ``formats.select_num_pc_chapter4``.
    Prediction and label are compared in normalised units: no dimensional scale enters (M_u :457-476).

    The M_u file assigns ``self.var_p = var_in`` and never sets ``self.var_in``, which it then reads (:38-39, :56): as written its
    constructor raises.  ``var_in`` is taken here the way the M_fU file takes it.
    ``apply_filter=True`` is rejected: both files replace ``result_array`` by a 2-D array in the filter branch (M_u :421) and then
    index it with four subscripts (:457-458), so the reference itself cannot process that input."""
    variant = "chapter5"

    def __init__(self, delta, shape, avance, var_p, var_in, hdf5_path, model_directory, inputs: str = "M_u",
                 model: SurrogateModel = None, device: int = 0, artifact_dir: str = None, max_frames: int = None):
        if inputs not in ("M_u", "M_fU"):
            raise ValueError("inputs is 'M_u' or 'M_fU'")
        from . import formats
        self.inputs = inputs
        self.c_in_expected = 3 if inputs == "M_u" else 2
        self.sdf_ch_expected = self.c_in_expected - 1
        maxs = None
        if model is None:
            model, maxs = load_artifacts(self.variant, model_directory, artifact_dir or os.getcwd(), var_p, var_in, None, "max_abs",
                                         shape, avance, self.c_in_expected, self.sdf_ch_expected,
                                         pca_stems=("ipca_input_more", "ipca_p_more"),
                                         pc_rule=lambda evr, var, side: formats.select_num_pc_chapter4(evr, var, inputs, side))
        if model.variant != self.variant or model.c_in != self.c_in_expected or model.sdf_ch != self.sdf_ch_expected or model.c_out != 1:
            raise ValueError(f"{inputs} takes a chapter5-variant model with {self.c_in_expected} input channels, the SDF last, and 1 output channel")
        super().__init__(delta, shape, avance, var_p, var_in, hdf5_path, model_directory, None, "max_abs", model, device,
                         artifact_dir, max_frames)
        self.maxs = maxs
        if maxs is not None and len(maxs) < self.c_in_expected + 1:
            raise ValueError(f"maxs must hold {self.c_in_expected + 1} values for {inputs}")
        self.avance = avance
        self.hdf5_path = hdf5_path

    def _max_abs(self) -> list:
        """[c_in + 1]: the scales of the c_in - 1 input channels, of the distance and of p (M_u :45, M_fU :45)."""
        n = self.c_in_expected + 1
        return [float(v) for v in (self.maxs[:n] if self.maxs is not None else (1.0,) * n)]

    def _mesh_maxs(self) -> np.ndarray:
        mx = self._max_abs()
        return np.asarray([mx[0], mx[1] if self.inputs == "M_u" else 1.0, mx[-2], mx[-1]], np.float64)

    def computeOnlyOnce(self, sim):
        """M_u :105-189 (M_fU likewise): 2-digit bounds (:115-119), every 2nd boundary point (:150-151), the pressure column
        decides interpolability (:174-178), no IDW fallback.  Returns 0."""
        from . import formats
        from .geometry import build_geometry_evaluator
        data, top_b, obst_b = formats.read_dataset(self.hdf5_path, sim, 0)
        self.indice = formats.first_index(data[0, 0, :, 0], formats.PAD_VALUE)
        cells = np.asarray(data[0, 0, :self.indice], np.float64)
        top = np.asarray(top_b[0, 0, :formats.first_index(top_b[0, 0, :, 0], formats.PAD_VALUE)], np.float64)
        obst = np.asarray(obst_b[0, 0, :formats.first_index(obst_b[0, 0, :, 0], formats.PAD_VALUE)], np.float64)
        return self._set_tables(build_geometry_evaluator(cells[:, 3:5], cells[:, 2], top, obst, self.delta, every=2, round_digits=2,
                                                         idw_fallback=False))

    def _frame_rows(self, sim, time) -> np.ndarray:
        from . import formats
        return formats.read_dataset(self.hdf5_path, sim, time)[0][0, 0, :self.indice]

    def _frame_prepare(self, d: np.ndarray, full: bool = True):
        """-> (U_max_norm as the float32 the statements give, the c_in cell columns float64): every frame is relevant."""
        Ux, Uy, p = d[:, 0:1], d[:, 1:2], d[:, 2:3]
        U_max_norm = np.max(np.sqrt(np.square(Ux) + np.square(Uy)))                       # M_u :203
        if self.inputs == "M_u":
            cols = [Ux / U_max_norm, Uy / U_max_norm, p / pow(U_max_norm, 2.0)]           # M_u :205-207
        else:
            cols = [d[:, 5:6] / pow(U_max_norm, 2.0), p / pow(U_max_norm, 2.0)]           # M_fU :203-208
        return U_max_norm, np.concatenate(cols, axis=1).astype(np.float64)

    @staticmethod
    def _no_filter(apply_filter):
        if apply_filter:
            raise ValueError("apply_filter=True: the reference replaces result_array by a 2-D array (M_u :421) and then indexes it "
                             "with four subscripts (:457-458); it cannot process that input, and neither does this evaluator")

    def timeStep(self, sim, time, save_plots=False, show_plots=False, apply_filter=False):
        """M_u :193-479 (M_fU :193-477) without plots and prints: frame (sim, time) -> the assembled normalised pressure image
        [Ny,Nx].  Kept: ``grid`` (c_in + 1 channels, normalised), ``cfd_results`` (its label channel), ``no_flow_bool``,
        ``U_max_norm``, ``last_metrics['p']``; the frame's two values are appended to ``pred_minus_true`` /
        ``pred_minus_true_squared``."""
        self._no_filter(apply_filter)
        if getattr(self, "tables", None) is None:
            raise RuntimeError("computeOnlyOnce has not been called")
        U_max_norm, cols = self._frame_prepare(self._frame_rows(sim, time))
        g = self._mesh_to_grid(cols)                                                      # :209-218, NaNs kept
        c, mx = self.c_in_expected, self._max_abs()
        grid = np.zeros((self.grid_shape_y, self.grid_shape_x, c + 1))
        grid[..., :c - 1] = g[..., :c - 1]
        grid[..., c - 1] = self.sdfunct[..., 0]
        grid[..., c] = g[..., c - 1]
        grid[np.isnan(grid)] = 0                                                          # :220
        for ch in range(c + 1):
            grid[..., ch] /= mx[ch]                                                       # :222-225
        self.grid = grid
        self.U_max_norm = float(U_max_norm)
        res = self._surrogate(*grid.shape[:2]).solve(grid[..., :c])[0, :, :, 0]           # :230-414
        self.cfd_results = grid[..., c]
        self.no_flow_bool = grid[..., c - 1] == 0
        self._record_p(error_metrics(res, self.cfd_results, self.no_flow_bool))           # :457-477
        return res

    def _record_p(self, m: dict) -> dict:
        self._record_metrics(m, "", "Error in p (normalised)")
        self.last_metrics["p"] = self.last_metrics.pop("delta_p")
        return m

    @property
    def FRAME_COLUMNS(self):        # the c_in - 1 input columns and the label column p / U^2
        return self.c_in_expected

    def _bind_frames(self, sur, apply_filter: bool):
        """What timeSteps needs on the handle, once per computeOnlyOnce (whose new plan drops them): the frame staging and the
        Chapter-4 binding with the simulation's SDF plane and scales."""
        if getattr(self, "_frames_tables", None) is self.tables and sur._frames_bound and sur._chapter4_bound:
            return
        sur.bind_frames(self.max_frames, self.FRAME_COLUMNS)
        sur.bind_chapter4_frames(self.sdfunct[..., 0], self._max_abs())
        self._frames_tables = self.tables

    def timeSteps(self, sim, times, apply_filter=False, fields=True, device_prep=False):
        """``timeStep`` for several frames of one simulation, sent ``max_frames`` at a time as ONE call each (``chapter4_frames``:
        cell columns -> planes -> image, truth -> solve -> the error sums on the device).  The per-frame host scalar and columns
        are those of ``timeStep``; ``pred_minus_true``, ``pred_minus_true_squared`` and ``last_metrics['p']`` are filled in frame
        order.  Returns the list of normalised p images; afterwards ``cfd_results``, ``no_flow_bool`` and ``U_max_norm`` hold what
        ``timeStep`` leaves on the last frame (``grid`` is not produced).
        ``fields=False``: a metrics-only sweep -- nothing but the sums comes back (8 doubles per frame), the metrics are taken
        from them, the return is one ``{'p': metrics}`` dict per frame and ``cfd_results`` is None.
        ``device_prep=True`` raises: the rows stage takes rows 8 to 16 wide, Chapter-4 rows are 6 wide."""
        self._no_filter(apply_filter)
        if device_prep:
            raise ValueError("device_prep=True: the rows stage (bind_rows) takes rows 8 to 16 columns wide; Chapter-4 dataset rows are 6 wide")
        return self._time_steps(sim, times, apply_filter, fields, device_prep)

    def _frames_start(self):
        sd = np.nan_to_num(np.asarray(self.sdfunct[..., 0], np.float64), nan=0.0) / self._max_abs()[-2]
        self.no_flow_bool = sd == 0

    def _frames_end(self, fields: bool):
        if not fields:
            self.cfd_results = None

    def _host_call(self, sur, cols, Us, apply_filter, fields):
        return sur.chapter4_frames(cols, want_result=fields, want_truth=fields)

    def _record_frame(self, sur, outs, j, slot, U, fields):
        """One frame of a call's (result, truth, raw) -> its p image, or its metric block for a metrics-only sweep."""
        res, truth, raw = outs
        if not fields:
            return {"p": self._record_p(sur.metrics_from_sums(raw[j, 0]))}
        self.cfd_results = truth[j]
        self._record_p(error_metrics(res[j], truth[j], self.no_flow_bool))
        return res[j]


def main_chapter4(delta=5e-3, model_directory="model_first_.h5", shape=128, avance=None, var_p=0.95, var_in=0.95,
                  hdf5_path="dataset_unsteadyCil_fu_bound.hdf5", inputs="M_u", sims=(0, 3, 6, 8), n_ts=10, apply_filter=False,
                  device: int = 0, artifact_dir: str = None, frames_per_call: int = 1, fields: bool = True):
    """``main`` of the two Chapter-4 evaluators (M_u :483-533, M_fU :481-531) with their hard-coded inputs as defaults
    (``avance = int(0.75 * shape)``, simulations 0, 3, 6, 8, ten time steps; the M_u file passes ``var_in = 0.995``):
    computeOnlyOnce + timeStep per frame, then BIAS / RMSE / STDE [%] from the accumulated per-frame values.  The reference
    prints them once, after the last simulation (:526-533); here they are printed and returned after every simulation, over
    everything accumulated so far, so that the last entry is the reference's.  Plots are not produced.
    ``frames_per_call`` > 1: the frames of a simulation go through ``EvaluationChapter4.timeSteps``, that many per call, instead of
    one ``timeStep`` each.  ``fields=False``: the same summary from ``timeSteps(..., fields=False)``, whose error sums are taken on
    the device: no field is copied back.  With the defaults the loop is the per-frame one."""
    EvaluationChapter4._no_filter(apply_filter)
    if avance is None:
        avance = int(0.75 * shape)
    ev = EvaluationChapter4(delta, shape, avance, var_p, var_in, hdf5_path, model_directory, inputs=inputs, device=device,
                            artifact_dir=artifact_dir, max_frames=frames_per_call)
    ev.pred_minus_true, ev.pred_minus_true_squared = [], []
    out = {"sims": [], "frames": []}
    batched = frames_per_call > 1 or not fields
    for sim in sims:
        ev.computeOnlyOnce(sim)
        for t0 in range(0, n_ts, frames_per_call if batched else 1):
            chunk = range(t0, min(t0 + (frames_per_call if batched else 1), n_ts))
            n0 = len(ev.pred_minus_true)
            if batched:
                ev.timeSteps(sim, chunk, apply_filter, fields=fields)
            else:
                ev.timeStep(sim, t0, False, False, apply_filter)
            for time, b, s in zip(chunk, ev.pred_minus_true[n0:], ev.pred_minus_true_squared[n0:]):
                out["frames"].append(dict(sim=sim, time=time, mean_err=b, mean_sq_err=s))
        s = _summary(ev.pred_minus_true, ev.pred_minus_true_squared)
        print("BIAS for the sim: " + str(s["BIAS"]))
        print("RMSE for the sim: " + str(s["RMSE"]))
        print("STDE for the sim: " + str(s["STDE"]))
        out["sims"].append(s)
    return out
