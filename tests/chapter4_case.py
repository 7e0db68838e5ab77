"""The dataset-driven case of the two Chapter-4 evaluators (Thesis_Work/Chapter4/MLP/M_u/Evaluation/Eval_dual_Dense_onlycil.py and
M_fU/Evaluation/Eval.py): a 6-column dataset on `synthetic.channel_mesh()` -- 138 x 300 grid, 14 blocks at shape 128 / avance 96 --
and the artefact directory `EvaluationChapter4` reads.  tests/golden/make_golden_chapter4_eval.py runs the reference's `timeStep` on
frame `FRAME` of this dataset with `model(inputs)` and writes tests/golden/chapter4_evaluator_138x300.npz."""
import os

import numpy as np

from psm_amd import geometry, synthetic

INPUTS = ("M_u", "M_fU")
C_IN = {"M_u": 3, "M_fU": 2}
# the `maxs` files: M_u (max_abs_Ux, max_abs_Uy, max_abs_dist, max_abs_p), M_fU (max_abs_fU, max_abs_dist, max_abs_p)
MAXS = {"M_u": (1.0, 0.41, 0.33, 0.9), "M_fU": (0.9, 0.33, 0.9)}
SHAPE, AVANCE, DELTA = 128, 96, 5e-3
FRAMES = 3
FRAME = 1                       # the frame of the fixture
P_STORED, P_KEPT = 32, 24       # components in the pickles, components both PC rules keep at var = 0.95


def frames():
    """-> (sim [1, FRAMES, N, 6] float32: Ux, Uy, p, Cx, Cy, f(U); top; obst) unpadded."""
    fr = [synthetic.channel_mesh(step=s) for s in range(FRAMES)]
    top, obst = fr[0][1], fr[0][2]
    N = fr[0][0].shape[0]
    sim = np.empty((1, FRAMES, N, 6), np.float32)
    for t, (a, _, _) in enumerate(fr):
        sim[0, t, :, 0:2] = a[:, 0:2]; sim[0, t, :, 2] = a[:, 4]; sim[0, t, :, 3:5] = a[:, 2:4]
        sim[0, t, :, 5] = 0.5 * (a[:, 0] ** 2 + a[:, 1] ** 2) + 0.2 * np.sin(4 * a[:, 2] + 0.15 * t) * a[:, 1]    # a synthetic f(U)
    return sim, top, obst


def tables(sim, top, obst):
    """The tables of computeOnlyOnce's parameters (M_u :115-119, :150-153): 2-digit bounds, every second boundary point, the
    pressure decides interpolability, no IDW fallback."""
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)          # the dataset stores float32
    cells = np.asarray(sim[0, 0], np.float64)
    return geometry.build_geometry_evaluator(cells[:, 3:5], cells[:, 2], f32(top), f32(obst), DELTA, every=2, round_digits=2,
                                             idw_fallback=False)


def model(inputs: str):
    m = synthetic.make_model("chapter5", p_in=P_KEPT, p_out=P_KEPT, c_in=C_IN[inputs])
    m.ov, m.sdf_ch = AVANCE, C_IN[inputs] - 1
    return m


def build_chapter4_dataset_case(directory: str, inputs: str):
    """Everything `EvaluationChapter4(delta, shape, avance, var_p, var_in, hdf5_path, model_directory, inputs)` reads from disk,
    written into `directory` in the reference's formats: the padded dataset (1 simulation x 3 frames, 6 columns, pad -100), `maxs`
    (4 values for M_u, 3 for M_fU), `maxs_PCA`, the pickled PCA objects under the `_more` names and a Keras-style Dense `.h5`.
    The first P_KEPT components of the pickles are those of `model(inputs)`."""
    import pickle
    from sklearn.decomposition import PCA
    import h5write
    sim_u, top, obst = frames()
    N = sim_u.shape[2]
    max_cells, max_pts = N + 37, max(len(top), len(obst)) + 11
    sim = np.full((1, FRAMES, max_cells, 6), -100.0, np.float32)
    sim[:, :, :N] = sim_u
    tb = np.full((1, FRAMES, max_pts, 2), -100.0, np.float32); ob = tb.copy()
    tb[0, :, :len(top)] = top; ob[0, :, :len(obst)] = obst
    h5write.write_h5(os.path.join(directory, "dataset.hdf5"), {"sim_data": sim, "top_bound": tb, "obst_bound": ob})
    np.savetxt(os.path.join(directory, "maxs"), np.array(MAXS[inputs]))
    m = model(inputs)
    full = synthetic.make_model("chapter5", p_in=P_STORED, p_out=P_STORED, c_in=C_IN[inputs])
    np.savetxt(os.path.join(directory, "maxs_PCA"), np.array([m.in_a, m.out_a]))
    evr = np.array([0.0395] * P_KEPT + [0.004] * (P_STORED - P_KEPT))     # cumulative ratio first exceeds 0.95 at index 24
    for stem, comp, more, mean in (("ipca_input_more", m.comp_in, full.comp_in, m.mean_in), ("ipca_p_more", m.comp_out, full.comp_out, m.mean_out)):
        o = PCA(n_components=P_STORED)
        o.components_, o.mean_, o.explained_variance_ratio_ = np.concatenate([comp, more[P_KEPT:]]), mean, evr
        with open(os.path.join(directory, stem + ".pkl"), "wb") as f:
            pickle.dump(o, f)
    h5write.write_keras_dense(os.path.join(directory, "model_first_.h5"), m.weights)
    return dict(sim=sim, top=top, obst=obst, N=N, model=m, dataset_path=os.path.join(directory, "dataset.hdf5"),
                model_path=os.path.join(directory, "model_first_.h5"))
