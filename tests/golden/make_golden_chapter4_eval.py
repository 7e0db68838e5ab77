#!/usr/bin/env python3
"""Generate tests/golden/chapter4_evaluator_138x300.npz by RUNNING THE REFERENCE'S OWN STATEMENTS: the whole ``timeStep`` body of
the two Chapter-4 evaluators (Thesis_Work/Chapter4/MLP/M_u/Evaluation/Eval_dual_Dense_onlycil.py and M_fU/Evaluation/Eval.py), from
``i = 0`` to the last ``append``, on frame ``chapter4_case.FRAME`` of the dataset of tests/chapter4_case.py.

Like make_golden.py, whose helpers this imports: the reference files are parsed with ``ast`` at run time and their statements are
compiled unmodified; prints, plots and the ``return`` are dropped; the PCA objects are real scikit-learn ones carrying the seeded
synthetic basis, the network is a NumPy Dense stack, and the one-time tables come from this build's geometry step with
``computeOnlyOnce``'s parameters (the method itself needs shapely).  Runs only where the reference is present; the test-suite reads
the ``.npz`` it writes.  No reference source text is stored: only numeric outputs.

Usage:  python tests/golden/make_golden_chapter4_eval.py
"""
from __future__ import annotations

import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import make_golden as mg  # noqa: E402
import chapter4_case as c4  # noqa: E402

PATHS = {"M_u": mg.C4E, "M_fU": mg.C4F}
CROP = (slice(40, 100), slice(120, 200))


def run_time_step(inputs, cells32, tab, model, maxs):
    """``timeStep`` of ``Evaluation`` in PATHS[inputs] on one frame's rows -> the fixture's entries for that file."""
    path = PATHS[inputs]
    tree = mg._tree(path)
    Ev = type("Ev", (), {"interpolate_fill": mg._method(tree, "Evaluation", "interpolate_fill", {"np": np}, path)})
    me = Ev()
    me.indice, me.vert, me.weights, me.indices = cells32.shape[0], tab.vtx_m2g, tab.wts_m2g, tab.indices
    me.sdfunct, me.grid_shape_y, me.grid_shape_x = tab.sdfunct[:, :, None], tab.ny, tab.nx
    if inputs == "M_u":
        me.max_abs_Ux, me.max_abs_Uy, me.max_abs_dist, me.max_abs_p = maxs
    else:
        me.max_abs_fU, me.max_abs_dist, me.max_abs_p = maxs
    me.avance, me.shape = model.ov, model.S
    me.pcainput, me.pcap = mg.sk_pca(model.comp_in, model.mean_in), mg.sk_pca(model.comp_out, model.mean_out)
    me.pc_in, me.pc_p = model.p_in, model.p_out
    me.max_abs_input_PCA, me.max_abs_p_PCA = model.in_a, model.out_a
    me.model = mg.dense_callable(model.weights)
    me.pred_minus_true, me.pred_minus_true_squared = [], []
    body = mg._find_fn(tree, "timeStep", "Evaluation").body
    i0 = next(i for i, st in enumerate(body) if mg._src(st).startswith("i = 0"))
    i1 = max(i for i, st in enumerate(body) if mg._src(st).startswith("self.pred_minus_true_squared.append("))
    drop = ("print(", "if save_plots")
    stmts = [st for st in body[i0:i1 + 1] if not isinstance(st, ast.Return) and not mg._src(st).startswith(drop)]
    loc = {"self": me, "data": cells32[None, None], "apply_filter": False, "save_plots": False, "show_plots": False}
    with np.errstate(all="ignore"):
        mg._run(stmts, {"np": np, "pow": pow}, loc, path)
    g = np.asarray(loc["grid"][0], np.float64)
    assert not g[..., model.c_in + 1:].any()              # the M_fU file allocates four channels and fills three
    g = g[..., :model.c_in + 1]
    field = np.asarray(loc["result_array"], np.float64)[0, :, :, 0]
    assert len(me.pred_minus_true) == 1 and not np.isnan(field).any()
    return dict(U_max_norm=np.float64(loc["U_max_norm"]), grid_sum=g.sum(axis=(0, 1)), grid_abs_sum=np.abs(g).sum(axis=(0, 1)),
                grid_crop=g[CROP].copy(), field=field, n_blocks=np.int64(loc["N"]), n_flow=np.int64(np.count_nonzero(g[..., model.c_in - 1])),
                norm=np.float64(loc["norm"]), BIAS_norm=np.float64(loc["BIAS_norm"]), RMSE_norm=np.float64(loc["RMSE_norm"]),
                STDE_norm=np.float64(loc["STDE_norm"]), pred_minus_true=np.float64(me.pred_minus_true[0]),
                pred_minus_true_squared=np.float64(me.pred_minus_true_squared[0]))


def main():
    sim, top, obst = c4.frames()
    tab = c4.tables(sim, top, obst)
    out = {}
    for inputs in c4.INPUTS:
        r = run_time_step(inputs, sim[0, c4.FRAME], tab, c4.model(inputs), c4.MAXS[inputs])
        print(f"{inputs}: grid {tab.ny} x {tab.nx}, {int(r['n_blocks'])} blocks, {int(r['n_flow'])} flow cells, U_max_norm={r['U_max_norm']:.7f}, "
              f"norm={r['norm']:.6f}, BIAS={r['BIAS_norm']:.4f}% RMSE={r['RMSE_norm']:.4f}% STDE={r['STDE_norm']:.4f}%, "
              f"max|field|={np.abs(r['field']).max():.4f}")
        out.update({f"{inputs}_{k}": v for k, v in r.items()})
    np.savez_compressed(os.path.join(HERE, "chapter4_evaluator_138x300.npz"), **out)


if __name__ == "__main__":
    main()
