"""`EvaluationChapter4(delta, shape, avance, var_p, var_in, hdf5_path, model_directory, inputs)` and `main_chapter4` driven from
files in the reference's formats (tests/chapter4_case.py: 6-column padded dataset, `maxs` with 4 or 3 values, `maxs_PCA`,
`ipca_*_more.pkl`, Keras-style `.h5`) on 138 x 300 with 14 blocks, for both `inputs`.

Reference: tests/golden/chapter4_evaluator_138x300.npz, written by tests/golden/make_golden_chapter4_eval.py from the whole
`timeStep` body of the two reference files on frame `chapter4_case.FRAME` of this dataset.  Bounds:
  * grid: the crop within 1e-12 * max|crop| and the channel sums within 1e-12 of the abs-sums, as tests/test_dataset_evaluator.py
    holds `evaluator_grid_138x300.npz` (the interpolation runs on the device in float64, in another summation order);
  * field: eps = (the tolerance tests/test_gpu_parity.py states for final fields) * max|field|;
  * metrics, what eps implies with d = pred - true over n flow cells: |mean(d') - mean(d)| <= eps, so |D mean_err| <= eps / norm;
    |mean(d'^2) - mean(d^2)| <= mean(|d' - d| * |d' + d|) <= eps * (2 * mean|d| + eps) <= 2 * rmse_abs * eps + eps^2 (mean|d| <=
    rmse_abs), so |D mean_sq_err| <= (2 * rmse_abs * eps + eps^2) / norm^2; BIAS and RMSE [%] move by at most e = 100 * eps / norm
    (the RMS is a norm), and STDE^2 = RMSE^2 - BIAS^2 by at most (2 * RMSE * e + e^2) + (2 * |BIAS| * e + e^2), which over
    STDE_got + STDE_ref >= STDE_ref bounds |D STDE|;
  * device sums against host passes over the same field: both are within test_field_errors.SUM_TOL * sum|d| (resp. * sum d^2) of
    the exact sums, so they differ by at most twice that.
Every GPU test prints what it measured before it asserts."""
import functools
import math
import re

import numpy as np
import pytest

import cases
import chapter4_case as c4
import test_gpu_parity
from oracle import psm_oracle as orc
from psm_amd import EvaluationChapter4, formats, main_chapter4, surrogate
from test_field_errors import SUM_TOL
from test_oracle_golden import oracle_model
from test_poisson_frames import same_bits

# "per-block offsets, final fields  : max abs <= 1e-4 * max|field|": the module states its tolerances in its docstring only
FIELD_TOL = float(re.search(r"final fields\s*:\s*max abs <= (\S+) \* max\|field\|", test_gpu_parity.__doc__).group(1))
CROP = (slice(40, 100), slice(120, 200))
_summary, error_metrics = surrogate._summary, surrogate.error_metrics


@pytest.fixture(scope="module", params=c4.INPUTS)
def ds(request, tmp_path_factory):
    inputs = request.param
    d = str(tmp_path_factory.mktemp("chapter4_" + inputs))
    c = c4.build_chapter4_dataset_case(d, inputs)
    c.update(dir=d, inputs=inputs, gold={k[len(inputs) + 1:]: v for k, v in cases.load_golden("chapter4_evaluator_138x300").items()
                                         if k.startswith(inputs + "_")})
    return c


def evaluator(c, **kw):
    return EvaluationChapter4(c4.DELTA, c4.SHAPE, c4.AVANCE, 0.95, 0.95, c["dataset_path"], c["model_path"], inputs=c["inputs"],
                              artifact_dir=c["dir"], **kw)


@functools.lru_cache(maxsize=None)
def host_tables():
    return c4.tables(*c4.frames())


def host_grid(ev, c, time):
    """The mirror's own frame preparation, then the host statements of timeStep in NumPy (M_u :209-225): -> (grid, U_max_norm)."""
    t = host_tables()
    U, cols = ev._frame_prepare(c["sim"][0, time, :c["N"]])
    n = cols.shape[1]
    idx = tuple(np.asarray(t.indices).T)
    grid = np.zeros((t.ny, t.nx, n + 1))
    for col, ch in zip(range(n), list(range(n - 1)) + [n]):
        grid[..., ch][idx] = orc.interpolate_fill(cols[:, col], t.vtx_m2g, t.wts_m2g)
    grid[..., n - 1] = t.sdfunct
    grid[np.isnan(grid)] = 0
    for ch, m in enumerate(c4.MAXS[c["inputs"]]):
        grid[..., ch] /= m
    return grid, U


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_both_pc_rules_arm_by_arm():
    """formats.select_num_pc_chapter4 on hand-made ratio vectors, every arm of M_u :55-56 and M_fU :55-56."""
    rule = formats.select_num_pc_chapter4
    a = np.array([0.0395] * 24 + [0.004] * 8)                 # cumulative: 0.948 after 24, 0.952 at index 24, 0.98 in all
    for inputs in c4.INPUTS:
        for side in ("p", "in"):
            assert rule(a, 0.95, inputs, side) == 24          # k = 24 > 1; M_u: no index above 0.995 -> argmax = 0 <= 64
    b = np.array([0.5, 0.46, 0.02, 0.01, 0.01])               # k = 1: not > 1 -> the cap
    assert [rule(b, 0.95, "M_u", s) for s in ("p", "in")] == [64, 64] and [rule(b, 0.95, "M_fU", s) for s in ("p", "in")] == [512, 512]
    assert rule(np.array([0.99, 0.01]), 0.95, "M_u", "p") == 64 and rule(np.array([0.99, 0.01]), 0.95, "M_fU", "in") == 512      # k = 0
    c = np.array([0.0135] * 70 + [0.011] * 5 + [0.0001] * 25)  # above 0.5 at 37, above 0.95 at 70, above 0.995 at 74
    assert int(np.argmax(np.cumsum(c) > 0.5)) == 37 and int(np.argmax(np.cumsum(c) > 0.95)) == 70 and int(np.argmax(np.cumsum(c) > 0.995)) == 74
    assert rule(c, 0.95, "M_u", "p") == 64                    # cap exceeded: 70 > 64
    assert rule(c, 0.5, "M_u", "p") == 64                     # M_u's FIXED second threshold: k = 37 <= 64, but the 0.95 index is 70
    assert rule(c, 0.5, "M_u", "in") == 64                    # the input side's fixed threshold is 0.995: index 74
    assert rule(c, 0.5, "M_fU", "p") == 37 and rule(c, 0.5, "M_fU", "in") == 37 and rule(c, 0.95, "M_fU", "p") == 70   # var is the second threshold
    d = np.array([0.0135] * 60 + [0.018] * 10)                 # above 0.5 at 37, above 0.95 at 67, never above 0.995
    assert rule(d, 0.5, "M_u", "p") == 64 and rule(d, 0.5, "M_u", "in") == 37      # p side: 67 > 64; input side: argmax of all-False = 0
    e = np.full(600, 0.0018)                                   # above 0.95 beyond index 512
    assert int(np.argmax(np.cumsum(e) > 0.95)) > 512 and rule(e, 0.95, "M_fU", "p") == 512 and rule(e, 0.95, "M_fU", "in") == 512
    for bad in (("M_x", "p"), ("M_u", "out")):
        with pytest.raises(ValueError):
            rule(a, 0.95, *bad)


def test_artifact_loader_reads_the_more_stems_and_both_maxs(ds):
    c, inputs = ds, ds["inputs"]
    c_in = c4.C_IN[inputs]
    rule = lambda evr, var, side: formats.select_num_pc_chapter4(evr, var, inputs, side)
    m, maxs = surrogate.load_artifacts("chapter5", c["model_path"], c["dir"], 0.95, 0.95, None, "max_abs", c4.SHAPE, c4.AVANCE, c_in, c_in - 1,
                                       pca_stems=("ipca_input_more", "ipca_p_more"), pc_rule=rule)
    assert (m.p_in, m.p_out, m.c_in, m.c_out, m.sdf_ch, m.ov, m.variant) == (24, 24, c_in, 1, c_in - 1, c4.AVANCE, "chapter5")
    assert len(maxs) == (4 if inputs == "M_u" else 3)
    np.testing.assert_allclose(maxs, c4.MAXS[inputs])
    np.testing.assert_array_equal(m.comp_in, c["model"].comp_in)
    np.testing.assert_array_equal(m.comp_out, c["model"].comp_out)
    np.testing.assert_array_equal(m.mean_out, c["model"].mean_out)
    assert (m.in_a, m.out_a) == (c["model"].in_a, c["model"].out_a)                 # maxs_PCA, read as for 'max_abs'
    for (W, b), (W2, b2) in zip(m.weights, c["model"].weights):
        np.testing.assert_array_equal(W, W2); np.testing.assert_array_equal(b, b2)
    with pytest.raises(FileNotFoundError, match="ipca_input"):                      # the defaults are unchanged: the plain stems
        surrogate.load_artifacts("chapter5", c["model_path"], c["dir"], 0.95, 0.95, 128, "max_abs", c4.SHAPE, c4.AVANCE, c_in, c_in - 1)
    ev = evaluator(c)
    assert (ev.pc_in, ev.pc_p, ev.inputs, ev.max_frames) == (24, 24, inputs, 1) and ev._max_abs() == [float(v) for v in c4.MAXS[inputs]]
    other = "M_fU" if inputs == "M_u" else "M_u"
    with pytest.raises(ValueError):                                                 # the other file's artefacts: another channel count
        EvaluationChapter4(c4.DELTA, c4.SHAPE, c4.AVANCE, 0.95, 0.95, c["dataset_path"], c["model_path"], inputs=other, artifact_dir=c["dir"])
    with pytest.raises(ValueError, match="inputs"):
        EvaluationChapter4(c4.DELTA, c4.SHAPE, c4.AVANCE, 0.95, 0.95, c["dataset_path"], c["model_path"], inputs="M_x", artifact_dir=c["dir"])


def test_filter_and_device_prep_are_refused(ds):
    ev = evaluator(ds, max_frames=2)
    with pytest.raises(ValueError, match=r":421.*:457-458"):
        ev.timeStep(0, 0, False, False, True)
    with pytest.raises(ValueError, match=r":421.*:457-458"):
        ev.timeSteps(0, [0, 1], apply_filter=True)
    with pytest.raises(ValueError, match="6 wide"):
        ev.timeSteps(0, [0, 1], device_prep=True)
    with pytest.raises(RuntimeError, match="computeOnlyOnce"):
        ev.timeSteps(0, [0, 1])
    with pytest.raises(ValueError, match=r":421"):
        main_chapter4(hdf5_path=ds["dataset_path"], model_directory=ds["model_path"], inputs=ds["inputs"], artifact_dir=ds["dir"],
                      avance=c4.AVANCE, sims=(0,), n_ts=1, apply_filter=True, frames_per_call=2)


def test_oracle_on_the_mirrors_host_grid_matches_the_reference_run(ds):
    """The mirror's frame preparation + timeStep's statements in NumPy give the fixture's grid (crop bit for bit, sums 1e-13) and
    U_max_norm; oracle.psm_oracle.solve_grid on that grid gives the fixture's field at the tolerance of tests/test_oracle_golden.py;
    error_metrics on it gives the reference's own metric values."""
    c, gold = ds, ds["gold"]
    c_in = c4.C_IN[c["inputs"]]
    grid, U = host_grid(evaluator(c), c, c4.FRAME)
    assert grid.shape == (138, 300, c_in + 1) and float(U) == float(gold["U_max_norm"]) and int(np.count_nonzero(grid[..., c_in - 1])) == int(gold["n_flow"])
    np.testing.assert_array_equal(grid[CROP], gold["grid_crop"])
    np.testing.assert_allclose(grid.sum(axis=(0, 1)), gold["grid_sum"], rtol=0, atol=1e-13 * gold["grid_abs_sum"].max())
    np.testing.assert_allclose(np.abs(grid).sum(axis=(0, 1)), gold["grid_abs_sum"], rtol=1e-13)
    sol = orc.solve_grid(grid[..., :c_in], oracle_model(c["model"]))
    ref = gold["field"]
    assert len(sol.x_blocks) == int(gold["n_blocks"]) == 14 and not np.isnan(ref).any()
    np.testing.assert_allclose(sol.fields[..., 0], ref, rtol=1e-6, atol=1e-6 * np.abs(ref).max())
    m = error_metrics(ref, grid[..., c_in], grid[..., c_in - 1] == 0)
    assert m["normVal"] == float(gold["norm"])
    for key, name in (("biasNorm", "BIAS_norm"), ("rmseNorm", "RMSE_norm"), ("stdeNorm", "STDE_norm"), ("mean_err", "pred_minus_true"),
                      ("mean_sq_err", "pred_minus_true_squared")):
        assert math.isclose(m[key], float(gold[name]), rel_tol=1e-12), (key, m[key], float(gold[name]))


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_gpu_time_step_against_the_reference_run(ds):
    c, gold = ds, ds["gold"]
    c_in = c4.C_IN[c["inputs"]]
    ev = evaluator(c)
    assert ev.computeOnlyOnce(0) == 0
    assert ev.indice == c["N"] and (ev.grid_shape_y, ev.grid_shape_x) == (138, 300) and ev._sur.B == 14 and ev._sur.geometry_bound
    ev.pred_minus_true, ev.pred_minus_true_squared = [], []
    res = ev.timeStep(0, c4.FRAME, False, False, False)
    ref = gold["field"]
    crop = np.abs(ev.grid[CROP] - gold["grid_crop"]).max() / np.abs(gold["grid_crop"]).max()
    sums = np.abs(ev.grid.sum(axis=(0, 1)) - gold["grid_sum"]) / gold["grid_abs_sum"]
    asums = np.abs(np.abs(ev.grid).sum(axis=(0, 1)) - gold["grid_abs_sum"]) / gold["grid_abs_sum"]
    eps = FIELD_TOL * np.abs(ref).max()
    err = np.abs(res - ref).max()
    print(f"{c['inputs']}: U_max_norm {ev.U_max_norm!r} (fixture {float(gold['U_max_norm'])!r}); grid crop {crop:.2e}, sums {sums.max():.2e}, "
          f"abs-sums {asums.max():.2e} (bounds 1e-12); field max |difference| {err:.3e}, eps = {FIELD_TOL} * {np.abs(ref).max():.4f} = {eps:.3e}")
    assert ev.U_max_norm == float(gold["U_max_norm"])
    assert ev.grid.shape == (138, 300, c_in + 1) and crop <= 1e-12 and sums.max() <= 1e-12 and asums.max() <= 1e-12
    assert res.shape == (138, 300) and np.isfinite(res).all() and err <= eps
    assert np.array_equal(ev.no_flow_bool, ev.grid[..., c_in - 1] == 0) and int((~ev.no_flow_bool).sum()) == int(gold["n_flow"])
    assert same_bits(np.ascontiguousarray(ev.cfd_results), np.ascontiguousarray(ev.grid[..., c_in]))
    m, norm = ev.last_metrics["p"], float(gold["norm"])
    rmse_abs = math.sqrt(float(gold["pred_minus_true_squared"])) * norm
    e = 100 * eps / norm
    B, R, S = float(gold["BIAS_norm"]), float(gold["RMSE_norm"]), float(gold["STDE_norm"])
    bounds = dict(mean_err=eps / norm, mean_sq_err=(2 * rmse_abs * eps + eps ** 2) / norm ** 2, biasNorm=e, rmseNorm=e,
                  stdeNorm=((2 * R * e + e ** 2) + (2 * abs(B) * e + e ** 2)) / S)
    want = dict(mean_err=float(gold["pred_minus_true"]), mean_sq_err=float(gold["pred_minus_true_squared"]), biasNorm=B, rmseNorm=R, stdeNorm=S)
    for key in bounds:
        print(f"{c['inputs']} {key}: got {m[key]:.9g}, reference {want[key]:.9g}, |difference| {abs(m[key] - want[key]):.3e} (bound {bounds[key]:.3e})")
    print(f"{c['inputs']} normVal: got {m['normVal']!r}, reference {norm!r}")
    assert all(abs(m[key] - want[key]) <= bounds[key] for key in bounds)
    assert abs(m["normVal"] - norm) <= 1e-12 * norm
    assert ev.pred_minus_true == [m["mean_err"]] and ev.pred_minus_true_squared == [m["mean_sq_err"]] and set(ev.last_metrics) == {"p"}


@pytest.mark.gpu
def test_gpu_batch_against_loop(ds):
    """timeSteps(0, range(3)) with max_frames 1 and 3 returns the fields of three timeStep calls of a second evaluator bit for bit,
    with its lists and attributes; fields=False returns metrics_from_sums of the raw sums chapter4_frames gives for the same
    columns, within twice SUM_TOL's share of error_metrics on the fields."""
    c = ds
    ref = evaluator(c)
    assert ref.computeOnlyOnce(0) == 0
    want, truth, want_m = [], [], []
    for time in range(c4.FRAMES):
        want.append(ref.timeStep(0, time))
        truth.append(np.ascontiguousarray(ref.cfd_results))
        want_m.append(dict(ref.last_metrics["p"]))
    for mf in (1, 3):
        ev = evaluator(c, max_frames=mf)
        assert ev.computeOnlyOnce(0) == 0
        out = ev.timeSteps(0, range(c4.FRAMES))
        same = [same_bits(np.ascontiguousarray(out[i]), np.ascontiguousarray(want[i])) for i in range(c4.FRAMES)]
        print(f"{c['inputs']} max_frames={mf}: fields identical to three timeStep calls {same}; truth of the last frame identical "
              f"{same_bits(np.ascontiguousarray(ev.cfd_results), truth[-1])}; guard trips {ev._sur.guard_trips}")
        assert len(out) == c4.FRAMES and all(same) and ev._sur.max_cases == mf and ev._sur.guard_trips == 0 and ev._sur.geometry_bound
        assert same_bits(np.ascontiguousarray(ev.cfd_results), truth[-1]) and np.array_equal(ev.no_flow_bool, ref.no_flow_bool)
        assert ev.U_max_norm == ref.U_max_norm and ev.last_metrics["p"] == want_m[-1] and set(ev.last_metrics) == {"p"}
        assert ev.pred_minus_true == ref.pred_minus_true and ev.pred_minus_true_squared == ref.pred_minus_true_squared
        got = ev.timeSteps(0, range(c4.FRAMES), fields=False)
        cols = np.stack([ev._frame_prepare(ev._frame_rows(0, t))[1] for t in range(c4.FRAMES)])
        raws = [ev._sur.chapter4_frames(cols[i:i + mf], want_result=False, want_truth=False)[2] for i in range(0, c4.FRAMES, mf)]
        raw = np.concatenate(raws)
        assert ev.cfd_results is None and len(ev.pred_minus_true) == 2 * c4.FRAMES
        flow = ~ref.no_flow_bool
        for i in range(c4.FRAMES):
            assert set(got[i]) == {"p"} and got[i]["p"] == ev._sur.metrics_from_sums(raw[i, 0])
            d = (want[i].astype(np.float64) - truth[i])[flow]
            norm = want_m[i]["normVal"]
            b1, b2 = 2 * SUM_TOL * np.abs(d).mean() / norm, 2 * SUM_TOL * (d * d).mean() / norm ** 2
            e1, e2 = abs(got[i]["p"]["mean_err"] - want_m[i]["mean_err"]), abs(got[i]["p"]["mean_sq_err"] - want_m[i]["mean_sq_err"])
            print(f"{c['inputs']} max_frames={mf} fields=False frame {i}: metrics are metrics_from_sums of the raw row; against error_metrics "
                  f"on the field |D mean_err| {e1:.2e} (bound {b1:.2e}), |D mean_sq_err| {e2:.2e} (bound {b2:.2e}), normVal identical "
                  f"{got[i]['p']['normVal'] == norm}")
            assert e1 <= b1 and e2 <= b2 and got[i]["p"]["normVal"] == norm
            assert ev.pred_minus_true[c4.FRAMES + i] == got[i]["p"]["mean_err"]


@pytest.mark.gpu
def test_gpu_main_chapter4(ds, capsys):
    """main_chapter4 per frame, frames_per_call=3 and fields=False: the summary after the simulation is _summary over the per-frame
    values of its own 'frames'; the batched run repeats the per-frame run's values, the metrics-only run stays within the sums' bound."""
    c = ds
    kw = dict(delta=c4.DELTA, model_directory=c["model_path"], shape=c4.SHAPE, avance=None, var_p=0.95, var_in=0.95, hdf5_path=c["dataset_path"],
              inputs=c["inputs"], sims=(0, 0), n_ts=c4.FRAMES, artifact_dir=c["dir"])
    runs = dict(per_frame=main_chapter4(**kw), batched=main_chapter4(**kw, frames_per_call=3), sums=main_chapter4(**kw, frames_per_call=3, fields=False))
    printed = capsys.readouterr().out
    assert printed.count("BIAS for the sim: ") == 6 and printed.count("STDE for the sim: ") == 6
    for name, out in runs.items():
        fr = out["frames"]
        assert [(f["sim"], f["time"]) for f in fr] == [(0, t) for t in range(c4.FRAMES)] * 2 and len(out["sims"]) == 2
        for k, n in ((0, c4.FRAMES), (1, 2 * c4.FRAMES)):             # over everything accumulated so far
            assert out["sims"][k] == _summary([f["mean_err"] for f in fr[:n]], [f["mean_sq_err"] for f in fr[:n]]), name
        print(f"{c['inputs']} main_chapter4 {name}: {out['sims'][-1]}")
    assert runs["batched"] == runs["per_frame"]
    w, g = runs["per_frame"], runs["sums"]
    worst = max(max(abs(a["mean_err"] - b["mean_err"]) / math.sqrt(b["mean_sq_err"]), abs(a["mean_sq_err"] - b["mean_sq_err"]) / b["mean_sq_err"])
                for a, b in zip(g["frames"], w["frames"]))
    print(f"{c['inputs']} main_chapter4 fields=False against per frame: worst |D mean_err| / rmse, |D mean_sq_err| / mean_sq_err = {worst:.2e} "
          f"(bound {2 * SUM_TOL})")
    assert worst <= 2 * SUM_TOL                                       # mean|d| <= rmse: the bound of test_gpu_batch_against_loop, relaxed to rmse
