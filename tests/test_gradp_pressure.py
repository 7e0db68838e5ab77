"""U -> p on the device for the gradP variant: psm_bind_integration once, then psm_integrate_gradp_device /
psm_solve_pressure_device / psm_solve_pressure per step (csrc/psm_integ.hip: two launches for a whole case batch).

Oracle: orc.integrate_gradp / orc.solve_grid in float64.  Bounds are the project's own for this operation: 1e-4 * max|p| for
the integration alone (test_mesh_path.py), 2e-4 * max|p| for solve + integration against the oracle chain
(test_dataset_evaluator.py).  The reference hard-wires row 200 for the cut; the synthetic obstacles do not cross it, so the
cut is passed explicitly by the rule of `cut_of`.  Every GPU test prints the ratios it measured before it asserts."""
import ctypes as C
import re

import numpy as np
import pytest

import cases
from hipmem import DeviceArray, hip
from oracle import psm_oracle as orc
from psm_amd import GridSurrogate, _lib, synthetic

NEW_ENTRIES = ("psm_bind_integration", "psm_unbind_integration", "psm_integrate_gradp_device", "psm_solve_pressure_device",
               "psm_solve_pressure")
INTEG_TOL, CHAIN_TOL = 1e-4, 2e-4

SINGLE = {(256, 256, 1): (128, 76), (272, 288, 11): (136, 85), (300, 300, 12): (150, 89)}    # (ny, nx, seed) -> cut
BATCH_CUTS = [(151, 75), (123, 60), (98, 126), (122, 103), (111, 148), (112, 122), (113, 81), (126, 110)]


def cut_of(sdf):
    """(cy, cx): middle row of the obstacle's rows (rounded up), middle column of the obstacle on that row."""
    solid = sdf == 0
    rows = np.where(solid.any(1))[0]
    cy = int((rows.min() + rows.max() + 1) // 2)
    cols = np.where(solid[cy])[0]
    return cy, int((cols.min() + cols.max()) // 2)


def oracle_model(m):
    sc = orc.Scaler(m.scaler_kind, m.in_a, m.in_b, m.out_a, m.out_b)
    return orc.Model(m.variant, m.c_in, m.c_out, m.comp_in, m.mean_in, m.comp_out, m.mean_out, m.weights, sc, m.out_scale,
                     m.S, m.ov, m.sdf_ch)


def oracle_gradp(grid, model, scale=1.0):
    return orc.solve_grid(grid.astype(np.float32).astype(np.float64), oracle_model(model)).fields * scale


def oracle_p(gradp, sdf, cut):
    ny, nx = sdf.shape
    return orc.integrate_gradp(np.asarray(gradp, np.float64), sdf, 1.0 / nx, 1.0 / ny, cut[0], cut[1])


def ratio(got, ref):
    assert np.isfinite(ref).all() and np.isfinite(got).all()
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def bind(sur, grids, cuts):
    g = np.asarray(grids)
    ny, nx = g.shape[-3:-1]
    cuts = np.asarray(cuts).reshape(-1, 2)
    return sur.bind_integration(g[..., 2], cuts[:, 0], cuts[:, 1], 1.0 / nx, 1.0 / ny)


# ---------------------------------------------------------------------------------------------------------------- 1
def test_new_entries_are_declared_bound_and_exported():
    """Every new name is in psm.h, in _lib.SIGNATURES and exported by the built library."""
    txt = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(psm_[a-z_0-9]+)\s*\(", txt))
    lib = _lib.load()
    for name in NEW_ENTRIES:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    for name in ("bind_integration", "unbind_integration", "integrate_device", "solve_pressure", "solve_pressure_device"):
        assert callable(getattr(GridSurrogate, name, None)), name


def test_the_cut_rule_gives_the_cuts_the_cases_were_checked_with():
    for (ny, nx, seed), cut in SINGLE.items():
        assert cut_of(synthetic.channel_grid(ny, nx, seed=seed)[..., 2]) == cut
    batch = synthetic.random_obstacle_cases(8, 256, 256, seed=3)
    assert [cut_of(g[..., 2]) for g in batch] == BATCH_CUTS
    assert cut_of(synthetic.channel_grid(200, 1500, seed=41)[..., 2]) == (100, 449)
    assert int((synthetic.channel_grid(256, 256, seed=1)[..., 2] == 1.0).sum()) == 40      # the quirk's second fix-up index


# ---------------------------------------------------------------------------------------------------------------- 2
def _wide_case():
    ny, nx = 200, 1500
    sdf = synthetic.channel_grid(ny, nx, seed=41)[..., 2]
    yy, xx = np.meshgrid(np.linspace(0.0, 1.0, ny), np.linspace(0.0, 7.5, nx), indexing="ij")
    rng = np.random.default_rng(5)
    gx = 3 * np.cos(3 * xx) * np.cos(2 * yy) + 0.05 * rng.standard_normal((ny, nx))
    gy = -2 * np.sin(3 * xx) * np.sin(2 * yy) + 0.05 * rng.standard_normal((ny, nx))
    gp = np.stack([gx, gy], -1)
    gp[sdf == 0] = 0.0
    return sdf, gp, cut_of(sdf), 7.5 / (nx - 1), 1.0 / (ny - 1)


def _integrate_on_device(sur, gradp):
    d_g = DeviceArray(np.asarray(gradp, np.float32)[None])
    d_p = DeviceArray(shape=(1,) + gradp.shape[:2], dtype=np.float32)
    sur.integrate_device(d_g.ptr, 1, d_p.ptr, 0)
    sur.synchronize()
    p = d_p.numpy()[0]
    d_g.free(); d_p.free()
    return p


@pytest.mark.gpu
def test_gpu_integration_alone_device_in_device_out():
    """Golden 320 x 384 case against the reference's own p, its sd2 variant (second fix-up index) against the oracle, the old
    host entry on the same input within the same bound; and a 200 x 1500 grid whose row sides span 8 / 17 chunks of a wave.
    Worst ratios observed on the MI355X (bound 1e-4): golden 4.1e-7, sd2 4.0e-7, host entry 4.1e-7, wide 4.0e-7."""
    ic = cases.build_integration_case()
    ny, nx = ic["sdfunct"].shape
    cx, cy = orc.integration_center(ic["sdfunct"], ic["min_x"], ic["max_x"], ic["X0"].min(), ic["delta"])
    dx, dy = (ic["max_x"] - ic["min_x"]) / (nx - 1), (ic["max_y"] - ic["min_y"]) / (ny - 1)
    gold = cases.load_golden("gradp_integration_320x384")
    model = synthetic.make_model("gradp", p_in=8, p_out=8)
    with GridSurrogate(model, ny, nx) as sur:
        assert sur.bind_integration(ic["sdfunct"], cy, cx, dx, dy)
        r_gold = ratio(_integrate_on_device(sur, ic["gradP"]), gold["p"])
        sur.set_integration(ic["sdfunct"], cy, cx, dx, dy)               # the old host entry: its own, independent geometry
        r_host = ratio(sur.integrate_gradp(ic["gradP"]), gold["p"])
        sd2 = ic["sdfunct"].copy()
        sd2[10:40, 50:90] = 1.2
        assert sur.bind_integration(sd2, cy, cx, dx, dy)
        ref2 = orc.integrate_gradp(ic["gradP"], sd2, dx, dy, cy, cx)
        r_sd2 = ratio(_integrate_on_device(sur, ic["gradP"]), ref2)
        r_host_gold_again = ratio(sur.integrate_gradp(ic["gradP"]), gold["p"])      # untouched by the second bind
    sdf, gp, cut, wdx, wdy = _wide_case()
    assert cut == (100, 449)
    ref = orc.integrate_gradp(gp, sdf, wdx, wdy, cut[0], cut[1])
    assert abs(np.abs(ref).max() - 1.51) < 0.01
    with GridSurrogate(model, 200, 1500) as sur:
        assert sur.bind_integration(sdf, cut[0], cut[1], wdx, wdy)
        r_wide = ratio(_integrate_on_device(sur, gp), ref)
    print(f"integration alone: golden {r_gold:.2e} sd2 {r_sd2:.2e} host entry {r_host:.2e} / {r_host_gold_again:.2e} wide {r_wide:.2e}")
    assert max(r_gold, r_sd2, r_host, r_host_gold_again, r_wide) <= INTEG_TOL


# ---------------------------------------------------------------------------------------------------------------- 3
def _solve_pressure_with_own_gradient(sur, grid, n=1, out_scale=None):
    """p and the solve's own gradient through psm_solve_pressure_device."""
    g = np.ascontiguousarray(np.asarray(grid, np.float32).reshape((n,) + grid.shape[-3:]))
    d_in = DeviceArray(g)
    d_g = DeviceArray(shape=g.shape[:3] + (2,), dtype=np.float32)
    d_p = DeviceArray(shape=g.shape[:3], dtype=np.float32)
    sur.solve_pressure_device(d_in.ptr, n, d_p.ptr, d_gradp=d_g.ptr, out_scale=out_scale)
    sur.synchronize()
    p, gp = d_p.numpy(), d_g.numpy()
    for d in (d_in, d_g, d_p):
        d.free()
    return p, gp


@pytest.mark.gpu
@pytest.mark.parametrize("pcs", [32, 128])
@pytest.mark.parametrize("ny,nx,seed", list(SINGLE))
def test_gpu_solve_pressure_single_case(ny, nx, seed, pcs):
    """psm_solve_pressure on the general path and on a bound geometry against integrate_gradp(solve_grid(...)) (2e-4), and the
    device's p against the oracle's integration of the device's OWN gradient (1e-4).
    Worst ratios observed on the MI355X over the six cases: chain 7.2e-7, stage-isolated 1.5e-7."""
    grid = synthetic.channel_grid(ny, nx, seed=seed)
    cut = SINGLE[(ny, nx, seed)]
    model = synthetic.make_model("gradp", p_in=pcs, p_out=pcs)
    ref = oracle_p(oracle_gradp(grid, model), grid[..., 2], cut)
    with GridSurrogate(model, ny, nx) as sur:
        assert bind(sur, grid, cut)
        for path in ("general", "bound"):
            if path == "bound":
                assert sur.bind_geometry(grid) and sur.geometry_bound
            p = sur.solve_pressure(grid)[0]
            p_dev, gp_dev = _solve_pressure_with_own_gradient(sur, grid)
            r_chain, r_dev = ratio(p, ref), ratio(p_dev[0], ref)
            r_stage = ratio(p_dev[0], oracle_p(gp_dev[0], grid[..., 2], cut))
            same = sur.solve(grid)[0]                                            # d_gradp is the field the solve entries write
            assert np.abs(gp_dev[0] - same).max() <= 1e-6 * np.abs(same).max()
            print(f"solve_pressure {ny}x{nx} p={pcs} {path}: chain {r_chain:.2e} / {r_dev:.2e} stage {r_stage:.2e} max|p| {np.abs(ref).max():.4f}")
            assert max(r_chain, r_dev) <= CHAIN_TOL and r_stage <= INTEG_TOL
        assert sur.guard_trips == 0


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.gpu
def test_gpu_solve_pressure_case_batch():
    """Eight cases, one geometry and one cut per slot: every case within the bounds of the single-case test, with and without a
    per-case out_scale, and case i of the batch against a single-case handle on grid i (1e-4).
    Worst ratios observed on the MI355X: chain 1.05e-6, stage-isolated 1.4e-7, batch against single 8.1e-7."""
    grids = synthetic.random_obstacle_cases(8, 256, 256, seed=3)
    cuts = [cut_of(g[..., 2]) for g in grids]
    assert cuts == BATCH_CUTS
    model = synthetic.make_model("gradp", p_in=32, p_out=32)
    scale = np.linspace(0.5, 2.25, 8)
    gp_ref = [oracle_gradp(g, model) for g in grids]
    worst = {"chain": 0.0, "stage": 0.0, "single": 0.0}
    with GridSurrogate(model, 256, 256, max_cases=8) as sur:
        assert bind(sur, grids, cuts)
        assert sur.bind_geometry(grids) and sur.geometry_bound
        for sc in (None, scale):
            p = sur.solve_pressure(grids, out_scale=sc)
            p_dev, gp_dev = _solve_pressure_with_own_gradient(sur, grids, n=8, out_scale=sc)
            for i in range(8):
                ref = oracle_p(gp_ref[i] * (1.0 if sc is None else sc[i]), grids[i, ..., 2], cuts[i])
                worst["chain"] = max(worst["chain"], ratio(p[i], ref), ratio(p_dev[i], ref))
                worst["stage"] = max(worst["stage"], ratio(p_dev[i], oracle_p(gp_dev[i], grids[i, ..., 2], cuts[i])))
        p_batch = sur.solve_pressure(grids)
        assert sur.guard_trips == 0
    for i in range(8):
        with GridSurrogate(model, 256, 256) as one:
            assert bind(one, grids[i], cuts[i])
            assert one.bind_geometry(grids[i])
            worst["single"] = max(worst["single"], ratio(p_batch[i], one.solve_pressure(grids[i])[0]))
    print("case batch: " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert worst["chain"] <= CHAIN_TOL and worst["stage"] <= INTEG_TOL and worst["single"] <= INTEG_TOL


# ---------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.gpu
def test_gpu_solve_pressure_is_stream_ordered():
    """Grid written by an asynchronous H2D copy on a caller stream, psm_solve_pressure_device on that stream, asynchronous D2H on
    that stream, ONE synchronise at the end; two steps with different velocities back to back give two different, correct
    fields.  Worst ratio observed on the MI355X: 6.6e-7."""
    h = hip()
    h.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    h.hipStreamSynchronize.argtypes = [C.c_void_p]
    h.hipStreamDestroy.argtypes = [C.c_void_p]
    h.hipHostMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.c_uint]
    h.hipHostFree.argtypes = [C.c_void_p]
    h.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    ny = nx = 256
    g1 = synthetic.channel_grid(ny, nx, seed=1)
    g2 = g1.copy()
    g2[..., :2] *= 0.6                                                   # same geometry, other velocities
    cut = SINGLE[(256, 256, 1)]
    model = synthetic.make_model("gradp", p_in=32, p_out=32)
    refs = [oracle_p(oracle_gradp(g, model), g[..., 2], cut) for g in (g1, g2)]
    n_in, n_out = ny * nx * 3 * 4, ny * nx * 4
    pin = [C.c_void_p() for _ in range(4)]                               # pinned: grid 1, grid 2, p 1, p 2
    for k, nb in enumerate((n_in, n_in, n_out, n_out)):
        assert h.hipHostMalloc(C.byref(pin[k]), nb, 0) == 0
    views = [np.ctypeslib.as_array(C.cast(pin[k], C.POINTER(C.c_float)), shape=s) for k, s in enumerate(((ny, nx, 3),) * 2 + ((ny, nx),) * 2)]
    views[0][...] = g1
    views[1][...] = g2
    views[2][...] = np.nan
    views[3][...] = np.nan
    st = C.c_void_p()
    assert h.hipStreamCreate(C.byref(st)) == 0
    d_in = [DeviceArray(shape=(1, ny, nx, 3), dtype=np.float32) for _ in range(2)]
    d_p = [DeviceArray(shape=(1, ny, nx), dtype=np.float32) for _ in range(2)]
    try:
        with GridSurrogate(model, ny, nx) as sur:
            assert bind(sur, g1, cut)
            assert sur.bind_geometry(g1)
            for k in range(2):
                assert h.hipMemcpyAsync(d_in[k].ptr, pin[k], n_in, 1, st) == 0
                sur.solve_pressure_device(d_in[k].ptr, 1, d_p[k].ptr, stream=st.value)
                assert h.hipMemcpyAsync(pin[2 + k], d_p[k].ptr, n_out, 2, st) == 0
            assert h.hipStreamSynchronize(st) == 0
            sur.synchronize()
            got = [views[2].copy(), views[3].copy()]
            assert sur.guard_trips == 0
    finally:
        for d in d_in + d_p:
            d.free()
        h.hipStreamDestroy(st)
        for q in pin:
            h.hipHostFree(q)
    r = [ratio(got[k], refs[k]) for k in range(2)]
    differ = float(np.abs(got[0] - got[1]).max() / np.abs(refs[0]).max())
    print(f"stream order: step 1 {r[0]:.2e} step 2 {r[1]:.2e}, the two fields differ by {differ:.2e} of max|p|")
    assert max(r) <= CHAIN_TOL and differ > 0.05


# ---------------------------------------------------------------------------------------------------------------- 6
@pytest.mark.gpu
def test_gpu_integration_state_and_geometry_errors():
    grid = synthetic.channel_grid(256, 256, seed=1)
    cut = SINGLE[(256, 256, 1)]
    model = synthetic.make_model("gradp", p_in=16, p_out=16)
    d_g = DeviceArray(shape=(2, 256, 256, 2), dtype=np.float32)
    d_p = DeviceArray(shape=(2, 256, 256), dtype=np.float32)

    def state_error(call):
        with pytest.raises(_lib.PsmError) as e:
            call()
        assert e.value.code == -2, e.value
        return str(e.value)

    with GridSurrogate(model, 256, 256, max_cases=2) as sur:
        want = sur.solve(grid)[0]
        assert "psm_bind_integration" in state_error(lambda: sur.integrate_device(d_g.ptr, 1, d_p.ptr))      # before the bind
        state_error(lambda: sur.solve_pressure(grid))
        assert bind(sur, grid, cut)
        assert "n_cases" in state_error(lambda: sur.integrate_device(d_g.ptr, 2, d_p.ptr))                   # bound: one case
        state_error(lambda: sur.solve_pressure(np.stack([grid, grid])))
        with pytest.raises(_lib.PsmError) as e:
            sur.integrate_device(0, 1, d_p.ptr)
        assert e.value.code == -1                                                                          # PSM_ERR_ARG
        assert np.isfinite(sur.solve_pressure(grid)).all()
        # unequal flow-cell counts on the cut columns (the obstacle's first column: 121 against 128) as ONE case of two
        sd = grid[..., 2]
        assert int((sd[:128, 45] != 0).sum()) == 121 and int((sd[:128, 44] != 0).sum()) == 128
        assert int((sd[128:, 45] != 0).sum()) == 121 and int((sd[128:, 44] != 0).sum()) == 128
        assert not sur.bind_integration(np.stack([sd, sd]), [cut[0], 128], [cut[1], 45], 1 / 256, 1 / 256)
        msg = _lib.last_error(sur.h)
        assert "case 1" in msg and "flow-cell counts" in msg
        assert "psm_bind_integration" in state_error(lambda: sur.solve_pressure(grid))                       # nothing bound
        np.testing.assert_array_equal(sur.solve(grid)[0], want)                                            # the solve is unaffected
        # a re-plan after the bind drops the binding
        assert bind(sur, grid, cut)
        assert sur.lib.psm_plan_grid(sur.h, 256, 256) == 0
        assert "psm_bind_integration" in state_error(lambda: sur.solve_pressure(grid))
        assert bind(sur, grid, cut)
        sur.unbind_integration()
        state_error(lambda: sur.integrate_device(d_g.ptr, 1, d_p.ptr))
    with GridSurrogate(synthetic.make_model("deltas", p_in=16, p_out=16), 256, 256) as one:                # c_out == 1
        with pytest.raises(_lib.PsmError) as e:
            one.bind_integration(grid[..., 2], cut[0], cut[1], 1 / 256, 1 / 256)
        assert e.value.code == -2 and "c_out" in str(e.value)
        with pytest.raises(_lib.PsmError) as e:
            one.integrate_device(d_g.ptr, 1, d_p.ptr)
        assert e.value.code == -2
    d_g.free(); d_p.free()
