"""SDF fold of the bound single-case encode: on a float32 handle whose SDF channel is the last one, a bound
single-case solve contracts the velocity channels only; the SDF channel's share of the coefficients is a constant of the binding
(per-row offset of the input scaler), and the bound-geometry contract becomes the SDF channel's VALUES, checked by the guard riders.

Parity with the general path (fields at the bound path's tolerance, the x_input stage and every later stage against the
stage-isolated float64 oracle), fold on / off, the guard on a grid with the bound pattern but other SDF values, the binding's
lifecycle, and the routes the fold must not touch.  Needs a real MI355X."""
import functools

import numpy as np
import pytest

from oracle import pca_stage_oracle as so
from psm_amd import GridSurrogate, _lib, synthetic
from hipmem import DeviceArray
from test_bound_geometry import same
from test_pca_stage_oracle import _grids, _model, _omodel, launched_kernels

pytestmark = pytest.mark.gpu

# name: (variant, c_in, p_in, p_out, ny, nx, encode family, oracle form)
CASES = {
    "gradp_pair": ("gradp", 3, 128, 128, 256, 256, "psm_encode_pair_kernel", "pair"),
    "deltas_one_tile": ("deltas", 3, 32, 32, 256, 256, "psm_encode_kernel", "f32"),
    "chapter5_c4": ("chapter5", 4, 96, 64, 256, 256, "psm_encode_kernel", "f32"),
    "deltas_odd_nx": ("deltas", 3, 128, 128, 256, 257, "psm_encode_pair_kernel", "pair"),        # unaligned rows (gradp plans > 32 blocks here)
    "deltas_160x288": ("deltas", 3, 128, 128, 160, 288, "psm_encode_pair_kernel", "pair"),
}


@functools.lru_cache(maxsize=None)
def model_of(variant, c_in, p_in, p_out):
    return _model(variant, c_in, p_in, p_out, widths=(512, 512, 512), seed=11)


@functools.lru_cache(maxsize=None)
def grids_of(name):
    """Two grids of one geometry that differ in the velocity channels only, and an all-flow grid (SDF 1 everywhere)."""
    variant, c_in, p_in, p_out, ny, nx = CASES[name][:6]
    sdf = c_in - 1
    g1 = _grids(1, ny, nx, c_in, seed=3)[0]
    g2 = g1.copy()
    rng = np.random.default_rng(5)
    for ch in range(sdf):
        g2[..., ch] = (g1[..., ch] * 0.7 + 0.05 * rng.standard_normal((ny, nx))).astype(np.float32) * (g1[..., sdf] != 0)
    flow = g1.copy()
    flow[..., sdf] = 1.0
    for g in (g1, g2, flow):
        g.setflags(write=False)
    return g1, g2, flow


@functools.lru_cache(maxsize=None)
def general_of(name):
    """General-path fields of the case's three grids on a handle that was never bound: computed once, shared, read-only."""
    variant, c_in, p_in, p_out, ny, nx = CASES[name][:6]
    with GridSurrogate(model_of(variant, c_in, p_in, p_out), ny, nx) as sur:
        out = tuple(sur.solve(g)[0] for g in grids_of(name))
    for f in out:
        f.setflags(write=False)
    return out


def scaled_sdf(g, sdf):
    """The same flow-cell pattern, the SDF values scaled by 1.01 on the flow cells."""
    b = g.copy()
    b[..., sdf] = (g[..., sdf] * np.float32(1.01)).astype(np.float32)
    assert np.array_equal(b[..., sdf] != 0, g[..., sdf] != 0) and not np.array_equal(b[..., sdf], g[..., sdf])
    return b


@pytest.mark.parametrize("name", list(CASES))
def test_parity_with_the_general_path(name, monkeypatch):
    variant, c_in, p_in, p_out, ny, nx, family, form = CASES[name]
    monkeypatch.setenv("PSM_KEEP_HIDDEN", "1")
    model = model_of(variant, c_in, p_in, p_out)
    g1, g2, flow = grids_of(name)
    want1, want2, want_flow = general_of(name)
    with GridSurrogate(model, ny, nx) as sur:
        assert sur.bind_geometry(g1)
        d_out = DeviceArray(shape=(1, ny, nx, model.c_out))
        for g, want in ((g1, want1), (g2, want2)):
            d_in = DeviceArray(g[None])
            names = launched_kernels(sur, d_in.ptr, 1, d_out.ptr)
            assert [n.split("<")[0] for n in names if "encode" in n] == [family], names
            same(d_out.numpy()[0], want)
            st = dict(x_input=sur.stage("x_input", 1), res=sur.stage("res", 1), block_pred=None,
                      hidden=[sur.stage("hidden", 1, layer=l) for l in range(len(model.weights) - 1)])
            res = so.check_solve(_omodel(model), g[None], st, form, 1, False)      # x_input: the full scaled coefficients, SDF part included
            assert res[0].name == "encode" and not [r for r in res if not r.ok], res
            same(sur.solve(g)[0], want)
            d_in.free()
        d_out.free()
        assert sur.guard_trips == 0 and sur.geometry_bound
        assert sur.bind_geometry(flow)
        got = sur.solve(flow)[0]
        assert np.array_equal(np.isnan(got), np.isnan(want_flow))
        same(got, want_flow)
        assert sur.guard_trips == 0


@pytest.mark.parametrize("name", ["gradp_pair", "deltas_one_tile"])
def test_fold_on_and_off(name, monkeypatch):
    variant, c_in, p_in, p_out, ny, nx, family, form = CASES[name]
    model = model_of(variant, c_in, p_in, p_out)
    g1, g2, _ = grids_of(name)
    want2 = general_of(name)[1]
    d_in, d_out = DeviceArray(g2[None]), DeviceArray(shape=(1, ny, nx, model.c_out))
    enc, fields = {}, {}
    for fold in ("1", "0"):
        monkeypatch.setenv("PSM_SDF_FOLD", fold)
        with GridSurrogate(model, ny, nx) as sur:
            assert sur.bind_geometry(g1)
            names = launched_kernels(sur, d_in.ptr, 1, d_out.ptr)
            enc[fold] = [n for n in names if "encode" in n]
            fields[fold] = d_out.numpy()[0].copy()
            same(fields[fold], want2)
            np.testing.assert_array_equal(sur.solve(g2)[0], fields[fold])
    assert enc["1"] == enc["0"] and len(enc["1"]) == 1 and enc["1"][0].startswith(family + "<")
    # plain launches and a captured graph, fold on
    monkeypatch.setenv("PSM_SDF_FOLD", "1")
    for graph in ("0", "1"):
        monkeypatch.setenv("PSM_GRAPH", graph)
        with GridSurrogate(model, ny, nx) as sur:
            assert sur.bind_geometry(g1)
            for _ in range(3):
                sur.solve_device(d_in.ptr, 1, d_out.ptr, 0)
            sur.synchronize()
            np.testing.assert_array_equal(d_out.numpy()[0], fields["1"])
            # the switch is part of the sequence key: the graph captured with the fold is not replayed without it
            monkeypatch.setenv("PSM_SDF_FOLD", "0")
            sur.solve_device(d_in.ptr, 1, d_out.ptr, 0)
            sur.synchronize()
            np.testing.assert_array_equal(d_out.numpy()[0], fields["0"])
            monkeypatch.setenv("PSM_SDF_FOLD", "1")
    d_in.free(); d_out.free()


def test_guard_compares_the_sdf_values():
    name = "gradp_pair"
    variant, c_in, p_in, p_out, ny, nx = CASES[name][:6]
    model = model_of(variant, c_in, p_in, p_out)
    a = grids_of(name)[0]
    b = scaled_sdf(a, c_in - 1)
    nan_b = a.copy(); nan_b[7, 9, c_in - 1] = np.nan
    with GridSurrogate(model, ny, nx) as ref:
        want_b = ref.solve(b)[0]
    with GridSurrogate(model, ny, nx) as sur:
        # host entry: the general-path field of b, one trip, binding dropped
        assert sur.bind_geometry(a)
        assert np.isfinite(sur.solve(a)[0]).all() and sur.guard_trips == 0
        got = sur.solve(b)[0]
        assert sur.guard_trips == 1 and not sur.geometry_bound
        assert "not the one bound" in _lib.last_error(sur.h)
        np.testing.assert_array_equal(got, want_b)
        # device entry: NaN everywhere, PSM_ERR_GEOMETRY at synchronize
        assert sur.bind_geometry(a)
        d_b, d_out = DeviceArray(b[None]), DeviceArray(shape=(1, ny, nx, model.c_out))
        sur.solve_device(d_b.ptr, 1, d_out.ptr, 0)
        with pytest.raises(_lib.PsmError) as e:
            sur.synchronize()
        assert e.value.code == -7
        assert np.isnan(d_out.numpy()).all()
        assert sur.guard_trips == 2 and not sur.geometry_bound
        d_b.free(); d_out.free()
        # a NaN in the SDF channel of the solved grid is a mismatch
        assert sur.bind_geometry(a)
        sur.solve(nan_b)
        assert sur.guard_trips == 3 and not sur.geometry_bound
        # one ring ticket
        assert sur.bind_geometry(a)
        t = sur.submit(b)
        f = sur.wait(t)[0]
        assert sur.guard_trips == 4 and not sur.geometry_bound
        np.testing.assert_array_equal(f, want_b)
        # the host-side check of the wrapper compares values too: the binding goes before the solve, no trip
        assert sur.bind_geometry(a)
        sur.check_bound = True
        np.testing.assert_array_equal(sur.solve(b)[0], want_b)
        assert sur.guard_trips == 4 and not sur.geometry_bound


@pytest.mark.parametrize("name", ["deltas_one_tile", "chapter5_c4"])
def test_fold_is_taken_on_the_one_tile_arm(name, monkeypatch):
    """psm_encode_kernel's arm: the same pattern with other SDF values trips the guard when the fold is taken and only then
    (with PSM_SDF_FOLD=0 the contract is the pattern, and the bound solve of that grid is a valid one)."""
    variant, c_in, p_in, p_out, ny, nx = CASES[name][:6]
    model = model_of(variant, c_in, p_in, p_out)
    a = grids_of(name)[0]
    b = scaled_sdf(a, c_in - 1)
    with GridSurrogate(model, ny, nx) as ref:
        want_b = ref.solve(b)[0]
    with GridSurrogate(model, ny, nx) as sur:
        assert sur.bind_geometry(a)
        got = sur.solve(b)[0]
        assert sur.guard_trips == 1 and not sur.geometry_bound
        np.testing.assert_array_equal(got, want_b)
        monkeypatch.setenv("PSM_SDF_FOLD", "0")
        assert sur.bind_geometry(a)
        same(sur.solve(b)[0], want_b)
        assert sur.guard_trips == 1 and sur.geometry_bound


def test_lifecycle():
    name = "deltas_one_tile"
    variant, c_in, p_in, p_out, ny, nx = CASES[name][:6]
    model = model_of(variant, c_in, p_in, p_out)
    a = grids_of(name)[0]
    b = _grids(1, ny, nx, c_in, seed=3)[0]
    other = synthetic.channel_grid(ny, nx, seed=3, cx=0.6, cy=0.4, r=0.1).astype(np.float32)
    b[..., c_in - 1] = other[..., 2]
    b[..., :c_in - 1] *= (b[..., c_in - 1:] != 0)
    assert not np.array_equal(a[..., c_in - 1] != 0, b[..., c_in - 1] != 0)
    with GridSurrogate(model, ny, nx) as ref:
        want_a, want_b = ref.solve(a)[0], ref.solve(b)[0]
    with GridSurrogate(model, ny, nx) as sur:
        assert sur.bind_geometry(a)
        same(sur.solve(a)[0], want_a)
        assert sur.bind_geometry(b)
        same(sur.solve(b)[0], want_b)
        assert sur.guard_trips == 0
        sur.unbind_geometry()
        np.testing.assert_array_equal(sur.solve(a)[0], want_a)
        np.testing.assert_array_equal(sur.solve(b)[0], want_b)


def _fields_both_settings(monkeypatch, make, solve):
    out = []
    for fold in ("1", "0"):
        monkeypatch.setenv("PSM_SDF_FOLD", fold)
        with make() as sur:
            out.append(solve(sur))
    return out


def test_routes_outside_the_scope_are_untouched(monkeypatch):
    """An SDF channel that is not the last one, a bf16 handle, a bound 8-case batch and an unbound handle never take the fold:
    bit-identical fields with and without PSM_SDF_FOLD=0."""
    g = synthetic.channel_grid(256, 256, seed=4).astype(np.float32)

    def bound(grid):
        def run(sur):
            assert sur.bind_geometry(grid)
            return sur.solve(grid)
        return run

    first = synthetic.make_model("deltas", p_in=32, p_out=32)          # SDF in channel 0 of three
    first.sdf_ch = 0
    g_first = np.ascontiguousarray(g[..., [2, 0, 1]])
    m = synthetic.make_model("deltas", p_in=32, p_out=32)
    batch = synthetic.random_obstacle_cases(8, 256, 256, seed=3).astype(np.float32)
    for make, solve in ((lambda: GridSurrogate(first, 256, 256), bound(g_first)),
                        (lambda: GridSurrogate(m, 256, 256, precision="bf16"), bound(g)),
                        (lambda: GridSurrogate(m, 256, 256, max_cases=8), bound(batch)),
                        (lambda: GridSurrogate(m, 256, 256), lambda sur: sur.solve(g))):
        on, off = _fields_both_settings(monkeypatch, make, solve)
        np.testing.assert_array_equal(on, off)
