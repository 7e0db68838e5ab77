"""Gaussian post-steps of assemble_prediction on the device (SM_call.py:352-363; csrc/psm_filter.hip): psm_bind_poststeps once,
then psm_filter_fields_device / psm_poststeps_device / psm_solve_poststeps_device / psm_solve_poststeps per step -- one launch per
separable pass for a whole case batch, at most four with the deltaU-change weighting.

Oracle: scipy.ndimage.gaussian_filter in float64 (the routine the reference calls); orc.solve_grid for the solve.  Bounds are the
project's own for these operations: 2e-6 absolute for the filter alone on unit-normal input (test_mesh_path.py), 1e-4 * max|reference|
for the post-step chain (test_mesh_path.py), 2e-4 * max(|want|, |field|) for solve + post-steps (test_poisson_features.py).  Every
GPU test prints what it measured before it asserts."""
import ctypes as C
import re

import numpy as np
import pytest
import scipy.ndimage as ndi

import cases
from hipmem import DeviceArray
from oracle import psm_oracle as orc
from psm_amd import GridSurrogate, _lib, synthetic
from test_oracle_golden import oracle_model

NEW_ENTRIES = ("psm_bind_poststeps", "psm_unbind_poststeps", "psm_filter_fields_device", "psm_poststeps_device",
               "psm_solve_poststeps_device", "psm_solve_poststeps")
NEW_METHODS = ("bind_poststeps", "unbind_poststeps", "filter_device", "poststeps_device", "solve_poststeps_device", "solve_poststeps")
FILTER_TOL, CHAIN_TOL, SOLVE_TOL = 2e-6, 1e-4, 2e-4
SIGMAS = ((10, 10), (50, 50), (2.5, 7.0))
S_FIELD, S_WEIGHT = (10, 10), (50, 50)


def gauss(f, sigma):
    return ndi.gaussian_filter(np.asarray(f, np.float64), sigma=sigma, order=0)


def chain(field, dU, prev, apply_filter):
    """(result, change, next) of SM_call.py:352-363 / :843-848 in float64."""
    res = gauss(field, S_FIELD) if apply_filter else np.asarray(field, np.float64)
    chg = gauss((res - prev) * gauss(dU, S_WEIGHT), S_FIELD)
    return res, chg, prev + chg


def rel(got, ref, scale=None):
    assert np.isfinite(ref).all() and np.isfinite(got).all()
    return float(np.abs(got - ref).max() / (np.abs(ref).max() if scale is None else scale))


def dev(a):
    return DeviceArray(np.ascontiguousarray(a, np.float32))


def free(*arrs):
    for d in arrs:
        d.free()


# ---------------------------------------------------------------------------------------------------------------- 1
def test_new_entries_are_declared_bound_and_exported():
    """Every new name is in psm.h, in _lib.SIGNATURES and exported by the built library; the GridSurrogate mirror exists."""
    txt = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(psm_[a-z_0-9]+)\s*\(", txt))
    lib = _lib.load()
    for name in NEW_ENTRIES:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    for name in NEW_METHODS:
        assert callable(getattr(GridSurrogate, name, None)), name


# NaN at the centre and near a corner, where the window reflects at both edges.  (2, 2) is two pixels from the corner along both
# axes: 21 x 57 + 13 x 31 = 1600 NaN outputs for sigma (2.5, 7) (radii 10 and 28).  The count of 1617 on record for this case
# (= 1197 + 14 x 30) belongs to the corner pixel (3, 1); both placements are checked.
NAN_CASES = {(2, 2): 1600, (3, 1): 1617}


def _nan_field(corner):
    f = np.random.default_rng(11).standard_normal((138, 300)).astype(np.float32)
    f[69, 150] = np.nan
    f[corner] = np.nan
    return f


def test_the_nan_cases_are_the_ones_that_were_counted():
    for corner, count in NAN_CASES.items():
        assert int(np.isnan(gauss(_nan_field(corner), (2.5, 7.0))).sum()) == count


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.gpu
@pytest.mark.parametrize("variant,ny,nx,n", [("deltas", 138, 300, 1), ("gradp", 256, 256, 3)])
def test_gpu_filter_alone_device_in_device_out(variant, ny, nx, n):
    """138 x 300: radius 200 wraps the 138 rows twice, 300 is no multiple of the 64-wide strip.  256 x 256 x 2 channels x 3 cases:
    channel and case strides.  Out of place and in place against SciPy (2e-6 on unit-normal input); case i of the batch is
    bit-identical to the same field filtered alone."""
    model = synthetic.make_model(variant, p_in=8, p_out=8)
    c = model.c_out
    f = np.random.default_rng(3).standard_normal((n, ny, nx, c)).astype(np.float32)
    worst = 0.0
    with GridSurrogate(model, ny, nx, max_cases=n) as sur:
        d_in, d_out, d_one = dev(f), DeviceArray(shape=f.shape), DeviceArray(shape=f.shape[1:])
        for sig in SIGMAS:
            sur.bind_poststeps(sig, S_WEIGHT)
            ref = np.stack([np.stack([gauss(f[i, ..., k], sig) for k in range(c)], -1) for i in range(n)])
            sur.filter_device(d_in.ptr, n, d_out.ptr)
            sur.synchronize()
            got = d_out.numpy()
            err = float(np.abs(got - ref).max())
            d_ip = dev(f)
            sur.filter_device(d_ip.ptr, n, d_ip.ptr)                  # in place
            sur.synchronize()
            inplace_same = np.array_equal(d_ip.numpy(), got)
            d_ip.free()
            alone_same = True
            for i in range(n):
                sur.filter_device(d_in.ptr + i * f[0].nbytes, 1, d_one.ptr)
                sur.synchronize()
                alone_same = alone_same and np.array_equal(d_one.numpy(), got[i])
            print(f"filter alone {ny}x{nx}x{c} n={n} sigma={sig}: max |got - scipy| {err:.2e}, in place identical {inplace_same}, case alone identical {alone_same}")
            worst = max(worst, err)
            assert err <= FILTER_TOL and inplace_same and alone_same
        free(d_in, d_out, d_one)
    print(f"filter alone {ny}x{nx}: worst {worst:.2e} (bound {FILTER_TOL})")


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.gpu
def test_gpu_filter_nan_pattern_is_scipys():
    """Plain tap sums: an output is NaN exactly where SciPy's is (1600 / 1617 outputs for two NaN pixels on 138 x 300, sigma (2.5, 7))."""
    with GridSurrogate(synthetic.make_model("deltas", p_in=8, p_out=8), 138, 300) as sur:
        sur.bind_poststeps((2.5, 7.0), S_WEIGHT)
        for corner, count in NAN_CASES.items():
            f = _nan_field(corner)
            ref = gauss(f, (2.5, 7.0))
            want = np.isnan(ref)
            d = dev(f[None])
            sur.filter_device(d.ptr, 1, d.ptr)
            sur.synchronize()
            got = d.numpy()[0]
            host = sur.gaussian_filter(f, (2.5, 7.0))                  # the host entry runs on the same kernels
            d.free()
            print(f"NaN at {corner}: device {int(np.isnan(got).sum())}, host entry {int(np.isnan(host).sum())}, scipy {int(want.sum())}")
            assert int(want.sum()) == count
            assert np.array_equal(np.isnan(got), want) and np.array_equal(np.isnan(host), want)
            assert np.abs(got[~want] - ref[~want]).max() <= FILTER_TOL


# ---------------------------------------------------------------------------------------------------------------- 4
def _poststeps(sur, fields, dU, prev, apply_filter, change=True, nxt=True, alias=False):
    """psm_poststeps_device on fresh device buffers -> (result, change | None, next | None)."""
    n = fields.shape[0]
    d_f, d_u, d_p = dev(fields), dev(dU), dev(prev)
    d_r = d_f if alias else DeviceArray(shape=fields.shape)
    d_c = DeviceArray(shape=fields.shape) if change else None
    d_n = DeviceArray(shape=fields.shape) if nxt else None
    sur.poststeps_device(d_f.ptr, n, d_r.ptr, apply_filter, d_u.ptr, d_p.ptr, d_c.ptr if change else 0, d_n.ptr if nxt else 0)
    sur.synchronize()
    out = (d_r.numpy(), d_c.numpy() if change else None, d_n.numpy() if nxt else None)
    free(*{id(d): d for d in (d_f, d_u, d_p, d_r, d_c, d_n) if d is not None}.values())
    return out


@pytest.mark.gpu
def test_gpu_poststeps_against_the_reference_run():
    """cases.build_filter_case() against the reference's own result / change (deltas_filters_256x256.npz) at 1e-4 * max|reference|."""
    grid, model, bp, dU, dPprev = cases.build_filter_case()
    gold = cases.load_golden("deltas_filters_256x256")
    lay = orc.block_layout("deltas", *grid.shape[:2])
    field = orc.assemble_deltas(bp, orc.extract_blocks(grid, lay, 3), lay).field
    with GridSurrogate(synthetic.make_model("deltas", p_in=8, p_out=8), 256, 256) as sur:
        sur.bind_poststeps(S_FIELD, S_WEIGHT)
        res, chg, nxt = _poststeps(sur, field[None], dU[None], dPprev[None], True)
    r_res, r_chg = rel(res[0], gold["result"]), rel(chg[0], gold["change"])
    r_nxt = rel(nxt[0], dPprev + gold["change"])
    print(f"post-steps against the reference run: result {r_res:.2e} change {r_chg:.2e} next {r_nxt:.2e} (bound {CHAIN_TOL})")
    assert max(r_res, r_chg, r_nxt) <= CHAIN_TOL


@pytest.mark.gpu
def test_gpu_poststeps_case_batch_and_optional_outputs():
    """Three random cases on 160 x 200 against the SciPy chain, apply_filter on and off; next == prev + change in float32; either
    of change / next left out; the result written over the input field."""
    rng = np.random.default_rng(21)
    n, ny, nx = 3, 160, 200
    fields = rng.standard_normal((n, ny, nx)).astype(np.float32)
    dU = np.abs(rng.standard_normal((n, ny, nx))).astype(np.float32)
    dU /= dU.max()
    prev = (0.3 * rng.standard_normal((n, ny, nx))).astype(np.float32)
    worst = 0.0
    with GridSurrogate(synthetic.make_model("deltas", p_in=8, p_out=8), ny, nx, max_cases=n) as sur:
        sur.bind_poststeps(S_FIELD, S_WEIGHT)
        for af in (True, False):
            res, chg, nxt = _poststeps(sur, fields, dU, prev, af)
            for i in range(n):
                want = chain(fields[i], dU[i], prev[i], af)
                r = [rel(g[i], w) for g, w in zip((res, chg, nxt), want)]
                print(f"post-steps batch case {i} apply_filter={af}: result {r[0]:.2e} change {r[1]:.2e} next {r[2]:.2e}")
                worst = max(worst, *r)
            if not af:
                assert np.array_equal(res, fields)                        # the unfiltered field is handed on as it is
            assert np.array_equal(nxt, prev + chg)                        # one float32 add
            only_c = _poststeps(sur, fields, dU, prev, af, nxt=False)
            only_n = _poststeps(sur, fields, dU, prev, af, change=False)
            alias = _poststeps(sur, fields, dU, prev, af, alias=True)
            assert only_c[2] is None and only_n[1] is None
            for other in (only_c, only_n, alias):
                assert np.array_equal(other[0], res)
            assert np.array_equal(only_c[1], chg) and np.array_equal(only_n[2], nxt)
            assert np.array_equal(alias[1], chg) and np.array_equal(alias[2], nxt)
            one = _poststeps(sur, fields[1:2], dU[1:2], prev[1:2], af)   # case 1 alone: bit-identical
            assert all(np.array_equal(a[0], b[1]) for a, b in zip(one, (res, chg, nxt)))
    print(f"post-steps batch: worst {worst:.2e} (bound {CHAIN_TOL})")
    assert worst <= CHAIN_TOL


# ---------------------------------------------------------------------------------------------------------------- 5
def _solve_poststeps(sur, grids, dU, prev, apply_filter, out_scale=None):
    """psm_solve_poststeps_device on fresh device buffers -> (result, change, next), each [n,Ny,Nx]."""
    n = grids.shape[0]
    d_g, d_u, d_p = dev(grids), dev(dU), dev(prev)
    outs = [DeviceArray(shape=dU.shape) for _ in range(3)]
    sur.solve_poststeps_device(d_g.ptr, n, outs[0].ptr, apply_filter, d_u.ptr, d_p.ptr, outs[1].ptr, outs[2].ptr, out_scale=out_scale)
    sur.synchronize()
    got = tuple(o.numpy() for o in outs)
    free(d_g, d_u, d_p, *outs)
    return got


def _solved_field(sur, grids, out_scale=None):
    n = grids.shape[0]
    d_g, d_f = dev(grids), DeviceArray(shape=grids.shape[:3] + (1,))
    sur.solve_device(d_g.ptr, n, d_f.ptr, out_scale=out_scale)
    sur.synchronize()
    f = d_f.numpy()[..., 0]
    free(d_g, d_f)
    return f


def _check_solve_chain(tag, sur, grids, fields_ref, dU, prev, out_scale=None):
    """Both apply_filter settings: against oracle solve + SciPy (2e-4) and, stage-isolated, SciPy on the device's own field (1e-4)."""
    n = grids.shape[0]
    own = _solved_field(sur, grids, out_scale)
    worst = [0.0, 0.0]
    for af in (True, False):
        got = _solve_poststeps(sur, grids, dU, prev, af, out_scale)
        for i in range(n):
            want = chain(fields_ref[i], dU[i], prev[i], af)
            iso = chain(own[i], dU[i], prev[i], af)
            fmax = np.abs(fields_ref[i]).max()
            r_chain = max(rel(g[i], w, max(np.abs(w).max(), fmax)) for g, w in zip(got, want))
            r_iso = max(rel(g[i], w) for g, w in zip(got, iso))
            print(f"solve + post-steps {tag} case {i} apply_filter={af}: chain {r_chain:.2e} stage-isolated {r_iso:.2e}")
            worst = [max(worst[0], r_chain), max(worst[1], r_iso)]
    assert worst[0] <= SOLVE_TOL and worst[1] <= CHAIN_TOL
    return worst


def _step_inputs(shape, seed):
    rng = np.random.default_rng(seed)
    dU = np.abs(rng.standard_normal(shape)).astype(np.float32)
    dU /= dU.max()
    return dU, (0.1 * rng.standard_normal(shape)).astype(np.float32)


@pytest.mark.gpu
def test_gpu_solve_poststeps_deltas_single_case():
    """Deltas at 256 x 256 on the general and on the geometry-bound path, with and without out_scale; a second step with new dU and
    prev through the same captured graph gives the new result."""
    grid = synthetic.delta_grid(256, 256, seed=2).astype(np.float32)
    model = synthetic.make_model("deltas", p_in=16, p_out=16)
    ref = orc.solve_grid(grid.astype(np.float64), oracle_model(model)).fields[None, ..., 0]
    dU, prev = _step_inputs((1, 256, 256), 9)
    with GridSurrogate(model, 256, 256) as sur:
        sur.bind_poststeps(S_FIELD, S_WEIGHT)
        for path in ("general", "bound"):
            if path == "bound":
                assert sur.bind_geometry(grid) and sur.geometry_bound
            for sc in (None, 1.75):
                _check_solve_chain(f"deltas {path} out_scale={sc}", sur, grid[None], ref * (sc or 1.0), dU, prev,
                                   None if sc is None else [sc])
        # same buffers, same graph, new contents
        d_g, d_u, d_p = dev(grid[None]), dev(dU), dev(prev)
        outs = [DeviceArray(shape=dU.shape) for _ in range(3)]
        step = lambda: (sur.solve_poststeps_device(d_g.ptr, 1, outs[0].ptr, True, d_u.ptr, d_p.ptr, outs[1].ptr, outs[2].ptr),
                        sur.synchronize(), [o.numpy() for o in outs])[2]
        first = step()
        dU2, prev2 = _step_inputs((1, 256, 256), 10)
        lib = _lib.load()
        for d, a in ((d_u, dU2), (d_p, prev2)):
            assert lib.psm_debug_copy_to_device(d.ptr, a.ctypes.data, a.nbytes) == 0
        second = step()
        want = chain(ref[0], dU2[0], prev2[0], True)
        r2 = max(rel(g[0], w, max(np.abs(w).max(), np.abs(ref).max())) for g, w in zip(second, want))
        moved = float(np.abs(second[2] - first[2]).max())
        print(f"second step through the same graph: chain {r2:.2e}, next moved by {moved:.2e}")
        assert r2 <= SOLVE_TOL and moved > 0.01 and np.array_equal(first[0], second[0])
        assert sur.guard_trips == 0
        free(d_g, d_u, d_p, *outs)


def _model4():
    m = synthetic.make_model("deltas", p_in=16, p_out=16, c_in=4, seed_pca=777, seed_w=5)
    m.sdf_ch = 3
    return m


@pytest.mark.gpu
def test_gpu_solve_poststeps_poisson_handle():
    """The 4-channel Poisson handle (mask = channel 3) on cases.build_poisson_case(), 160 x 200."""
    c = cases.build_poisson_case()
    model = _model4()
    grid, _ = orc.poisson_features(c["ux"], c["uy"], c["dux"], c["duy"], c["sdfunct"], c["L"], c["U"], c["k"], c["max_abs"])
    om = oracle_model(model)
    om.out_scale = 0.51 * c["U"] ** 2
    ref = orc.solve_grid(grid, om).fields[None, ..., 0]
    dU, prev = _step_inputs((1, 160, 200), 9)
    with GridSurrogate(model, 160, 200) as sur:
        sur.bind_poststeps(S_FIELD, S_WEIGHT)
        g = sur.poisson_features(c["ux"], c["uy"], c["dux"], c["duy"], c["sdfunct"], c["L"], c["U"], c["k"], c["max_abs"])
        _check_solve_chain("poisson", sur, g[None], ref, dU, prev, [0.51 * c["U"] ** 2])


@pytest.mark.gpu
def test_gpu_solve_poststeps_case_batch():
    """Three deltas cases in one replay; case i is bit-identical to a one-case call on grid i."""
    grids = np.stack([synthetic.delta_grid(256, 256, seed=2, step=s) for s in range(3)]).astype(np.float32)
    model = synthetic.make_model("deltas", p_in=16, p_out=16)
    om = oracle_model(model)
    ref = np.stack([orc.solve_grid(g.astype(np.float64), om).fields[..., 0] for g in grids])
    dU, prev = _step_inputs((3, 256, 256), 12)
    with GridSurrogate(model, 256, 256, max_cases=3) as sur:
        sur.bind_poststeps(S_FIELD, S_WEIGHT)
        _check_solve_chain("batch", sur, grids, ref, dU, prev)
        batch = _solve_poststeps(sur, grids, dU, prev, True)
        one = _solve_poststeps(sur, grids[2:3], dU[2:3], prev[2:3], True)
        own3, own1 = _solved_field(sur, grids), _solved_field(sur, grids[2:3])
    if np.array_equal(own3[2], own1[0]):                                  # the solve itself is not promised bit-identical across batch sizes
        assert all(np.array_equal(b[2], o[0]) for b, o in zip(batch, one))
    else:
        assert max(rel(b[2], o[0]) for b, o in zip(batch, one)) <= CHAIN_TOL


# ---------------------------------------------------------------------------------------------------------------- 6
@pytest.mark.gpu
def test_gpu_host_entry_equals_the_device_path():
    """psm_solve_poststeps (host buffers, synchronous) gives the device path's result bit for bit, with the weighting and filter-only,
    and on the two-channel gradP handle (filter only)."""
    grid = synthetic.delta_grid(256, 256, seed=2).astype(np.float32)
    dU, prev = _step_inputs((1, 256, 256), 9)
    with GridSurrogate(synthetic.make_model("deltas", p_in=16, p_out=16), 256, 256) as sur:
        sur.bind_poststeps(S_FIELD, S_WEIGHT)
        for af in (True, False):
            want = _solve_poststeps(sur, grid[None], dU, prev, af, [1.5])
            res, chg, nxt = sur.solve_poststeps(grid, af, dU, prev, out_scale=[1.5])
            same = [np.array_equal(res[..., 0], want[0]), np.array_equal(chg, want[1]), np.array_equal(nxt, want[2])]
            print(f"host entry apply_filter={af}: identical to the device path {same}")
            assert all(same)
        res, chg, nxt = sur.solve_poststeps(grid, True)                   # filter only
        assert chg is None and nxt is None and np.array_equal(res[..., 0], _solve_poststeps(sur, grid[None], dU, prev, True)[0])
    g3 = synthetic.channel_grid(256, 256, seed=1).astype(np.float32)
    with GridSurrogate(synthetic.make_model("gradp", p_in=16, p_out=16), 256, 256) as sur:
        sur.bind_poststeps(S_FIELD, S_WEIGHT)
        res, _, _ = sur.solve_poststeps(g3, True)
        plain = sur.solve(g3)
        err = max(float(np.abs(res[0, ..., k] - gauss(plain[0, ..., k], S_FIELD)).max()) for k in range(2))
        print(f"gradP host entry, filter only: max |got - scipy(own field)| {err:.2e} of max|field| {np.abs(plain).max():.2e}")
        assert err <= CHAIN_TOL * np.abs(plain).max()


# ---------------------------------------------------------------------------------------------------------------- 7
def _free_bytes():
    import hipmem
    h = hipmem.hip()
    h.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    assert h.hipDeviceSynchronize() == 0
    free_b, total = C.c_size_t(), C.c_size_t()
    assert h.hipMemGetInfo(C.byref(free_b), C.byref(total)) == 0
    return free_b.value


@pytest.mark.gpu
def test_gpu_poststeps_errors_and_lifetime():
    grid = synthetic.delta_grid(256, 256, seed=2).astype(np.float32)
    d_a, d_b = DeviceArray(shape=(2, 256, 256, 2)), DeviceArray(shape=(2, 256, 256, 2))

    def error(code, call):
        with pytest.raises(_lib.PsmError) as e:
            call()
        assert e.value.code == code, e.value
        return str(e.value)

    with GridSurrogate(synthetic.make_model("deltas", p_in=16, p_out=16), 256, 256, max_cases=2) as sur:
        want = sur.solve(grid)[0]
        assert "psm_bind_poststeps" in error(-2, lambda: sur.filter_device(d_a.ptr, 1, d_b.ptr))               # before the bind
        error(-2, lambda: sur.poststeps_device(d_a.ptr, 1, d_b.ptr, True, d_a.ptr, d_a.ptr))
        error(-2, lambda: sur.solve_poststeps(grid, True))
        for bad in ((0.0, 10.0), (10.0, -1.0), (2e4, 10.0), (float("nan"), 10.0)):
            error(-1, lambda: sur.bind_poststeps(bad, S_WEIGHT))                                               # PSM_ERR_ARG
            error(-1, lambda: sur.bind_poststeps(S_FIELD, bad))
        error(-2, lambda: sur.filter_device(d_a.ptr, 1, d_b.ptr))                                              # a refused bind binds nothing
        sur.bind_poststeps(S_FIELD, S_WEIGHT)
        error(-1, lambda: sur.filter_device(d_a.ptr, 3, d_b.ptr))                                              # n_cases > max_cases
        error(-1, lambda: sur.filter_device(0, 1, d_b.ptr))
        error(-1, lambda: sur.poststeps_device(d_a.ptr, 1, d_b.ptr, True, d_a.ptr, 0))                         # dU without prev
        assert np.isfinite(sur.solve_poststeps(grid, True)[0]).all()
        assert sur.lib.psm_plan_grid(sur.h, 256, 256) == 0                                                   # a re-plan drops the binding
        assert "psm_bind_poststeps" in error(-2, lambda: sur.solve_poststeps(grid, True))
        sur.bind_poststeps(S_FIELD, S_WEIGHT)
        sur.unbind_poststeps()
        error(-2, lambda: sur.filter_device(d_a.ptr, 1, d_b.ptr))
        np.testing.assert_array_equal(sur.solve(grid)[0], want)                                              # the solve is unaffected
        sur.bind_poststeps(S_FIELD, S_WEIGHT)                                                                # no leak over bind / unbind
        sur.solve_poststeps(grid, True)
        sur.unbind_poststeps()
        before = _free_bytes()
        for _ in range(5):
            sur.bind_poststeps(S_FIELD, S_WEIGHT)
            sur.solve_poststeps(grid, True)
            sur.unbind_poststeps()
        after = _free_bytes()
        print(f"device memory over 5 bind / step / unbind cycles: {before - after} bytes")
        assert before - after < (2 << 20)
    with GridSurrogate(synthetic.make_model("gradp", p_in=16, p_out=16), 256, 256) as two:                     # c_out == 2
        two.bind_poststeps(S_FIELD, S_WEIGHT)
        two.filter_device(d_a.ptr, 1, d_b.ptr)                                                               # filter only: any c_out
        two.synchronize()
        assert "c_out" in error(-2, lambda: two.poststeps_device(d_a.ptr, 1, d_b.ptr, True, d_a.ptr, d_a.ptr))
        assert "c_out" in error(-2, lambda: two.solve_poststeps_device(d_a.ptr, 1, d_b.ptr, True, d_a.ptr, d_a.ptr))
    free(d_a, d_b)


# ---------------------------------------------------------------------------------------------------------------- 8
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3])
def test_gpu_poststeps_take_at_most_four_launches(n):
    """psm_time_kernels on a deltas handle with post-steps bound stamps the step of psm_solve_poststeps_device with the weighting:
    at most 4 dispatches of the psm_gauss1d_kernel family per step, whatever the batch."""
    steps = 3
    grids = np.stack([synthetic.delta_grid(256, 256, seed=2, step=s) for s in range(n)]).astype(np.float32)
    with GridSurrogate(synthetic.make_model("deltas", p_in=16, p_out=16), 256, 256, max_cases=n) as sur:
        d_g, d_f = dev(grids), DeviceArray(shape=(n, 256, 256, 1))
        cap = 64
        names, ms, cnt, nk = C.create_string_buffer(cap * 64), (C.c_double * cap)(), (C.c_int64 * cap)(), C.c_int32()

        def launches():
            sur._chk(sur.lib.psm_time_kernels(sur.h, C.c_void_p(d_g.ptr), n, C.c_void_p(d_f.ptr), steps, names, ms, cnt, cap, C.byref(nk)))
            assert nk.value <= cap
            return {names.raw[k * 64:(k + 1) * 64].split(b"\0", 1)[0].decode(): cnt[k] for k in range(nk.value)}
        before = launches()
        sur.bind_poststeps(S_FIELD, S_WEIGHT)
        after = launches()
        free(d_g, d_f)
    fam = {k: v for k, v in after.items() if k.startswith("psm_gauss1d_kernel")}
    print(f"n={n}: filter dispatches over {steps} steps {fam}; solve dispatches {sum(before.values())}")
    assert not any(k.startswith("psm_gauss1d_kernel") for k in before)
    assert fam and all(v % steps == 0 for v in fam.values())
    assert 0 < sum(fam.values()) // steps <= 4
    assert sum(after.values()) - sum(fam.values()) == sum(before.values())        # the solve's own launches are the same
