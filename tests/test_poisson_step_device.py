"""pressureSM_Poisson time step on the device (SM_call.py:588-848): psm_bind_features once, then psm_features_device (the two
feature launches for a whole case batch, per-step scalars read from device memory) and psm_poisson_step_device / psm_poisson_step
(features -> 4-channel deltas solve -> Gaussian post-steps as one graph replay).

Inputs: three cases at 138 x 300 (41 400 pixels = 161 full 256-pixel workgroups + 184 pixels: the tail workgroup of every case is
partly idle) with three obstacles, velocity scales, L and U, so per-case strides, statistics and scalars all differ; case 2 carries
three NaN velocities.  Plus cases.build_poisson_case() (160 x 200) with the reference's own image (poisson_features_160x200).

Oracle: orc.poisson_features -> orc.solve_grid -> scipy.ndimage.gaussian_filter in float64.  Bounds are the project's own:
3e-7 * max|reference| for the image (test_poisson_features.py: one float32 rounding of float64 arithmetic), 2e-4 * max(|want|, |field|)
for solve + post-steps (SOLVE_TOL of test_poststeps_device.py).  Every GPU test prints what it measured before it asserts."""
import functools
import re

import numpy as np
import pytest
import scipy.ndimage as ndi

import cases
from hipmem import DeviceArray
from oracle import psm_oracle as orc
from psm_amd import GridSurrogate, _lib, synthetic
from test_oracle_golden import oracle_model

NEW_ENTRIES = ("psm_bind_features", "psm_unbind_features", "psm_features_device", "psm_poisson_step_device", "psm_poisson_step")
NEW_METHODS = ("bind_features", "unbind_features", "features_device", "poisson_step_device", "poisson_step")
FEATURE_TOL, SOLVE_TOL = 3e-7, 2e-4
S_FIELD, S_WEIGHT = (10, 10), (50, 50)
NY, NX, N = 138, 300, 3
K, MAX_ABS = 0.5, (2.7, 0.031, 0.027, 0.29)
P_SCALE = 0.51                                            # max_abs_delta_p: out_scale = P_SCALE * U^2 (SM_call.py:816)
BRANCHES = ((1254, 38471, 1675), (0, 40605, 795), (0, 41233, 167))   # pixels below / inside / above mean +- k std, per case
NAN_AT = (("ux", 5, 7), ("dux", 100, 250), ("uy", 137, 299))


# ------------------------------------------------------------------------------------------------------- inputs, computed once
@functools.lru_cache(maxsize=None)
def inputs():
    out = []
    for i in range(N):
        kw = dict(obstacle=("circle", "rectangle", "plate")[i], cx=0.25 + 0.15 * i, cy=0.4 + 0.1 * i, r=0.08 + 0.03 * i)
        g = synthetic.channel_grid(NY, NX, seed=61 + i, **kw)
        d = synthetic.delta_grid(NY, NX, seed=71 + i, step=2 + i, **kw)
        sdf = 0.3 * g[..., 2]
        c = dict(ux=(1.3 + 0.4 * i) * g[..., 0], uy=(1.3 + 0.4 * i) * g[..., 1], dux=0.05 * d[..., 0], duy=0.05 * d[..., 1])
        for a in c.values():
            a[sdf == 0] = 0.0
        if i == 2:
            for name, y, x in NAN_AT:
                c[name][y, x] = np.nan
        c.update(sdfunct=sdf, L=0.25 + 0.1 * i, U=float(np.nanmax(np.sqrt(c["ux"] ** 2 + c["uy"] ** 2))), k=K, max_abs=MAX_ABS)
        out.append(c)
    return tuple(out)


def oracle_image(c):
    return orc.poisson_features(c["ux"], c["uy"], c["dux"], c["duy"], c["sdfunct"], c["L"], c["U"], c["k"], c["max_abs"])


@functools.lru_cache(maxsize=None)
def oracle_images():
    return tuple(oracle_image(c)[0] for c in inputs())


@functools.lru_cache(maxsize=None)
def model4():
    m = synthetic.make_model("deltas", p_in=48, p_out=40, c_in=4, seed_pca=777, seed_w=5)
    m.sdf_ch = 3
    return m


@functools.lru_cache(maxsize=None)
def oracle_fields():
    """orc.solve_grid of every oracle image with out_scale = P_SCALE * U^2, float64 [N][NY][NX]."""
    om = oracle_model(model4())
    out = []
    for c, img in zip(inputs(), oracle_images()):
        om.out_scale = P_SCALE * c["U"] ** 2
        out.append(orc.solve_grid(img, om).fields[..., 0])
    return tuple(out)


@functools.lru_cache(maxsize=None)
def step_inputs():
    rng = np.random.default_rng(9)
    dU = np.abs(rng.standard_normal((N, NY, NX))).astype(np.float32)
    dU /= dU.max()
    return dU, (0.1 * rng.standard_normal((N, NY, NX))).astype(np.float32)


def vel_planes(cs):
    return np.ascontiguousarray(np.stack([np.stack([c["ux"], c["uy"], c["dux"], c["duy"]]) for c in cs]), dtype=np.float64)


def lu_of(cs):
    return np.array([[c["L"], c["U"]] for c in cs], np.float64)


def scales(cs):
    return [P_SCALE * c["U"] ** 2 for c in cs]


def gauss(f, sigma):
    return ndi.gaussian_filter(np.asarray(f, np.float64), sigma=sigma, order=0)


def chain(field, dU, prev, apply_filter):
    """(result, change, next) of SM_call.py:352-363 / :843-848 in float64."""
    res = gauss(field, S_FIELD) if apply_filter else np.asarray(field, np.float64)
    chg = gauss((res - prev) * gauss(dU, S_WEIGHT), S_FIELD)
    return res, chg, prev + chg


def rel(got, ref, scale):
    assert np.isfinite(ref).all() and np.isfinite(got).all()
    return float(np.abs(got - ref).max() / scale)


def dev32(a):
    return DeviceArray(np.ascontiguousarray(a, np.float32))


def free(*arrs):
    for d in arrs:
        d.free()


def error(code, call):
    with pytest.raises(_lib.PsmError) as e:
        call()
    assert e.value.code == code, e.value
    return str(e.value)


def surrogate(n=N, ny=NY, nx=NX):
    return GridSurrogate(model4(), ny, nx, max_cases=n)


def bind_all(sur, cs):
    sur.bind_poststeps(S_FIELD, S_WEIGHT)
    sur.bind_features(np.stack([c["sdfunct"] for c in cs]), K, MAX_ABS)


def step_device(sur, d_vel, n, lu, sc, af, d_u, d_p):
    """psm_poisson_step_device on fresh output buffers -> (result, change, next) [n,NY,NX]."""
    outs = [DeviceArray(shape=(n, sur.ny, sur.nx)) for _ in range(3)]
    sur.poisson_step_device(d_vel.ptr, n, lu, outs[0].ptr, af, d_u.ptr, d_p.ptr, outs[1].ptr, outs[2].ptr, out_scale=sc)
    sur.synchronize()
    got = tuple(o.numpy() for o in outs)
    free(*outs)
    return got


def step_by_hand(sur, d_vel, n, lu, sc, af, d_u, d_p):
    """psm_features_device into a buffer of the test's, then psm_solve_poststeps_device on it -> (result, change, next), image."""
    d_img = DeviceArray(shape=(n, sur.ny, sur.nx, 4))
    outs = [DeviceArray(shape=(n, sur.ny, sur.nx)) for _ in range(3)]
    sur.features_device(d_vel.ptr, n, lu, d_img.ptr)
    sur.solve_poststeps_device(d_img.ptr, n, outs[0].ptr, af, d_u.ptr, d_p.ptr, outs[1].ptr, outs[2].ptr, out_scale=sc)
    sur.synchronize()
    got, img = tuple(o.numpy() for o in outs), d_img.numpy()
    free(d_img, *outs)
    return got, img


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


def test_the_inputs_are_the_ones_that_were_counted():
    """The reference alone stays finite on all three cases and every branch of the transform is taken: 1254 / 38 471 / 1675 pixels
    below / inside / above the central range in case 0, none below in cases 1 and 2.  41 400 pixels leave a tail workgroup."""
    assert NY * NX == 161 * 256 + 184
    for i, c in enumerate(inputs()):
        grid, term = oracle_image(c)
        lo, hi = term.mean() - K * term.std(), term.mean() + K * term.std()
        got = (int((term < lo).sum()), int(((term >= lo) & (term <= hi)).sum()), int((term > hi).sum()))
        assert np.isfinite(grid).all() and got == BRANCHES[i], (i, got)
    c2 = inputs()[2]
    assert all(np.isnan(c2[name][y, x]) and c2["sdfunct"][y, x] != 0 for name, y, x in NAN_AT)
    assert len({c["U"] for c in inputs()}) == 3


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.gpu
def test_gpu_features_device_case_batch():
    """Three cases in one call: image i is the host entry's on case i bit for bit and within 3e-7 * max of the oracle; NaN inputs
    give 0; channel 3 is float32(sdf / 0.29); two of the three bound cases write nothing past the second image."""
    cs = inputs()
    with surrogate() as sur:
        sur.bind_features(np.stack([c["sdfunct"] for c in cs]), K, MAX_ABS)      # the features alone need no post-step binding
        d_vel, d_img = DeviceArray(vel_planes(cs)), DeviceArray(shape=(N, NY, NX, 4))
        sur.features_device(d_vel.ptr, N, lu_of(cs), d_img.ptr)
        sur.synchronize()
        got = d_img.numpy()
        for i, c in enumerate(cs):
            host = sur.poisson_features(c["ux"], c["uy"], c["dux"], c["duy"], c["sdfunct"], c["L"], c["U"], K, MAX_ABS)
            ref = oracle_images()[i]
            same, err = np.array_equal(got[i], host), float(np.abs(got[i] - ref).max() / np.abs(ref).max())
            sdf_same = np.array_equal(got[i, ..., 3], (c["sdfunct"] / MAX_ABS[3]).astype(np.float32))
            print(f"features case {i}: identical to the host entry {same}, |got - oracle| / max {err:.2e} (bound {FEATURE_TOL}), "
                  f"SDF channel exact {sdf_same}")
            assert same and err <= FEATURE_TOL and sdf_same
        # a NaN delta-velocity is that pixel's 0; a NaN velocity zeroes the source term there and next to it (all within the bound above)
        nan_out = float(got[2, 100, 250, 1])
        print(f"channel 1 at the NaN delta-velocity: {nan_out}; image finite {bool(np.isfinite(got).all())}")
        assert np.isfinite(got).all() and nan_out == 0.0
        sentinel = np.full((N, NY, NX, 4), -7.5, np.float32)
        d_two = DeviceArray(sentinel)
        sur.features_device(d_vel.ptr, 2, lu_of(cs[:2]), d_two.ptr)
        sur.synchronize()
        two = d_two.numpy()
        print(f"two of three cases: first two images identical {np.array_equal(two[:2], got[:2])}, third untouched {bool((two[2] == -7.5).all())}")
        assert np.array_equal(two[:2], got[:2]) and (two[2] == -7.5).all()
        free(d_vel, d_img, d_two)


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.gpu
def test_gpu_features_device_against_the_reference_run():
    """One case at 160 x 200 against the reference's own image (poisson_features_160x200.npz)."""
    c, gold = cases.build_poisson_case(), cases.load_golden("poisson_features_160x200")
    with surrogate(1, 160, 200) as sur:
        sur.bind_features(c["sdfunct"], c["k"], c["max_abs"])
        d_vel, d_img = DeviceArray(vel_planes([c])), DeviceArray(shape=(1, 160, 200, 4))
        sur.features_device(d_vel.ptr, 1, [[c["L"], c["U"]]], d_img.ptr)
        sur.synchronize()
        got = d_img.numpy()[0]
        free(d_vel, d_img)
    err = float(np.abs(got - gold["grid"]).max() / np.abs(gold["grid"]).max())
    print(f"features against the reference run: {err:.2e} (bound {FEATURE_TOL})")
    assert err <= FEATURE_TOL


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.gpu
def test_gpu_replay_carries_the_scalars():
    """The same buffers twice through psm_poisson_step_device with (L, U) and out_scale changed in between: the second call has
    the first one's graph key, and still gives the composition by hand with ITS values."""
    cs = inputs()
    dU, prev = step_inputs()
    with surrogate() as sur:
        bind_all(sur, cs)
        d_vel, d_u, d_p = DeviceArray(vel_planes(cs)), dev32(dU), dev32(prev)
        outs = [DeviceArray(shape=(N, NY, NX)) for _ in range(3)]
        results = []
        for lu, sc in ((lu_of(cs), scales(cs)), (lu_of(cs) * np.array([1.5, 0.8]), [1.7 * s for s in scales(cs)])):
            sur.poisson_step_device(d_vel.ptr, N, lu, outs[0].ptr, True, d_u.ptr, d_p.ptr, outs[1].ptr, outs[2].ptr, out_scale=sc)
            sur.synchronize()
            got = [o.numpy() for o in outs]
            want, _ = step_by_hand(sur, d_vel, N, lu, sc, True, d_u, d_p)
            same = [np.array_equal(g, w) for g, w in zip(got, want)]
            print(f"step with L, U = {lu.tolist()}: identical to features_device -> solve_poststeps_device {same}")
            assert all(same) and np.isfinite(got[0]).all()
            results.append(got)
        moved = float(np.abs(results[1][0] - results[0][0]).max())
        print(f"second call through the same graph: result moved by {moved:.3e}")
        assert moved > 0 and not np.array_equal(results[0][2], results[1][2])
        free(d_vel, d_u, d_p, *outs)


# ---------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.gpu
def test_gpu_poisson_step_device_case_batch():
    """Three cases with the weighting, apply_filter both ways, on the general and on the geometry-bound path: the composition by
    hand bit for bit, the float64 chain within 2e-4; then three steps with next handed on as prev."""
    cs = inputs()
    dU, prev = step_inputs()
    lu, sc = lu_of(cs), scales(cs)
    fields = oracle_fields()
    with surrogate() as sur:
        bind_all(sur, cs)
        d_vel, d_u, d_p = DeviceArray(vel_planes(cs)), dev32(dU), dev32(prev)
        d_bind = None
        for path in ("general", "bound"):
            if path == "bound":
                _, img = step_by_hand(sur, d_vel, N, lu, sc, True, d_u, d_p)
                d_bind = DeviceArray(img)
                assert sur.bind_geometry(d_bind.ptr, on_device=True, n_cases=N) and sur.geometry_bound
            for af in (True, False):
                got = step_device(sur, d_vel, N, lu, sc, af, d_u, d_p)
                want, _ = step_by_hand(sur, d_vel, N, lu, sc, af, d_u, d_p)
                same = [np.array_equal(g, w) for g, w in zip(got, want)]
                worst = 0.0
                for i in range(N):
                    ref = chain(fields[i], dU[i], prev[i], af)
                    fmax = np.abs(fields[i]).max()
                    worst = max(worst, *(rel(g[i], w, max(np.abs(w).max(), fmax)) for g, w in zip(got, ref)))
                print(f"poisson step {path} apply_filter={af}: identical to the composition by hand {same}, chain {worst:.2e} (bound {SOLVE_TOL})")
                assert all(same) and worst <= SOLVE_TOL
        assert sur.guard_trips == 0 and sur.geometry_bound
        # three steps, next -> prev through ping-pong buffers
        d_res, d_chg = DeviceArray(shape=(N, NY, NX)), DeviceArray(shape=(N, NY, NX))
        pp = [d_p, DeviceArray(shape=(N, NY, NX))]
        ref_prev = [prev[i].astype(np.float64) for i in range(N)]
        for s in range(3):
            sur.poisson_step_device(d_vel.ptr, N, lu, d_res.ptr, True, d_u.ptr, pp[s & 1].ptr, d_chg.ptr, pp[(s + 1) & 1].ptr, out_scale=sc)
            sur.synchronize()
            nxt = pp[(s + 1) & 1].numpy()
            worst = 0.0
            for i in range(N):
                _, _, ref_prev[i] = chain(fields[i], dU[i], ref_prev[i], True)
                worst = max(worst, rel(nxt[i], ref_prev[i], max(np.abs(ref_prev[i]).max(), np.abs(fields[i]).max())))
            print(f"step {s} of 3 with next fed back: {worst:.2e} (bound {SOLVE_TOL})")
            assert worst <= SOLVE_TOL
        assert sur.guard_trips == 0
        free(d_vel, d_u, d_res, d_chg, d_bind, *pp)


# ---------------------------------------------------------------------------------------------------------------- 6
@pytest.mark.gpu
def test_gpu_host_entry_equals_the_device_path():
    """psm_poisson_step (host buffers, synchronous) gives the device entry's result bit for bit; on a geometry bound from other
    obstacles it solves again on the general path: one guard trip, the binding dropped, the same bound against the chain."""
    cs = inputs()
    dU, prev = step_inputs()
    lu, sc = lu_of(cs), scales(cs)
    vel = vel_planes(cs)
    with surrogate() as sur:
        bind_all(sur, cs)
        d_vel, d_u, d_p = DeviceArray(vel), dev32(dU), dev32(prev)
        for af in (True, False):
            want = step_device(sur, d_vel, N, lu, sc, af, d_u, d_p)
            res, chg, nxt = sur.poisson_step(vel, lu, out_scale=sc, apply_filter=af, dU=dU, prev=prev)
            same = [np.array_equal(res[..., 0], want[0]), np.array_equal(chg, want[1]), np.array_equal(nxt, want[2])]
            print(f"host entry apply_filter={af}: identical to the device entry {same}")
            assert all(same)
        res, chg, nxt = sur.poisson_step(vel, lu, out_scale=sc)                  # no weighting, no filter: the assembled field
        worst = max(rel(res[i, ..., 0], oracle_fields()[i], np.abs(oracle_fields()[i]).max()) for i in range(N))
        print(f"host entry, plain solve: {worst:.2e} (bound {SOLVE_TOL})")
        assert chg is None and nxt is None and worst <= SOLVE_TOL
        # the images of the cases in another order: every slot is bound to another obstacle than the one it then solves
        _, img = step_by_hand(sur, d_vel, N, lu, sc, True, d_u, d_p)
        other = np.ascontiguousarray(img[[1, 2, 0]])
        assert not np.array_equal(other[..., 3] != 0, img[..., 3] != 0)
        assert sur.bind_geometry(other) and sur.geometry_bound and sur.guard_trips == 0
        got = sur.poisson_step(vel, lu, out_scale=sc, apply_filter=True, dU=dU, prev=prev)
        worst = 0.0
        for i in range(N):
            ref = chain(oracle_fields()[i], dU[i], prev[i], True)
            fmax = np.abs(oracle_fields()[i]).max()
            worst = max(worst, *(rel(g[i].reshape(NY, NX), w, max(np.abs(w).max(), fmax)) for g, w in zip(got, ref)))
        print(f"host entry on another geometry: chain {worst:.2e} (bound {SOLVE_TOL}), guard trips {sur.guard_trips}, bound {sur.geometry_bound}")
        assert worst <= SOLVE_TOL and sur.guard_trips == 1 and not sur.geometry_bound
        assert "not the one bound" in _lib.last_error(sur.h)
        free(d_vel, d_u, d_p)


# ---------------------------------------------------------------------------------------------------------------- 7
@pytest.mark.gpu
def test_gpu_poisson_step_errors():
    """State and argument errors; none of them enqueues anything (the output buffers keep their sentinel)."""
    cs = inputs()
    lu = lu_of(cs)
    sdf = np.stack([c["sdfunct"] for c in cs])
    with surrogate() as sur:
        d_vel, d_img = DeviceArray(vel_planes(cs)), DeviceArray(shape=(N, NY, NX, 4))
        d_out = DeviceArray(np.full((N, NY, NX), -7.5, np.float32))
        step = lambda n=N, l=lu: sur.poisson_step_device(d_vel.ptr, n, l, d_out.ptr, False)
        assert "psm_bind_features" in error(-2, lambda: sur.features_device(d_vel.ptr, N, lu, d_img.ptr))      # nothing bound
        assert "psm_bind_features" in error(-2, step)
        for bad_ma in ((2.7, 0.0, 0.027, 0.29), (2.7, 0.031, 0.027, 0.0)):
            error(-1, lambda: sur.bind_features(sdf, K, bad_ma))
        error(-1, lambda: sur.bind_features(sdf, float("nan"), MAX_ABS))
        error(-1, lambda: sur.bind_features(np.concatenate([sdf, sdf[:1]]), K, MAX_ABS))                     # more than max_cases
        assert "psm_bind_features" in error(-2, step)                                                        # a refused bind binds nothing
        sur.bind_features(sdf[:2], K, MAX_ABS)
        assert "psm_bind_poststeps" in error(-2, lambda: step(2, lu[:2]))                                    # no post-step binding yet
        assert "psm_bind_poststeps" in error(-2, lambda: sur.poisson_step(vel_planes(cs[:2]), lu[:2]))
        sur.bind_poststeps(S_FIELD, S_WEIGHT)
        error(-1, step)                                                                                      # three cases, two bound
        error(-1, lambda: sur.features_device(d_vel.ptr, 3, lu, d_img.ptr))
        for bad_u in (0.0, float("nan"), float("inf")):
            l2 = lu[:2].copy()
            l2[1, 1] = bad_u
            error(-1, lambda: step(2, l2))
            error(-1, lambda: sur.features_device(d_vel.ptr, 2, l2, d_img.ptr))
        error(-1, lambda: sur.features_device(d_vel.ptr, 1, lu[:1], d_img.ptr + 4))                          # image not 16-byte aligned
        sur.synchronize()
        assert (d_out.numpy() == -7.5).all()                                                                 # nothing was enqueued
        step(2, lu[:2])
        sur.synchronize()
        out = d_out.numpy()
        assert np.isfinite(out[:2]).all() and (out[:2] != -7.5).any() and (out[2] == -7.5).all()
        assert sur.lib.psm_plan_grid(sur.h, NY, NX) == 0                                                     # a re-plan drops the binding
        assert "psm_bind_features" in error(-2, lambda: sur.features_device(d_vel.ptr, 1, lu[:1], d_img.ptr))
        sur.bind_features(sdf, K, MAX_ABS)
        sur.unbind_features()
        assert "psm_bind_features" in error(-2, lambda: sur.features_device(d_vel.ptr, 1, lu[:1], d_img.ptr))
        free(d_vel, d_img, d_out)
    three = synthetic.make_model("deltas", p_in=16, p_out=16)                                                # c_in == 3
    with GridSurrogate(three, NY, NX) as sur3:
        assert "c_in" in error(-2, lambda: sur3.bind_features(sdf[0], K, MAX_ABS))

