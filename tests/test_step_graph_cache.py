"""The cached graphs of the steps around a solve (StepCall / GraphKey, csrc/psm_handle.h; solve_device, csrc/psm_api_step.cpp) beside
each other in one handle: four entries that differ in their stages only -- psm_solve_grid_device (no stage), psm_solve_poststeps_device
(post), psm_poisson_step_device (feat + post) and psm_poisson_frames_device (frames + feat + post) -- alternate on the same device
buffers of a PSM_GRAPH=1 handle, so that each is captured once and replayed once while the others' graphs are in the cache.  A
stage that is in the sequence but not in the key would replay another entry's graph: the outputs would be another step's.

Reference: a second handle that launches plainly (PSM_GRAPH=0), same model, same bindings, same buffers' contents, same calls in
the same order.  Same kernels, same arguments, same order: every output is compared bit for bit.

Shape: 256 x 256 (9 blocks), c_in == 4, two cases / frames; the mesh is a hand-made table set of 200 cells on that grid (random
simplices, as set (b) of test_poisson_frames.py); k = 7 columns: the four velocities, one extra plane, the weighting pair."""
import numpy as np
import pytest

from hipmem import DeviceArray
from psm_amd import GridSurrogate, synthetic
from test_poisson_frames import same_bits
from test_poisson_step_device import K as K_ARCSINH
from test_poisson_step_device import MAX_ABS, S_FIELD, S_WEIGHT, error, free, model4

NY = NX = 256
N, K_COLS, N_CELLS = 2, 7, 200


def inputs():
    rng = np.random.default_rng(1801)
    ng = NY * NX
    vtx = rng.integers(0, N_CELLS, (ng, 3)).astype(np.int32)
    w = rng.random((ng, 2)) * 0.5
    wts = np.ascontiguousarray(np.c_[w, 1.0 - w.sum(axis=1)])
    cell = rng.permutation(ng)
    indices = np.c_[cell // NX, cell % NX].astype(np.int32)
    sdf = np.ascontiguousarray(0.3 * synthetic.channel_grid(NY, NX, seed=5)[..., 2], np.float64)      # 0 in the obstacle
    grid = rng.standard_normal((N, NY, NX, 4)).astype(np.float32)
    grid[..., 3] = (sdf / MAX_ABS[3]).astype(np.float32)[None]
    vel = np.ascontiguousarray(rng.standard_normal((N, 4, NY, NX)) * (sdf != 0))
    cols = np.ascontiguousarray(rng.standard_normal((N, N_CELLS, K_COLS)))
    cols[..., K_COLS - 2] = np.abs(cols[..., K_COLS - 2])
    dU = np.abs(rng.standard_normal((N, NY, NX))).astype(np.float32)
    prev = (0.1 * rng.standard_normal((N, NY, NX))).astype(np.float32)
    lu = np.array([[0.25, 1.3], [0.35, 1.7]])
    return dict(vtx=vtx, wts=wts, indices=indices, sdf=sdf, grid=grid, vel=vel, cols=cols, dU=dU, prev=prev, lu=lu, scale=[0.9, 2.2])


def run_sequence(x):
    """One handle, made under the PSM_GRAPH of the moment: the four entries twice in turn, then psm_unbind_features and the
    post-step entry once more.  -> (outputs per call in order, the error psm_poisson_step_device then gives)."""
    with GridSurrogate(model4(), NY, NX, max_cases=N) as sur:
        sur.set_mesh(x["vtx"], x["wts"], x["indices"], x["sdf"], N_CELLS)
        sur.bind_features(np.repeat(x["sdf"][None], N, axis=0), K_ARCSINH, MAX_ABS)
        sur.bind_poststeps(S_FIELD, S_WEIGHT)
        sur.bind_frames(N, K_COLS)
        d_grid, d_vel, d_cols, d_dU, d_prev = (DeviceArray(x[k]) for k in ("grid", "vel", "cols", "dU", "prev"))
        d_field = DeviceArray(shape=(N, NY, NX, 1))
        d_res, d_chg, d_nxt = (DeviceArray(shape=(N, NY, NX)) for _ in range(3))
        d_extra = DeviceArray(shape=(N, 1, NY, NX), dtype=np.float64)
        post = (d_res, d_chg, d_nxt)

        def clear(*arrs):                                 # a call that wrote nothing would otherwise show the call before it
            for d in arrs:
                z = np.zeros(d.shape, d.dtype)
                assert sur.lib.psm_debug_copy_to_device(d.ptr, z.ctypes.data, z.nbytes) == 0

        def solve():
            clear(d_field)
            sur.solve_device(d_grid.ptr, N, d_field.ptr, out_scale=x["scale"])
            sur.synchronize()
            return [d_field.numpy()]

        def poststeps():
            clear(*post)
            sur.solve_poststeps_device(d_grid.ptr, N, d_res.ptr, True, d_dU.ptr, d_prev.ptr, d_chg.ptr, d_nxt.ptr, out_scale=x["scale"])
            sur.synchronize()
            return [d.numpy() for d in post]

        def poisson_step():
            clear(*post)
            sur.poisson_step_device(d_vel.ptr, N, x["lu"], d_res.ptr, True, d_dU.ptr, d_prev.ptr, d_chg.ptr, d_nxt.ptr, out_scale=x["scale"])
            sur.synchronize()
            return [d.numpy() for d in post]

        def poisson_frames():
            clear(*post, d_extra)
            sur.poisson_frames_device(d_cols.ptr, N, K_COLS, x["lu"], d_res.ptr, True, True, d_extra.ptr, d_chg.ptr, d_nxt.ptr, out_scale=x["scale"])
            sur.synchronize()
            return [d.numpy() for d in post] + [d_extra.numpy()]

        outs = [call() for _ in range(2) for call in (solve, poststeps, poisson_step, poisson_frames)]
        sur.unbind_features()                             # drops the graphs with a feature stage, and only those
        outs.append(poststeps())
        msg = error(-2, poisson_step)                     # PSM_ERR_STATE
        assert sur.guard_trips == 0
        free(d_grid, d_vel, d_cols, d_dU, d_prev, d_field, d_res, d_chg, d_nxt, d_extra)
    return outs, msg


@pytest.mark.gpu
def test_gpu_cached_step_graphs_replay_beside_each_other(monkeypatch):
    x = inputs()
    monkeypatch.setenv("PSM_GRAPH", "0")
    plain, msg_plain = run_sequence(x)
    monkeypatch.setenv("PSM_GRAPH", "1")
    graph, msg_graph = run_sequence(x)
    names = ["solve_grid", "solve_poststeps", "poisson_step", "poisson_frames"] * 2 + ["solve_poststeps after psm_unbind_features"]
    assert len(plain) == len(graph) == len(names)
    for i, (name, a, b) in enumerate(zip(names, plain, graph)):
        same = [same_bits(p, g) for p, g in zip(a, b)]
        finite = [float(np.isfinite(g).mean()) for g in b]
        print(f"call {i} {name} ({'capture' if i < 4 else 'replay'}): outputs identical to the plain launches {same}, finite share {finite}")
        assert len(a) == len(b) and all(same)
        assert all(np.isfinite(g).any() and np.any(g != 0) for g in b), f"{name}: an output was not written"
    # the four steps are four different results (the comparison above could not tell one graph replayed for another if they were not)
    assert not same_bits(graph[1][0], graph[2][0]) and not same_bits(graph[2][0], graph[3][0])
    # the second round and the call behind the unbind repeat the first round's bits: same inputs, same route
    for i in range(4):
        assert all(same_bits(p, q) for p, q in zip(graph[i], graph[4 + i])), names[i]
    assert all(same_bits(p, q) for p, q in zip(graph[1], graph[8]))
    print(f"psm_poisson_step_device after psm_unbind_features: {msg_graph!r}")
    assert "psm_bind_features" in msg_plain and "psm_bind_features" in msg_graph
