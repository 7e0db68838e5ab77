"""The input-trust score on the device (psm_bind_trust / psm_trust_last*, include/psm.h) against the float64 oracle of
tests/trust_oracle.py, whose docstring derives the three bounds used here:

* SUM(n, z)      float64 summation alone (lengths K and p_in^2): two evaluations of the definition on the same float32 mu, C and z~;
* BOUND_A        = SUM + the float32 storage of mu and C (and, where the reference image is float64, of x): the issue's bound (a);
* COEFF(delta)   = 2 |delta| |(I - G) z| + |G|_2 |delta|^2 with delta = z~ - z measured, the issue's allowance in (b).

Check (a) uses SUM alone: its oracle runs on the float32 values the handle stores, so storage adds nothing there.

Shapes (block 128): deltas 160 x 200 (B = 4, last block row and column snapped to the edge, origins not 16-byte aligned), gradp
138 x 300 (B = 14), the four-channel Poisson model 160 x 200; p_in 5 and 40 (ld_in padding live); a random basis with G != I and a
QR-orthonormalised one; routes: general, bind_geometry (folded encode), a batch of 3 (rows no multiple of 32) and a batch of 33 on
the deltas grid (132 rows: the packed large-batch route).  Every test prints what it measured before it asserts.

Measured on MI355X: see the figures under each test's name in profiles/r29_trust.txt."""
import ctypes as C
import functools

import numpy as np
import pytest

import trust_oracle as to
from hipmem import DeviceArray
from oracle import psm_oracle as orc
from psm_amd import GridSurrogate, SolverEnsemble, SolverModule, _lib, synthetic

pytestmark = pytest.mark.gpu

S = 128
SHAPES = {"deltas": ("deltas", 160, 200, 3, 4), "gradp": ("gradp", 138, 300, 3, 14), "poisson": ("deltas", 160, 200, 4, 4)}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@functools.lru_cache(maxsize=None)
def model_of(kind, P, basis):
    variant, _, _, c_in, _ = SHAPES[kind]
    m = synthetic.make_model(variant, p_in=P, p_out=8, c_in=c_in, seed_pca=900 + P)
    m.sdf_ch = c_in - 1
    if basis == "random":                                  # rows of norm 1..2, not orthogonal: G != I
        rng = np.random.default_rng(31 + P)
        K = S * S * c_in
        m.comp_in = rng.standard_normal((P, K)) / np.sqrt(K) * (1.0 + rng.random((P, 1))) + 0.3 / np.sqrt(K)
        assert np.abs(m.comp_in @ m.comp_in.T - np.eye(P)).max() > 0.05
    return m


@functools.lru_cache(maxsize=None)
def images(kind, n, seed=0):
    """[n, Ny, Nx, c_in] float32, the SDF last (zero in the obstacle)."""
    _, ny, nx, c_in, _ = SHAPES[kind]
    out = []
    for i in range(n):
        g = (synthetic.delta_grid if kind != "gradp" else synthetic.channel_grid)(ny, nx, seed=40 + 13 * seed + i, cx=0.3 + 0.02 * (i % 7))
        if c_in == 4:
            g = np.concatenate([0.4 * np.random.default_rng(seed * 100 + i).standard_normal((ny, nx, 1)), g], axis=-1)
        out.append(g)
    return np.ascontiguousarray(np.stack(out), np.float32)


def origins(kind):
    variant, ny, nx, _, B = SHAPES[kind]
    lay = orc.block_layout(variant, ny, nx, S)
    assert lay.B == B
    return lay.origins


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def rows_of(kind, imgs, c_in):
    return np.concatenate([to.blocks_of(g, origins(kind), S, c_in) for g in imgs])


def bound_a(n, z, model, x_norm=0.0):
    """The issue's bound (a), absolute: float64 summation + float32 storage of mu and C (and of an x that is not float32 already)."""
    C64, mu = np.asarray(model.comp_in, np.float64), np.asarray(model.mean_in, np.float64)
    big = np.maximum(n, np.einsum("bk,bk->b", z @ C64, z @ C64))
    e_x = to.U32 * x_norm
    return to.sum_bound(n, z, C64, C64.shape[1]) + to.storage_bound(big, z, mu, C64) + 2.0 * np.sqrt(big) * e_x + e_x * e_x


def check_solve(sur, kind, model, imgs, label):
    """(a), (b), (c) where the basis is orthonormal, (g) for the solve that just ran on `imgs`.  Returns the device rows."""
    n_cases, c_in, P = len(imgs), model.c_in, model.p_in
    t = sur.trust_last()
    again = sur.trust_last()
    assert t["n"].shape == (n_cases, sur.B)
    n_dev, spe_dev = t["n"].reshape(-1), t["spe"].reshape(-1)
    zt = to.unscale(sur.stage("x_input", n_cases), model)
    x = rows_of(kind, imgs, c_in)
    C32, mu32, C64, mu64 = f32(model.comp_in), f32(model.mean_in), np.asarray(model.comp_in, np.float64), np.asarray(model.mean_in, np.float64)
    K = C64.shape[1]
    # (a) the kernels' arithmetic: the definition at the device's own z~, on the float32 mu and C
    n_a, spe_a = to.score_identity(x, mu32, C32, zt)
    tol_a = to.sum_bound(n_a, zt, C32, K)
    ea_n, ea_s = np.abs(n_dev - n_a) / tol_a, np.abs(spe_dev - spe_a) / tol_a
    # (b) end to end: the all-float64 pipeline
    z = to.encode(x, mu64, C64)
    n_b, spe_b = to.score(x, mu64, C64, z)
    A = bound_a(n_b, z, model)
    tol_b = to.coefficient_bound(zt - z, z, C64) + A
    eb_n, eb_s = np.abs(n_dev - n_b) / A, np.abs(spe_dev - spe_b) / tol_b
    expl = 1.0 - spe_dev / n_dev
    print(f"{label}: rows {len(n_dev)} explained {expl.min():.6f}..{expl.max():.6f}; (a) |dn| {ea_n.max():.3f} |dspe| {ea_s.max():.3f} of SUM "
          f"(SUM/n {np.max(tol_a / n_a):.2e}); (b) |dn| {eb_n.max():.3e} of BOUND_A, |dspe| {eb_s.max():.3e} of COEFF + BOUND_A "
          f"(|dspe|/n {np.max(np.abs(spe_dev - spe_b) / n_b):.2e}, allowed/n {np.max(tol_b / n_b):.2e}, |delta|/|z| {np.max(np.linalg.norm(zt - z, axis=1) / np.linalg.norm(z, axis=1)):.2e})")
    same = np.array_equal(bits(t["n"]), bits(again["n"])) and np.array_equal(bits(t["spe"]), bits(again["spe"]))
    ec = None
    if np.abs(C64 @ C64.T - np.eye(P)).max() < 1e-12:      # (c) orthonormal basis: explained == |z~|^2 / n
        ec = np.abs(spe_dev - (n_dev - np.einsum("bp,bp->b", zt, zt))) / bound_a(n_dev, zt, model)
        print(f"{label}: (c) |explained - |z~|^2 / n| n = {ec.max():.3e} of BOUND_A")
    assert np.isfinite(n_dev).all() and np.isfinite(spe_dev).all() and (n_dev > 0).all()
    assert ea_n.max() <= 1.0 and ea_s.max() <= 1.0, "(a)"
    assert eb_n.max() <= 1.0 and eb_s.max() <= 1.0, "(b)"
    assert ec is None or ec.max() <= 1.0, "(c)"
    assert same, "(g) two calls on one solve differ"
    return t


@pytest.mark.parametrize("basis", ("random", "qr"))
@pytest.mark.parametrize("P", (5, 40))
@pytest.mark.parametrize("kind", tuple(SHAPES))
def test_routes(kind, P, basis):
    """(a), (b), (c), (g) on the general route, a batch of 3 and the bound (folded) route of one handle; the device entry gives
    the host entry's bits; binding and calling trust leaves the field's bits alone."""
    model = model_of(kind, P, basis)
    _, ny, nx, c_in, B = SHAPES[kind]
    g1, g3 = images(kind, 1), images(kind, 3, seed=1)
    with GridSurrogate(model, ny, nx, max_cases=3) as plain:
        want = [plain.solve(g1).copy(), plain.solve(g3).copy()]
    with GridSurrogate(model, ny, nx, max_cases=3) as sur:
        assert sur.B == B
        sur.bind_trust()
        got = [sur.solve(g1).copy()]
        t1 = check_solve(sur, kind, model, g1, f"{kind} p_in {P} {basis} general")
        d = DeviceArray(np.full((1, B, 2), -7.0))
        sur.trust_last_device(d.ptr)
        sur.synchronize()
        dev = d.numpy()
        assert np.array_equal(bits(dev[..., 0]), bits(t1["n"])) and np.array_equal(bits(dev[..., 1]), bits(t1["spe"]))
        got.append(sur.solve(g3).copy())
        check_solve(sur, kind, model, g3, f"{kind} p_in {P} {basis} batch of 3")
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, want)), "trust changed a field"
        bound = sur.bind_geometry(g1[0])
        assert bound or kind == "poisson"                           # the four-channel model may stay on the general route
        sur.solve(g1)
        tb = check_solve(sur, kind, model, g1, f"{kind} p_in {P} {basis} {'bound' if bound else 'general again'}")
        assert np.array_equal(bits(tb["n"]), bits(t1["n"]))         # the same image: n does not depend on the route


@pytest.mark.parametrize("P,basis", ((40, "random"), (5, "qr")))
def test_large_batch(P, basis):
    """33 cases on the deltas grid: 132 block rows, the packed large-batch route."""
    model = model_of("deltas", P, basis)
    _, ny, nx, _, _ = SHAPES["deltas"]
    g = images("deltas", 33, seed=2)
    with GridSurrogate(model, ny, nx, max_cases=33) as sur:
        sur.bind_trust()
        sur.solve(g)
        check_solve(sur, "deltas", model, g, f"deltas p_in {P} {basis} batch of 33")


def test_cancellation_and_mean_block():
    """(d) a block in mu + rowspace(C) of an orthonormal basis: |spe| <= BOUND_A (+ the squared residual the float32 image itself
    leaves, bounded from the measured |z~ - a|).  (e) a block equal to the float32 mean: n == 0 and spe == 0 exactly."""
    kind, P = "deltas", 40
    model = model_of(kind, P, "qr")
    _, ny, nx, c_in, B = SHAPES[kind]
    C32, mu32 = f32(model.comp_in), f32(model.mean_in)
    a = np.random.default_rng(5).standard_normal(P) * 3.0
    g = images(kind, 2, seed=3).copy()
    (y0, x0), (y1, x1) = origins(kind)[0], origins(kind)[0]
    g[0, y0:y0 + S, x0:x0 + S, :] = (mu32 + a @ C32).reshape(S, S, c_in).astype(np.float32)
    g[1, y1:y1 + S, x1:x1 + S, :] = mu32.reshape(S, S, c_in).astype(np.float32)
    with GridSurrogate(model, ny, nx, max_cases=2) as sur:
        sur.bind_trust()
        sur.solve(g)
        t = sur.trust_last()
        zt = to.unscale(sur.stage("x_input", 2), model)
    n, spe = t["n"][0, 0], t["spe"][0, 0]
    x = to.blocks_of(g[0], origins(kind)[:1], S, c_in)
    rho = to.U32 * np.linalg.norm(x) + np.linalg.norm(C32, 2) * np.linalg.norm(zt[0] - a) + to.U32 * (np.linalg.norm(mu32) + np.sqrt(P) * np.linalg.norm(a))
    A = bound_a(np.array([n]), zt[:1], model)[0]
    print(f"(d) n {n:.6e} spe {spe:.3e} spe/n {spe / n:.3e}; BOUND_A/n {A / n:.3e}, image residual^2/n {rho * rho / n:.3e}, |z~ - a|/|a| {np.linalg.norm(zt[0] - a) / np.linalg.norm(a):.2e}")
    print(f"(e) n {t['n'][1, 0]!r} spe {t['spe'][1, 0]!r}")
    assert t["n"][1, 0] == 0.0 and t["spe"][1, 0] == 0.0, "(e)"
    assert abs(spe) <= A + rho * rho, "(d)"


def test_case_independence():
    """(f) in a batch of 3, another image for case 1 changes case 1's rows only: the others keep their bits."""
    kind, P = "gradp", 40
    model = model_of(kind, P, "random")
    _, ny, nx, _, _ = SHAPES[kind]
    g = images(kind, 3, seed=1).copy()
    with GridSurrogate(model, ny, nx, max_cases=3) as sur:
        sur.bind_trust()
        sur.solve(g)
        t1 = sur.trust_last()
        g[1] = images(kind, 1, seed=7)[0]
        sur.solve(g)
        t2 = sur.trust_last()
    for q in ("n", "spe"):
        assert np.array_equal(bits(t1[q][[0, 2]]), bits(t2[q][[0, 2]])), q
        assert not np.array_equal(bits(t1[q][1]), bits(t2[q][1])), q
    print(f"(f) cases 0 and 2 bit-identical, case 1 moved by {np.abs(t1['spe'][1] - t2['spe'][1]).max():.3e}")


# ------------------------------------------------------------------------------------------------------- (h) the solver boundary
def _geo(g):
    return orc.Geometry(g.ny, g.nx, np.asarray(g.vtx_m2g), np.asarray(g.wts_m2g), np.asarray(g.vtx_g2m), np.asarray(g.wts_g2m),
                        np.asarray(g.indices), np.asarray(g.sdfunct, np.float64).reshape(g.ny, g.nx))


def check_boundary(label, model, variant, image64, got, zt):
    """`.trust()` of one case against the oracle on the oracle's own float64 image, under the bounds of (b); zt: the device's z~."""
    ny, nx = image64.shape[:2]
    lay = orc.block_layout(variant, ny, nx, S)
    x = to.blocks_of(image64, lay.origins, S, model.c_in)
    C64, mu64 = np.asarray(model.comp_in, np.float64), np.asarray(model.mean_in, np.float64)
    z = to.encode(x, mu64, C64)
    n_ref, spe_ref = to.score(x, mu64, C64, z)
    xn = np.linalg.norm(x, axis=1)
    A = bound_a(n_ref, z, model, x_norm=xn)
    coeff = to.coefficient_bound(zt - z, z, C64)
    en, es = np.abs(got["n"] - n_ref) / A, np.abs(got["spe"] - spe_ref) / (coeff + A)
    total = 1.0 - spe_ref.sum() / n_ref.sum()
    print(f"{label}: B {lay.B} explained {got['explained'].min():.6f}..{got['explained'].max():.6f} (oracle total {total:.6f}, got {got['explained_total']:.6f}); "
          f"|dn| {en.max():.3e} of BOUND_A, |dspe| {es.max():.3e} of COEFF + BOUND_A (|dspe|/n {np.max(np.abs(got['spe'] - spe_ref) / n_ref):.2e})")
    assert got["n"].shape == (lay.B,) and got["explained_min"] == got["explained"].min()
    assert en.max() <= 1.0 and es.max() <= 1.0
    assert got["explained_total"] == float(1.0 - got["spe"].sum() / got["n"].sum())


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def test_solver_module_absolute():
    model = synthetic.make_model("chapter5", p_in=8, p_out=8)
    maxs = (1.3, 0.6, 1.0, 0.5)
    a0, top, obst = synthetic.channel_mesh()
    a3 = np.ascontiguousarray(synthetic.channel_mesh(step=3)[0])
    p = []
    for trust in (True, False):
        sm = SolverModule(model, maxs, trust=trust)
        sm.init_func(a0, top, obst)
        try:
            p.append(sm.py_func(a3).copy())
            if trust:
                got, tables, zt = sm.trust(), sm.tables, to.unscale(sm._sur.stage("x_input", 1), model)
            else:
                with pytest.raises(RuntimeError, match="without trust=True"):
                    sm.trust()
        finally:
            sm._sur.close()
    assert _same(p[0], p[1]), "trust=True changed p"
    image, _ = orc.mesh_to_grid(a3, _geo(tables), maxs[0], maxs[1])
    check_boundary("SolverModule absolute", model, "chapter5", image, got, zt)


def test_solver_module_poisson():
    from test_poisson_solve import K, MAXS5, PHI, Tabs, columns, plane
    from test_poisson_step_device import model4
    model = model4()
    a0, top, obst = synthetic.channel_mesh()
    a0, a3 = np.ascontiguousarray(a0), np.ascontiguousarray(synthetic.channel_mesh(step=3)[0])
    p = []
    for trust in (True, False):
        sm = SolverModule(model, MAXS5, step="poisson", phi=PHI, k=K, weighting=False, apply_filter=False, trust=trust)
        sm.init_func(a0, top, obst)
        try:
            p.append(sm.py_func(a3).copy())
            if trust:
                got, g, zt = sm.trust(), sm.tables, to.unscale(sm._sur.stage("x_input", 1), model)
        finally:
            sm._sur.close()
    assert _same(p[0], p[1]) and np.abs(p[0] - a3[:, 4]).max() > 0, "trust=True changed p, or the step was a priming step"
    t = Tabs(g.ny, g.nx, len(a0), g.vtx_m2g, g.wts_m2g, g.indices, g.sdfunct, g.vtx_g2m, g.wts_g2m)
    cols, U, _ = columns(a0, a0, a3)
    pl = [plane(t, cols[:, q]) for q in range(4)]
    image, _ = orc.poisson_features(pl[0], pl[1], pl[2], pl[3], t.sdf, PHI, U, K, MAXS5[:4])
    check_boundary("SolverModule poisson", model, "deltas", np.nan_to_num(image), got, zt)


def test_solver_ensemble_gradp():
    model = synthetic.make_model("gradp", p_in=8, p_out=8)
    maxs5 = (2.5, 0.6, 0.35, 40.0, 25.0)
    a0, top, obst = synthetic.channel_mesh()
    a0, a3 = np.ascontiguousarray(a0), np.ascontiguousarray(synthetic.channel_mesh(step=3)[0])
    p = []
    for trust in (True, False):
        ens = SolverEnsemble(model, maxs5, max_cases=2, geometry="scipy", step="gradp", trust=trust)
        ens.init_func([a0, a3], [top, top], [obst, obst])
        try:
            p.append(np.concatenate(ens.py_func([a3, a0])))
            if trust:
                got, tables, zt = ens.trust(), ens.tables, to.unscale(ens._sur.stage("x_input", 2), model)
        finally:
            ens._sur.close()
    assert _same(p[0], p[1]), "trust=True changed p"
    assert len(got) == 2
    for k, cells in enumerate((a3, a0)):
        image, _ = orc.mesh_to_grid(cells, _geo(tables[k]), maxs5[0], maxs5[1], sdf_div=maxs5[2], fill=True)
        B = len(got[k]["n"])
        check_boundary(f"SolverEnsemble gradp case {k}", model, "gradp", image, got[k], zt[k * B:(k + 1) * B])


# ------------------------------------------------------------------------------------------------------- (i) refusals
def test_refusals():
    kind, P = "deltas", 5
    model = model_of(kind, P, "random")
    _, ny, nx, c_in, B = SHAPES[kind]
    g = images(kind, 1)
    lib = _lib.load()
    out = np.full(B * 2, -7.0)
    outp = out.ctypes.data_as(C.POINTER(C.c_double))
    n = C.c_int32(-1)
    ci = np.ascontiguousarray(model.comp_in, np.float64)
    cip = ci.ctypes.data_as(C.POINTER(C.c_double))
    d = DeviceArray(np.full((B + 1) * 2, -7.0))

    def untouched():
        return (out == -7.0).all() and (d.numpy() == -7.0).all() and n.value == -1

    # a handle that was never planned
    cfg = _lib.psm_config(abi_version=_lib.PSM_ABI_VERSION, variant=1, block=S, c_in=3, c_out=1, p_in=P, p_out=8, n_dense=2, sdf_channel=2, max_cases=1)
    h = C.c_void_p()
    assert lib.psm_create(C.byref(cfg), C.byref(h)) == 0
    try:
        assert lib.psm_bind_trust(h, cip) == -2 and lib.psm_trust_last(h, C.byref(n), outp, out.size) == -2
        assert lib.psm_trust_last_device(h, C.c_void_p(d.ptr), None) == -2 and lib.psm_bind_trust(None, cip) == -1
    finally:
        lib.psm_destroy(h)
    with GridSurrogate(model, ny, nx) as sur:
        hh = sur.h
        assert lib.psm_trust_last(hh, C.byref(n), outp, out.size) == -2 and "psm_bind_trust" in _lib.last_error(hh)      # unbound
        assert lib.psm_trust_last_device(hh, C.c_void_p(d.ptr), None) == -2
        assert lib.psm_bind_trust(hh, None) == -1
        sur.bind_trust()
        assert lib.psm_trust_last(hh, C.byref(n), outp, out.size) == -2 and "no solve" in _lib.last_error(hh)            # no solve since the plan
        sur.solve(g)
        assert lib.psm_trust_last_device(hh, None, None) == -1
        assert lib.psm_trust_last_device(hh, C.c_void_p(d.ptr + 4), None) == -1 and "aligned" in _lib.last_error(hh)
        assert lib.psm_trust_last(hh, C.byref(n), outp, B * 2 - 1) == -1 and lib.psm_trust_last(hh, C.byref(n), None, out.size) == -1
        ticket = sur.submit(g)                                  # the last solve ran on a ring slot
        sur.wait(ticket)
        assert lib.psm_trust_last(hh, C.byref(n), outp, out.size) == -2 and "ring" in _lib.last_error(hh)
        assert lib.psm_trust_last_device(hh, C.c_void_p(d.ptr), None) == -2
        sur.synchronize()
        assert untouched(), "a refused call wrote something"
        sur.solve(g)                                            # a valid solve behind the refusals: correct
        check_solve(sur, kind, model, g, "after the refusals")
        assert lib.psm_trust_last(hh, C.byref(n), outp, out.size) == 0 and n.value == 1 and (out != -7.0).all()
        out[:] = -7.0
        n.value = -1
        ia = np.ascontiguousarray(np.broadcast_to(np.asarray(model.in_a, np.float64), (P,)))
        ib = np.ascontiguousarray(np.broadcast_to(np.asarray(model.in_b, np.float64), (P,)))
        oa, ob = np.ones(8), np.ones(8)
        dp = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))
        assert lib.psm_set_scaler(hh, dp(ia), dp(ib), dp(oa), dp(ob)) == 0                                                # a model setter drops the binding
        assert lib.psm_trust_last(hh, C.byref(n), outp, out.size) == -2 and "psm_bind_trust" in _lib.last_error(hh)
        sur.bind_trust()
        assert lib.psm_plan_grid(hh, ny, nx) == 0                                                                        # and so does the plan
        assert lib.psm_trust_last(hh, C.byref(n), outp, out.size) == -2
        sur.bind_trust()
        sur.unbind_trust()
        assert lib.psm_trust_last(hh, C.byref(n), outp, out.size) == -2
        assert untouched()
    with GridSurrogate(model, ny, nx, precision="bf16") as sur:
        assert lib.psm_bind_trust(sur.h, cip) == -5 and "bf16" in _lib.last_error(sur.h)
        sur.solve(g)
        assert lib.psm_trust_last(sur.h, C.byref(n), outp, out.size) == -5 and lib.psm_trust_last_device(sur.h, C.c_void_p(d.ptr), None) == -5
    bad = synthetic.make_model("deltas", p_in=P, p_out=8, scaler_kind="max_abs")
    bad.in_a = np.inf                                           # 1 / in_a == 0: the scaler cannot be undone
    with GridSurrogate(bad, ny, nx) as sur:
        assert lib.psm_bind_trust(sur.h, cip) == -1 and "scaler" in _lib.last_error(sur.h)
        sur.solve(g)
        assert lib.psm_trust_last(sur.h, C.byref(n), outp, out.size) == -2
    assert untouched()
    print("refusals: STATE (unplanned, unbound, no solve, ring, binding dropped by a setter / the plan / unbind), ARG (null, misaligned, short, scaler), UNSUPPORTED (bf16)")
