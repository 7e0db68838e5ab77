"""Every stored stage of the PCA path against a stage-isolated float64 oracle (oracle/pca_stage_oracle.py): encode, each Dense
layer (keep mode reads the hidden activations back), head and decode, each recomputed once from what the device stored for
that stage's input and held element by element to an a-priori float32 bound E.

CPU: the checker's own sharpness -- the oracle's exact outputs pass far inside E, faults confined to one stage are flagged
on that stage -- and the x6 split claim the encode bound relies on.
GPU: solves over variants, c_in 1-4, aligned and odd grids, component counts around the 32 / 64 / 128 tile edges, one case
to 432 block rows, f32 / x6 / bf16, bound and general path; keep mode changes no launch and no bit of the fields; stale
stages are refused.

c_in = 1 stays accepted (the SDF as the only channel is a valid input of every variant's layout): all ten c_in = 1 encode
instantiations run in test_gpu_every_encode_form.

Faults the bound cannot see: anything below E.  E is a worst case: the measured ratios below leave room for errors two to
three orders above the observed rounding (encode: ~1500x) -- e.g. an x6 form that lost the lo plane of one operand (<= 2^-16
of each product, below the six-term accumulation depth the bound allows), or a different but valid summation order.

Not covered (the issue's remaining parts): the reassembly (offsets, paste, shift) and the fused bound-path decode + paste /
chain_dots / closed form stay with check_against_oracle in test_gpu_parity.py (normwise), so the injected faults "offset taken
from a neighbour", "overlap column from the wrong block", "shift applied twice" and "NaN mask off by one row" are not
modelled; LayerNormalization and the Conv1D head.  SWEPT below lists
what this module launches; not_swept_reason says why each other table entry is not.

Measured on an MI355X (test_zz_report prints it; GPU part of the module 12.8 s with the four PSM_DECODE_MTC rows, 74 of the 220 table entries launched; the ratios are unchanged by those rows), worst
|dev - r| / E: encode 1.1e-3 (f32 form, c_in = 1, odd Nx; pair 7.3e-4, x6 2.9e-4, x6_mt 3.9e-5), dense0 0.060, dense1-2 0.0025,
head 0.031, decode 0.153 (32 components)."""
import ctypes as C

import numpy as np
import pytest

from oracle import pca_stage_oracle as so
from oracle import psm_oracle as orc

# ---------------------------------------------------------------------------------------------------------------------
# CPU: the checker is sharp
# ---------------------------------------------------------------------------------------------------------------------
_GRID = {"deltas": (256, 256), "gradp": (256, 256), "chapter5": (256, 300)}
_SDF = {1: 0, 2: 1, 3: 2, 4: 3}


def _model(variant, c_in, p_in=40, p_out=24, widths=(64, 48), seed=3):
    from psm_amd import synthetic
    m = synthetic.make_model(variant, p_in=p_in, p_out=p_out, c_in=c_in, seed_pca=100 + c_in, seed_w=seed,
                             weights=synthetic.he_dense_stack(p_in, list(widths), p_out, seed))
    m.sdf_ch = _SDF[c_in]
    return m


def _omodel(m):
    sc = orc.Scaler(m.scaler_kind, m.in_a, m.in_b, m.out_a, m.out_b)
    return orc.Model(m.variant, m.c_in, m.c_out, m.comp_in, m.mean_in, m.comp_out, m.mean_out, m.weights, sc, m.out_scale,
                     m.S, m.ov, m.sdf_ch)


def _grids(n, ny, nx, c_in, seed=0):
    from psm_amd import synthetic
    g = np.stack([synthetic.channel_grid(ny, nx, seed=seed + k) for k in range(n)]).astype(np.float32)
    if c_in == 4:
        return np.concatenate([g[..., :1] * g[..., 1:2], g], axis=-1).astype(np.float32)
    return np.ascontiguousarray(g[..., 3 - c_in:])


def _setup(variant, c_in, precision, n=1):
    m = _omodel(_model(variant, c_in))
    g = _grids(n, *_GRID[variant], c_in)
    form = "bf16" if precision == "bf16" else "x6"
    return m, g, form, so.exact_stages(m, g, form, precision == "bf16")


@pytest.mark.parametrize("variant,c_in,precision,n", [("deltas", 1, "f32", 1), ("gradp", 2, "bf16", 1), ("chapter5", 3, "f32", 1),
                                                      ("deltas", 4, "bf16", 1), ("gradp", 3, "f32", 2), ("chapter5", 4, "f32", 1),
                                                      ("deltas", 2, "f32", 1), ("gradp", 1, "bf16", 1)])
def test_checker_passes_exact_outputs(variant, c_in, precision, n):
    m, g, form, st = _setup(variant, c_in, precision, n)
    for f in (form, "f32", "pair", "x6_mt") if precision == "f32" else (form,):
        res = so.check_solve(m, g, st, f, None if f == "x6_mt" else 1, precision == "bf16")
        assert [r.name for r in res] == ["encode", "dense0", "dense1", "head", "decode"]
        for r in res:
            assert r.ok and r.ratio <= 0.1, (f, r)          # one float32 rounding of the float64 value: far inside E


def _fault(name, m, g, st, bf):
    """-> (stage name, faulty stages): each fault confined to one stage, the others exact."""
    st = {k: ([a.copy() for a in v] if isinstance(v, list) else v.copy()) for k, v in st.items()}
    xb = so.blocks_of(g, m)
    rows = xb.shape[0]
    W = m.weights
    if name == "k_slice_dropped_from_one_slab":                     # one 64-pixel slice of block row 1 missing from its slab
        xs = xb.copy()
        xs[1].reshape(-1, m.c_in)[17 * 64:18 * 64] = np.asarray(m.mean_in, np.float32).reshape(-1, m.c_in)[17 * 64:18 * 64]
        coeff, _ = so.encode_reference(xs, m, bf)
        st["x_input"][1] = np.asarray(m.scaler.fwd(coeff[1]), np.float32)
        return "encode", st
    if name == "last_partial_row_tile_from_next_row":              # rows of the last (partial) 32-row tile shifted by one
        t0 = (rows - 1) // 32 * 32
        h = st["hidden"][0]
        h[t0:-1] = h[t0 + 1:].copy()
        return "dense0", st
    if name == "component_tile_shifted_by_a_column":               # one 32-column tile of the decoded blocks read one column late
        bp = st["block_pred"].reshape(rows, -1)
        bp[:, 160:192] = bp[:, 161:193].copy()
        return "decode", st
    if name == "bias_group_missing":                               # 16 output columns without their bias
        v, _ = so.dense_reference(st["hidden"][0], W[1][0], np.where(np.arange(len(W[1][1])) // 16 == 1, 0, W[1][1]), bf)
        st["hidden"][1] = np.maximum(v, 0).astype(np.float32)
        return "dense1", st
    if name == "last_16k_group_skipped":                           # the last 16 k of layer 1 not accumulated
        Wd = np.array(W[1][0], copy=True)
        Wd[-16:] = 0
        v, _ = so.dense_reference(st["hidden"][0], Wd, W[1][1], bf)
        st["hidden"][1] = np.maximum(v, 0).astype(np.float32)
        return "dense1", st
    if name == "case_rows_from_next_case":
        B = rows // g.shape[0]
        st["res"][:B] = st["res"][B:2 * B]
        return "head", st
    if name == "nan_in_a_row_the_reference_has_finite":            # a NaN row where the reference row is finite
        st["hidden"][1][3] = np.nan
        return "dense1", st
    if name == "head_scaler_applied_twice":
        sa, sb = so.scaler_out(m.scaler, st["res"].shape[1])
        st["res"] = (st["res"] * sa + sb).astype(np.float32)
        return "head", st
    if name == "decode_res_truncated_to_bf16":                     # truncation instead of round to nearest even
        r = st["res"].view(np.uint32) & np.uint32(0xFFFF0000)
        C_ = so.bf16(m.comp_out).astype(np.float64)
        st["block_pred"] = orc.pca_decode(r.view(np.float32).astype(np.float64), C_, m.mean_out, m.S, m.c_out).astype(np.float32)
        return "decode", st
    raise KeyError(name)


_FAULTS = ["k_slice_dropped_from_one_slab", "last_partial_row_tile_from_next_row", "component_tile_shifted_by_a_column",
           "bias_group_missing", "last_16k_group_skipped", "case_rows_from_next_case", "nan_in_a_row_the_reference_has_finite",
           "head_scaler_applied_twice", "decode_res_truncated_to_bf16"]


@pytest.mark.parametrize("fault,precision", [(f, p) for f in _FAULTS for p in ("f32", "bf16")
                                             if p == "bf16" or f != "decode_res_truncated_to_bf16"])
def test_checker_flags_injected_fault(fault, precision):
    m, g, form, st = _setup("gradp", 3, precision, n=2)
    stage, bad = _fault(fault, m, g, st, precision == "bf16")
    res = {r.name: r for r in so.check_solve(m, g, bad, form, 1, precision == "bf16")}
    assert not res[stage].ok, (fault, res[stage])
    order = list(res)                 # the stages in front of the faulty one read exact inputs and stored exact outputs
    assert all(res[k].ok for k in order[:order.index(stage)]), res


def _split3(x):
    x = np.asarray(x, np.float32)
    h = so.bf16(x)
    r1 = (x - h).astype(np.float32)
    mid = so.bf16(r1)
    r2 = (r1 - mid).astype(np.float32)
    return h, mid, so.bf16(r2)


def test_x6_split_drops_at_most_2_pow_minus_23_of_a_product():
    """psm_split3 (three bf16 planes by successive round-to-nearest-even): the x6 forms keep hh hm mh hl lh mm; the dropped
    ml + lm + ll is <= 2^-23 |a||b| for normal operands.  Near the float32 subnormal range the lo plane is a bf16 subnormal and
    the split is no longer exact: the residual a - (hi + mid + lo) is then below the smallest bf16 subnormal spacing, 2^-133."""
    rng = np.random.default_rng(5)
    a = (rng.standard_normal(200000) * 2.0 ** rng.integers(-100, 100, 200000)).astype(np.float32)
    b = (rng.standard_normal(200000) * 2.0 ** rng.integers(-100, 100, 200000)).astype(np.float32)
    ah, am, al = (v.astype(np.float64) for v in _split3(a))
    bh, bm, bl = (v.astype(np.float64) for v in _split3(b))
    assert np.array_equal(ah + am + al, a.astype(np.float64))
    dropped = am * bl + al * bm + al * bl
    assert np.all(np.abs(dropped) <= 2.0 ** -23 * np.abs(a.astype(np.float64) * b))
    tiny = (rng.standard_normal(100000) * 2.0 ** rng.integers(-149, -110, 100000)).astype(np.float32)
    th, tm, tl = (v.astype(np.float64) for v in _split3(tiny))
    assert np.all(np.abs(tiny.astype(np.float64) - (th + tm + tl)) <= 2.0 ** -133)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: every stage of every run through the checker
# ---------------------------------------------------------------------------------------------------------------------
_FORMS = {"psm_encode_kernel": "f32", "psm_encode_pair_kernel": "pair", "psm_encode_x6_kernel": "x6",
          "psm_encode_x6_mt_kernel": "x6_mt", "psm_encode_bf16_kernel": "bf16"}
_STATS = {}
_RAN = set()
_DONE = set()                      # GPU tests that completed (the coverage assertion needs all of them)


def launched_kernels(sur, d_grid, n_cases, d_fields):
    """The kernels one solve launches, in launch order (psm_time_kernels, steps = 1: PSM_LAUNCH records the template expression of
    every dispatch): spaces, the '#layerN' suffix of Dense launches and defaulted template arguments normalised away, so that
    the names compare with the library's demangled symbols (psm_dense_kernel<1,false,16,true> = <1,false,16,true,false>)."""
    cap = 64
    names = C.create_string_buffer(cap * 64)
    ms, cnt, nk = (C.c_double * cap)(), (C.c_int64 * cap)(), C.c_int32()
    sur._chk(sur.lib.psm_time_kernels(sur.h, C.c_void_p(d_grid), n_cases, C.c_void_p(d_fields), 1, names, ms, cnt, cap, C.byref(nk)))
    out = []
    for k in range(min(nk.value, cap)):
        raw = names.raw[k * 64:(k + 1) * 64].split(b"\0", 1)[0].decode()
        assert len(raw) < 63, f"kernel name cut at 63 characters: {raw}"
        nm = raw.split("#", 1)[0].replace(" ", "")
        if nm.startswith("psm_dense_kernel<") and nm.count(",") == 3:
            nm = nm[:-1] + ",false>"
        if nm not in out:
            out.append(nm)
    return out


def _hidden(sur, n_layers, n_cases):
    return [sur.stage("hidden", n_cases, layer=l) for l in range(n_layers - 1)]


def _solve(model, grids, precision="f32", bind=False, keep=True, misalign=False):
    """One solve through psm_time_kernels (steps = 1, out_scale 1) on ws0 -> (kernel names, stages, fields).  misalign: the grid
    starts 4 bytes past a 16-byte boundary (the only way c_in = 4 reaches the encode forms for unaligned rows)."""
    from hipmem import DeviceArray
    from psm_amd import GridSurrogate
    n, ny, nx = grids.shape[:3]
    with GridSurrogate(model, ny, nx, max_cases=n, precision=precision) as sur:
        if bind:
            assert sur.bind_geometry(grids if n > 1 else grids[0], n_cases=n) if n > 1 else sur.bind_geometry(grids[0])
        flat = np.concatenate([np.zeros(1, np.float32), grids.ravel()]) if misalign else grids
        d_in, d_out = DeviceArray(flat), DeviceArray(shape=(n, ny, nx, model.c_out))
        names = launched_kernels(sur, d_in.ptr + (4 if misalign else 0), n, d_out.ptr)
        fields = d_out.numpy()
        rows = n * sur.B
        st = dict(x_input=sur.stage("x_input", n), res=sur.stage("res", n))
        st["hidden"] = _hidden(sur, len(model.weights), n) if keep else None
        st["block_pred"] = None if bind else sur.stage("block_pred", n)
        d_in.free(), d_out.free()
    return names, st, fields


def _check(tag, model, grids, precision="f32", bind=False, misalign=False):
    names, st, fields = _solve(model, grids, precision, bind, misalign=misalign)
    _RAN.update(names)
    enc = [n for n in names if n.split("<")[0] in _FORMS]
    assert len(enc) == 1, names
    form = _FORMS[enc[0].split("<")[0]]
    res = so.check_solve(_omodel(model), grids, st, form, None if form == "x6_mt" else 1, precision == "bf16")
    for r in res:
        w = _STATS.get(r.name, (0.0, ""))
        if r.ratio >= w[0]:
            _STATS[r.name] = (r.ratio, tag)
        fam = f"{r.name}:{form}"
        if r.ratio >= _STATS.get(fam, (0.0, ""))[0]:
            _STATS[fam] = (r.ratio, tag)
    bad = [r for r in res if not r.ok]
    assert not bad, (tag, names, bad)
    return names, fields


_CONFIGS = {
    # name: (variant, c_in, (ny, nx), p_in, p_out, n_cases, precision, env, bind)
    "deltas_c3_p32_one": ("deltas", 3, (256, 256), 32, 32, 1, "f32", {}, False),
    "gradp_c2_p128_pair": ("gradp", 2, (256, 256), 128, 128, 1, "f32", {}, False),
    "chapter5_c4_odd_nx": ("chapter5", 4, (300, 257), 100, 96, 1, "f32", {}, False),
    "deltas_c1_n8_x6": ("deltas", 1, (256, 256), 40, 64, 8, "f32", {}, False),
    "gradp_c3_p160_n5_packed": ("gradp", 3, (256, 256), 160, 160, 5, "f32", {}, False),
    "deltas_c3_n48_x6_mt": ("deltas", 3, (256, 256), 64, 128, 48, "f32", {}, False),
    "deltas_c3_n8_f32": ("deltas", 3, (256, 256), 48, 96, 8, "f32", {"PSM_X6": "0"}, False),
    "chapter5_c3_one_x6": ("chapter5", 3, (256, 300), 33, 64, 1, "f32", {"PSM_X6": "1"}, False),
    "deltas_bf16_one": ("deltas", 3, (256, 256), 64, 128, 1, "bf16", {}, False),
    "gradp_bf16_n5": ("gradp", 3, (256, 256), 48, 64, 5, "bf16", {}, False),
    "deltas_bound_one": ("deltas", 3, (256, 256), 32, 32, 1, "f32", {}, True),
    "gradp_bound_n4": ("gradp", 3, (256, 256), 64, 96, 4, "f32", {}, True),
    "deltas_bound_bf16": ("deltas", 3, (256, 256), 64, 128, 1, "bf16", {}, True),
    # decode + paste of a bound case batch with two / three 32-row tiles per chunk (the gradp grid has 30 blocks).  8 cases = 240 block
    # rows, eight tiles: four full chunks of two, two full chunks of three and a ragged one; 3 cases = 90 rows, three tiles: a full
    # and a ragged chunk of two, exactly one chunk of three.  The stage oracle reads no stage behind `res` on a bound geometry, so
    # what these launches paste is held to the fields of the same solve with one tile per chunk, bit for bit (the tiles per chunk
    # change which rows share a pass over the basis, not the order of any row's sum), and through them to the float64 oracle.
    "gradp_bound_n8_mtc2": ("gradp", 3, (256, 256), 64, 96, 8, "f32", {"PSM_DECODE_MTC": "2"}, True),
    "gradp_bound_n8_mtc3": ("gradp", 3, (256, 256), 64, 96, 8, "f32", {"PSM_DECODE_MTC": "3"}, True),
    "gradp_bound_n3_mtc2": ("gradp", 3, (256, 256), 64, 96, 3, "f32", {"PSM_DECODE_MTC": "2"}, True),
    "gradp_bound_n3_mtc3": ("gradp", 3, (256, 256), 64, 96, 3, "f32", {"PSM_DECODE_MTC": "3"}, True),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(_CONFIGS))
def test_gpu_stages_within_bound(name, monkeypatch):
    variant, c_in, (ny, nx), p_in, p_out, n, precision, env, bind = _CONFIGS[name]
    monkeypatch.setenv("PSM_KEEP_HIDDEN", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    model = _model(variant, c_in, p_in, p_out, widths=(512, 512, 512), seed=11)
    grids = _grids(n, ny, nx, c_in, seed=7)
    names, fields = _check(name, model, grids, precision, bind)
    if "PSM_DECODE_MTC" in env:
        mtc = env["PSM_DECODE_MTC"]
        assert any(k.startswith(f"psm_decode_paste_batch_kernel<{mtc},") for k in names), names
        monkeypatch.delenv("PSM_DECODE_MTC")
        names1, _, fields1 = _solve(model, grids, precision, bind)
        assert any(k.startswith("psm_decode_paste_batch_kernel<1,") for k in names1), names1
        np.testing.assert_array_equal(fields, fields1)
        for c in (0, n - 1):             # and against the float64 oracle, the bound test_gpu_parity.py holds bound-path fields to
            ref = orc.solve_grid(grids[c].astype(np.float64), _omodel(model)).fields
            ok = ~np.isnan(ref)
            np.testing.assert_array_equal(np.isnan(fields[c]), ~ok)
            err = np.abs(fields[c][ok] - ref[ok]).max() / np.abs(ref[ok]).max()
            print(f"\n{name} case {c}: max |field - oracle| / max |oracle| = {err:.3g}")
            assert err <= 2e-4, (name, c, err)
    _DONE.add(name)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 5])
def test_gpu_keep_mode_changes_no_launch_and_no_bit(n, monkeypatch):
    """Keep mode changes output pointers only: the same instantiations, bit-identical fields (one case: fused reduce + first
    layer; five cases of 30 blocks: packed Dense chain)."""
    model = _model("gradp", 3, 96, 64, widths=(512, 512, 512), seed=13)
    grids = _grids(n, 256, 256, 3, seed=9)
    monkeypatch.setenv("PSM_KEEP_HIDDEN", "0")
    n0, _, f0 = _solve(model, grids, keep=False)
    monkeypatch.setenv("PSM_KEEP_HIDDEN", "1")
    n1, f1 = _check(f"keep n={n}", model, grids)
    assert n0 == n1
    assert np.array_equal(f0, f1)
    _DONE.add(f"keep_{n}")


_ENC_FORMS = {"psm_encode_kernel": (32, 1, "f32"), "psm_encode_pair_kernel": (128, 1, "f32"), "psm_encode_x6_kernel": (48, 1, "f32"),
              "psm_encode_x6_mt_kernel": (48, 12, "f32"), "psm_encode_bf16_kernel": (48, 1, "bf16")}


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("c_in", [1, 2, 3, 4])
def test_gpu_every_encode_form(c_in, aligned, monkeypatch):
    """Each of the five encode forms (one f32 row tile of one component tile; the pair form; x6 (PSM_X6=1, one row tile); the M-tiled x6
    from 96 rows; bf16) at this c_in, rows 16-byte aligned or not (odd Nx; c_in = 4 through a grid pointer off by one float)."""
    monkeypatch.setenv("PSM_KEEP_HIDDEN", "1")
    nx = 256 if aligned else 257
    for kern, (p_in, n, precision) in _ENC_FORMS.items():
        model = _model("deltas", c_in, p_in, 32, widths=(64,), seed=5)
        grids = _grids(n, 256, nx, c_in, seed=3)
        with monkeypatch.context() as mp:
            if kern == "psm_encode_x6_kernel":       # x6 on one row tile: four channels' LDS planes fit only there
                mp.setenv("PSM_X6", "1")
            names, _ = _check(f"encode {kern} c_in={c_in} aligned={aligned}", model, grids, precision,
                              misalign=not aligned and c_in == 4)
        assert f"{kern}<{c_in},{str(aligned).lower()}>" in names, names
    _DONE.add(f"encode_{c_in}_{aligned}")


@pytest.mark.gpu
def test_gpu_stale_stages_are_refused(monkeypatch):
    """BLOCK_PRED after a bound solve and every stage after a ring solve are PSM_ERR_STATE; a synchronous general solve makes them
    readable again."""
    from psm_amd import GridSurrogate, _lib, synthetic
    model = synthetic.make_model("deltas", p_in=32, p_out=32)
    g = synthetic.channel_grid(256, 256, seed=1).astype(np.float32)
    with GridSurrogate(model, 256, 256) as sur:
        sur.solve(g)
        assert sur.stage("block_pred").shape[0] == sur.B
        assert sur.bind_geometry(g)
        sur.solve(g)
        with pytest.raises(_lib.PsmError) as e:
            sur.stage("block_pred")
        assert e.value.code == -2
        sur.stage("x_input"), sur.stage("offsets")
        for k in range(3 * 8):                             # PSM_RING_SLOTS = 8: from the second turn on, tickets replay slot graphs
            sur.solve(g)
            sur.wait(sur.submit(g))
            for s in ("x_input", "res", "offsets", "shift"):
                with pytest.raises(_lib.PsmError) as e:
                    sur.stage(s)
                assert e.value.code == -2, (k, s)
        sur.solve(g)
        sur.stage("x_input")
        with pytest.raises(_lib.PsmError) as e:            # stage numbers are checked before the state
            sur._chk(sur.lib.psm_read_stage(sur.h, _lib.STAGE_HIDDEN + 7, np.empty(1 << 20, np.float32).ctypes.data_as(C.POINTER(C.c_float)), 1 << 20))
        assert e.value.code == -1
    with monkeypatch.context() as mp:                         # PSM_GRAPH=1: a replay puts back the state its capture left
        mp.setenv("PSM_GRAPH", "1")
        with GridSurrogate(model, 256, 256, max_cases=2) as sur:
            from hipmem import DeviceArray
            g2 = np.stack([g, g])
            d1, d2, o = DeviceArray(g), DeviceArray(g2), DeviceArray(shape=(2, 256, 256, 1))
            assert sur.bind_geometry(g)
            for rep in range(3):                             # first pass captures, the next two replay
                sur._chk(sur.lib.psm_solve_grid_device(sur.h, C.c_void_p(d2.ptr), 2, None, C.c_void_p(o.ptr), None))
                assert sur.stage("block_pred", 2).shape[0] == 2 * sur.B, rep          # general path (2 cases)
                sur._chk(sur.lib.psm_solve_grid_device(sur.h, C.c_void_p(d1.ptr), 1, None, C.c_void_p(o.ptr), None))
                with pytest.raises(_lib.PsmError) as e:                                # bound path (the bound case count)
                    sur.stage("block_pred")
                assert e.value.code == -2, rep
            d1.free(), d2.free(), o.free()
    with GridSurrogate(model, 256, 256) as sur:              # hidden stages need keep mode
        sur.solve(g)
        with pytest.raises(_lib.PsmError) as e:
            _hidden(sur, 2, 1)
        assert e.value.code == -2


# ---------------------------------------------------------------------------------------------------------------------
# The solve-path instantiations of the built library, and which of them this module launches
# ---------------------------------------------------------------------------------------------------------------------
def _b(v):
    return "true" if v else "false"


def solve_path_table():
    """Every solve-path instantiation the launchers compile (the stage files psm_encode / psm_dense / psm_decode / psm_assemble / psm_bound .hip, and psm_bf16.hip), as demangled without spaces."""
    t = set()
    for kern in _ENC_FORMS:
        t |= {f"{kern}<{c},{_b(al)}>" for c in (1, 2, 3, 4) for al in (False, True)}
    t |= {"psm_reduce_kernel", "psm_reduce_dense1_kernel<false>", "psm_reduce_dense1_kernel<true>", "psm_conv1d_kernel",
          "psm_chain_kernel", "psm_paste_kernel", "psm_act_dots_kernel", "psm_res_dots_kernel"}
    t |= {f"psm_dense_kernel<{n},{_b(bf)},{r},false,{_b(ln)}>" for n in (1, 2, 4) for bf in (0, 1) for r in (16, 32) for ln in (0, 1)}
    t |= {f"psm_dense_kernel<{n},false,{r},true,false>" for n in (1, 2, 4) for r in (16, 32)}
    t |= {f"psm_layernorm_kernel<{k}>" for k in (0, 8, 16)} | {f"psm_decode128_kernel<{m}>" for m in (1, 2, 3, 4)}
    t |= {f"psm_decode_kernel<{m},{g}>" for m in (1, 2, 4) for g in (4, 16)} | {f"psm_decode_bf16_kernel<{m}>" for m in (1, 2, 4)}
    t |= {f"psm_{k}_kernel<{c}>" for k in ("strips", "assemble", "chain_dots") for c in (1, 2)}
    t |= {f"psm_decode_paste_kernel<{m},{c},{l},{a}>" for m in (1, 2) for c in (1, 2) for l in (32, 64, 96, 128) for a in (0, 1, 2)}
    t |= {f"psm_decode_paste_batch_kernel<{m},{c},{l},{a}>" for m in (1, 2, 3) for c in (1, 2) for l in (32, 64, 96, 128)
          for a in (0, 1, 2)}
    return t


# kernel families of the library outside this table, and where they are tested
OUT_OF_SCOPE = {
    **{f"psm_{k}_kernel": "convolutional path (test_unet_layer_oracle.py)"
       for k in ("conv3x3", "conv_stem", "head1x1", "pair32", "pair_stem16", "pair_up16")},
    **{f"psm_{k}_kernel": "mesh <-> grid (test_mesh_path.py)"
       for k in ("interp_to_grid", "to_grid", "to_mesh", "umax", "umax_partial", "stage_cells")},
    **{f"psm_{k}_kernel": "Poisson features, filter, gradP integration (test_grid_stage_oracle.py: elementwise float64 oracles)"
       for k in ("poisson_grid", "poisson_term", "gauss1d", "integ_rows", "integ_cols", "integ_write")},
    **{f"psm_{k}_kernel": "geometry bind (test_bound_geometry.py)" for k in ("bind_rows", "bind_fold", "bind_own", "bind_copy", "pair_fold")},
    "psm_split_basis_kernel": "x6 basis split, once per handle", "psm_stage_in_kernel": "ring stage-in (test_ring.py)",
    "psm_label_blocks_kernel": "evaluator labels (test_block_error.py)", "psm_block_error_kernel": "evaluator (test_block_error.py)",
}

# launched by this module's GPU tests (test_zz_coverage asserts exactly this set)
SWEPT = {
    "psm_assemble_kernel<1>", "psm_assemble_kernel<2>", "psm_chain_dots_kernel<2>", "psm_chain_kernel",
    "psm_decode128_kernel<1>", "psm_decode128_kernel<4>", "psm_decode_bf16_kernel<1>", "psm_decode_bf16_kernel<4>",
    "psm_decode_kernel<1,4>", "psm_decode_kernel<2,4>", "psm_decode_kernel<4,4>", "psm_decode_paste_batch_kernel<1,2,96,2>",
    "psm_decode_paste_batch_kernel<2,2,96,2>", "psm_decode_paste_batch_kernel<3,2,96,2>",
    "psm_decode_paste_kernel<1,1,128,1>", "psm_decode_paste_kernel<1,1,32,2>", "psm_dense_kernel<1,false,16,false,false>",
    "psm_dense_kernel<1,false,32,false,false>", "psm_dense_kernel<1,true,16,false,false>",
    "psm_dense_kernel<1,true,32,false,false>", "psm_dense_kernel<2,false,32,false,false>",
    "psm_dense_kernel<4,false,16,false,false>", "psm_dense_kernel<4,false,16,true,false>",
    "psm_dense_kernel<4,false,32,false,false>", "psm_dense_kernel<4,false,32,true,false>", "psm_dense_kernel<4,true,16,false,false>",
    "psm_dense_kernel<4,true,32,false,false>", "psm_encode_bf16_kernel<1,false>", "psm_encode_bf16_kernel<1,true>",
    "psm_encode_bf16_kernel<2,false>", "psm_encode_bf16_kernel<2,true>", "psm_encode_bf16_kernel<3,false>",
    "psm_encode_bf16_kernel<3,true>", "psm_encode_bf16_kernel<4,false>", "psm_encode_bf16_kernel<4,true>",
    "psm_encode_kernel<1,false>", "psm_encode_kernel<1,true>", "psm_encode_kernel<2,false>", "psm_encode_kernel<2,true>",
    "psm_encode_kernel<3,false>", "psm_encode_kernel<3,true>", "psm_encode_kernel<4,false>", "psm_encode_kernel<4,true>",
    "psm_encode_pair_kernel<1,false>", "psm_encode_pair_kernel<1,true>", "psm_encode_pair_kernel<2,false>",
    "psm_encode_pair_kernel<2,true>", "psm_encode_pair_kernel<3,false>", "psm_encode_pair_kernel<3,true>",
    "psm_encode_pair_kernel<4,false>", "psm_encode_pair_kernel<4,true>", "psm_encode_x6_kernel<1,false>",
    "psm_encode_x6_kernel<1,true>", "psm_encode_x6_kernel<2,false>", "psm_encode_x6_kernel<2,true>",
    "psm_encode_x6_kernel<3,false>", "psm_encode_x6_kernel<3,true>", "psm_encode_x6_kernel<4,false>",
    "psm_encode_x6_kernel<4,true>", "psm_encode_x6_mt_kernel<1,false>", "psm_encode_x6_mt_kernel<1,true>",
    "psm_encode_x6_mt_kernel<2,false>", "psm_encode_x6_mt_kernel<2,true>", "psm_encode_x6_mt_kernel<3,false>",
    "psm_encode_x6_mt_kernel<3,true>", "psm_encode_x6_mt_kernel<4,false>", "psm_encode_x6_mt_kernel<4,true>",
    "psm_paste_kernel", "psm_reduce_dense1_kernel<false>", "psm_reduce_dense1_kernel<true>", "psm_reduce_kernel",
    "psm_res_dots_kernel", "psm_strips_kernel<1>", "psm_strips_kernel<2>"
}


def not_swept_reason(k):
    """Why a table entry is not in SWEPT."""
    if k.startswith(("psm_layernorm_kernel", "psm_conv1d_kernel")) or (k.startswith("psm_dense_kernel") and k.endswith(",true>")):
        return "LayerNormalization / Conv1D head: not read back, not swept here (test_attention.py, test_conv1d_head.py, normwise)"
    if k.startswith("psm_decode_paste_batch_kernel<2") or k.startswith("psm_decode_paste_batch_kernel<3"):
        return "reachable with PSM_DECODE_MTC=2 / 3 (read per handle): launched at two fields, 96 components, x6 only, their fields held bit for bit to the one-tile form; the other C / LDR / arithmetic combinations are not launched by this module yet"
    if k == "psm_act_dots_kernel":
        return "runs only inside psm_read_stage(OFFSETS / SHIFT) after a closed-form solve"
    return "reachable, not launched by this module yet"


def test_library_holds_exactly_the_solve_path_table():
    """The built library's PCA-path kernels are the table above (220): a kernel added to a launcher fails here until listed.  Every
    other kernel family of the library is named in OUT_OF_SCOPE."""
    import os
    from kernel_symbols import library_kernels
    from psm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} not built")
    lib = library_kernels(_lib.LIB_PATH)
    table = solve_path_table()
    assert len(table) == 220
    fams = {k.split("<")[0] for k in table}
    assert not {k.split("<")[0] for k in lib} - fams - set(OUT_OF_SCOPE), sorted({k.split("<")[0] for k in lib} - fams - set(OUT_OF_SCOPE))
    solve = {k for k in lib if k.split("<")[0] in fams}
    assert solve == table, (sorted(solve - table)[:10], sorted(table - solve)[:10])
    assert SWEPT <= table


_ALL_GPU_TESTS = set(_CONFIGS) | {"keep_1", "keep_5"} | {f"encode_{c}_{a}" for c in (1, 2, 3, 4) for a in (True, False)}


@pytest.mark.gpu
def test_zz_report():
    for k, (v, tag) in sorted(_STATS.items()):
        print(f"\nstage oracle: worst |dev - r| / E of {k}: {v:.3g} ({tag})")
    table = solve_path_table()
    print(f"kernels launched: {len(_RAN & table)} of {len(table)}: {sorted(_RAN & table)}")
    assert not (_RAN - table - set(OUT_OF_SCOPE)), sorted(_RAN - table)
    missing = _ALL_GPU_TESTS - _DONE
    if missing:
        pytest.skip(f"coverage needs the whole module; not run or failed: {sorted(missing)}")
    assert _RAN & table == SWEPT, ("not launched:", sorted(SWEPT - _RAN), "launched, not in SWEPT:", sorted((_RAN & table) - SWEPT))
