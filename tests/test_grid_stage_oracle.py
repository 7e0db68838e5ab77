"""The kernels that run around a solve on the grid -- Gaussian post-steps (csrc/psm_filter.hip), gradP -> p integration
(csrc/psm_integ.hip), Poisson input features (csrc/psm_features.hip) -- against elementwise float64 oracles with a-priori bounds
(oracle/grid_stage_oracle.py), at the tile and chunk edges of each kernel, through the shape-free host entries
(psm_gaussian_filter, psm_set_integration + psm_integrate_gradp, psm_poisson_features) and the device-batched entries of two
handles planned at 129 x 131 with max_cases = 3.

CPU: a float32 (features: float64) restatement of each kernel's own summation order lies at <= 0.5 of its bound on every named
case -- a condition on the reference alone: it checks the derivation of each bound -- and every planted fault exceeds the bound
on a named case and is flagged on its own kernel only.
GPU: every test prints its worst |dev - ref| / E before it asserts <= 1 and the equality of the NaN patterns.

What the bounds cannot see: anything below E.  On unit-normal input a dropped edge tap (e^-8 of the weight) is below E; the
impulse images, where E is gamma x one tap per output, are what catches it.

Measured on an MI355X (test_zz_report prints it; the GPU part of the module runs in 1.4 s, no test above 0.1 s), worst
|dev - ref| / E: filter 0.262 on random fields through the host entry (19 x 67, radius 1; 0.0067 / 0.0010 / 0.0075 on the 605- /
721- / 1281-tap cases), 0.0023 on the impulse images with and without the NaN, 0.056 device-batched, 0.039 over the post-step
chain; integration 0.048 on random gradients (9 x 70, cut (1, 64)), 0.0086 on the impulse gradients, 0.012 device-batched;
features channel 0 0.997 -- E there is one float32 rounding of a float64 value, which a correctly rounded store attains; before
the store the float64 restatement lies at <= 0.0075 of the mean / std term -- and channels 1-3 bit-equal to float32(oracle).
No kernel defect was found.  The library does not report which LDS grant (160 KB: 604-tap chunks, 64 KB: 228-tap chunks) its
filter launches saw; the multi-chunk cases split under either, and the summation order -- hence every bit of the output -- is
the same under both."""
import functools

import numpy as np
import pytest
import scipy.ndimage as ndi

from oracle import grid_stage_oracle as go
from oracle import psm_oracle as orc

NY, NX, NCASES = 129, 131, 3

# ---------------------------------------------------------------------------------------------------------------------
# named cases
# ---------------------------------------------------------------------------------------------------------------------
FILTER_FIELDS = ([((1, 1), (0.3, 160.0)), ((3, 5), (0.1, 0.1)), ((3, 5), (0.3, 0.2))]
                 + [((19, 67), (r / 4, r / 4)) for r in range(1, 9)]                       # 3 .. 17 taps: every nt % 4, nfull 0 .. 4
                 + [(s, (2.5, 7.0)) for s in ((15, 63), (16, 64), (17, 65))]               # axis-0 tile - 1, exact, + 1
                 + [(s, (2.5, 7.0)) for s in ((5, 255), (5, 256), (5, 257), (6, 258), (7, 259))]     # axis-1 tile edges, nx % 4 = 3 0 1 2 3
                 + [((33, 259), (1.0, 75.6)),                                              # 605 taps: one more than a 604-tap chunk
                    ((17, 65), (80.0, 90.0)),                                              # 641 / 721 taps, radius wraps the extent ~19 times
                    ((20, 70), (160.0, 0.5))])                                             # 1281 taps: three chunks
FILTER_IDS = [f"{s[0]}x{s[1]}-{g[0]:g}-{g[1]:g}" for s, g in FILTER_FIELDS]
IMPULSE_ROWS, IMPULSE_COLS = (0, 15, 16, 351, 703), (0, 63, 64, 65)
IMPULSE_T_COLS = (0, 255, 256, 749, 1499)
IMPULSES = [f"rows_{r}" for r in IMPULSE_ROWS] + ["cols", "rows_nan", "cols_nan"]


@functools.lru_cache(maxsize=None)
def filter_field(i):
    shape, sigma = FILTER_FIELDS[i]
    x = np.random.default_rng(100 + i).standard_normal(shape).astype(np.float32)
    return x, sigma, go.gauss_stage(x, 0.0, sigma)


@functools.lru_cache(maxsize=None)
def impulse(name):
    """704 x 66, sigma (80, 0.1): one row of IMPULSE_ROWS per image (axis 1 has radius 0: the four columns do not mix); its transpose
    case 6 x 1500, sigma (0.1, 80): one column of IMPULSE_T_COLS per row.  *_nan: one NaN at the centre of the image."""
    if name.startswith("rows"):
        x, sigma = np.zeros((704, 66), np.float32), (80.0, 0.1)
        x[351 if name == "rows_nan" else int(name[5:]), list(IMPULSE_COLS)] = 1.0
        if name == "rows_nan":
            x[352, 33] = np.nan
    else:
        x, sigma = np.zeros((6, 1500), np.float32), (0.1, 80.0)
        x[np.arange(5), list(IMPULSE_T_COLS)] = 1.0
        if name == "cols_nan":
            x[3, 750] = np.nan
    return x, sigma, go.gauss_stage(x, 0.0, sigma)


INTEG_SHAPES = [(2, 3, 1, 1), (2, 3, 1, 2), (9, 70, 1, 64), (9, 130, 8, 65), (257, 67, 256, 1), (513, 131, 257, 66),
                (7, 200, 3, 199), (15, 193, 7, 129)]
IMP = (257, 131, 128, 65)
IMPULSE_GX = sorted({0, 63, 64, IMP[3] - 2, IMP[3] - 1, IMP[3], IMP[1] - 1})   # dp/dx = 1 at one pixel of these columns (cx - 2 = 63, cx - 1 = 64)
IMPULSE_GY = [0, IMP[2] - 1, IMP[2], 255, 256]                                # dp/dy = 1 at one pixel of column 0 / nx-1, these rows
INTEG_NAMES = (["%dx%d_%d_%d" % s for s in INTEG_SHAPES] + ["fixups_beyond_lane_63", "four_indices", "empty_selection"]
               + [f"gx_{c}" for c in IMPULSE_GX] + [f"gy_{s}_{r}" for s in ("l", "r") for r in IMPULSE_GY])


def _gradients(ny, nx, seed):
    return np.random.default_rng(seed).standard_normal((ny, nx, 2)).astype(np.float32)


def integ_geometry(name):
    """-> (gradp float32 [ny,nx,2], sdf, cy, cx)."""
    if name == "fixups_beyond_lane_63":
        ny, nx, cy, cx = 12, 200, 6, 100
        sdf = np.full((ny, nx), 0.5)
        sdf[2:5, 20:40] = 70.3            # index 70: the second 64-lane chunk of the fix-up pre-pass
        sdf[8:10, 150:160] = 65.9         # rows beyond the taller half: read by no quadrant-local row
        sdf[5:7, 98:102] = 0.0            # solids on both cut columns, equal counts
        return _gradients(ny, nx, 7), sdf, cy, cx
    if name in ("four_indices", "five_indices"):
        ny, nx, cy, cx = 9, 130, 4, 65
        sdf = np.full((ny, nx), 0.5)
        sdf[1, 10:13] = (3.2, 64.9, 5.7)  # {0, 3, 64, 5}: replacement values that are differences of two distinct prefix sums
        if name == "five_indices":
            sdf[1, 13] = 7.1
        return _gradients(ny, nx, 8), sdf, cy, cx
    if name == "empty_selection":
        ny, nx, cy, cx = 9, 70, 4, 30
        sdf = np.full((ny, nx), 0.5)
        sdf[:cy, cx - 1:cx + 1] = 0.0     # both cut columns solid over the whole top half
        return _gradients(ny, nx, 9), sdf, cy, cx
    if name.startswith("g"):
        ny, nx, cy, cx = IMP
        g = np.zeros((ny, nx, 2), np.float32)
        if name.startswith("gx"):
            g[100 if int(name[3:]) % 2 else 200, int(name[3:]), 0] = 1.0
        else:
            g[int(name[5:]), 0 if name[3] == "l" else nx - 1, 1] = 1.0
        return g, np.full((ny, nx), 0.5), cy, cx
    ny, nx, cy, cx = INTEG_SHAPES[["%dx%d_%d_%d" % s for s in INTEG_SHAPES].index(name)]
    return _gradients(ny, nx, ny * 1000 + nx), np.full((ny, nx), 0.5), cy, cx


@functools.lru_cache(maxsize=None)
def integ_case(name):
    g, sdf, cy, cx = integ_geometry(name)
    ny, nx = sdf.shape
    dx, dy = 1.0 / nx, 1.0 / ny
    return g, sdf, dx, dy, cy, cx, go.integ_bound(g, sdf, dx, dy, cy, cx)


FEATURE_SHAPES = [(2, 2), (2, 3), (3, 2), (16, 16), (2, 128), (2, 129), (257, 257)]
FEATURE_IDS = ["%dx%d" % s for s in FEATURE_SHAPES]
L_, U_, K_, MAX_ABS = 0.3, 1.7, 2.5, (3.1, 0.7, 0.9, 1.3)


@functools.lru_cache(maxsize=None)
def feature_case(shape):
    """Random velocities; a solid corner; from 16 x 16 on also a solid border row, an interior patch and one NaN velocity cell
    next to the border (images with a row of two keep the corner only: a solid border row would leave no cell with a gradient)."""
    ny, nx = shape
    rng = np.random.default_rng(ny * 1000 + nx)
    ux, uy, dux, duy = (rng.standard_normal((ny, nx)) for _ in range(4))
    sdf = 0.1 + rng.random((ny, nx))
    sdf[0, 0] = 0.0
    nan = np.zeros((ny, nx), bool)
    if min(ny, nx) >= 16:
        sdf[:2, :2] = 0.0
        sdf[0, :] = 0.0                   # the first row: the last rows stay in the flow, so the last workgroups' partials are not zero
        sdf[ny // 2:ny // 2 + 3, nx // 2:nx // 2 + 2] = 0.0
        nan[ny // 4, 1] = True
    elif nx >= 128:
        nan[0, nx // 2] = True
    for a in (ux, uy, dux, duy):
        a[sdf == 0] = 0.0
        a[nan] = np.nan
    args = (ux, uy, dux, duy, sdf, L_, U_, K_, MAX_ABS)
    return args, nan, go.features_bound(*args)


# ---------------------------------------------------------------------------------------------------------------------
# CPU: each mirror inside its bound
# ---------------------------------------------------------------------------------------------------------------------
MIRROR_MAX = 0.5


@pytest.mark.parametrize("i", range(len(FILTER_FIELDS)), ids=FILTER_IDS)
def test_filter_mirror_inside_bound_fields(i):
    x, sigma, (y, E) = filter_field(i)
    r = max(go.worst_ratio(go.filter_mirror(x, sigma, chunk), y, E) for chunk in (604, 228))
    print(f"filter mirror {FILTER_IDS[i]}: {r:.3g}")
    assert r <= MIRROR_MAX
    with np.errstate(invalid="ignore"):
        assert go.worst_ratio(ndi.gaussian_filter(x.astype(np.float64), sigma, order=0), y, E) <= 1e-6      # same operation as SciPy's


@pytest.mark.parametrize("name", IMPULSES)
def test_filter_mirror_inside_bound_impulses(name):
    x, sigma, (y, E) = impulse(name)
    r = go.worst_ratio(go.filter_mirror(x, sigma), y, E)
    print(f"filter mirror impulse {name}: {r:.3g}")
    assert r <= MIRROR_MAX
    if name.endswith("nan"):
        nan = np.isnan(y)
        assert nan.sum() == 641 and (y[~nan] != 0).any()            # one NaN under 641 taps; finite values beside it


@pytest.mark.parametrize("name", INTEG_NAMES)
def test_integ_mirror_inside_bound(name):
    g, sdf, dx, dy, cy, cx, (p, E) = integ_case(name)
    r = go.worst_ratio(go.integ_mirror(g, sdf, dx, dy, cy, cx), p, E)
    print(f"integration mirror {name}: {r:.3g}")
    assert r <= MIRROR_MAX


@pytest.mark.parametrize("shape", FEATURE_SHAPES, ids=FEATURE_IDS)
def test_features_mirror_inside_bound(shape):
    """The float64 restatement before the store against the bound without the store's rounding: this is what checks the mean / std
    term.  (A correctly rounded float32 store alone reaches 1.0 of a one-rounding bound, so the stored value is held to E itself.)"""
    args, nan, (grid, E) = feature_case(shape)
    E64 = go.features_bound(*args, cast=False)[1]
    r64 = go.worst_ratio(go.features_mirror(*args, cast=False)[..., 0], grid[..., 0], E64[..., 0])
    m = go.features_mirror(*args)
    r = go.worst_ratio(m[..., 0], grid[..., 0], E[..., 0])
    print(f"features mirror {shape}: channel 0 before the store {r64:.3g}, stored {r:.3g}")
    assert r64 <= MIRROR_MAX and r <= 1.0
    assert np.array_equal(m[..., 1:], grid[..., 1:].astype(np.float32))
    assert (E[..., 1:] == 0).all() and np.isfinite(E).all()


def test_named_geometries_are_ones_the_reference_processes():
    """Equal flow-cell counts on the cut columns, int(sdf) inside both block rows, at most 4 distinct int(sdf) per row; finite p
    except under the empty selection; the five-index row is refused."""
    for name in INTEG_NAMES:
        g, sdf, dx, dy, cy, cx, (p, E) = integ_case(name)
        fix, mask, npair = go.integ_tables(sdf, cy, cx)
        assert max(len(f) for f in fix) <= go.MAX_FIX
        if name == "empty_selection":
            want = np.zeros(p.shape, bool)
            want[:cy, :cx] = True
            assert npair[0] == 0 and np.array_equal(np.isnan(p), want)
        else:
            assert min(npair) > 0 and np.isfinite(p).all() and np.isfinite(E).all()
    assert max(len(f) for f in go.integ_tables(*integ_geometry("four_indices")[1:])[0]) == 4
    assert max(v for f in go.integ_tables(*integ_geometry("fixups_beyond_lane_63")[1:])[0] for v, _ in f) == 70
    with pytest.raises(go.Unsupported):
        go.integ_tables(*integ_geometry("five_indices")[1:])
    for variant in ("gradp", "deltas"):                                 # both handles of the GPU part plan
        assert orc.block_layout(variant, NY, NX).B >= 1


# ---------------------------------------------------------------------------------------------------------------------
# CPU: planted faults
# ---------------------------------------------------------------------------------------------------------------------
def _filter_ratio(case, fault=None, chunk=604):
    x, sigma, (y, E) = impulse(case) if isinstance(case, str) else filter_field(case)
    return go.worst_ratio(go.filter_mirror(x, sigma, chunk, fault), y, E)


def _integ_ratio(case, fault=None):
    g, sdf, dx, dy, cy, cx, (p, E) = integ_case(case)
    return go.worst_ratio(go.integ_mirror(g, sdf, dx, dy, cy, cx, fault), p, E)


def _features_ratio(case, fault=None):
    args, nan, (grid, E) = feature_case(case)
    m = go.features_mirror(*args, fault=fault)
    return max(go.worst_ratio(m[..., 0], grid[..., 0], E[..., 0]), go.worst_ratio(m[..., 1:], grid[..., 1:].astype(np.float32), E[..., 1:]))


_RATIO = {"filter": _filter_ratio, "integration": _integ_ratio, "features": _features_ratio}
_QUIET = {"filter": FILTER_IDS.index("17x65-2.5-7"), "integration": "9x70_1_64", "features": (16, 16)}      # the other kernels' clean run
_F17 = FILTER_IDS.index("17x65-2.5-7")
FAULTS = [("filter", "chunk_first_tap_dropped", "cols"), ("filter", "chunk_first_tap_dropped", "rows_351"),
          ("filter", "whole_sample_reflection", _F17), ("filter", "column_64_from_63", _F17),
          ("filter", "fourth_output_row_shifted", _F17), ("filter", "nan_from_slack", "cols_nan"), ("filter", "nan_from_slack", "rows_nan"),
          ("integration", "chunk_carry_dropped", "9x130_8_65"), ("integration", "right_side_inclusive", "2x3_1_1"),
          ("integration", "right_side_writes_cut_column", "9x70_1_64"), ("integration", "bottom_half_from_cut_row", "9x70_1_64"),
          ("integration", "npair_swapped", "9x70_1_64"), ("integration", "fixup_beyond_lane_63_ignored", "fixups_beyond_lane_63"),
          ("integration", "fixup_beyond_lane_63_ignored", "four_indices"), ("integration", "last_single_row_skipped", "9x70_1_64"),
          ("features", "partials_beyond_256_not_folded", (257, 257)), ("features", "border_difference_halved", (16, 16))]


@functools.lru_cache(maxsize=None)
def _clean(kernel):
    return _RATIO[kernel](_QUIET[kernel])


@pytest.mark.parametrize("kernel,fault,case", FAULTS, ids=[f"{k}-{f}-{c}" for k, f, c in FAULTS])
def test_planted_fault_exceeds_the_bound_on_its_kernel(kernel, fault, case):
    ratios = {k: (_RATIO[k](case, fault) if k == kernel else _clean(k)) for k in _RATIO}
    print(f"{fault} on {case}: " + " ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    assert [k for k, v in ratios.items() if v > 1] == [kernel]
    assert _RATIO[kernel](case) <= (1.0 if kernel == "features" else MIRROR_MAX)      # the same case without the fault


def test_a_dropped_edge_tap_is_below_the_bound_on_unit_normal_input():
    """Why the impulse images exist: the fault the impulses flag passes on the 605-tap random field."""
    i = FILTER_IDS.index("33x259-1-75.6")
    assert _filter_ratio(i, "chunk_first_tap_dropped") <= 1 < _filter_ratio("cols", "chunk_first_tap_dropped")
    assert _filter_ratio("cols", "chunk_first_tap_dropped", 228) > 1


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
_STATS = {}


def _hold(kernel, family, name, dev, ref, E):
    r = go.worst_ratio(dev, ref, E)
    print(f"{kernel} / {family} / {name}: worst |dev - ref| / E = {r:.3g}, NaN pattern equal {np.array_equal(np.isnan(dev), np.isnan(ref))}")
    _STATS[(kernel, family)] = max(_STATS.get((kernel, family), 0.0), r)
    assert np.array_equal(np.isnan(dev), np.isnan(ref)) and r <= 1.0, (kernel, family, name, r)
    return r


@pytest.fixture(scope="module")
def handles():
    from psm_amd import GridSurrogate, synthetic
    sur = {v: GridSurrogate(synthetic.make_model(v, p_in=8, p_out=8), NY, NX, max_cases=NCASES) for v in ("gradp", "deltas")}
    print("LDS grant of the filter launches: not reported by the library (604-tap chunks with 160 KB, 228-tap chunks with 64 KB)")
    yield sur
    for s in sur.values():
        s.close()


def _dev(a):
    from hipmem import DeviceArray
    return DeviceArray(np.ascontiguousarray(a, np.float32))


def _empty(shape):
    from hipmem import DeviceArray
    return DeviceArray(shape=shape)


# ---- filter ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(FILTER_FIELDS)), ids=FILTER_IDS)
def test_gpu_filter_host_entry_fields(handles, i):
    x, sigma, (y, E) = filter_field(i)
    _hold("filter", "host entry, random fields", FILTER_IDS[i], handles["deltas"].gaussian_filter(x, sigma), y, E)


@pytest.mark.gpu
@pytest.mark.parametrize("name", IMPULSES)
def test_gpu_filter_host_entry_impulses(handles, name):
    """Every output a single tap or a few reflected taps, the bound relative to that tap; with the NaN: NaN exactly where SciPy
    has it across the chunk boundaries, finite values inside the bound."""
    x, sigma, (y, E) = impulse(name)
    _hold("filter", "host entry, NaN" if name.endswith("nan") else "host entry, impulses", name, handles["gradp"].gaussian_filter(x, sigma), y, E)


@pytest.mark.gpu
@pytest.mark.parametrize("sigma", [(0.3, 75.6), (2.5, 7.0)], ids=["0.3-75.6", "2.5-7"])
def test_gpu_filter_device_batch(handles, sigma):
    """psm_filter_fields_device, c = 2, n = 3 on the 129 x 131 plan: out of place and in place; case i alone is bit-identical."""
    sur = handles["gradp"]
    f = np.random.default_rng(31).standard_normal((NCASES, NY, NX, 2)).astype(np.float32)
    sur.bind_poststeps(sigma, (50.0, 50.0))
    d_in, d_out, d_ip, d_one = _dev(f), _empty(f.shape), _dev(f), _empty(f.shape[1:])
    sur.filter_device(d_in.ptr, NCASES, d_out.ptr)
    sur.filter_device(d_ip.ptr, NCASES, d_ip.ptr)
    sur.synchronize()
    got, inplace = d_out.numpy(), d_ip.numpy()
    for i in range(NCASES):
        for k in range(2):
            y, E = go.gauss_stage(f[i, ..., k], 0.0, sigma)
            _hold("filter", "device batch", f"sigma {sigma} case {i} channel {k}", got[i, ..., k], y, E)
        sur.filter_device(d_in.ptr + i * f[0].nbytes, 1, d_one.ptr)
        sur.synchronize()
        assert np.array_equal(d_one.numpy(), got[i]), f"case {i} alone differs from case {i} of the batch"
    assert np.array_equal(inplace, got)
    for d in (d_in, d_out, d_ip, d_one):
        d.free()


S_FIELD, S_WEIGHT = (2.5, 7.0), (50.0, 75.6)         # the weight filter: 401 / 605 taps, two chunks in the pass with the epilogue


def _poststeps(sur, fields, dU, prev, apply_filter, change=True, nxt=True, alias=False):
    n = fields.shape[0]
    d_f, d_u, d_p = _dev(fields), _dev(dU), _dev(prev)
    d_r = d_f if alias else _empty(fields.shape)
    d_c = _empty(fields.shape) if change else None
    d_n = _empty(fields.shape) if nxt else None
    sur.poststeps_device(d_f.ptr, n, d_r.ptr, apply_filter, d_u.ptr, d_p.ptr, d_c.ptr if change else 0, d_n.ptr if nxt else 0)
    sur.synchronize()
    out = {"result": d_r.numpy(), "change": d_c.numpy() if change else None, "next": d_n.numpy() if nxt else None}
    for d in {id(d): d for d in (d_f, d_u, d_p, d_r, d_c, d_n) if d is not None}.values():
        d.free()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("apply_filter", [True, False], ids=["filtered", "unfiltered"])
def test_gpu_poststeps_device_chain(handles, apply_filter):
    """psm_poststeps_device, n = 3, against poststep_chain; change / next each left out, the result over the input, case 1 alone."""
    sur = handles["deltas"]
    rng = np.random.default_rng(41)
    fields = rng.standard_normal((NCASES, NY, NX)).astype(np.float32)
    dU = np.abs(rng.standard_normal((NCASES, NY, NX))).astype(np.float32)
    prev = (0.3 * rng.standard_normal((NCASES, NY, NX))).astype(np.float32)
    sur.bind_poststeps(S_FIELD, S_WEIGHT)
    got = _poststeps(sur, fields, dU, prev, apply_filter)
    for i in range(NCASES):
        ref = go.poststep_chain(fields[i], dU[i], prev[i], apply_filter, S_FIELD, S_WEIGHT)
        for key, (v, E) in ref.items():
            _hold("filter", "post-step chain", f"apply_filter={apply_filter} case {i} {key}", got[key][i], v, E)
    only_c = _poststeps(sur, fields, dU, prev, apply_filter, nxt=False)
    only_n = _poststeps(sur, fields, dU, prev, apply_filter, change=False)
    alias = _poststeps(sur, fields, dU, prev, apply_filter, alias=True)
    one = _poststeps(sur, fields[1:2], dU[1:2], prev[1:2], apply_filter)
    assert only_c["next"] is None and only_n["change"] is None
    for other, keys in ((only_c, ("result", "change")), (only_n, ("result", "next")), (alias, ("result", "change", "next"))):
        for key in keys:
            assert np.array_equal(other[key], got[key]), key
    for key in ("result", "change", "next"):
        assert np.array_equal(one[key][0], got[key][1]), key


# ---- integration -----------------------------------------------------------------------------------------------------
def _host_integrate(sur, name):
    g, sdf, dx, dy, cy, cx, (p, E) = integ_case(name)
    sur.set_integration(sdf, cy, cx, dx, dy)
    return sur.integrate_gradp(g), p, E


@pytest.mark.gpu
@pytest.mark.parametrize("name", INTEG_NAMES)
def test_gpu_integration_host_entry(handles, name):
    """Random gradients on the edge shapes, fix-up indices beyond lane 63, four distinct indices on a row, the empty selection (NaN
    on rows < cy, columns < cx as in the oracle), and the impulse gradients whose p is a step function."""
    got, p, E = _host_integrate(handles["gradp"], name)
    family = "impulse gradients" if name.startswith("g") else "random gradients"
    _hold("integration", "host entry, " + family, name, got, p, E)


@pytest.mark.gpu
def test_gpu_integration_refuses_five_indices_and_keeps_the_geometry(handles):
    from psm_amd import _lib
    sur = handles["gradp"]
    before, p, E = _host_integrate(sur, "four_indices")
    g5, sdf5, cy, cx = integ_geometry("five_indices")
    with pytest.raises(_lib.PsmError) as e:
        sur.set_integration(sdf5, cy, cx, 1.0 / sdf5.shape[1], 1.0 / sdf5.shape[0])
    assert e.value.code == -5, e.value                                   # PSM_ERR_UNSUPPORTED
    after = sur.integrate_gradp(integ_case("four_indices")[0])
    assert np.array_equal(before, after)
    _hold("integration", "host entry, random gradients", "four_indices after a refused geometry", after, p, E)


@pytest.mark.gpu
def test_gpu_integration_ignores_inner_dpdy(handles):
    """dp/dy enters through columns 0 and nx-1 only: changing it anywhere else leaves p bit-identical."""
    sur = handles["gradp"]
    g, sdf, dx, dy, cy, cx, _ = integ_case("15x193_7_129")
    sur.set_integration(sdf, cy, cx, dx, dy)
    base = sur.integrate_gradp(g)
    g2 = g.copy()
    g2[:, 1:-1, 1] = np.random.default_rng(5).standard_normal(g2[:, 1:-1, 1].shape).astype(np.float32) * 100
    assert np.array_equal(sur.integrate_gradp(g2), base)
    g2[:, 0, 1] += 1.0
    assert not np.array_equal(sur.integrate_gradp(g2), base)


@pytest.mark.gpu
def test_gpu_integration_device_batch(handles):
    """psm_bind_integration on the 129 x 131 plan, n = 3, cuts (1,1), (64,65), (128,130): each case against its own oracle and
    bit-identical to the same case bound alone."""
    sur = handles["gradp"]
    cuts = [(1, 1), (64, 65), (128, 130)]
    sdf = np.full((NCASES, NY, NX), 0.5)
    sdf[1, 10:20, 30:50] = 40.2                                          # a second fix-up index on rows of both halves of case 1
    sdf[1, 60:70, 64:66] = 0.0                                           # solids on both cut columns, either side of the cut row
    g = np.random.default_rng(51).standard_normal((NCASES, NY, NX, 2)).astype(np.float32)
    dx, dy = 1.0 / NX, 1.0 / NY
    assert sur.bind_integration(sdf, [c[0] for c in cuts], [c[1] for c in cuts], dx, dy)
    d_g, d_p, d_one = _dev(g), _empty((NCASES, NY, NX)), _empty((1, NY, NX))
    sur.integrate_device(d_g.ptr, NCASES, d_p.ptr)
    sur.synchronize()
    got = d_p.numpy()
    for i, (cy, cx) in enumerate(cuts):
        p, E = go.integ_bound(g[i], sdf[i], dx, dy, cy, cx)
        _hold("integration", "device batch", f"case {i} cut {(cy, cx)}", got[i], p, E)
    for i, (cy, cx) in enumerate(cuts):
        assert sur.bind_integration(sdf[i], cy, cx, dx, dy)
        sur.integrate_device(d_g.ptr + i * g[0].nbytes, 1, d_one.ptr)
        sur.synchronize()
        assert np.array_equal(d_one.numpy()[0], got[i]), f"case {i} bound alone differs from case {i} of the batch"
    sur.unbind_integration()
    for d in (d_g, d_p, d_one):
        d.free()


# ---- features --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape", FEATURE_SHAPES, ids=FEATURE_IDS)
def test_gpu_features_host_entry(handles, shape):
    """Channels 1-3 bit-equal to float32(oracle), channel 0 inside its bound; the SDF channel exactly 0 on solids, the velocity
    channels exactly 0 on the NaN cell; channel 0 of every cell whose term is masked (solid, NaN, or next to one) is one value."""
    args, nan, (grid, E) = feature_case(shape)
    got = handles["deltas"].poisson_features(*args)
    assert got.dtype == np.float32 and got.shape == grid.shape
    _hold("features", "channel 0", "%dx%d" % shape, got[..., 0], grid[..., 0], E[..., 0])
    same = np.array_equal(got[..., 1:], grid[..., 1:].astype(np.float32))
    print(f"features {shape}: channels 1-3 bit-equal to float32(oracle): {same}")
    _STATS[("features", "channels 1-3 bit-equal")] = min(_STATS.get(("features", "channels 1-3 bit-equal"), 1.0), float(same))
    assert same
    solid = args[4] == 0
    assert (got[..., 3][solid] == 0).all() and (got[..., 1:3][solid] == 0).all() and (got[..., 1:3][nan] == 0).all()
    masked = go._neighbourhood(solid | nan)
    assert len(set(got[..., 0][masked].tolist())) == 1


@pytest.mark.gpu
def test_zz_report():
    for (kernel, family), v in sorted(_STATS.items()):
        print(f"\ngrid stage oracle: {kernel} / {family}: worst {v:.3g}")
    assert all(v <= 1.0 for v in _STATS.values())
