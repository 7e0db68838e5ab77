"""Elementwise float64 oracles of the kernels that run around a solve on the grid -- the Gaussian post-steps (csrc/psm_filter.hip),
the gradP -> p integration (csrc/psm_integ.hip) and the Poisson input features (csrc/psm_features.hip) -- each with an a-priori
bound E on what a correct implementation in the kernel's precision may differ by, and a NumPy restatement ("mirror") of the
kernel's own summation order in the kernel's precision.  Pure NumPy / SciPy: nothing here touches a GPU.

Notation: u = 2^-24 (float32 unit roundoff), gamma(n) = n u / (1 - n u): n float32 roundings on the longest path of a sum bound
its error by gamma(n) times the sum of the magnitudes (Higham, Accuracy and Stability of Numerical Algorithms, 4.2: any order).

The mirrors exist for the CPU tests only: `mirror inside the bound` checks the derivations below against an independent float32
run of the same order, and the planted faults (argument `fault`) check that the bound is tight enough to see them."""
import warnings

import numpy as np
from scipy.ndimage import correlate1d

from oracle import psm_oracle as orc

U32 = 2.0 ** -24
U64 = 2.0 ** -53
F32 = np.float32


def gamma(n, u=U32):
    return n * u / (1.0 - n * u)


class Unsupported(ValueError):
    """A geometry the reference itself cannot process (PSM_ERR_UNSUPPORTED of psm_set_integration)."""


def worst_ratio(dev, ref, E):
    """max |dev - ref| / E over the finite reference values; the NaN patterns must agree (-> inf otherwise); where E == 0 the value
    must be the reference's exactly."""
    dev, ref, E = np.asarray(dev, np.float64), np.asarray(ref, np.float64), np.asarray(E, np.float64)
    if dev.shape != ref.shape or not np.array_equal(np.isnan(dev), np.isnan(ref)):
        return float("inf")
    ok = ~np.isnan(ref)
    if not ok.any():
        return 0.0
    d, e = np.abs(dev[ok] - ref[ok]), E[ok]
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d == 0, 0.0, np.where(e > 0, d / e, np.inf))
    return float(np.max(r))


# =====================================================================================================================
# Gaussian post-steps
# =====================================================================================================================
def gauss_radius(sigma):
    return int(4.0 * float(sigma) + 0.5)


def gauss_weights(sigma):
    """scipy.ndimage._gaussian_kernel1d, order 0, truncate 4: float64 taps (the library rounds each to float32)."""
    r = gauss_radius(sigma)
    x = np.arange(-r, r + 1, dtype=np.float64)
    p = np.exp(-0.5 / (float(sigma) * float(sigma)) * x * x)
    return p / p.sum()


def _corr(a, w, axis):
    with np.errstate(invalid="ignore"):
        return correlate1d(np.asarray(a, np.float64), w, axis=axis, mode="reflect")


def gauss_stage(x, Ex, sigma):
    """-> (y, Ey): y = G_x(G_y(x)) in float64 (axis 0 first, as the kernel and SciPy do), Ey the bound on a float32 implementation
    that sums the n_a taps of axis a in ANY order with FMAs from an input already uncertain by Ex:
        t = G_y(x)      E1 = G_y(Ex) + gamma(n_y + 2) G_y(|x|) + u |t|
        y = G_x(t)      Ey = G_x(E1) + gamma(n_x + 2) G_x(|t|) + u |y|
    n_a FMAs are n_a roundings on the path of a product; + 2 covers the float32 rounding of the tap and leaves one to spare; the
    last term is the rounding of the stored value."""
    x = np.asarray(x, np.float64)
    Ex = np.broadcast_to(np.asarray(Ex, np.float64), x.shape)
    wy, wx = gauss_weights(sigma[0]), gauss_weights(sigma[1])
    t = _corr(x, wy, 0)
    E1 = _corr(Ex, wy, 0) + gamma(len(wy) + 2) * _corr(np.abs(x), wy, 0) + U32 * np.abs(t)
    y = _corr(t, wx, 1)
    Ey = _corr(E1, wx, 1) + gamma(len(wx) + 2) * _corr(np.abs(t), wx, 1) + U32 * np.abs(y)
    return y, Ey


def poststep_chain(field, dU, prev, apply_filter, sigma_field=(10.0, 10.0), sigma_weight=(50.0, 50.0)):
    """SM_call.py:352-363 / :843-848 with the bound carried along: result = G(field) (or the field itself), w = G(dU),
    t = (result - prev) w, change = G(t), next = prev + change.  -> {"result" | "change" | "next": (value, E)}.
    The product: d = result - prev is one rounding of operands uncertain by Er; t = d w one more, w uncertain by Ew."""
    field, dU, prev = (np.asarray(a, np.float64) for a in (field, dU, prev))
    if apply_filter:
        res, Er = gauss_stage(field, 0.0, sigma_field)
    else:
        res, Er = field, np.zeros_like(field)
    w, Ew = gauss_stage(dU, 0.0, sigma_weight)
    d = res - prev
    Ed = Er + U32 * (np.abs(d) + Er)
    t = d * w
    Et = (Ed * (np.abs(w) + Ew) + np.abs(d) * Ew) * (1 + U32) + U32 * np.abs(t)
    chg, Ec = gauss_stage(t, Et, sigma_field)
    nxt = prev + chg
    En = Ec + U32 * (np.abs(nxt) + Ec)
    return {"result": (res, Er), "change": (chg, Ec), "next": (nxt, En)}


def _reflect(i, n, whole_sample=False):
    i = np.asarray(i, np.int64)
    if whole_sample:                                   # fault: d c b | a b c d | c b a, period 2n - 2
        if n == 1:
            return np.zeros_like(i)
        j = np.mod(i, 2 * n - 2)
        return np.where(j < n, j, 2 * n - 2 - j)
    j = np.mod(i, 2 * n)
    return np.where(j < n, j, 2 * n - 1 - j)


def _fma32(a, b, c):
    """float32 fmaf: the product of two float32 is exact in float64; one float64 rounding of the sum below the float32 one."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def _mirror_pass(x, sigma, axis, tap_chunk, fault):
    w = gauss_weights(sigma).astype(F32)
    r = (len(w) - 1) // 2
    x = np.moveaxis(np.asarray(x, F32), axis, 0)
    n = x.shape[0]
    pos = np.arange(n)
    acc = np.zeros_like(x)
    for t in range(len(w)):                            # ascending taps; the chunks only re-stage, the accumulators are carried
        if fault == "chunk_first_tap_dropped" and t == tap_chunk:
            continue
        src = x[_reflect(pos + t - r, n, fault == "whole_sample_reflection")]
        acc = _fma32(np.broadcast_to(w[t], src.shape), src, acc)
    if fault == "nan_from_slack":                      # the value one past the window multiplied (by zero) into the output
        with np.errstate(invalid="ignore"):
            acc = acc + F32(0) * x[_reflect(pos + r + 1, n)]
    return np.moveaxis(acc, 0, axis)


def filter_mirror(x, sigma, tap_chunk=604, fault=None):
    """psm_gauss1d_kernel<0, 0> then <1, 0> in float32: every output the FMA chain over its taps in ascending order."""
    x = np.array(x, F32)
    if fault == "column_64_from_63" and x.shape[1] > 64:          # the first column of the second 64-wide strip staged from its neighbour
        x[:, 64] = x[:, 63]
    t = _mirror_pass(x, sigma[0], 0, tap_chunk, fault)
    if fault == "fourth_output_row_shifted" and t.shape[0] > 4:    # output j = 3 of a thread written from the row below
        t[3] = t[4]
    return _mirror_pass(t, sigma[1], 1, tap_chunk, fault)


# =====================================================================================================================
# gradP -> p integration
# =====================================================================================================================
MAX_FIX = 4          # PSM_INTEG_MAX_FIX


def integ_tables(sdf, cy, cx):
    """The host tables of one geometry (integ_tables of psm_api_integ.cpp): fix[a] = [(v, u)] by quadrant-local row a (element v
    of a block row becomes -(ccc[v] - ccc[u]), u = -1: ccc[u] = 0), mask [ny] (bit 0: flow cell at column cx, bit 1: at cx-1),
    npair (top, bottom).  Raises Unsupported where the reference raises."""
    sdf = np.asarray(sdf, np.float64)
    ny, nx = sdf.shape
    if not (1 <= cy < ny and 1 <= cx < nx):
        raise ValueError("cut outside the grid")
    wmin = min(cx, nx - cx + 1)
    fix = []
    for a in range(max(cy, ny - cy)):
        nn = sdf[a].astype(int)
        nn = np.where(nn < 0, nn + wmin, nn)
        last = {}
        for k, v in enumerate(nn):
            last[int(v)] = k
        if len(last) > MAX_FIX:
            raise Unsupported("more distinct int(sdf) values on a row than supported")
        if min(last) < 0 or max(last) >= wmin:
            raise Unsupported("int(sdfunct) indexes outside a quadrant row")
        fix.append([(v, int(nn[k - 1]) if k > 0 else -1) for v, k in sorted(last.items())])
    mask = (sdf[:, cx] != 0).astype(np.uint8) | ((sdf[:, cx - 1] != 0).astype(np.uint8) << 1)
    npair = []
    for rows in (slice(0, cy), slice(cy, ny)):
        nl, nr = int((mask[rows] & 1).sum()), int((mask[rows] >> 1).sum())
        if nl != nr:
            raise Unsupported("flow-cell counts of the two cut columns differ")
        npair.append(nl)
    return fix, mask, tuple(npair)


def _magnitude_field(block, sdfunct, dx, dy, direction_x=1, direction_y=1):
    """orc.integrate_field on magnitudes with every subtraction turned into an addition: an upper bound on the sum of the
    magnitudes of everything any evaluation order of Phat[a, b] adds up (path sums, replacement values, reference corner)."""
    gx, gy = np.abs(np.asarray(block[..., 0], np.float64)), np.abs(np.asarray(block[..., 1], np.float64))
    h, w = gx.shape
    S = np.empty((h, w))
    for i in range(h):
        aaa = gx[i].copy()
        ccc = np.cumsum(aaa)
        nn = sdfunct[i, :].astype(int)
        aaa[nn] = ccc[nn] + np.concatenate(([0.0], ccc[nn]))[:-1]
        S[i] = np.cumsum(aaa) * abs(dx)
    Sy = np.cumsum(gy, axis=0) * abs(dy)
    ij = -1 if direction_x == -1 else 0
    ii = -1 if direction_y == -1 else 0
    return Sy[:, ij][:, None] + Sy[ii, ij] + S + S[:, ij][:, None]


def integ_depth(ny, nx, cx):
    """Float32 roundings on the longest path from a gradient value to a stored p, read from psm_integ.hip:
      rows kernel, a side of ceil(w / 64) chunks: an element passes the 6 levels of psm_wave_scan and the `+ carry` of its own
        chunk and, inside the carry, the same 7 of every later chunk: 7 nch.  A fix-up value -(cv - cu) is a difference (1) of two
        such sums of the pre-pass (7 nch) and then enters the second scan (7 nch).  `(incl - first) * dx`: 2, and dx itself is
        rounded to float32: 1.                                                        d_row = 14 nch + 4
      cols kernel, ceil(ny / 256) chunks: wave scan 6, then `tot` (the next carry) adds the four wave sums one by one: at most 4
        more per chunk; in its own chunk an element meets `off` (at most 3 adds) and `s + off`: inside the 10.  `- row0` / `- own`,
        `* dy`, dy rounded: 3.                                                        d_col = 10 nchc + 3
      stitching: d = (yl + v.z) - (yr + v.w): 2; per-thread accumulation over the chunks: nchc; 6 shuffle levels; the fold of the
        four waves: 3; the division: 1; `addl - corr`: 1; `prow[x] +=`: 1.            d_fix = nchc + 14
    A value reaches p either through the row scan or through the column scan, then (left quadrants) through the stitching mean:
      d = max(d_row, d_col) + d_fix."""
    nch = (max(cx, nx - cx + 1) + 63) // 64
    nchc = (ny + 255) // 256
    return max(14 * nch + 4, 10 * nchc + 3) + nchc + 14


def integ_bound(gradp, sdf, dx, dy, cy, cx):
    """-> (p, E): p = orc.integrate_gradp in float64, E = gamma(d) S with S the four-quadrant recipe on magnitudes and d =
    integ_depth.  NaN (empty selection on a cut column) in p is NaN in E: the comparison is then on the pattern."""
    gradp, sdf = np.asarray(gradp, np.float64), np.asarray(sdf, np.float64)
    ny, nx = sdf.shape
    with np.errstate(invalid="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)           # "Mean of empty slice": the NaN is the expected value
        p = orc.integrate_gradp(gradp, sdf, dx, dy, cy, cx)
        S = np.empty((ny, nx))
        for rows, dy_dir in ((slice(0, cy), 1), (slice(cy, ny), -1)):
            sr = _magnitude_field(gradp[rows, cx - 1:], sdf, dx, dy, -1, dy_dir)
            sl = _magnitude_field(gradp[rows, :cx], sdf, dx, dy, 1, dy_dir)
            ml, mr = sdf[rows, cx] != 0, sdf[rows, cx - 1] != 0
            S[rows, cx - 1:] = sr
            S[rows, :cx] = sl + (sl[:, -1][ml].mean() + sr[:, 0][mr].mean())
    return p, gamma(integ_depth(ny, nx, cx)) * S


def _wave_scan(v):
    """psm_wave_scan over the last axis (64 lanes), float32: Hillis-Steele, 6 levels."""
    v = np.array(v, F32)
    o = 1
    while o < 64:
        t = v.copy()
        with np.errstate(invalid="ignore"):
            v[..., o:] = t[..., o:] + t[..., :-o]
        o <<= 1
    return v


def _chunks(v, n):
    """[len] -> [ceil(len / n), n], zero padded."""
    k = max(1, (len(v) + n - 1) // n)
    out = np.zeros(k * n, F32)
    out[:len(v)] = v
    return out.reshape(k, n)


def _mirror_row(gx, fix, side, dx, fault):
    """One wave of psm_integ_rows_kernel: block row gx [w] -> the scaled scan by block column [w]."""
    w = len(gx)
    fv = [v if 0 <= v < w else -1 for v, _ in fix]
    if fault == "fixup_beyond_lane_63_ignored":
        fv = [v if v < 64 else -1 for v in fv]
    fu = [u if v >= 0 else -1 for v, (_, u) in zip(fv, fix)]
    cv, cu = [F32(0)] * len(fix), [F32(0)] * len(fix)
    last = min(max(fv + fu + [-1]), w - 1)
    carry = F32(0)
    for c, chunk in enumerate(_chunks(gx, 64)):
        base = 64 * c
        if base > last:
            break
        s = _wave_scan(chunk) + carry
        for e in range(len(fix)):
            if base <= fv[e] < base + 64:
                cv[e] = s[fv[e] - base]
            if base <= fu[e] < base + 64:
                cu[e] = s[fu[e] - base]
        carry = s[63]
    x = np.array(gx, F32)
    for e in range(len(fix)):
        if fv[e] >= 0:
            x[fv[e]] = -(cv[e] - cu[e])
    if side:
        x = x[::-1]
    out = np.empty(w, F32)
    carry, first = F32(0), F32(0)
    for c, chunk in enumerate(_chunks(x, 64)):
        incl = _wave_scan(chunk) + carry
        if side == 0:
            if c == 0:
                first = incl[0]
            o = (incl - first) * dx
        else:
            excl = np.concatenate(([carry], incl[:-1])).astype(F32)
            o = -(incl if fault == "right_side_inclusive" else excl) * dx
        carry = F32(0) if fault == "chunk_carry_dropped" else incl[63]
        m = min(64, w - 64 * c)
        out[64 * c:64 * c + m] = o[:m]
    return out[::-1] if side else out


def integ_mirror(gradp, sdf, dx, dy, cy, cx, fault=None):
    """psm_integ_rows_kernel + psm_integ_cols_kernel in float32 in the kernels' own order: 64-wide scans with a carry, the right
    side backwards, the bottom half from row ny-1, fix-ups by (v, u), the four-wave fold and the stitching mean."""
    g = np.asarray(gradp, F32)
    ny, nx = g.shape[:2]
    fix, mask, npair = integ_tables(sdf, cy, cx)
    if fault == "npair_swapped":
        npair = npair[::-1]
    dx, dy = F32(dx), F32(dy)
    p = np.zeros((ny, nx), F32)
    aux = np.zeros((ny, 4), F32)
    for y in range(ny):
        if fault == "last_single_row_skipped" and y == ny - 1 and ny % 2:
            continue
        f = fix[y if y < cy else y - cy]
        left = _mirror_row(g[y, :cx, 0], f, 0, dx, fault)
        right = _mirror_row(g[y, cx - 1:, 0], f, 1, dx, fault)
        p[y, :cx] = left
        p[y, cx:] = right[1:]
        if fault == "right_side_writes_cut_column":
            p[y, cx - 1] = right[0]
        aux[y] = (g[y, 0, 1], g[y, nx - 1, 1], left[-1], right[0])
    # cols kernel: scan position i -> row y
    i = np.arange(ny)
    top = i < cy
    yy = np.where(top, i, i if fault == "bottom_half_from_cut_row" else ny - 1 - (i - cy))
    n256 = (ny + 255) // 256 * 256
    own = np.zeros((4, n256), F32)
    own[0, :ny] = np.where(top, aux[yy, 0], 0)
    own[1, :ny] = np.where(top, 0, aux[yy, 0])
    own[2, :ny] = np.where(top, aux[yy, 1], 0)
    own[3, :ny] = np.where(top, 0, aux[yy, 1])
    yl, yr = np.zeros(ny, F32), np.zeros(ny, F32)
    acc = np.zeros((2, 256), F32)
    carry = np.zeros(4, F32)
    with np.errstate(invalid="ignore", divide="ignore"):
        for base in range(0, ny, 256):
            s = _wave_scan(own[:, base:base + 256].reshape(4, 4, 64))          # [quantity][wave][lane]
            wsum = s[:, :, 63]
            off = np.empty((4, 4), F32)
            tot = carry.copy()
            for q in range(4):
                off[:, q] = tot                                                # carry + the waves before
                tot = tot + wsum[:, q]
            carry = tot
            so = (s + off[:, :, None]).reshape(4, 256)
            o = own[:, base:base + 256]
            m = min(256, ny - base)
            idx = i[base:base + m]
            tp = top[base:base + m]
            l = np.where(tp, (so[0, :m] - aux[0, 0]) * dy, -(so[1, :m] - o[1, :m]) * dy).astype(F32)
            r = np.where(tp, (so[2, :m] - aux[0, 1]) * dy, -(so[3, :m] - o[3, :m]) * dy).astype(F32)
            y = yy[idx]
            d = (np.where(mask[y] & 1, l + aux[y, 2], F32(0)) - np.where(mask[y] & 2, r + aux[y, 3], F32(0))).astype(F32)
            acc[0, :m] += np.where(tp, d, F32(0))
            acc[1, :m] += np.where(tp, F32(0), d)
            yl[y], yr[y] = l, r
        t = acc.reshape(2, 4, 64)
        for o in (32, 16, 8, 4, 2, 1):                                         # lane 0 of the __shfl_down tree
            t = t[..., :o] + t[..., o:2 * o]
        red = t[..., 0]
        corr = [((red[q, 0] + red[q, 1]) + red[q, 2] + red[q, 3]) / F32(npair[q]) for q in range(2)]
        for y in range(ny):
            al = yl[y] - (corr[0] if y < cy else corr[1])
            p[y, :cx] += al
            p[y, cx:] += yr[y]
    return p


# =====================================================================================================================
# Poisson input features
# =====================================================================================================================
def _neighbourhood(bad):
    b = bad.copy()
    b[1:, :] |= bad[:-1, :]
    b[:-1, :] |= bad[1:, :]
    b[:, 1:] |= bad[:, :-1]
    b[:, :-1] |= bad[:, 1:]
    return b


def features_bound(ux, uy, dux, duy, sdfunct, L, U, k, max_abs, cast=True):
    """-> (grid [ny,nx,4] float64, E [ny,nx,4]).
    Channels 1-3 are the reference's own float64 statements (x / U, NaN -> 0, / max_abs) followed by one cast: E = 0 there, the
    kernel's values are float32(grid) bit for bit.
    Channel 0 = asinh(scale(term; lo, hi)) / max_abs[0] differs through
      * the term: the same products and sums, but `* (L L / (U U))` for `* L**2 / U**2` and free FMA contraction: a few float64
        roundings, 16 u64 of the magnitudes;
      * mean and standard deviation: the kernel folds per-workgroup (sum, sum of squares) and takes var = s2 / n - mean^2, the
        reference np.mean / np.std.  Any order of n additions errs by at most n u64 of the magnitudes, so
            |d var| <= n u64 (mean^2 + var) 2,  |d std| = |d var| / (2 std) <= delta std,  delta = n u64 (mean^2 + var) / var
            |d mean| <= n u64 mean|t| <= n u64 sqrt(mean^2 + var) <= delta std
        (a relative bound on the mean alone would be void at mean -> 0, hence delta (|mean| + std) below);
      * lo = mean - k std, hi = mean + k std: |d lo|, |d hi| <= |d mean| + |k| |d std|, pushed through the three branches (each
        continuous with its neighbour at lo / hi, so a cell within the uncertainty of a threshold is covered by the larger of the
        two slopes), through asinh' = 1 / sqrt(1 + s^2), and then one float32 rounding (left out with cast=False: the bound on the
        float64 value before the store, which is what a float64 restatement of the kernel's order has to meet)."""
    grid, term = orc.poisson_features(ux, uy, dux, duy, sdfunct, L, U, k, max_abs)
    E = np.zeros_like(grid)
    n = term.size
    mean, var = float(np.mean(term)), float(np.var(term))
    sd = np.sqrt(var)
    with np.errstate(all="ignore"):
        delta = n * U64 * (mean * mean + var) / var
        dm, dsd = delta * (abs(mean) + sd), delta * sd
        dlo = dhi = dm + abs(k) * dsd
        lo, hi = mean - k * sd, mean + k * sd
        dt = 16 * U64 * np.abs(term)
        t = term
        slope = {"below": np.abs(t) / lo ** 2 * dlo + dt / abs(lo), "above": np.abs(t) / hi ** 2 * dhi + dt / abs(hi),
                 "mid": 2 * (np.abs(t - hi) * dlo + np.abs(t - lo) * dhi) / (hi - lo) ** 2 + 2 * dt / abs(hi - lo)}
        near_lo, near_hi = np.abs(t - lo) <= 2 * (dlo + dt), np.abs(t - hi) <= 2 * (dhi + dt)
        ds = np.where(t < lo, slope["below"], np.where(t > hi, slope["above"], slope["mid"]))
        ds = np.where(near_lo, np.maximum(slope["below"], slope["mid"]), ds)
        ds = np.where(near_hi, np.maximum(slope["above"], slope["mid"]), ds)
        scaled = np.where(t < lo, -1.0 - (t - lo) / lo, np.where(t > hi, 1.0 + (t - hi) / hi, 2.0 * (t - lo) / (hi - lo) - 1.0))
        f0 = np.arcsinh(scaled)
        df0 = ds / np.sqrt(1.0 + scaled * scaled) + 8 * U64 * np.abs(f0)
        E[..., 0] = df0 / abs(max_abs[0])
        if cast:                                       # |fl(v') - v| <= |v' - v| + u |v'|, plus half the smallest subnormal
            E[..., 0] = E[..., 0] * (1 + U32) + U32 * np.abs(grid[..., 0]) + 2.0 ** -149
    return grid, E


def _tree256(v):
    """block_sum of psm_features.hip over the last axis (256 values): red[tid] += red[tid + s], s = 128 .. 1."""
    v = np.array(v, np.float64)
    s = 128
    while s > 0:
        v = v[..., :s] + v[..., s:2 * s]
        s >>= 1
    return v[..., 0]


def features_mirror(ux, uy, dux, duy, sdfunct, L, U, k, max_abs, fault=None, cast=True):
    """psm_poisson_term_kernel + psm_poisson_grid_kernel in float64 in the kernels' own order: 256-pixel partials (tree), folded by a
    stride-256 loop, then the tree again; var = s2 / n - mean^2.  -> grid [ny,nx,4] float32 (float64 before the store with cast=False)."""
    ux, uy = np.array(ux, np.float64), np.array(uy, np.float64)
    sdf = np.asarray(sdfunct, np.float64)
    ny, nx = sdf.shape
    solid = sdf == 0

    def grad(v):
        v = v.copy()
        v[solid] = np.nan
        bad = _neighbourhood(np.isnan(v))
        gy, gx = np.zeros_like(v), np.zeros_like(v)
        with np.errstate(invalid="ignore"):
            gy[1:-1] = (v[2:] - v[:-2]) / 2.0
            gx[:, 1:-1] = (v[:, 2:] - v[:, :-2]) / 2.0
            h = 2.0 if fault == "border_difference_halved" else 1.0
            gy[0], gy[-1] = (v[1] - v[0]) / h, (v[-1] - v[-2]) / h
            gx[:, 0], gx[:, -1] = (v[:, 1] - v[:, 0]) / h, (v[:, -1] - v[:, -2]) / h
        gy[bad] = 0.0
        gx[bad] = 0.0
        return gy, gx

    dUx_dy, dUx_dx = grad(ux)
    dUy_dy, dUy_dx = grad(uy)
    term = (dUx_dx * dUx_dx + 2 * dUx_dy * dUy_dx + dUy_dy * dUy_dy) * (L * L / (U * U))
    n = ny * nx
    nwg = (n + 255) // 256
    flat = np.zeros(nwg * 256)
    flat[:n] = term.ravel()
    part = np.stack([_tree256(flat.reshape(nwg, 256)), _tree256((flat * flat).reshape(nwg, 256))])     # [2][nwg]
    fold = np.zeros((2, 256))
    for w0 in range(0, nwg, 256):
        if fault == "partials_beyond_256_not_folded" and w0 > 0:
            break
        m = min(256, nwg - w0)
        fold[:, :m] += part[:, w0:w0 + m]
    s1, s2 = _tree256(fold)
    mean = s1 / n
    var = max(s2 / n - mean * mean, 0.0)
    sd = np.sqrt(var)
    lo, hi = mean - k * sd, mean + k * sd
    with np.errstate(all="ignore"):
        sc = np.where(term < lo, -1.0 - (term - lo) / lo, np.where(term > hi, 1.0 + (term - hi) / hi, 2.0 * (term - lo) / (hi - lo) - 1.0))
        f = np.stack([np.arcsinh(sc), np.asarray(dux, np.float64) / U, np.asarray(duy, np.float64) / U, sdf], -1)
    f[np.isnan(f)] = 0.0
    f = f / np.asarray(max_abs, np.float64)
    return f.astype(F32) if cast else f
