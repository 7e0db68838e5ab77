"""Stage-isolated float64 oracle of the PCA path (GridSurrogate): every stage is recomputed ONCE, in float64, from what the
device stored for that stage's input, and every element is held to an a-priori float32 bound E written next to the code it
comes from.  Nothing is propagated, so no bf16 rounding flip has to be allowed for.

  encode    float32 grid            -> X_INPUT      psm_encode*_kernel + psm_reduce_kernel / psm_reduce_dense1_kernel
  dense l   X_INPUT or kept H(l-1)  -> H(l), RES    psm_dense_kernel, the first layer of psm_reduce_dense1_kernel
  decode    RES                     -> BLOCK_PRED   psm_decode*_kernel (general path; the bound path never stores the blocks)

u = 2^-24 (float32 unit roundoff), gamma_n = n u / (1 - n u).  A float32 sum of products whose summation tree has depth n
differs from the exact sum by at most gamma_n times the sum of the absolute products (Higham, Accuracy and Stability of
Numerical Algorithms, 2nd ed., 3.1; a fused multiply-add rounds once, so it is covered too).  The float32 rounding of
float64 model data (basis, mean, scaler) counts as one more level of the tree.

Not checked here, and why: the reassembly (strip means, offset chain, paste, shift) and the fused decode + paste of the
bound path stay with check_against_oracle (tests/test_gpu_parity.py, normwise); LayerNormalization (densePCA_attention) and
the Conv1D head are refused by check_solve -- their float32 moments and the Conv1D activations are not read back."""
from dataclasses import dataclass

import numpy as np

from . import psm_oracle as orc

U = 2.0 ** -24
PIX_PER_SLICE = 64          # psm_kernels.h PSM_PIX_PER_SLICE: pixels of one block row that one encode K slice covers


def gamma(n: int) -> float:
    nu = n * U
    assert nu < 0.5, n
    return nu / (1.0 - nu)


def bf16(x) -> np.ndarray:
    """float32 -> bfloat16 round to nearest even, as float32 (v_cvt_pk_bf16_f32, the (__bf16) casts, f2bf on the host)."""
    return orc.bf16_round(np.asarray(x, np.float32))


@dataclass
class StageResult:
    name: str
    ratio: float            # worst |dev - r| / E over the elements both sides give finite
    bad: int                # elements with |dev - r| > E
    nan_mismatch: int       # positions where exactly one of dev, r is NaN
    worst: tuple            # index of the worst element

    @property
    def ok(self) -> bool:
        return self.bad == 0 and self.nan_mismatch == 0


def compare(name, dev, r, E) -> StageResult:
    """Every element: |dev - r| <= E; NaN positions must match exactly."""
    dev = np.asarray(dev, np.float64)
    r = np.asarray(r, np.float64)
    E = np.broadcast_to(np.asarray(E, np.float64), r.shape)
    assert dev.shape == r.shape, (name, dev.shape, r.shape)
    nd, nr = np.isnan(dev), np.isnan(r)
    d = np.abs(dev - r)
    d[nd | nr] = 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(d == 0.0, 0.0, d / E)
    q[np.isnan(q)] = np.inf
    k = np.unravel_index(int(np.argmax(q)), q.shape) if q.size else ()
    return StageResult(name, float(q.max()) if q.size else 0.0, int(np.count_nonzero(d > E)), int(np.count_nonzero(nd != nr)),
                       tuple(int(i) for i in k))


# ---- scaler: X_INPUT = coeff * ia + ib, RES = v * sa + sb (psm_api_model.cpp: ia, ib, sa, sb are float32 of float64 values) ----
def scaler_in(sc: orc.Scaler, p: int):
    a, b = (np.broadcast_to(np.asarray(v, np.float64), (p,)) for v in (sc.in_a, sc.in_b))
    if sc.kind == "max_abs":
        return 1.0 / a, np.zeros(p)
    if sc.kind == "std":
        return 1.0 / b, -a / b
    return 1.0 / (b - a), -a / (b - a)


def scaler_out(sc: orc.Scaler, p: int):
    a, b = (np.broadcast_to(np.asarray(v, np.float64), (p,)) for v in (sc.out_a, sc.out_b))
    if sc.kind == "max_abs":
        return a, np.zeros(p)
    if sc.kind == "std":
        return b, a
    return b - a, a


# ---- encode + slab reduce + input scaler -----------------------------------------------------------------------------------
ENCODE_FORMS = ("f32", "pair", "x6", "x6_mt", "bf16")


def encode_depth(form: str, c_in: int, S: int = 128, kgroups: int = 1) -> int:
    """Depth of the float32 summation tree of one X_INPUT element, counted from the launched form (not K = S^2 c_in):
      slab    one wave per component tile runs the MFMA chain over the slab's K slices, 64 c_in products per slice:
              f32 / bf16 one slice per slab; pair (psm_encode_pair_kernel) two slices chained + one LDS sum of the halves;
              x6 six MFMA terms per product, each its own float32 accumulation; x6_mt (psm_encode_x6_mt_kernel) one slab per
              K group of ceil(n_slices / kgroups) consecutive slices
      reduce  psm_reduce_kernel (and psm_reduce_dense1_kernel, same order): per wave ceil(n_slabs / 16) slabs in order, then
              the 16 wave sums in order; then the scaler's multiply-add
    +1 for the product rounding of the float32 MFMA."""
    ks = PIX_PER_SLICE * c_in
    n_slices = S * S // PIX_PER_SLICE
    if form == "pair":
        slabs, chain = n_slices // 2, 2 * ks + 1
    elif form == "x6":
        slabs, chain = n_slices, 6 * ks
    elif form == "x6_mt":            # kgroups None: the launcher's limits (<= 8 slices per group, <= n_slices groups)
        slabs = n_slices if kgroups is None else kgroups
        chain = 6 * ks * (8 if kgroups is None else -(-n_slices // kgroups))
    elif form in ("f32", "bf16"):
        slabs, chain = n_slices, ks
    else:
        raise ValueError(form)
    return chain + 1 + -(-slabs // 16) + 16


def x6_dropped(absum: np.ndarray, sum_t: np.ndarray, sum_c: np.ndarray) -> np.ndarray:
    """What the x6 forms lose per output.  The three dropped split terms (mid x lo, lo x mid, lo x lo of a = hi + mid + lo,
    psm_split3): |mid| <= 2^-8 |a|, |lo| <= 2^-16 |a| (each plane is the bf16 rounding of the exact float32 remainder), so
    <= 2^-23 |a| |b| per product, as the comment above psm_split3 states.  Near the float32 subnormal range the lo plane is a
    bf16 subnormal and the split is inexact by at most 2^-134 per operand (half the bf16 subnormal spacing): a product then
    loses at most 2^-134 (|a| + |b|) + 2^-268 more, bounded here by 2^-133 (sum|t| + sum|c|) per output.  Both claims are
    checked by tests/test_pca_stage_oracle.py (test_x6_split_...).  absum = sum |t||c|, sum_t = sum |t| over the row, sum_c =
    sum |c| over the component."""
    return 2.0 ** -23 * absum + 2.0 ** -133 * (sum_t + sum_c)


def encode_reference(xb: np.ndarray, model: orc.Model, bf16_ops: bool = False):
    """xb [rows, S, S, c_in] float32 blocks -> (coefficients r [rows, p_in] float64, sum |t| |c| [rows, p_in]) with
    t = fl32(x - mu) taken in float32 as every encode kernel takes it; bf16 handles round t and c as psm_encode_bf16_kernel."""
    flat = np.asarray(xb, np.float32).reshape(xb.shape[0], -1)
    t = flat - np.asarray(model.mean_in, np.float32)
    c = np.asarray(model.comp_in, np.float32)
    if bf16_ops:
        t, c = bf16(t), bf16(c)
    t64, c64 = t.astype(np.float64), c.astype(np.float64)
    return orc.pca_encode(t64, c64, np.zeros(t.shape[1])), np.abs(t64) @ np.abs(c64).T


def _abs_sums(xb, model):
    t = np.asarray(xb, np.float32).reshape(xb.shape[0], -1) - np.asarray(model.mean_in, np.float32)
    return np.abs(t.astype(np.float64)).sum(axis=1)[:, None], np.abs(np.asarray(model.comp_in, np.float32).astype(np.float64)).sum(axis=1)[None, :]


def check_encode(xb, model, x_input, form, kgroups=1) -> StageResult:
    """X_INPUT against Scaler.fwd of the float64 coefficients:  E = gamma_(d+1) (|ia| sum |t||c| + |ib|) [+ |ia| x6 terms]."""
    coeff, absum = encode_reference(xb, model, form == "bf16")
    p = coeff.shape[1]
    ia, ib = scaler_in(model.scaler, p)
    r = model.scaler.fwd(coeff)
    d = encode_depth(form, model.c_in, model.S, kgroups)
    E = gamma(d + 1) * (np.abs(ia) * absum + np.abs(ib))
    if form in ("x6", "x6_mt"):
        E = E + np.abs(ia) * x6_dropped(absum, *_abs_sums(xb, model)) * (1 + 2 * U)
    return compare("encode", x_input, r, E)


# ---- Dense layers ----------------------------------------------------------------------------------------------------------
def dense_reference(h, W, b, bf16_ops: bool = False):
    """Stored input h [rows, K] -> (v = h W + b float64, E = gamma_(K+2) (|h|^T |W| + |b|)).  psm_dense_kernel: K products
    per output in MFMA chains of 16 k split over at most 8 waves and summed in LDS (depth <= K), + bias (+1), product
    rounding (+1).  bf16 handles: h and W rounded as the kernel rounds them (products exact in float32)."""
    h32, W32 = np.asarray(h, np.float32), np.asarray(W, np.float32)
    if bf16_ops:
        h32, W32 = bf16(h32), bf16(W32)
    h64, W64 = h32.astype(np.float64), W32.astype(np.float64)
    b64 = np.asarray(b, np.float32).astype(np.float64)
    K = h64.shape[1]
    return h64 @ W64 + b64, gamma(K + 2) * (np.abs(h64) @ np.abs(W64) + np.abs(b64))


def check_hidden(l, h_in, W, b, h_out, bf16_ops=False) -> StageResult:
    """Hidden layer: r = relu(v); ReLU passes E unchanged."""
    v, E = dense_reference(h_in, W, b, bf16_ops)
    return compare(f"dense{l}", h_out, np.maximum(v, 0.0), E)


def check_head(h_in, W, b, res, scaler, bf16_ops=False) -> StageResult:
    """Head layer + output scaler (in the head's epilogue): r = Scaler.inv(v), E = gamma_(K+6) (|sa| (|h|^T|W| + |b|) + |sb|):
    the float32 sa / sb and the multiply-add are four more levels of the same tree."""
    v, E = dense_reference(h_in, W, b, bf16_ops)
    K = np.asarray(h_in).shape[1]
    sa, sb = scaler_out(scaler, v.shape[1])
    Ev = E / gamma(K + 2)
    return compare("head", res, scaler.inv(v), gamma(K + 6) * (np.abs(sa) * Ev + np.abs(sb)))


# ---- decode (general path) ------------------------------------------------------------------------------------------------
def check_decode(res, model, block_pred, row_scale, bf16_ops=False) -> StageResult:
    """Stored RES -> BLOCK_PRED = (res' C + mean) * scale, res' = RES (bf16-rounded on bf16 handles, as psm_decode_bf16_kernel):
    E = gamma_(P+3) (|res'| |C| + |mean|) |scale| -- P products per output in one MFMA chain, + mean, * scale, and the float32
    basis / mean."""
    r_in = np.asarray(res, np.float32)
    C = np.asarray(model.comp_out, np.float64)
    if bf16_ops:
        r_in, C = bf16(r_in), bf16(C).astype(np.float64)
    r64 = r_in.astype(np.float64)
    mean = np.asarray(model.mean_out, np.float64)
    S, c_out, P = model.S, model.c_out, r64.shape[1]
    sc = np.asarray(row_scale, np.float64).reshape(-1, 1, 1, 1)
    r = orc.pca_decode(r64, C, mean, S, c_out) * sc
    E = gamma(P + 3) * (np.abs(r64) @ np.abs(C) + np.abs(mean)).reshape(r.shape) * np.abs(sc)
    return compare("decode", block_pred, r, E)


# ---- one solve ---------------------------------------------------------------------------------------------------------------
def blocks_of(grids, model) -> np.ndarray:
    """[n, Ny, Nx, >= c_in] float32 grids -> the solve's block rows [n B, S, S, c_in] float32, case-major."""
    g = np.asarray(grids, np.float32)
    lay = orc.block_layout(model.variant, g.shape[1], g.shape[2], model.S, model.overlap())
    return np.concatenate([orc.extract_blocks(gc, lay, model.c_in) for gc in g], axis=0)


def check_solve(model, grids, stages, form, kgroups=1, bf16_ops=False, row_scale=None):
    """stages: what the device stored -- 'x_input' [rows, p_in], 'hidden' [[rows, n_out(l)]] (keep mode), 'res' [rows, p_out],
    'block_pred' [rows, S, S, c_out] or None (bound path).  -> [StageResult], one per stage, each from the device's own input."""
    if len(model.conv1d) or model.attention:
        raise NotImplementedError("LayerNormalization and the Conv1D head are not read back")
    xb = blocks_of(grids, model)
    out = [check_encode(xb, model, stages["x_input"], form, kgroups)]
    hid = stages["hidden"]
    W = model.weights
    assert len(hid) == len(W) - 1
    h_in = stages["x_input"]
    for l in range(len(W) - 1):
        out.append(check_hidden(l, h_in, *W[l], hid[l], bf16_ops))
        h_in = hid[l]
    out.append(check_head(h_in, *W[-1], stages["res"], model.scaler, bf16_ops))
    if stages.get("block_pred") is not None:
        rs = np.ones(xb.shape[0]) if row_scale is None else row_scale
        out.append(check_decode(stages["res"], model, stages["block_pred"], rs, bf16_ops))
    return out


def exact_stages(model, grids, form, bf16_ops=False, row_scale=None):
    """The oracle's own outputs, each stage computed in float64 from the previous one and rounded ONCE to float32: what a
    perfect device stores.  -> dict as check_solve takes it."""
    xb = blocks_of(grids, model)
    coeff, _ = encode_reference(xb, model, bf16_ops)
    x = np.asarray(model.scaler.fwd(coeff), np.float32)
    hid, h = [], x
    for W, b in model.weights[:-1]:
        v, _ = dense_reference(h, W, b, bf16_ops)
        h = np.maximum(v, 0.0).astype(np.float32)
        hid.append(h)
    v, _ = dense_reference(h, *model.weights[-1], bf16_ops)
    res = np.asarray(model.scaler.inv(v), np.float32)
    r_in = bf16(res) if bf16_ops else res
    C = bf16(model.comp_out).astype(np.float64) if bf16_ops else np.asarray(model.comp_out, np.float64)
    rs = np.ones(xb.shape[0]) if row_scale is None else np.asarray(row_scale, np.float64)
    bp = (orc.pca_decode(r_in.astype(np.float64), C, model.mean_out, model.S, model.c_out) * rs.reshape(-1, 1, 1, 1)).astype(np.float32)
    return dict(x_input=x, hidden=hid, res=res, block_pred=bp)
