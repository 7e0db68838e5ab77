"""CPU oracle of the convolutional surrogate path (SURVEY.md §8 row a-conv) -- TEST INFRASTRUCTURE ONLY.

**Parity unpinned.**  The project's north star names a Conv2D / U-Net forward pass, but nothing in the
reference repository defines one: its CNN folders are empty placeholders
(Thesis_Work/Chapter4/README.md:3) and the model called "U-Net" at python_module.py:131 contains only Dense
layers.  There are no weights, no layer list and no outputs to compare with.  This file therefore states a
build-defined network ("UNet-S", the spec SURVEY.md §8 gives) in plain NumPy; tests/test_unet.py cross-checks
it against ``torch.nn.functional.conv2d`` / ``max_pool2d`` / ``interpolate`` on the CPU and then uses it as
the checker of the HIP kernels.  Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may
import it.

UNet-S (NHWC, float32; Keras conventions: kernels HWIO ``[kh, kw, c_in, c_out]``, 'same' zero padding):

  enc_l  (l = 0..L-1): [2x2 max-pool of enc_{l-1} if l > 0] -> conv3x3(w_l)+ReLU -> conv3x3(w_l)+ReLU
  dec_l  (l = L-2..0): concat(nearest-neighbour 2x upsample of the level below, enc_l) on the channel axis
                       (upsampled channels first) -> conv3x3(w_l)+ReLU -> conv3x3(w_l)+ReLU
  head               : conv1x1(w_0 -> c_out), linear

with widths w = (16, 32, 64, 128, 256): 18 3x3 convolutions + the head, 7.0 GFLOP for a 256x256x3 image.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Tuple

import numpy as np

WIDTHS_S = (16, 32, 64, 128, 256)


@dataclass
class ConvSpec:
    name: str
    k: int          # kernel edge (3 or 1)
    c_in: int
    c_out: int
    level: int      # resolution level of the convolution's output (0 = full resolution)
    src: str        # 'input' | 'prev' | 'pool' (2x2 max-pool of prev) | 'up+skip' (upsample(prev) ++ enc_level)
    relu: bool


def unet_specs(c_in: int = 3, widths=WIDTHS_S, c_out: int = 1) -> List[ConvSpec]:
    L = len(widths)
    s: List[ConvSpec] = []
    for l in range(L):
        cin = c_in if l == 0 else widths[l - 1]
        s.append(ConvSpec(f"enc{l}a", 3, cin, widths[l], l, "input" if l == 0 else "pool", True))
        s.append(ConvSpec(f"enc{l}b", 3, widths[l], widths[l], l, "prev", True))
    for l in range(L - 2, -1, -1):
        s.append(ConvSpec(f"dec{l}a", 3, widths[l + 1] + widths[l], widths[l], l, "up+skip", True))
        s.append(ConvSpec(f"dec{l}b", 3, widths[l], widths[l], l, "prev", True))
    s.append(ConvSpec("head", 1, widths[0], c_out, 0, "prev", False))
    return s


def he_weights(specs: List[ConvSpec], seed: int = 7) -> List[Tuple[np.ndarray, np.ndarray]]:
    """Seeded He-normal kernels (HWIO) and small biases, float32."""
    rng = np.random.default_rng(seed)
    out = []
    for sp in specs:
        fan_in = sp.k * sp.k * sp.c_in
        W = (rng.standard_normal((sp.k, sp.k, sp.c_in, sp.c_out)) * np.sqrt(2.0 / fan_in)).astype(np.float32)
        b = (rng.standard_normal(sp.c_out) * 0.05).astype(np.float32)
        out.append((W, b))
    return out


def conv2d_same(x: np.ndarray, W: np.ndarray, b: np.ndarray, relu: bool) -> np.ndarray:
    """x [H,W,Cin] -> [H,W,Cout]; zero 'same' padding; accumulation in float64, result float32."""
    k = W.shape[0]
    r = k // 2
    H, Wd, _ = x.shape
    xp = np.zeros((H + 2 * r, Wd + 2 * r, x.shape[2]), np.float64)
    xp[r:r + H, r:r + Wd] = x
    acc = np.zeros((H, Wd, W.shape[3]), np.float64)
    for ky in range(k):
        for kx in range(k):
            acc += xp[ky:ky + H, kx:kx + Wd] @ W[ky, kx].astype(np.float64)
    acc += b.astype(np.float64)
    if relu:
        acc = np.maximum(acc, 0.0)
    return acc.astype(np.float32)


def max_pool2(x: np.ndarray) -> np.ndarray:
    H, W, C = x.shape
    return x[:H - H % 2, :W - W % 2].reshape(H // 2, 2, W // 2, 2, C).max(axis=(1, 3))


def upsample2(x: np.ndarray) -> np.ndarray:
    return np.repeat(np.repeat(x, 2, axis=0), 2, axis=1)


def bf16_round(x) -> np.ndarray:
    """float32 -> nearest bfloat16 (ties to even), returned as float32 (what v_cvt_pk_bf16_f32 does)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def unet_forward(grid: np.ndarray, weights, widths=WIDTHS_S, return_all: bool = False, precision: str = "f32"):
    """grid [H,W,c_in] float32 (H, W multiples of 2**(L-1)) -> [H,W,c_out] float32; activations are rounded to
    float32 after every layer like the device path stores them.  precision 'bf16': the input of every 3x3
    convolution (after pooling / upsampling / concatenation) and its kernel are rounded to bf16 first, products
    exact, accumulation wide -- the device's bf16 operand path; biases, the 1x1 head and the stored activations
    stay float32."""
    L = len(widths)
    rnd = bf16_round if precision == "bf16" else (lambda v: v)
    conv3 = lambda x, Wb: conv2d_same(rnd(x), rnd(Wb[0]), Wb[1], True)
    x = np.asarray(grid, np.float32)
    acts, enc, i = [], [], 0
    for l in range(L):
        if l > 0:
            x = max_pool2(x)
        for _ in range(2):
            x = conv3(x, weights[i]); acts.append(x); i += 1
        enc.append(x)
    for l in range(L - 2, -1, -1):
        x = np.concatenate([upsample2(x), enc[l]], axis=-1)
        for _ in range(2):
            x = conv3(x, weights[i]); acts.append(x); i += 1
    x = conv2d_same(x, *weights[i], False); acts.append(x)
    return (x, acts) if return_all else x


def unet_flops(H: int, W: int, c_in: int = 3, widths=WIDTHS_S, c_out: int = 1) -> int:
    tot = 0
    for sp in unet_specs(c_in, widths, c_out):
        tot += 2 * (H >> sp.level) * (W >> sp.level) * sp.k * sp.k * sp.c_in * sp.c_out
    return tot


# ---------------------------------------------------------------------------------------------------------------------
# Layer-isolated elementwise checker of the device's activations (tests/test_unet_layer_oracle.py).
#
# unet_forward above propagates the oracle from the input image, so its comparison with a bf16 device run has to allow
# for rounding flips that spread downstream (a relative L2 of 1e-2).  The checker below does not propagate anything:
# convolution i is recomputed ONCE, in float64, from the activations the device itself stored for its inputs, and every
# output element is held to an a-priori bound of float32 accumulation.
#
#   Xop, Wop  the layer's input and kernel as the device multiplies them: bf16_round() of both in bf16 mode, as they are
#             in float32 mode (the x6 form splits both exactly into three bf16 planes)
#   r         max(conv(Xop, Wop) + b, 0) in float64, unrounded
#   A         conv(|Xop|, |Wop|) + |b|, the magnitude that bounds the accumulation error
#   E         (9 c_in + 8) * 2^-24 * A
#
# E is the float32 bound for a sum of n = 9 c_in products plus the bias in ANY order and any bracketing (each partial sum
# is rounded once: |error| <= (n - 1) u sum|terms| to first order, u = 2^-24), with slack for what else the device adds:
# the rounding of float32 products (float32 mode; bf16 x bf16 products are exact), up to 7 more roundings where the split-K
# slabs of a split layer are summed (ksplit <= 8), and, for x6, the dropped hi-lo / lo-mid / lo-lo plane products (each
# below 2^-26 of its product, i.e. < 2^-24 * A together).
#
# What is asserted depends on how the output is stored:
#   float32 (split producers, float32 mode, PSM_UNET_F32_ACT):  |dev - r| <= E for every element;
#   bf16    (finished activations of bf16 mode, fused pairs):   bf16_round(r - E) <= dev <= bf16_round(r + E) for every element
#           (the device's float32 value lies in [r - E, r + E] and both roundings are monotone, so this is exact), and the
#           elements with dev != bf16_round(r) -- a float32 value within E of a rounding boundary -- are at most 1 % of the
#           non-zero outputs.  Measured on an MI355X over tests/test_unet_layer_oracle.py: 0.108 % at worst.  A store that
#           truncates instead of rounding to nearest changes 24-35 % of them.
# ---------------------------------------------------------------------------------------------------------------------

U24 = 2.0 ** -24
BF16_MISMATCH_MAX = 0.01


def bf16_trunc(x) -> np.ndarray:
    """float32 -> bfloat16 by truncation (a WRONG store; the checker's mutation tests use it)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)
    return u.view(np.float32).reshape(np.shape(x))


def conv_nhwc64(x: np.ndarray, W: np.ndarray) -> np.ndarray:
    """x [n,H,W,Cin], W [k,k,Cin,Cout] -> [n,H,W,Cout] float64, zero 'same' padding, no bias."""
    k = W.shape[0]
    r = k // 2
    n, H, Wd, C = x.shape
    xp = np.zeros((n, H + 2 * r, Wd + 2 * r, C), np.float64)
    xp[:, r:r + H, r:r + Wd] = x
    W = np.asarray(W, np.float64)
    acc = np.zeros((n, H, Wd, W.shape[3]), np.float64)
    for ky in range(k):
        for kx in range(k):
            acc += xp[:, ky:ky + H, kx:kx + Wd] @ W[ky, kx]
    return acc


def layer_input(specs: List[ConvSpec], i: int, grid: np.ndarray, acts) -> np.ndarray:
    """The input of convolution i built from STORED activations acts[j] [n,H,W,C] (grid [n,H,W,c_in] for the first one)."""
    sp = specs[i]
    if sp.src == "input":
        return np.asarray(grid, np.float32)
    prev = acts[i - 1]
    if sp.src == "prev":
        return prev
    if sp.src == "pool":
        return np.stack([max_pool2(p) for p in prev])
    skip = acts[skip_index(specs, i)]
    return np.concatenate([np.repeat(np.repeat(prev, 2, axis=1), 2, axis=2), skip], axis=-1)


def skip_index(specs: List[ConvSpec], i: int) -> int:
    """Convolution whose output is concatenated into convolution i (src 'up+skip'): the last encoder layer of its level."""
    return [s.name for s in specs].index(f"enc{specs[i].level}b")


def layer_reference(x: np.ndarray, W: np.ndarray, b: np.ndarray, bf16: bool, relu: bool = True, ks_in: int = 1):
    """-> (r, E): the unrounded float64 output and its elementwise error bound (see the block comment above).  ks_in > 1 (bf16
    mode): the input arrives as float32 partial-sum slabs that the device's loader finishes itself, while the stored copy the
    checker reads was finished on the host; both add the slabs in slab order, but a value finished one float32 ulp apart may round
    to a different bf16 operand, so E also takes conv(|bf16(X (1 + d)) - bf16(X (1 - d))|, |Wop|), d = (ks_in + 2) * 2^-24."""
    x = np.asarray(x, np.float32)
    Xop = bf16_round(x) if bf16 else x
    Wop = bf16_round(W) if bf16 else np.asarray(W, np.float32)
    b64 = np.asarray(b, np.float64)
    r = conv_nhwc64(Xop.astype(np.float64), Wop) + b64
    if relu:
        r = np.maximum(r, 0.0)
    A = conv_nhwc64(np.abs(Xop).astype(np.float64), np.abs(Wop)) + np.abs(b64)
    k = W.shape[0]
    E = (k * k * W.shape[2] + 8) * U24 * A
    if bf16 and ks_in > 1:
        d = (ks_in + 2) * U24
        x64 = x.astype(np.float64)
        spread = np.abs(bf16_round((x64 * (1 + d)).astype(np.float32)).astype(np.float64) -
                        bf16_round((x64 * (1 - d)).astype(np.float32)).astype(np.float64))
        E = E + conv_nhwc64(spread, np.abs(Wop))
    return r, E


@dataclass
class LayerCheck:
    name: str
    stored: str           # 'f32' | 'bf16' | 'head'
    ok: bool
    ratio: float          # worst |dev - r| / E (f32 and head layers; 0 for bf16-stored ones)
    mismatch: float       # fraction of non-zero outputs with dev != bf16_round(r) (bf16-stored layers)
    bad: int              # elements outside the bound


def _ratio(err, E):
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(E > 0, err / np.where(E > 0, E, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(q.max()) if q.size else 0.0


def check_stored(name: str, dev: np.ndarray, r: np.ndarray, E: np.ndarray, stored_bf16: bool) -> LayerCheck:
    dev = np.asarray(dev, np.float32)
    if dev.shape != r.shape:
        return LayerCheck(name, "bf16" if stored_bf16 else "f32", False, np.inf, 1.0, int(r.size))
    if not stored_bf16:
        err = np.abs(dev.astype(np.float64) - r)
        bad = int(np.count_nonzero(~(err <= E)))
        return LayerCheck(name, "f32", bad == 0, _ratio(err, E), 0.0, bad)
    lo = bf16_round((r - E).astype(np.float32))
    hi = bf16_round((r + E).astype(np.float32))
    outside = ~((dev >= lo) & (dev <= hi))
    bad = int(np.count_nonzero(outside))
    rb = bf16_round(r.astype(np.float32))
    nz = max(1, int(np.count_nonzero(rb)))
    mism = int(np.count_nonzero(dev != rb)) / nz
    return LayerCheck(name, "bf16", bad == 0 and mism <= BF16_MISMATCH_MAX, 0.0, mism, bad)


def check_head(name: str, act: np.ndarray, Wh: np.ndarray, bh: np.ndarray, dev: np.ndarray, act_rel: float = 0.0) -> LayerCheck:
    """1x1 head against the float64 1x1 of the STORED activation act [n,H,W,c].  act_rel = 0: the head read exactly those values
    (separate head launch on a float32 activation, or a fused head whose layer stores float32); act_rel = 2^-8: a fused head
    reads the float32 registers v whose bf16 rounding was stored, |v - bf16(v)| <= 2^-8 |bf16(v)| (half an ulp of 8 significant
    bits; 2^-9 would be too tight: a pixel with a single non-zero channel comes within 5 % of the 2^-8 bound on the device)."""
    a = np.asarray(act, np.float64)
    w = np.asarray(Wh, np.float64).reshape(Wh.shape[-2], Wh.shape[-1])
    r = a @ w + np.asarray(bh, np.float64)
    mag = np.abs(a) @ np.abs(w)
    E = act_rel * mag + (w.shape[0] + 2) * U24 * ((1 + act_rel) * mag + np.abs(np.asarray(bh, np.float64)))
    err = np.abs(np.asarray(dev, np.float64) - r)
    bad = int(np.count_nonzero(~(err <= E)))
    return LayerCheck(name, "head", bad == 0, _ratio(err, E), 0.0, bad)


def check_unet_layers(grid, weights, acts, field, layout, c_in: int = 3, widths=WIDTHS_S, c_out: int = 1) -> List[LayerCheck]:
    """Every convolution of one forward pass, each against its own float64 recomputation from the stored activations.
    grid [n,H,W,c_in]; acts[i] [n,H_l,W_l,C] the stored output of convolution i (None: not stored -- that layer and its
    consumers are skipped); field [n,H,W,c_out] or None; layout[i]: dict with 'bf16' (the precision mode), 'out_bf16' (layer i
    is stored as bf16), 'ks_in' (deepest split of its producers) and, for the last 3x3 layer, 'fuse_head'."""
    specs = unet_specs(c_in, widths, c_out)
    out = []
    for i, sp in enumerate(specs):
        lay = layout[i]
        if sp.k == 1:
            if field is None or acts[i - 1] is None:
                continue
            prev = layout[i - 1]
            rel = 2.0 ** -8 if (prev.get("fuse_head") and prev["out_bf16"]) else 0.0
            out.append(check_head(sp.name, acts[i - 1], *weights[i], field, rel))
            continue
        if acts[i] is None or (sp.src != "input" and acts[i - 1] is None) or (sp.src == "up+skip" and acts[skip_index(specs, i)] is None):
            continue
        x = layer_input(specs, i, grid, acts)
        r, E = layer_reference(x, *weights[i], bf16=lay["bf16"], relu=sp.relu, ks_in=lay.get("ks_in", 1))
        out.append(check_stored(sp.name, acts[i], r, E, lay["out_bf16"]))
    return out


def exact_layer_outputs(grid, weights, widths=WIDTHS_S, c_in: int = 3, c_out: int = 1, precision: str = "f32", out_bf16=None):
    """What a correct device would store: every layer computed from the stored outputs of its producers and stored as float32
    (or, where out_bf16[i], as its bf16 rounding).  -> (acts, field); the reference the checker's mutation tests start from."""
    specs = unet_specs(c_in, widths, c_out)
    bf = precision == "bf16"
    acts = []
    field = None
    for i, sp in enumerate(specs):
        if sp.k == 1:
            a = acts[i - 1].astype(np.float64)
            field = (a @ np.asarray(weights[i][0], np.float64)[0, 0] + weights[i][1]).astype(np.float32)
            break
        r, _ = layer_reference(layer_input(specs, i, grid, acts), *weights[i], bf16=bf, relu=sp.relu)
        v = r.astype(np.float32)
        acts.append(bf16_round(v) if (out_bf16 is not None and out_bf16[i]) else v)
    return acts, field
