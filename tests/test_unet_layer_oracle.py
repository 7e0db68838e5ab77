"""Every convolution kernel of the convolutional path against a layer-isolated float64 oracle (oracle/unet_oracle.py,
check_unet_layers): each layer recomputed once from the activations the device itself stored for its inputs, every output
element held to the a-priori float32 accumulation bound E -- no propagation, so no bf16 rounding flips to allow for.

CPU: the checker's own sharpness (injected faults must be flagged, exact outputs must pass), and the list of kernel
instantiations in the built library against the dispatch mirror below.
GPU: sweeps of plans (set_choices, PSM_UNET_FORCE and the planner switches) that together launch every reachable kernel
instantiation; the module's last test asserts that they did.

Measured on an MI355X over this module (test_zz_report_and_coverage prints it; asserted: |dev - r| <= E, and at most
oracle.unet_oracle.BF16_MISMATCH_MAX = 1 % of a bf16-stored layer's non-zero outputs with dev != bf16_round(r)):
  float32 mode: worst |dev - r| / E 0.195 (1595 layer checks; 1x1 heads 0.168);
  bf16 mode:    worst |dev - r| / E 0.066 on float32-stored layers, worst bf16 mismatch 0.108 % (2366 layer checks);
  fused 1x1 heads of bf16 layers: worst 0.954 of their bound -- the stored bf16 activation is half a bf16 ulp, up to 2^-8 of its
  value, away from the float32 registers the head reads, and a pixel with one non-zero channel meets that bound almost exactly."""
import itertools
import os
import re

import numpy as np
import pytest

from kernel_symbols import library_kernels
from oracle import unet_oracle as uo

# ---------------------------------------------------------------------------------------------------------------------
# The kernel a plan_detail row launches: a mirror of psm_unet.hip (launch_variant, launch_variant_abf, psm_launch_conv_stem),
# psm_unet_pair.hip (psm_launch_conv_pair) and the forward pass of psm_unet_api.cpp.  Symbols are written as the demangled
# template id without spaces, e.g. "psm_conv3x3_kernel<8,2,2,2,0,1,true,2,true,false,2>".
# ---------------------------------------------------------------------------------------------------------------------
_VARIANT = {(0, 1): (8, 2, 1, 1), (0, 2): (8, 2, 2, 2), (1, 4): (2, 2, 4, 1), (2, 4): (16, 4, 4, 4), (3, 2): (16, 4, 2, 2),
            (4, 4): (8, 2, 4, 4)}
_SRC_TO_S = {0: 0, 1: 0, 2: 2, 3: 1, 4: 3}       # plan_detail source -> SRC template argument (PSM_SRC_SAME / MAXPOOL / UPSAMPLE, 3 = seam)


def _b(v):
    return "true" if v else "false"


def _conv(v, S, K, bf, nb, abf=False, x6=False, kw=1):
    th, wm, nct, wn = v
    return f"psm_conv3x3_kernel<{th},{wm},{nct},{wn},{S},{K},{_b(bf)},{nb},{_b(abf)},{_b(x6)},{kw}>"


def conv_symbol(d, c_in0=None):
    """Symbol of the generic / stem 3x3 launch of one plan_detail row (d: dict as UNetSurrogate.plan_detail returns)."""
    if d["stem"] == 1:
        c0 = c_in0
        kg = (9 * c0 + 15) // 16
        return "psm_conv_stem_kernel<2,3>" if c0 == 3 else "psm_conv_stem_kernel<3,4>" if c0 == 4 else f"psm_conv_stem_kernel<{kg},0>"
    arr = d["arrangement"]
    v = _VARIANT[(arr, d["nct"] if arr == 0 else {1: 4, 2: 4, 3: 2, 4: 4}[arr])]
    one = bool(d["one"])
    if arr >= 2:                                                  # launch_variant_abf: finished bf16 inputs only
        return _conv(v, _SRC_TO_S[d["src"]], 1, True, 1 if one else 2, abf=True)
    bf = bool(d["bf16"])
    if d["stem"] == 2:
        S, K = -1, 1
    else:
        S = _SRC_TO_S[d["src"]]
        km = d["km"]
        K = 1 if km <= 1 else 2 if km <= 2 else 4 if km <= 4 else 8
    nct = v[2]
    if K == 1 and S >= 0 and S != 3 and bf and d["in_bf"]:
        if v[0] == 8 and nct <= 2 and d["kw"] == 2 and not one:
            return _conv(v, S, 1, True, 2, abf=True, kw=2)
        return _conv(v, S, 1, True, 1 if one else 2, abf=True)
    if S >= 0 and nct <= 2 and d["x6"]:
        return _conv(v, S, K, True, 2, x6=True)
    if one and K == 1:
        return _conv(v, S, 1, bf, 1)
    return _conv(v, S, K, bf, 2)


def pair_symbol(d, c_in0, cm, head):
    keep = _b(d["keep"])
    if d["pair_kind"] == 0:
        return f"psm_pair_stem16_kernel<{c_in0},{keep}>"
    if cm == 16:
        return f"psm_pair_up16_kernel<{keep},{_b(head)}>"
    return f"psm_pair32_kernel<{2 if d['pair_kind'] == 2 else 1},{keep}>"


def plan_symbols(details, specs):
    """[symbol or None] per convolution: the kernel its launch runs (None: computed by another layer's launch)."""
    out = []
    for i, (d, sp) in enumerate(zip(details, specs)):
        if sp.k == 1:
            out.append(None if details[i - 1]["fuse_head"] else "psm_head1x1_kernel")
        elif d["pair"] == 2:
            out.append(None)
        elif d["pair"] == 1:
            out.append(pair_symbol(d, specs[0].c_in, sp.c_out, details[i + 1]["fuse_head"]))
        else:
            out.append(conv_symbol(d, specs[0].c_in))
    return out


def dispatch_symbols():
    """Every symbol the mirror can name: the instantiation list the launchers compile."""
    s = {"psm_head1x1_kernel"}
    for c0 in range(1, 8):
        s.add(conv_symbol(dict(stem=1), c0))
    for arr, nct, src, stem, in_bf, x6, kw, km, one, bf in itertools.product(
            range(5), (1, 2, 4), range(5), (0, 2), (0, 1), (0, 1), (1, 2), (1, 2, 4, 8), (0, 1), (0, 1)):
        if (arr == 0) != (nct != 4) or (arr >= 2 and (not bf or not in_bf or src == 4 or stem or km > 1 or x6)):
            continue
        if stem and src != 0:
            continue
        s.add(conv_symbol(dict(arrangement=arr, nct=nct, src=src, stem=stem, in_bf=in_bf, x6=x6, kw=kw, km=km, one=one, bf16=bf)))
    for keep in (0, 1):
        for c0 in (3, 4):
            s.add(pair_symbol(dict(pair_kind=0, keep=keep), c0, 16, False))
        for head in (False, True):
            s.add(pair_symbol(dict(pair_kind=1, keep=keep), 3, 16, head))
        for kind in (1, 2):
            s.add(pair_symbol(dict(pair_kind=kind, keep=keep), 3, 32, False))
    return s


def _c(th, wm, nct, wn, S, K, bf, nb, abf=False, x6=False, kw=1):
    return _conv((th, wm, nct, wn), S, K, bf, nb, abf, x6, kw)


# Instantiations no plan can reach, each with the reason.
UNREACHABLE = {
    # the generic form on unaligned channels (SRC -1) only runs the first layer on the raw image, c_in <= 16 (psm_unet_create): one
    # chunk of 16 (float32) or 32 (bf16) channels, so the double-buffered build (NB = 2) never launches
    **{_c(*v, -1, 1, bf, 2): "c_in <= 16 is one chunk" for v in [(8, 2, 1, 1), (8, 2, 2, 2), (2, 2, 4, 1)] for bf in (False, True)},
    # float32 (non-x6) chunks are 16 channels and every width is a multiple of 16: the concatenation seam always lies on a chunk
    # boundary, so the seam-inside-a-chunk loader (SRC 3) is reached by bf16 and x6 layers (32-channel chunks) only
    **{_c(*v, 3, K, False, nb): "widths are multiples of 16: no seam inside a float32 chunk"
       for v in [(8, 2, 1, 1), (8, 2, 2, 2), (2, 2, 4, 1)] for K, nb in [(1, 1), (1, 2), (2, 2), (4, 2), (8, 2)]},
    # a 16-channel upsample pair without a fused head needs its second convolution stored as bf16 for a 3x3 consumer; that
    # consumer is the next decoder layer, whose upsample source then has 16 channels -- a seam inside a 32-channel chunk, which
    # reads float32 -- so the planner never forms such a pair (the 16-channel upsample pair is always the last level's, head fused)
    **{f"psm_pair_up16_kernel<{_b(k)},false>": "its output would feed a seam-inside-chunk consumer (float32 inputs)" for k in (False, True)},
}

_KERNEL_RE = re.compile(r"(psm_(?:conv3x3|conv_stem|head1x1|pair_stem16|pair_up16|pair32)_kernel)(<[^>]*>)?\(")


def library_conv_kernels(lib_path):
    """Kernel symbols of the convolutional path in the gfx950 code objects of the built library (kernel_symbols.py)."""
    return library_kernels(lib_path, _KERNEL_RE)


def test_library_kernels_match_the_dispatch_mirror():
    """The built library holds exactly the instantiations the mirror above names (206 generic 3x3, 6 stem, the 1x1 head, 12 fused
    pairs): a kernel added to the launchers fails here until the mirror -- and with it the GPU coverage assertion -- knows it."""
    from psm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} not built")
    lib = library_conv_kernels(_lib.LIB_PATH)
    mirror = dispatch_symbols()
    assert sum(s.startswith("psm_conv3x3_kernel") for s in lib) == 206
    assert sum(s.startswith("psm_conv_stem_kernel") for s in lib) == 6
    assert sum(s.startswith("psm_pair") for s in lib) == 12
    assert lib == mirror, (sorted(lib - mirror)[:10], sorted(mirror - lib)[:10])
    assert set(UNREACHABLE) <= lib
    assert len(lib) - len(UNREACHABLE) == 202


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the checker is sharp
# ---------------------------------------------------------------------------------------------------------------------
_MUT_NET = dict(c_in=3, widths=(16, 32), c_out=1)
_MUT_SHAPES = [(8, 16, 2), (30, 14, 2), (512, 16, 2)]          # the last: a 512-row level


def _mut_setup(ny, nx, n, precision, seed=3):
    specs = uo.unet_specs(**_MUT_NET)
    W = uo.he_weights(specs, seed=seed)
    g = np.random.default_rng(seed).standard_normal((n, ny, nx, _MUT_NET["c_in"])).astype(np.float32)
    out_bf = [precision == "bf16"] * (len(specs) - 1)
    acts, field = uo.exact_layer_outputs(g, W, precision=precision, out_bf16=out_bf, **_MUT_NET)
    layout = [dict(bf16=precision == "bf16", out_bf16=precision == "bf16", ks_in=1, fuse_head=False) for _ in specs]
    return specs, W, g, acts, field, layout


def _store(v, precision, trunc=False):
    v = np.asarray(v, np.float32)
    if precision != "bf16":
        return v
    return uo.bf16_trunc(v) if trunc else uo.bf16_round(v)


def _recompute(specs, W, i, x, precision, w_override=None):
    Wi, bi = W[i]
    r, _ = uo.layer_reference(x, w_override if w_override is not None else Wi, bi, bf16=precision == "bf16")
    return r


def _fault(name, specs, W, g, acts, precision):
    """-> (layer index, faulty stored output of that layer)."""
    dec = [s.name for s in specs].index("dec0a")
    mid = [s.name for s in specs].index("enc1b")
    x = uo.layer_input(specs, dec, g, acts)
    if name == "truncating_bf16_store":
        return mid, _store(_recompute(specs, W, mid, uo.layer_input(specs, mid, g, acts), precision), precision, trunc=True)
    if name == "tap_dropped_in_edge_ring":
        r = _recompute(specs, W, dec, x, precision)
        Wd = W[dec][0].copy()
        Wd[0, 0] = 0
        rd = _recompute(specs, W, dec, x, precision, Wd)
        ring = np.ones(r.shape[1:3], bool)
        ring[8:-8, 8:-8] = False
        r[:, ring] = rd[:, ring]
        return dec, _store(r, precision)
    if name == "last_8_channels_lost_on_last_two_rows":
        xl = x.copy()
        xl[:, -2:, :, -8:] = 0
        return dec, _store(_recompute(specs, W, dec, xl, precision), precision)
    if name == "skip_and_upsample_swapped_at_the_seam":
        up = x.shape[-1] - specs[uo.skip_index(specs, dec)].c_out
        xs = np.concatenate([x[..., up:], x[..., :up]], axis=-1)
        return dec, _store(_recompute(specs, W, dec, xs, precision), precision)
    if name == "one_output_channel_scaled":
        r = _recompute(specs, W, dec, x, precision)
        r[..., 5] *= 1 + 2.0 ** -7
        return dec, _store(r, precision)
    if name == "case_written_from_the_next_case":
        r = _recompute(specs, W, dec, x, precision)
        return dec, _store(np.concatenate([r[1:2], r[1:]], axis=0), precision)
    raise KeyError(name)


_FAULTS = ["truncating_bf16_store", "tap_dropped_in_edge_ring", "last_8_channels_lost_on_last_two_rows",
           "skip_and_upsample_swapped_at_the_seam", "one_output_channel_scaled", "case_written_from_the_next_case"]


@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_checker_passes_exact_outputs(precision):
    for ny, nx, n in _MUT_SHAPES:
        specs, W, g, acts, field, layout = _mut_setup(ny, nx, n, precision)
        res = uo.check_unet_layers(g, W, acts, field, layout, **_MUT_NET)
        assert len(res) == len(specs)
        for r in res:
            assert r.ok and r.bad == 0 and r.mismatch == 0.0, (ny, nx, r)
            assert r.ratio <= 0.1, r                         # one float32 rounding of the float64 value: far inside E


@pytest.mark.parametrize("fault,precision", [(f, p) for p in ("bf16", "f32") for f in _FAULTS
                                             if p == "bf16" or f != "truncating_bf16_store"])     # a float32 store does not round
def test_checker_flags_injected_fault(fault, precision):
    """Each fault is confined to one layer (the rest exact) and must be flagged on that layer on at least one of three shapes,
    one of them a 512-row level -- where the chained relative-L2 bound of test_unet.py lets an edge fault through."""
    flagged = []
    for ny, nx, n in _MUT_SHAPES:
        specs, W, g, acts, field, layout = _mut_setup(ny, nx, n, precision)
        i, bad = _fault(fault, specs, W, g, acts, precision)
        acts = list(acts)
        acts[i] = bad
        res = {r.name: r for r in uo.check_unet_layers(g, W, acts, None, layout, **_MUT_NET)}
        flagged.append(not res[specs[i].name].ok)
    assert any(flagged), (fault, precision, flagged)


def test_truncation_changes_a_quarter_of_the_outputs():
    """The 1 % mismatch cap against what a truncating store does (24-35 % of the non-zero outputs)."""
    specs, W, g, acts, field, layout = _mut_setup(96, 160, 1, "bf16")
    i, bad = _fault("truncating_bf16_store", specs, W, g, acts, "bf16")
    r, E = uo.layer_reference(uo.layer_input(specs, i, g, acts), *W[i], bf16=True)
    res = uo.check_stored("x", bad, r, E, True)
    assert res.mismatch > 0.2 and not res.ok


def test_checker_head_bounds():
    rng = np.random.default_rng(1)
    act = np.maximum(rng.standard_normal((2, 6, 10, 16)), 0).astype(np.float32)
    Wh = rng.standard_normal((1, 1, 16, 3)).astype(np.float32)
    bh = rng.standard_normal(3).astype(np.float32)
    exact = (act.astype(np.float64) @ Wh[0, 0].astype(np.float64) + bh).astype(np.float32)
    assert uo.check_head("h", act, Wh, bh, exact).ok
    assert not uo.check_head("h", act, Wh, bh, exact * (1 + 2.0 ** -12)).ok
    # a fused head reads the float32 values whose bf16 rounding was stored
    act_bf = uo.bf16_round(act)
    assert uo.check_head("h", act_bf, Wh, bh, exact, act_rel=2.0 ** -8).ok
    assert not uo.check_head("h", act_bf, Wh, bh, exact + 0.05, act_rel=2.0 ** -8).ok


# ---------------------------------------------------------------------------------------------------------------------
# GPU: every layer of every run through the checker; the kernels launched are collected for the coverage assertion
# ---------------------------------------------------------------------------------------------------------------------
_RAN = set()                       # kernel symbols launched by this module's runs
_SWEEPS_DONE = set()               # sweep tests that completed (the coverage assertion needs all of them)
_STATS = {}                        # precision -> worst ratio / mismatch, with the layer and run that set it


def _record(precision, tag, res):
    st = _STATS.setdefault(precision, {"ratio": (0.0, ""), "mismatch": (0.0, ""), "head": (0.0, ""), "layers": 0})
    for r in res:
        st["layers"] += 1
        key, val = ("head", r.ratio) if r.stored == "head" else ("ratio", r.ratio) if r.stored == "f32" else ("mismatch", r.mismatch)
        if val >= st[key][0]:
            st[key] = (val, f"{tag} {r.name}")


def _grids(n, ny, nx, c_in, seed):
    return np.random.default_rng(seed).standard_normal((n, ny, nx, c_in)).astype(np.float32)


def _read_acts(net, n_layers, n):
    from psm_amd import _lib
    acts = []
    for i in range(n_layers - 1):
        try:
            acts.append(net.activation(i, n))
        except _lib.PsmError:                  # kept on chip by a fused pair without keep_activations
            acts.append(None)
    return acts


def _layout(details, specs):
    return [dict(bf16=bool(d["bf16"]), out_bf16=bool(d["bf16"]) and (bool(d["out_bf"]) or d["pair"] != 0), ks_in=d["km"],
                 fuse_head=bool(d["fuse_head"])) for d in details]


def _check(tag, precision, specs, W, grids, acts, field, details, c_in, widths, c_out):
    res = uo.check_unet_layers(grids, W, acts, field, _layout(details, specs), c_in, widths, c_out)
    _record(precision, tag, res)
    bad = [r for r in res if not r.ok]
    assert not bad, (tag, bad[:3])
    return res


def _run(c_in, widths, c_out, ny, nx, precision, n=1, keep=True, seed=0, choices=None, max_cases=None, check=True, tag=""):
    """One handle, one forward pass of n cases, every stored layer through the checker.  -> (field, acts, details)."""
    from psm_amd import UNetSurrogate
    specs = uo.unet_specs(c_in, widths, c_out)
    W = uo.he_weights(specs, seed=seed + 100)
    g = _grids(n, ny, nx, c_in, seed)
    with UNetSurrogate(W, ny, nx, c_in=c_in, c_out=c_out, widths=widths, max_cases=max_cases or n, precision=precision,
                       keep_activations=keep, choices=choices) as net:
        field = net.forward(g)
        details = [net.plan_detail(i) for i in range(len(specs))]
        acts = _read_acts(net, len(specs), n)
    _RAN.update(s for s in plan_symbols(details, specs) if s)
    if check:
        _check(tag or f"{precision} c_in={c_in} {widths} {ny}x{nx}x{n}", precision, specs, W, g, acts, field, details, c_in, widths, c_out)
    return field, acts, details


# ---- sweeps of forced plans (PSM_UNET_FORCE = "layer:arrangement:nct:ksplit,...") ------------------------------------
_SWEEP_NETS = [dict(c_in=3, widths=(64, 256, 256), c_out=16),     # unaligned image (generic SRC -1), 8-way splits at every source
               dict(c_in=4, widths=(64, 64, 64), c_out=1),        # aligned image (generic SAME), upsample layers of <= 8 chunks
               dict(c_in=5, widths=(64, 272, 272), c_out=3),      # seam inside a 32-channel chunk behind 8-way split producers
               dict(c_in=9, widths=(64, 48, 80), c_out=1)]        # seams inside a chunk, odd chunk counts, short layers
_PATTERNS = ("k1", "k2", "k4", "k8", "alt_a", "alt_b")


def _force(net, precision, arr, nct, pattern, x6_on):
    """PSM_UNET_FORCE string: every 3x3 layer (but the stem kernel's) to (arr, nct) where its channel count allows, split per pattern."""
    specs = uo.unet_specs(**net)
    items = []
    for i, sp in enumerate(specs):
        if sp.k != 3:
            continue
        feeds = specs[i + 1].k == 3
        stem_layer = sp.src == "input" and 9 * sp.c_in <= 64 and sp.c_out <= 16
        if stem_layer:
            continue
        a, t = (arr, nct) if nct <= (sp.c_out + 15) // 16 else (0, 1)
        x6 = precision == "f32" and x6_on and sp.src != "input" and sp.c_in >= 64 and a == 0
        chunks = -(-sp.c_in // (32 if precision == "bf16" or x6 else 16))
        full = min(8, chunks)
        ks = {"k1": 1, "k2": min(2, chunks), "k4": min(4, chunks), "k8": full,
              "alt_a": full if sp.name.endswith("a") else 1, "alt_b": full if sp.name.endswith("b") else 1}[pattern]
        items.append(f"{i}:{a}:{t}:{ks if feeds else 1}")
    return ",".join(items)


def _sweep(monkeypatch, precision, variants, patterns, env, name):
    for net in _SWEEP_NETS:
        for (arr, nct), pat in itertools.product(variants, patterns):
            with monkeypatch.context() as mp:
                mp.setenv("PSM_UNET_NO_PAIR", "1")
                for k, v in env.items():
                    mp.setenv(k, v)
                mp.setenv("PSM_UNET_FORCE", _force(net, precision, arr, nct, pat, env.get("PSM_UNET_X6") != "0"))
                _run(**net, ny=12, nx=20, precision=precision, n=2, seed=arr * 7 + nct, tag=f"{name} {arr}/{nct} {pat} {net['widths']}")
    _SWEEPS_DONE.add(name)


_SWEEPS = {
    "f32": ("f32", [(0, 1), (0, 2), (1, 4)], _PATTERNS, {"PSM_UNET_X6": "0"}),
    "x6": ("f32", [(0, 1), (0, 2)], _PATTERNS, {}),
    "bf16_f32act": ("bf16", [(0, 1), (0, 2), (1, 4)], _PATTERNS, {"PSM_UNET_F32_ACT": "1", "PSM_UNET_KW": "0"}),
    "bf16_abf": ("bf16", [(0, 1), (0, 2), (1, 4), (2, 4), (3, 2), (4, 4)], ("k1", "alt_a", "alt_b", "k8"), {"PSM_UNET_KW": "0"}),
    "bf16_kw": ("bf16", [(0, 1), (0, 2)], ("k1", "alt_a"), {"PSM_UNET_KW": "-2"}),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(_SWEEPS))
def test_gpu_forced_plan_sweep(name, monkeypatch):
    precision, variants, patterns, env = _SWEEPS[name]
    _sweep(monkeypatch, precision, variants, patterns, env, name)


# ---- the planner's own plans on small networks: every stem, seams inside chunks, odd chunk counts ----------------------
_SMALL = [((16, 48, 80), (20, 36)), ((16, 32), (14, 30)), ((16, 32, 48, 96), (24, 40))]


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_gpu_small_networks_every_stem(precision):
    """c_in 1..7 take the six stem kernels (K = 9 c_in flattened), 9 the generic kernel on unaligned channels, 16 the aligned one;
    c_out 1 / 3 / 16; widths whose concatenation seam lies inside a 32-channel chunk and whose layers have odd chunk counts."""
    for j, c_in in enumerate((1, 2, 3, 4, 5, 6, 7, 9, 16)):
        widths, (ny, nx) = _SMALL[j % 3]
        details = _run(c_in, widths, (1, 3, 16)[j % 3], ny, nx, precision, n=2, seed=j)[2]
        assert details[0]["stem"] == (1 if c_in <= 7 else 2 if c_in % 4 else 0), (c_in, details[0])
    _SWEEPS_DONE.add(f"small_{precision}")


_SWITCHES = [{"PSM_UNET_NO_STEM": "1"}, {"PSM_UNET_NO_HEAD_FUSION": "1"}, {"PSM_UNET_F32_ACT": "1"}, {"PSM_UNET_NO_SPLIT": "1"},
             {"PSM_UNET_SPLIT_MIN_CHUNKS": "1"}, {"PSM_UNET_KSPLIT_MAX": "2"}, {"PSM_UNET_PAIR_MIN": "1", "PSM_UNET_PAIR32": "0"},
             {"PSM_UNET_PAIR_MIN": "1"}, {}]


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_gpu_planner_switches(precision, monkeypatch):
    for env in _SWITCHES:
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            _run(3, (16, 32, 64, 128), 1, 56, 88, precision, n=2, seed=5, tag=f"{precision} {env}")
    _SWEEPS_DONE.add(f"switches_{precision}")


# ---- fused level pairs: keep and no keep give the same bits ---------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("c_in", [3, 4])
def test_gpu_fused_pairs_keep_and_no_keep(c_in, monkeypatch):
    """Every pair kernel (stem, pool, 32- and 16-channel upsample with the fused head) at a size that is not a multiple of the
    30 x 14 tile on either axis at any level, three cases: with keep_activations both convolutions of every pair through the
    checker; without it the same plan must give a bit-identical field and bit-identical stored outputs."""
    monkeypatch.setenv("PSM_UNET_PAIR_MIN", "1")
    widths, ny, nx = (16, 32, 64), 44, 52
    f1, a1, d1 = _run(c_in, widths, 1, ny, nx, "bf16", n=3, keep=True, seed=c_in, tag=f"pairs keep c_in={c_in}")
    assert sum(d["pair"] == 1 for d in d1) == 4, d1                 # enc0, enc1, dec1, dec0
    f2, a2, d2 = _run(c_in, widths, 1, ny, nx, "bf16", n=3, keep=False, seed=c_in, tag=f"pairs c_in={c_in}")
    assert [dict(d, keep=0) for d in d1] == [dict(d, keep=0) for d in d2]
    assert np.array_equal(f1, f2)
    stored = [i for i, a in enumerate(a2) if a is not None]
    assert stored and all(np.array_equal(a1[i], a2[i]) for i in stored)
    assert all(a2[i] is None for i, d in enumerate(d2) if d["pair"] == 1)
    _SWEEPS_DONE.add(f"pairs_{c_in}")


# ---- partial batches, determinism ------------------------------------------------------------------------------------
_PARTIAL = {
    "split": ("f32", {"PSM_UNET_NO_PAIR": "1"}, "k8"),
    "pair": ("bf16", {"PSM_UNET_PAIR_MIN": "1"}, None),
    "kw": ("bf16", {"PSM_UNET_KW": "-2", "PSM_UNET_NO_PAIR": "1"}, "k1"),
}


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(_PARTIAL))
def test_gpu_partial_batch_matches_the_full_batch(kind, monkeypatch):
    """max_cases = 5: forward(5), then forward(2) on the same handle.  Split-K slabs are laid out [ksplit][max_cases][H][W][C] and
    pair tiles are built for the planned batch; cases 0-1 of the short pass must be bit-identical to the same inputs inside the
    full batch, and both passes pass the checker.  Two passes of one plan are bit-identical."""
    from psm_amd import UNetSurrogate
    precision, env, pattern = _PARTIAL[kind]
    c_in, widths, c_out = (3, (16, 32, 64), 1) if kind == "pair" else (4, (64, 128, 128), 1)
    ny, nx = (44, 52) if kind == "pair" else (20, 36)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if pattern:
        monkeypatch.setenv("PSM_UNET_FORCE", _force(dict(c_in=c_in, widths=widths, c_out=c_out), precision, 0, 2, pattern, True))
    specs = uo.unet_specs(c_in, widths, c_out)
    W = uo.he_weights(specs, seed=31)
    g = _grids(5, ny, nx, c_in, 31)
    with UNetSurrogate(W, ny, nx, c_in=c_in, c_out=c_out, widths=widths, max_cases=5, precision=precision, keep_activations=True) as net:
        details = [net.plan_detail(i) for i in range(len(specs))]
        f5 = net.forward(g)
        a5 = _read_acts(net, len(specs), 5)
        f5b = net.forward(g)
        a5b = _read_acts(net, len(specs), 5)
        f2 = net.forward(g[:2])
        a2 = _read_acts(net, len(specs), 2)
    _RAN.update(s for s in plan_symbols(details, specs) if s)
    if kind == "split":
        assert max(d["ksplit"] for d in details) == 8
    if kind == "pair":
        assert any(d["pair"] == 1 for d in details)
    if kind == "kw":
        assert any(d["kw"] == 2 for d in details)
    assert np.array_equal(f5, f5b) and all(np.array_equal(x, y) for x, y in zip(a5, a5b))        # deterministic
    assert np.array_equal(f2, f5[:2])
    for i, (x, y) in enumerate(zip(a2, a5)):
        assert np.array_equal(x, y[:2]), specs[i].name
    _check(f"partial {kind} n=5", precision, specs, W, g, a5, f5, details, c_in, widths, c_out)
    _check(f"partial {kind} n=2", precision, specs, W, g[:2], a2, f2, details, c_in, widths, c_out)
    _SWEEPS_DONE.add(f"partial_{kind}")


# ---- the bench's configurations with the planner's own plan ----------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("precision,ny,nx,n", [("bf16", 512, 512, 1), ("f32", 512, 512, 1), ("bf16", 256, 256, 8)])
def test_gpu_planner_plan_bench_sizes(precision, ny, nx, n):
    """UNet-S at the sizes bench.py times, the planner's plan: every layer through the checker (keep_activations), and the
    timed build without keep gives the same bits."""
    fk, _, dk = _run(3, uo.WIDTHS_S, 1, ny, nx, precision, n=n, keep=True, seed=9, tag=f"bench {precision} {ny}x{nx}x{n}")
    f, _, d = _run(3, uo.WIDTHS_S, 1, ny, nx, precision, n=n, keep=False, seed=9, check=False)
    assert [dict(x, keep=0) for x in dk] == [dict(x, keep=0) for x in d]
    assert np.array_equal(fk, f)
    _SWEEPS_DONE.add(f"bench_{precision}_{ny}_{n}")


# ---- the 2^31 guard ------------------------------------------------------------------------------------------------
def _largest_case_elems(c_in, widths, ny, nx, bf16):
    worst = ny * nx * c_in
    for sp in uo.unet_specs(c_in, widths, 1)[:-1]:
        H, W = ny >> sp.level, nx >> sp.level
        worst = max(worst, (4 + H + 32) * (4 + W + 64) * sp.c_out if bf16 else H * W * sp.c_out)
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_gpu_plan_rejects_per_case_offsets_of_2_31(precision):
    """The 3x3 loaders address a case's tensors with 32-bit element offsets: a single 16384 x 16384 case with 16-channel level-0
    activations (2^32 elements) must be refused at plan time, before anything is allocated or launched; the largest width
    that stays below 2^31 at 8192 rows plans.  No forward pass at these sizes."""
    from psm_amd import UNetSurrogate, _lib
    widths = (16, 32)
    W = uo.he_weights(uo.unet_specs(1, widths, 1), seed=1)
    assert _largest_case_elems(1, widths, 16384, 16384, precision == "bf16") >= 2 ** 31
    with pytest.raises(_lib.PsmError) as e:
        UNetSurrogate(W, 16384, 16384, c_in=1, widths=widths, precision=precision)
    assert e.value.code == -1 and "2^31" in str(e.value)
    ny = 8192
    nx = max(x for x in range(2, 20000, 2) if _largest_case_elems(1, widths, ny, x, precision == "bf16") < 2 ** 31)
    with pytest.raises(_lib.PsmError) as e:
        UNetSurrogate(W, ny, nx + 2, c_in=1, widths=widths, precision=precision)
    assert "2^31" in str(e.value)
    with UNetSurrogate(W, ny, nx, c_in=1, widths=widths, precision=precision) as net:
        assert net.flops > 0


# ---- coverage --------------------------------------------------------------------------------------------------------
_ALL_SWEEPS = (set(_SWEEPS) | {"small_f32", "small_bf16", "switches_f32", "switches_bf16", "pairs_3", "pairs_4", "partial_split",
                               "partial_pair", "partial_kw", "bench_bf16_512_1", "bench_f32_512_1", "bench_bf16_256_8"})


@pytest.mark.gpu
def test_zz_report_and_coverage():
    """The runs above launched every instantiation the launchers can reach: the dispatch mirror's list minus UNREACHABLE."""
    for prec, st in sorted(_STATS.items()):
        print(f"\nlayer oracle, {prec} mode: {st['layers']} layer checks; worst |dev - r| / E of float32-stored layers {st['ratio'][0]:.3g} "
              f"({st['ratio'][1]}); worst bf16 mismatch {st['mismatch'][0]:.4%} ({st['mismatch'][1] or 'no bf16-stored layer'}); "
              f"worst head ratio {st['head'][0]:.3g} ({st['head'][1]})")
    missing_runs = _ALL_SWEEPS - _SWEEPS_DONE
    if missing_runs:
        pytest.skip(f"coverage needs the whole module; not run or failed: {sorted(missing_runs)}")
    expected = dispatch_symbols() - set(UNREACHABLE)
    print(f"kernels launched: {len(_RAN)} of {len(expected)} reachable")
    assert not (_RAN & set(UNREACHABLE)), sorted(_RAN & set(UNREACHABLE))
    assert _RAN == expected, ("not launched:", sorted(expected - _RAN), "unknown:", sorted(_RAN - expected))
