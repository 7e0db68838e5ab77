"""The bookkeeping of the three evaluators' ``timeSteps`` without a GPU: what is returned and recorded must not depend on whether the
host (``device_prep=False``) or the device (``device_prep=True``) prepared the frames.  The GPU suite holds this on real fields
(test_frame_rows.py); here the surrogate is a stand-in whose entries return canned, seeded, finite arrays per dataset frame, so
that only the host code around the calls is under test: the frame loop, the skip rule, the slots of irrelevant frames, chunks of
``max_frames`` with a shorter last one, the lists, ``last_metrics``, ``U_max_norm``, ``frame_metrics`` and ``label_planes``.

The stand-in also holds the calls to the statements quoted in test_frame_rows.py: the columns a host-mode call sends are those of
``host_deltas`` / ``host_poisson`` / ``host_gradp`` bit for bit (a frame is recognised by them), and U2, (L, U) and the out-scale
carry the bits of the quoted scalars; the rows entries mark as irrelevant exactly the frames the quoted skip rule drops.

Datasets: the files of test_frame_rows' fixtures; the deltas and Poisson evaluators read the variant whose frame 1 is irrelevant
(``still_dataset``).  times: seven frames with max_frames = 2 -- the rows mode sends 2 + 2 + 2 + 1, the host mode the five relevant
ones as 2 + 2 + 1; the gradP evaluator (no skip rule) five frames as 2 + 2 + 1."""
import numpy as np
import pytest

import test_deltas_frames as tdf
import test_frame_rows as tfr
import test_gradp_frames as tgf
import test_poisson_frames as tpf
from psm_amd import GridSurrogate, formats
from test_frame_rows import ds_deltas, ds_gradp, ds_poisson, equal     # noqa: F401  (the fixtures are used by name)

SHAPE = {"deltas": (9, 11), "poisson": (9, 11), "gradp": (203, 13)}     # the gradP cut reads row 200
MAX_FRAMES = 2
TIMES = {"deltas": [0, 1, 2, 2, 0, 1, 2], "poisson": [0, 1, 2, 2, 0, 1, 2], "gradp": [0, 1, 1, 0, 1]}
STILL = 1                                                               # the irrelevant frame of still_dataset
N_RAW = {"deltas": 2, "poisson": 3, "gradp": 4}


def canned(kind, t, ny, nx):
    """The arrays of dataset frame t (-1: the unspecified content of an irrelevant frame's slot), every raw row with n > 0."""
    rng = np.random.default_rng(4242 + 17 * t)
    raw = np.empty((N_RAW[kind], 8))
    for r in raw:
        n, s1, spread = float(rng.integers(50, 90)), rng.normal(), rng.random(4) + 0.5
        r[:] = (n, s1, s1 * s1 / n + rng.random() + 0.1, -spread[0], spread[1], -spread[2], spread[3], 0.0)
    f32 = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    if kind == "deltas":
        return dict(result=f32(ny, nx), truth=rng.standard_normal((ny, nx)), raw=raw)
    if kind == "poisson":
        return dict(result=f32(ny, nx, 1), change=f32(ny, nx), next=f32(ny, nx), extra=rng.standard_normal((2, ny, nx)), raw=raw)
    return dict(gradp=f32(ny, nx, 2), p=f32(ny, nx), truth=rng.standard_normal((3, ny, nx)), raw=raw)


class StandIn:
    """What ``timeSteps`` asks of a GridSurrogate.  ``frames``: the dataset's rows per time; ``quoted(d)`` -> (cols, scalars): the
    statements of test_frame_rows.py on one frame's rows."""
    guard_trips = 0
    metrics_from_sums = GridSurrogate.metrics_from_sums                 # host arithmetic of the library, no GPU

    def __init__(self, kind, frames, quoted, base, phi=None, exy=None):
        self.kind, (self.ny, self.nx), self.max_cases = kind, SHAPE[kind], MAX_FRAMES
        self.quoted, self.base, self.phi, self.exy = quoted, base, phi, exy
        self._frames_bound = self._feat_bound = self._post_bound = self._deltas_bound = self._gradp_bound = False
        self._rows_bound = 0
        self.by_rows = {d.tobytes(): t for t, d in enumerate(frames)}
        self.scalars = [quoted(d)[1] for d in frames]
        self.by_cols = {quoted(d)[0].tobytes(): t for t, d in enumerate(frames) if self.scalars[t][3]}
        self.sent = []                                                  # (entry, frames of the call)

    # -- the bindings: flags only
    def bind_poststeps(self, *a):
        self._post_bound = True

    def bind_features(self, sdf, k, max_abs):
        assert np.shape(sdf) == (MAX_FRAMES,) + SHAPE[self.kind]
        self._feat_bound = True

    def bind_frames(self, n_frames, k):
        assert n_frames == MAX_FRAMES and k == tfr.KINDS[self.kind][1]
        self._frames_bound, self._deltas_bound, self._gradp_bound, self._rows_bound = True, False, False, 0

    def bind_deltas_frames(self, sdf, max_abs):
        assert self._frames_bound
        self._deltas_bound = True

    def bind_gradp_frames(self, sdf, max_abs, cy, cx, dx, dy):
        assert self._frames_bound and cy == 200
        self._gradp_bound = True
        return True

    def bind_rows(self, width):
        assert self._frames_bound
        self._rows_bound = int(width)

    # -- the frame entries
    def _stack(self, name, ts, keys, wants):
        assert 1 <= len(ts) <= MAX_FRAMES
        self.sent.append((name, len(ts)))
        frames = [canned(self.kind, t, self.ny, self.nx) for t in ts]
        return [np.stack([f[key] for f in frames]) if want else None for key, want in zip(keys, wants)]

    def _host(self, cols):
        """The frames of a host-mode call, recognised by the bits of their columns -> (times, their quoted scalars)."""
        assert cols.dtype == np.float64 and cols.ndim == 3
        ts = [self.by_cols[c.tobytes()] for c in cols]                  # KeyError: not the quoted statements' columns
        return ts, [self.scalars[t] for t in ts]

    def _rows(self, rows):
        """The frames of a rows-mode call -> (times with -1 for an irrelevant frame, scalars [n,8])."""
        assert rows.dtype == np.float32 and rows.ndim == 3 and rows.shape[2] <= self._rows_bound
        ts = [self.by_rows[d.tobytes()] for d in rows]
        sc = np.array([self.scalars[t] for t in ts], np.float64)
        return [t if sc[j, 3] else -1 for j, t in enumerate(ts)], sc

    def deltas_frames(self, cols, U2, out_scale=None, apply_filter=False, want_result=True, want_truth=True, want_raw=True):
        assert self._deltas_bound
        ts, sc = self._host(cols)
        assert equal([float(u) for u in U2], [s[4] for s in sc]) and equal([float(s) for s in out_scale], [s[5] for s in sc])
        return tuple(self._stack("deltas_frames", ts, ("result", "truth", "raw"), (want_result, want_truth, want_raw)))

    def deltas_rows(self, rows, base, apply_filter=False, want_result=True, want_truth=True, want_raw=True):
        assert self._deltas_bound and base == self.base
        ts, sc = self._rows(rows)
        return (*self._stack("deltas_rows", ts, ("result", "truth", "raw"), (want_result, want_truth, want_raw)), sc)

    def _poisson_host(self, cols, LU, out_scale):
        assert self._feat_bound and self._post_bound
        ts, sc = self._host(cols)
        assert equal([[float(v) for v in lu] for lu in LU], [[float(self.phi), s[0]] for s in sc])
        assert equal([float(s) for s in out_scale], [s[5] for s in sc])
        return ts

    def poisson_frames(self, cols, LU, out_scale=None, apply_filter=False, weighting=True, want_extra=True):
        assert weighting and want_extra
        return tuple(self._stack("poisson_frames", self._poisson_host(cols, LU, out_scale), ("result", "change", "next", "extra"), (1, 1, 1, 1)))

    def poisson_frames_errors(self, cols, LU, out_scale=None, apply_filter=False):
        return self._stack("poisson_frames_errors", self._poisson_host(cols, LU, out_scale), ("raw",), (1,))[0]

    def poisson_rows(self, rows, base, phi=1.0, apply_filter=False, weighting=True, want_extra=True):
        assert self._feat_bound and self._post_bound and base == self.base and phi == self.phi and weighting and want_extra
        ts, sc = self._rows(rows)
        return (*self._stack("poisson_rows", ts, ("result", "change", "next", "extra"), (1, 1, 1, 1)), sc)

    def poisson_rows_errors(self, rows, base, phi=1.0, apply_filter=False):
        assert self._feat_bound and self._post_bound and base == self.base and phi == self.phi
        ts, sc = self._rows(rows)
        return self._stack("poisson_rows_errors", ts, ("raw",), (1,))[0], sc

    def gradp_frames(self, cols, out_scale=None, apply_filter=False, want_gradp=True, want_p=True, want_truth=True):
        assert self._gradp_bound and out_scale is None
        ts, _ = self._host(cols)
        return tuple(self._stack("gradp_frames", ts, ("gradp", "p", "truth", "raw"), (want_gradp, want_p, want_truth, True)))

    def gradp_rows(self, rows, ex, ey, apply_filter=False, want_gradp=True, want_p=True, want_truth=True):
        assert self._gradp_bound and isinstance(ex, float) and isinstance(ey, float) and (ex, ey) == self.exy
        ts, sc = self._rows(rows)
        return (*self._stack("gradp_rows", ts, ("gradp", "p", "truth", "raw"), (want_gradp, want_p, want_truth, True)), sc)


def primed(kind, ds, path=None):
    """The evaluator of the fixture's files with what computeOnlyOnce leaves on it set by hand (a small SDF plane with a solid
    rectangle across the gradP cut's row and a NaN) and the stand-in in the place of its surrogate."""
    ev = {"deltas": tdf.evaluator, "poisson": tpf.evaluator, "gradp": tgf.evaluator}[kind](ds, max_frames=MAX_FRAMES)
    if path is not None:
        ev.dataset_path = path
    ny, nx = SHAPE[kind]
    sdf = np.ones((ny, nx))
    sdf[ny - 8:ny - 2, 3:7] = 0.0
    sdf[0, 1] = np.nan
    ev.indice, ev.grid_shape_y, ev.grid_shape_x, ev.sdfunct, ev.tables = ds["N"], ny, nx, sdf[:, :, None], object()
    frames = [formats.read_dataset(ev.dataset_path, 0, t)[0][0, 0, :ev.indice] for t in range(ds["sim"].shape[1])]
    with np.errstate(all="ignore"):
        if kind == "gradp":
            ev.min_x, ev.max_x, ev.min_y, ev.max_y = np.float32(-0.25), np.float32(1.2), np.float32(-0.3), np.float32(0.33)
            ev.X0_min = -0.25
            ex, ey = ev.max_x - ev.min_x, ev.max_y - ev.min_y
            ev._sur = StandIn(kind, frames, lambda d: tfr.host_gradp(d, ex, ey), None, exy=(float(ex), float(ey)))
        elif kind == "poisson":
            ev._sur = StandIn(kind, frames, lambda d: tfr.host_poisson(d, ev.max_abs_delta_p), ev.max_abs_delta_p, phi=tfr.PHI)
        else:
            ev._sur = StandIn(kind, frames, lambda d: tfr.host_deltas(d, float(ev.maxs[3])), float(ev.maxs[3]))
    return ev


ATTRS = ("cfd_results", "no_flow_bool", "deltap_res", "p_pred", "gradP", "max_abs_p", "center_p_x", "center_p_y", "frame_metrics")


def sweep(kind, ev, times, fields, device_prep):
    kw = {"phi": tfr.PHI} if kind == "poisson" else {}
    n0 = len(ev._sur.sent)
    got = tfr.run(kind, ev, times, fields, device_prep, **kw)
    keep = lambda v: np.array(v, copy=True) if isinstance(v, np.ndarray) else [dict(m) for m in v] if isinstance(v, list) else v
    got["attrs"] = {name: keep(getattr(ev, name)) for name in ATTRS if hasattr(ev, name)}
    got["attrs"]["no_flow_bool"] = got["attrs"]["no_flow_bool"].astype(np.float32)      # `equal` compares float arrays by their bits
    got["sent"] = ev._sur.sent[n0:]
    return got


def check(kind, ev, times, relevant, all_irrelevant):
    n_rel = sum(relevant)
    chunks = lambda n: [MAX_FRAMES] * (n // MAX_FRAMES) + ([n % MAX_FRAMES] if n % MAX_FRAMES else [])
    assert len(times) % MAX_FRAMES and 0 < n_rel                        # a shorter last call
    for fields in (False, True):
        off = sweep(kind, ev, times, fields, False)
        on = sweep(kind, ev, times, fields, True)
        tfr.compare(off, on, f"{kind} fields={fields}")
        assert [not isinstance(o, int) for o in on["out"]] == relevant and all(o == 0 for o, r in zip(on["out"], relevant) if not r)
        assert equal(off["labels"], on["labels"]) and equal(off["attrs"], on["attrs"]), (off["attrs"].keys(), on["attrs"].keys())
        assert [n for _, n in off["sent"]] == chunks(n_rel) and [n for _, n in on["sent"]] == chunks(len(times))
        assert all(len(v) in (0, n_rel) for v in on["lists"].values()) and len(on["lists"]["pred_minus_true"]) == n_rel
        if kind == "gradp":
            assert len(on["attrs"]["frame_metrics"]) == n_rel and set(on["last"]) == {"reference", "p", "dp_dx", "dp_dy"}
        if kind == "poisson" and fields:
            assert [p is not None for p in on["labels"]] == relevant
        for device_prep in (False, True):
            before = {name: len(getattr(ev, name, None) or []) for name in tfr.LISTS}
            kw = {"phi": tfr.PHI} if kind == "poisson" else {}
            assert ev.timeSteps(0, all_irrelevant, fields=fields, device_prep=device_prep, **kw) == [0] * len(all_irrelevant)
            assert before == {name: len(getattr(ev, name, None) or []) for name in tfr.LISTS}


def test_deltas_bookkeeping_is_the_same_with_device_prep_on_and_off(ds_deltas):
    ev = primed("deltas", ds_deltas, tfr.still_dataset(ds_deltas, "still_bookkeeping.hdf5"))
    check("deltas", ev, TIMES["deltas"], [t != STILL for t in TIMES["deltas"]], [STILL, STILL, STILL])


def test_poisson_bookkeeping_is_the_same_with_device_prep_on_and_off(ds_poisson):
    ev = primed("poisson", ds_poisson, tfr.still_dataset(ds_poisson, "still_bookkeeping.hdf5"))
    check("poisson", ev, TIMES["poisson"], [t != STILL for t in TIMES["poisson"]], [STILL, STILL, STILL])


def test_gradp_bookkeeping_is_the_same_with_device_prep_on_and_off(ds_gradp):
    """No skip rule: every frame is relevant, and the all-irrelevant call is the empty one."""
    ev = primed("gradp", ds_gradp)
    check("gradp", ev, TIMES["gradp"], [True] * len(TIMES["gradp"]), [])
