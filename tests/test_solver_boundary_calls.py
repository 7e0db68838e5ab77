"""What ``SolverModule`` and ``SolverEnsemble`` ask of the library and of ``GridSurrogate``, without a device: every C entry with its
scalar arguments, every ``GridSurrogate`` construction, ``close`` and ``bind_*`` call, what each method returned and, for a refused
call, the exception's type and full message -- both classes x the four steps x both geometries, then the refusals.

``tests/golden/solver_boundary_calls.txt`` was recorded once, with this file run as a script, from the ``solver.py`` that held the two
classes as two hand-kept copies with a ladder of step names in every method; it is never regenerated from later code.  The three
refusals of a bad ``out`` under step='absolute' were then edited by hand to the message the other three steps give: that step used
to hand such an ``out`` to the library unchecked.

The stand-ins (tests/test_evaluator_bookkeeping.py's ``StandIn`` is the precedent): ``solver.GridSurrogate`` and ``_lib.load`` are
replaced by recorders whose entries return 0, fill ``psm_geometry_shape``'s and the state entries' ``byref`` outputs, the sdfunct of
``psm_geometry_build`` and the offsets of ``psm_mesh_cases``, and read the four ``maxs`` of ``psm_set_geometry`` /
``psm_set_geometry_cases`` / ``psm_set_case`` back as values; ``geometry.build_geometry`` returns a small table object (the call
sequence is what is recorded, not qhull).  A record line: ``> call`` opens a method call, the indented lines are what it asked
for, ``= ...`` is what it returned and ``! Type: message`` how it was refused."""
import ctypes as C
import importlib
import os
import sys

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "solver_boundary_calls.txt")
NY, NX = 5, 6
MAXS_AT = {"psm_set_geometry": 10, "psm_set_geometry_cases": 11, "psm_set_case": 1}      # the argument that points at the four maxs
STATE = {"psm_delta_state": (1, 3), "psm_poisson_solve_state": (2, 5)}
STEPS = ("absolute", "delta", "poisson", "gradp")
MAXS = {"absolute": (1.5, 2.5, 0.5, 4.0), "delta": (1.5, 2.5, 0.5, 4.0), "poisson": (7.0, 1.5, 2.5, 0.5, 4.0), "gradp": (1.5, 2.5, 0.5, 3.0, 6.0)}
KW = {"absolute": {}, "delta": {}, "poisson": dict(phi=0.1, k=2.0, weighting=False, sigma_field=(3, 4)),
      "gradp": dict(apply_filter=True, sigma_weight=(5, 6), reference="none")}


def sdf_plane(nx=NX):
    sd = np.ones((NY, nx))
    sd[2, 2:4] = 0.0                                                   # a solid stretch off the rim: gradp_default_cut finds its row
    return sd.reshape(-1)


def fmt(v):
    if v is None or isinstance(v, (bool, str)):
        return str(v)
    if isinstance(v, (int, np.integer)):
        return str(int(v))
    if isinstance(v, (float, np.floating)):
        return repr(float(v))
    if isinstance(v, np.ndarray):
        return {"float64": "f64", "float32": "f32", "int32": "i32", "int64": "i64"}.get(v.dtype.name, v.dtype.name) + str(list(v.shape)).replace(" ", "")
    if isinstance(v, C.Array):
        return "*x%d" % len(v) if v._type_ is C.c_void_p else str([int(x) for x in v])
    if isinstance(v, (tuple, list)):
        return "(" + ", ".join(fmt(x) for x in v) + ")"
    if isinstance(v, (C._Pointer, C._SimpleCData)) or type(v).__name__ == "CArgObject":
        return "*"
    return type(v).__name__


class Lib:
    """The library: every entry is recorded and returns 0."""

    def __init__(self, log):
        self.log, self.case_cells = log, []

    def __getattr__(self, name):
        if not name.startswith("psm_"):
            raise AttributeError(name)

        def entry(*args):
            shown = [fmt(a) for a in args]
            if name in MAXS_AT:
                shown[MAXS_AT[name]] = fmt([args[MAXS_AT[name]][i] for i in range(4)])
            self.log.append("    " + name + "(" + ", ".join(shown) + ")")
            if name == "psm_geometry_shape":
                args[3]._obj.value, args[4]._obj.value = NY, NX
            elif name == "psm_geometry_build":
                np.ctypeslib.as_array(args[11], (NY * NX,))[:] = sdf_plane()
            elif name in ("psm_set_geometry_cases", "psm_init_geometry_cases"):
                self.case_cells = [int(x) for x in args[2 if name == "psm_set_geometry_cases" else 3]]
            elif name == "psm_mesh_cases":
                if args[1] is not None:
                    args[1]._obj.value = len(self.case_cells)
                if args[2] is not None:
                    args[2][0] = 0
                    for k, n in enumerate(self.case_cells):
                        args[2][k + 1] = args[2][k] + n
            elif name in STATE:
                args[1]._obj.value, args[2]._obj.value = STATE[name]
            return 0
        return entry


def surrogate_class(log, lib, real):
    """``GridSurrogate``: the construction, ``close`` and every ``bind_*`` are recorded; the handle is a name."""
    count = [0]

    class Surrogate:
        GRADP_REFERENCES = real.GRADP_REFERENCES

        def __init__(self, model, ny, nx, max_cases=1, device=0):
            count[0] += 1
            self.lib, self.h, self.ny, self.nx, self.max_cases = lib, "h%d" % count[0], int(ny), int(nx), int(max_cases)
            log.append("    GridSurrogate(%s) -> %s" % (", ".join(fmt(a) for a in (model, ny, nx, max_cases, device)), self.h))

        def _chk(self, rc):
            return rc

        def close(self):
            log.append("    %s.close()" % self.h)

        def __getattr__(self, name):
            if not name.startswith("bind_"):
                raise AttributeError(name)
            return lambda *a, **kw: log.append("    %s.%s(%s)" % (self.h, name, ", ".join([fmt(x) for x in a] + ["%s=%s" % (k, fmt(v)) for k, v in kw.items()])))
    return Surrogate


def build_geometry_standin(log):
    class Tables:
        pass

    def build_geometry(array, top, obst, delta):
        log.append("    build_geometry(%s)" % ", ".join(fmt(a) for a in (array, top, obst, delta)))
        t, n = Tables(), array.shape[0]
        t.ny, t.nx = NY, NX if n < 9 else NX + 1                       # nine cells or more: another grid shape
        ng = t.ny * t.nx
        t.vtx_m2g, t.wts_m2g, t.indices = np.zeros((ng, 3), np.int64), np.full((ng, 3), 1 / 3), np.zeros((ng, 2), np.int64)
        t.vtx_g2m, t.wts_g2m, t.sdfunct = np.zeros((n, 3), np.int64), np.full((n, 3), 1 / 3), sdf_plane(t.nx)
        return t
    return build_geometry


def cells(n, seed):
    a = np.random.default_rng(seed).standard_normal((n, 5))
    a[:, 2] = np.linspace(-0.25, 1.25, n)                               # Cx, Cy: the bounds gradp_grid_metrics reads
    a[:, 3] = np.linspace(-0.3, 0.35, n)
    return a


def returned(r, out=None):
    if out is not None and r is out:
        return "is out"
    if isinstance(r, list):
        return "%d pieces of %s" % (len(r), fmt([len(p) for p in r]))
    if isinstance(r, tuple):
        return repr(r)
    return fmt(r)


class Recorder:
    def __init__(self, solver):
        self.solver, self.log = solver, []

    def call(self, label, fn, out=None):
        self.log.append("> " + label)
        try:
            r = fn()
        except Exception as e:                                          # the refusal is the record
            text = str(e)
            if isinstance(e, AttributeError) and text.startswith("'NoneType' object has no attribute"):
                text = "'NoneType' object has no attribute ..."        # no refusal of its own: which attribute of the missing handle is read first is not held
            self.log.append("! %s: %s" % (type(e).__name__, text))
            return False
        self.log.append("= " + returned(r, out))
        return True

    def attrs(self, m):
        names = ("step", "maxs", "tables", "cell_off", "cut_used", "cuts_used")
        shown = ["%s=%s" % (n, fmt(getattr(m, n)) if n != "tables" else ("native" if m.tables == "native" else "scipy")) for n in names if hasattr(m, n)]
        self.log.append("  attrs " + " ".join(shown))

    def make(self, cls, step_, geometry_, **over):
        kw = dict(maxs=MAXS[step_], geometry=geometry_, step=step_, **KW[step_])
        if cls == "SolverEnsemble":
            kw["max_cases"] = 3
        kw.update(over)
        return getattr(self.solver, cls)("model", **kw)

    def scenario(self, cls, step, geometry):
        call, ens = self.call, cls == "SolverEnsemble"
        self.log.append("== %s step=%s geometry=%s" % (cls, step, geometry))
        made = []
        if not call("construct", lambda: made.append(self.make(cls, step, geometry)) or "made"):
            return
        m = made[0]
        top, obst = np.zeros((3, 2)), np.ones((4, 2))
        if ens:
            a, b = [cells(6, 1), cells(7, 2)], [cells(6, 3), cells(7, 4)]
            init = lambda: m.init_func(a, [top, top], [obst, obst])
        else:
            a, b = cells(6, 1), cells(6, 3)
            init = lambda: m.init_func(a, top, obst)
        call("init_func", init)
        self.attrs(m)
        call("init_func again", init)
        call("prime", lambda: m.prime(b))
        call("state", lambda: m.state)
        call("reset_state", lambda: m.reset_state())
        call("py_func", lambda: m.py_func(b))
        if ens:
            if call("py_func_begin", lambda: m.py_func_begin(b)):
                call("py_func_end", lambda: m.py_func_end())
        else:
            out = np.empty(6)
            call("py_func out", lambda: m.py_func(b, 0, out), out)
            call("py_func placeholder", lambda: m.py_func(b, 3))
            if call("py_func_begin", lambda: m.py_func_begin(b)):
                call("py_func_end", lambda: m.py_func_end())
            if call("py_func_begin out", lambda: m.py_func_begin(b, out)):
                call("py_func_end", lambda: m.py_func_end(), out)
            call("pin", lambda: m.pin(b, out))
            pinned = getattr(m, "_pinned", None)
            self.log.append("  pinned " + ("(array, out)" if pinned and pinned[0] is b and pinned[1] is out else "?"))
            call("unpin", lambda: m.unpin())
            call("pin strided", lambda: m.pin(b[:, ::2]))
        # -- the refusals behind init_func
        if ens:
            call("py_func [N,4]", lambda: m.py_func([b[0][:, :4], b[1]]))
            call("prime [N,4]", lambda: m.prime([b[0][:, :4], b[1]]))
            call("py_func_begin [N,4]", lambda: m.py_func_begin([b[0][:, :4], b[1]]))
            for label, bad in (("one case", b[:1]), ("three cases", b + b[:1]), ("a case of the wrong cell count", [b[1], b[0]])):
                call("py_func " + label, lambda: m.py_func(bad))
                call("prime " + label, lambda: m.prime(bad))
                call("py_func_begin " + label, lambda: m.py_func_begin(bad))
            call("init_func four cases", lambda: m.init_func(a + a, [top] * 4, [obst] * 4))
            call("init_func unequal lists", lambda: m.init_func(a, [top], [obst, obst]))
            call("init_func no case", lambda: m.init_func([], [], []))
        else:
            call("py_func [N,4]", lambda: m.py_func(b[:, :4]))
            call("prime [N,4]", lambda: m.prime(b[:, :4]))
            call("py_func_begin [N,4]", lambda: m.py_func_begin(b[:, :4]))
            for label, bad in (("float32 out", np.empty(6, np.float32)), ("short out", np.empty(5)), ("strided out", np.empty(12)[::2])):
                call("py_func " + label, lambda: m.py_func(b, 0, bad), bad)
                if call("py_func_begin " + label, lambda: m.py_func_begin(b, bad)):
                    call("py_func_end", lambda: m.py_func_end(), bad)

    def before_init(self, cls, step):
        self.log.append("== %s step=%s before init_func" % (cls, step))
        m = self.make(cls, step, "native")
        x = [cells(6, 1), cells(7, 2)] if cls == "SolverEnsemble" else cells(6, 1)
        self.call("prime", lambda: m.prime(x))
        self.call("state", lambda: m.state)
        self.call("reset_state", lambda: m.reset_state())
        self.call("py_func", lambda: m.py_func(x))
        self.call("py_func_begin", lambda: m.py_func_begin(x))
        self.call("py_func_end", lambda: m.py_func_end())
        if cls == "SolverModule":
            self.call("pin", lambda: m.pin(x))
            self.call("unpin", lambda: m.unpin())

    def constructor(self, cls):
        self.log.append("== %s constructor refusals" % cls)
        for label, step, over in (("bad step", "absolute", dict(step="relative")), ("bad geometry", "absolute", dict(geometry="qhull")),
                                  ("bad geometry and step", "absolute", dict(geometry="qhull", step="relative")),
                                  ("poisson four maxs", "poisson", dict(maxs=MAXS["absolute"])), ("gradp four maxs", "gradp", dict(maxs=MAXS["absolute"])),
                                  ("absolute five maxs", "absolute", dict(maxs=MAXS["gradp"])),
                                  ("poisson no phi", "poisson", dict(phi=None)), ("poisson no k", "poisson", dict(k=None)),
                                  ("gradp bad reference", "gradp", dict(reference="inlet")), ("gradp default reference", "gradp", dict(reference="outlet")),
                                  ("gradp a cut", "gradp", dict(cut=(2, 3) if cls == "SolverModule" else [(2, 3), (1, 2)], apply_filter=None))):
            made = []
            if self.call(label, lambda: made.append(self.make(cls, step, "native", **over)) or "made"):
                self.attrs(made[0])

    def given_cut(self, cls):
        """step='gradp' with the cut given and the filter left at its default: the bind without the post-steps."""
        self.log.append("== %s step=gradp, the cut given, apply_filter default" % cls)
        ens = cls == "SolverEnsemble"
        m = self.make(cls, "gradp", "scipy", cut=[(2, 3), (1, 2)] if ens else (2, 3), apply_filter=None, reference="outlet")
        top, obst = np.zeros((3, 2)), np.ones((4, 2))
        self.call("init_func", (lambda: m.init_func([cells(6, 1), cells(7, 2)], [top, top], [obst, obst])) if ens else (lambda: m.init_func(cells(6, 1), top, obst)))
        self.attrs(m)

    def run(self):
        solver = self.solver
        _lib, geometry = solver._lib, importlib.import_module(solver.__package__ + ".geometry")   # the modules this solver.py itself imports
        lib = Lib(self.log)
        saved = solver.GridSurrogate, _lib.load, geometry.build_geometry
        solver.GridSurrogate, _lib.load, geometry.build_geometry = surrogate_class(self.log, lib, saved[0]), (lambda: lib), build_geometry_standin(self.log)
        try:
            for cls in ("SolverModule", "SolverEnsemble"):
                for step in STEPS:
                    for geometry_kind in ("scipy", "native"):
                        self.scenario(cls, step, geometry_kind)
                for step in STEPS:
                    self.before_init(cls, step)
                self.constructor(cls)
                self.given_cut(cls)
            self.log.append("== SolverEnsemble scipy, cases of different grid shapes")
            top, obst = np.zeros((3, 2)), np.ones((4, 2))
            for step in STEPS:
                m = self.make("SolverEnsemble", step, "scipy")
                self.call("init_func " + step, lambda: m.init_func([cells(6, 1), cells(9, 2)], [top, top], [obst, obst]))
        finally:
            solver.GridSurrogate, _lib.load, geometry.build_geometry = saved
        return self.log


def record(solver=None):
    if solver is None:
        from psm_amd import solver
    return Recorder(solver).run()


def test_solver_boundary_calls_are_the_recorded_ones():
    with open(GOLDEN) as f:
        want = f.read().splitlines()
    got = record()
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "line %d differs:\n  recorded: %s\n  now:      %s\n  (in %s)" % (
            i + 1, w, g, next(l for l in reversed(want[:i + 1]) if l.startswith("==")))
    assert len(got) == len(want), "%d lines now, %d recorded; the first one beyond: %s" % (len(got), len(want), (got + want)[min(len(got), len(want))])


if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]
    sys.stdout.write("\n".join(record()) + "\n")
