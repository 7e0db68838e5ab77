"""Solver boundary for a case batch (psm_set_geometry_cases / psm_init_geometry_cases / psm_solve_cases*): K meshes with their
own obstacles on one handle, advanced by one call.  Host side without a GPU (header, exports, the table builder under
ASan / UBSan, the example builds); on the GPU every case against the NumPy oracle's ``py_func_mesh`` on the same tables, one
case against ``psm_solve`` bit for bit, the isolation of the cases from each other, the other entries, the errors, the Python
mirror and the C++ example.

Four meshes of the 1.5 x 0.7 channel with different obstacles: all give a 138 x 300 grid, with 16 021 / 16 165 / 15 838 /
16 222 cells and 874 / 510 / 1326 / 378 solid pixels, so a mixed-up offset, table or U_max cannot pass."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess
import warnings

import numpy as np
import pytest

import cases
from oracle import psm_oracle as orc
from psm_amd import GridSurrogate, SolverEnsemble, _lib, geometry, synthetic
from test_oracle_golden import oracle_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.dirname(_lib.LIB_PATH)
CSRC = os.path.join(PKG, "csrc")
SYMBOLS = ("psm_set_geometry_cases", "psm_init_geometry_cases", "psm_solve_cases_device", "psm_solve_cases",
           "psm_solve_cases_begin", "psm_solve_cases_end", "psm_mesh_cases")
OBSTACLES = (dict(), dict(cx=0.55, cy=0.05, R=0.06), dict(cx=0.9, cy=-0.08, R=0.1, step=2), dict(cx=0.3, cy=0.1, R=0.05, step=1))
SHAPE, CELLS, SOLID = (138, 300), (16021, 16165, 15838, 16222), (874, 510, 1326, 378)
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)


# ---- shared inputs and references (built once, never modified) ---------------------------------------------------------
class Ensemble:
    def __init__(self):
        _, _, _, self.model, self.maxs = cases.build_mesh_case()
        self.om = oracle_model(self.model)
        self.mesh = [synthetic.channel_mesh(**kw) for kw in OBSTACLES]                     # (array, top, obst) per case
        # a second time step: other fields on the same cells
        self.step2 = [synthetic.channel_mesh(**dict(kw, step=kw.get("step", 0) + 3))[0] for kw in OBSTACLES]
        self.tabs = [geometry.build_geometry_native(a, t, o) for a, t, o in self.mesh]
        self.geo = [orc.Geometry(g.ny, g.nx, g.vtx_m2g, g.wts_m2g, g.vtx_g2m, g.wts_g2m, g.indices, g.sdfunct) for g in self.tabs]
        self._ref = {}

    def array(self, k, step=0):
        return self.step2[k] if step else self.mesh[k][0]

    def ref(self, k, step=0):
        """The oracle's py_func on case k's tables (computed once per (case, step))."""
        if (k, step) not in self._ref:
            self._ref[(k, step)] = orc.py_func_mesh(self.array(k, step), self.geo[k], self.om, self.maxs)[0]
        return self._ref[(k, step)]


@pytest.fixture(scope="module")
def ens():
    return Ensemble()


def _ptrs(arrays):
    return (C.c_void_p * len(arrays))(*[None if a is None else a.ctypes.data for a in arrays])


def set_cases(sur, tabs, n_cells, maxs, drop_g2m_of=None):
    """psm_set_geometry_cases with the tables of ``tabs`` -> (status, message)."""
    cols = [[np.ascontiguousarray(getattr(g, f), dt) for g in tabs]
            for f, dt in (("vtx_m2g", np.int32), ("wts_m2g", np.float64), ("indices", np.int32), ("sdfunct", np.float64),
                          ("vtx_g2m", np.int32), ("wts_g2m", np.float64))]
    if drop_g2m_of is not None:
        cols[4][drop_g2m_of] = cols[5][drop_g2m_of] = None
    mx = np.asarray(maxs, np.float64)
    rc = sur.lib.psm_set_geometry_cases(sur.h, len(tabs), (C.c_int64 * len(tabs))(*n_cells), tabs[0].ny, tabs[0].nx,
                                        *[_ptrs(c) for c in cols], mx.ctypes.data_as(_dp), 0, 0, 0.05)
    return rc, _lib.last_error(sur.h)


def case_set(ens, order, max_cases=4):
    sur = GridSurrogate(ens.model, *SHAPE, max_cases)
    rc, msg = set_cases(sur, [ens.tabs[k] for k in order], [CELLS[k] for k in order], ens.maxs)
    assert rc == 0, msg
    return sur


def pack(ens, order, step=0):
    return np.ascontiguousarray(np.concatenate([ens.array(k, step) for k in order]), np.float64)


def solve_cases(sur, cells, entry="psm_solve_cases"):
    p = np.full(cells.shape[0], -7.0)
    rc = getattr(sur.lib, entry)(sur.h, cells.ctypes.data_as(_dp), p.ctypes.data_as(_dp))
    assert rc == 0, _lib.last_error(sur.h)
    return p


def split(p, order):
    off = np.concatenate([[0], np.cumsum([CELLS[k] for k in order])])
    return [p[off[i]:off[i + 1]] for i in range(len(order))]


def check_against_oracle(p, array, ref):
    kept = ref == array[:, 4]                               # near-wall / negative-weight cells keep the previous p
    assert 0 < kept.sum() < len(ref)
    np.testing.assert_array_equal(p[kept], array[kept, 4])
    err, bound = np.abs(p - ref).max(), 2e-4 * np.abs(ref).max()
    print(f"max|p - ref| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound


# ---- without a GPU ------------------------------------------------------------------------------------------------------
def test_the_four_meshes_share_a_grid_and_differ_in_everything_else(ens):
    assert [(g.ny, g.nx) for g in ens.tabs] == [SHAPE] * 4
    assert tuple(len(m[0]) for m in ens.mesh) == CELLS
    assert tuple(int((g.sdfunct == 0).sum()) for g in ens.tabs) == SOLID
    assert len(orc.block_layout("chapter5", *SHAPE).tags) >= 4


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_header_compiles_as_c99_with_the_case_entries(tmp_path):
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                        os.path.join(ROOT, "tests", "native", "abi_c_check_cases.c"), "-o", str(tmp_path / "a.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_library_exports_the_case_entries():
    lib = _lib.load()
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.psm_abi_version() == 4                       # functions were added, nothing changed


def test_null_handle_is_refused():
    lib = _lib.load()
    assert lib.psm_mesh_cases(None, None, None) == -1
    n = (C.c_int64 * 1)(10)
    none = _ptrs([None])
    assert lib.psm_set_geometry_cases(None, 1, n, 4, 4, none, none, none, none, none, none, None, 0, 0, 0.05) == -1


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_case_tables_are_clean_under_asan_ubsan(tmp_path):
    """Validation, offsets and derived tables of psm_set_geometry_cases and of the single mesh of psm_set_geometry, with and
    without its grid->mesh tables (csrc/psm_mesh_tables.cpp: no device needed), in a stand-alone program under AddressSanitizer + UBSan."""
    exe = str(tmp_path / "mesh_cases_sanitized")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                        os.path.join(ROOT, "tests", "native", "mesh_cases_sanitized.cpp"), os.path.join(CSRC, "psm_mesh_tables.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "case sets built: 60, refused: 60, single meshes: 20" in r.stdout


def _build_example(out):
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "ensemble_batched_host.cpp"),
           "-L", PKG, "-lpsm_hip", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-o", out]
    return subprocess.run(cmd, capture_output=True, text=True)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_batched_example_builds_against_the_c_abi(tmp_path):
    r = _build_example(str(tmp_path / "ensemble_batched_host"))
    assert r.returncode == 0, r.stderr[-2000:]


# ---- on the GPU ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_three_cases_one_call_match_the_oracle_for_two_steps(ens):
    order = (0, 1, 2)
    with case_set(ens, order) as sur:
        assert sur.geometry_bound                           # the K geometries are bound for this entry
        n, off = C.c_int32(), (C.c_int64 * 4)()
        assert sur.lib.psm_mesh_cases(sur.h, C.byref(n), off) == 0
        assert n.value == 3 and list(off) == [0, 16021, 32186, 48024]
        for step in (0, 1):                                 # the second step: new fields through the same handle
            for k, p in zip(order, split(solve_cases(sur, pack(ens, order, step)), order)):
                check_against_oracle(p, ens.array(k, step), ens.ref(k, step))


@pytest.mark.gpu
def test_a_case_does_not_care_about_its_slot_or_its_neighbours(ens):
    """The same cases submitted in another order (and with another neighbour) on a fresh handle: every case within the bound
    path's float32 summation-order bound of the first run."""
    first, second = (0, 1, 2), (2, 3, 1)
    with case_set(ens, first) as sur:
        a = dict(zip(first, split(solve_cases(sur, pack(ens, first)), first)))
    with case_set(ens, second) as sur:
        b = dict(zip(second, split(solve_cases(sur, pack(ens, second)), second)))
    check_against_oracle(b[3], ens.array(3), ens.ref(3))
    for k in (1, 2):
        err, bound = np.abs(a[k] - b[k]).max(), 2e-5 * np.abs(a[k]).max()
        print(f"case {k}: max|p - p'| = {err:.3e}, bound {bound:.3e}")
        assert err <= bound


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 2])
def test_one_case_is_psm_solve_bit_for_bit(ens, k):
    """psm_solve_cases with one case against psm_solve on a handle given the same tables, at the seven velocity scales of
    tests/test_embed_host.py: a U_max one ulp off changes every pressure of the step."""
    g, n = ens.tabs[k], CELLS[k]
    mx = np.asarray(ens.maxs, np.float64)
    with GridSurrogate(ens.model, *SHAPE, 1) as one, case_set(ens, (k,), max_cases=4) as sur:
        v1, w1 = np.ascontiguousarray(g.vtx_m2g, np.int32), np.ascontiguousarray(g.wts_m2g, np.float64)
        v2, w2 = np.ascontiguousarray(g.vtx_g2m, np.int32), np.ascontiguousarray(g.wts_g2m, np.float64)
        idx, sdf = np.ascontiguousarray(g.indices, np.int32), np.ascontiguousarray(g.sdfunct, np.float64)
        one._chk(one.lib.psm_set_geometry(one.h, n, g.ny, g.nx, v1.ctypes.data_as(_ip), w1.ctypes.data_as(_dp), idx.ctypes.data_as(_ip),
                                          sdf.ctypes.data_as(_dp), v2.ctypes.data_as(_ip), w2.ctypes.data_as(_dp), mx.ctypes.data_as(_dp), 0, 0, 0.05))
        assert one.geometry_bound and sur.geometry_bound
        for s in range(7):
            cells = np.ascontiguousarray(ens.array(k), np.float64).copy()
            cells[:, :2] *= 1.0 + 0.01 * s
            ref = np.empty(n)
            one._chk(one.lib.psm_solve(one.h, cells.ctypes.data_as(_dp), n, 0, ref.ctypes.data_as(_dp)))
            got = solve_cases(sur, cells)
            assert np.isfinite(ref).all()
            np.testing.assert_array_equal(got, ref)


@pytest.mark.gpu
def test_a_nan_velocity_stays_in_its_case(ens):
    """One NaN velocity in case 1: its U_max is NaN like np.max's, so (as the oracle computes it) the image is zero and every
    cell that does not keep its previous p is NaN; cases 0 and 2 are bit for bit what they were."""
    order = (0, 1, 2)
    cells = pack(ens, order)
    bad = cells.copy()
    bad[CELLS[0] + 1234, 0] = np.nan
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref = orc.py_func_mesh(bad[CELLS[0]:CELLS[0] + CELLS[1]], ens.geo[1], ens.om, ens.maxs)[0]
    kept = ~np.isnan(ref)
    assert 0 < kept.sum() < len(ref) and (ref[kept] == ens.array(1)[kept, 4]).all()        # what the oracle gives
    with case_set(ens, order) as sur:
        clean = split(solve_cases(sur, cells), order)
        got = split(solve_cases(sur, bad), order)
    np.testing.assert_array_equal(np.isnan(got[1]), np.isnan(ref))
    np.testing.assert_array_equal(got[1][kept], ref[kept])
    np.testing.assert_array_equal(got[0], clean[0])
    np.testing.assert_array_equal(got[2], clean[2])
    assert np.isfinite(clean[1]).all()


@pytest.mark.gpu
def test_begin_end_and_the_device_entry_equal_the_synchronous_call(ens):
    import hipmem
    order = (3, 0, 1)
    cells = pack(ens, order)
    with case_set(ens, order) as sur:
        ref = solve_cases(sur, cells)
        p = np.full(len(cells), -7.0)
        assert sur.lib.psm_solve_cases_begin(sur.h, cells.ctypes.data_as(_dp), p.ctypes.data_as(_dp)) == 0
        assert sur.lib.psm_solve_cases_end(sur.h) == 0
        np.testing.assert_array_equal(p, ref)
        d_cells, d_p = hipmem.DeviceArray(cells), hipmem.DeviceArray(shape=(len(cells),), dtype=np.float64)
        assert sur.lib.psm_solve_cases_device(sur.h, d_cells.ptr, d_p.ptr, None) == 0, _lib.last_error(sur.h)
        sur.synchronize()
        np.testing.assert_array_equal(d_p.numpy(), ref)
        d_cells.free(); d_p.free()
        # caller arrays registered with psm_host_register: the two copies go straight from / into them
        out = np.full(len(cells), -7.0)
        sur.host_register(cells); sur.host_register(out)
        assert sur.lib.psm_solve_cases(sur.h, cells.ctypes.data_as(_dp), out.ctypes.data_as(_dp)) == 0
        sur.host_unregister(cells); sur.host_unregister(out)
        np.testing.assert_array_equal(out, ref)


@pytest.mark.gpu
def test_general_path_gives_the_same_pressures(ens, monkeypatch):
    order = (0, 1, 2)
    cells = pack(ens, order)
    with case_set(ens, order) as sur:
        bound = solve_cases(sur, cells)
    monkeypatch.setenv("PSM_NO_BIND", "1")
    with case_set(ens, order) as sur:
        assert not sur.geometry_bound
        general = solve_cases(sur, cells)
    for b, g in zip(split(bound, order), split(general, order)):
        err, lim = np.abs(b - g).max(), 2e-5 * np.abs(g).max()
        print(f"max|bound - general| = {err:.3e}, bound {lim:.3e}")
        assert err <= lim


@pytest.mark.gpu
def test_errors_are_reported_and_leave_the_handle_usable(ens):
    order = (0, 1)
    cells = pack(ens, order)
    dp = lambda a: a.ctypes.data_as(_dp)
    with case_set(ens, order, max_cases=2) as sur:
        lib, h = sur.lib, sur.h
        ref = solve_cases(sur, cells)
        p = np.empty(len(cells))
        # more cases than max_cases; a missing grid -> mesh table: refused before the handle is touched
        rc, msg = set_cases(sur, ens.tabs[:3], CELLS[:3], ens.maxs)
        assert rc == -1 and "max_cases" in msg
        rc, msg = set_cases(sur, ens.tabs[:2], CELLS[:2], ens.maxs, drop_g2m_of=1)
        assert rc == -1 and "case 1" in msg and "grid->mesh" in msg
        np.testing.assert_array_equal(solve_cases(sur, cells), ref)
        # a case of another grid shape through psm_init_geometry_cases
        wide = synthetic.channel_mesh(Lx=1.6)
        m = [ens.mesh[0], wide]
        a, t, o = ([np.ascontiguousarray(x[i], np.float64) for x in m] for i in range(3))
        cnt = lambda arrs: (C.c_int64 * 2)(*[len(x) for x in arrs])
        rc = lib.psm_init_geometry_cases(h, 2, _ptrs(a), cnt(a), _ptrs(t), cnt(t), _ptrs(o), cnt(o))
        assert rc == -1 and "case 1" in _lib.last_error(h) and "grid shape" in _lib.last_error(h)
        np.testing.assert_array_equal(solve_cases(sur, cells), ref)
        # psm_solve on a case set
        assert lib.psm_solve(h, dp(cells), CELLS[0], 0, dp(p)) == -2 and "case set" in _lib.last_error(h)
        # one step in flight
        assert lib.psm_solve_cases_end(h) == -2 and "in flight" in _lib.last_error(h)
        assert lib.psm_solve_cases_begin(h, dp(cells), dp(p)) == 0
        assert lib.psm_solve_cases_begin(h, dp(cells), dp(p)) == -2 and "in flight" in _lib.last_error(h)
        assert lib.psm_solve_cases_end(h) == 0
        np.testing.assert_array_equal(p, ref)
        # a new plan drops the case set; setting it again restores the path
        assert lib.psm_plan_grid(h, *SHAPE) == 0
        assert lib.psm_solve_cases(h, dp(cells), dp(p)) == -2 and "psm_set_geometry_cases" in _lib.last_error(h)
        assert lib.psm_mesh_cases(h, None, None) == -2
        rc, msg = set_cases(sur, ens.tabs[:2], CELLS[:2], ens.maxs)
        assert rc == 0, msg
        np.testing.assert_array_equal(solve_cases(sur, cells), ref)
        # the single mesh of psm_set_geometry takes the case set's place: psm_solve_cases* is refused, psm_solve works
        g = ens.tabs[0]
        cols = [np.ascontiguousarray(getattr(g, f), dt) for f, dt in (("vtx_m2g", np.int32), ("wts_m2g", np.float64), ("indices", np.int32),
                                                                      ("sdfunct", np.float64), ("vtx_g2m", np.int32), ("wts_g2m", np.float64))]
        mx = np.asarray(ens.maxs, np.float64)
        sur._chk(lib.psm_set_geometry(h, CELLS[0], g.ny, g.nx, cols[0].ctypes.data_as(_ip), dp(cols[1]), cols[2].ctypes.data_as(_ip), dp(cols[3]),
                                      cols[4].ctypes.data_as(_ip), dp(cols[5]), dp(mx), 0, 0, 0.05))
        assert lib.psm_solve_cases(h, dp(cells), dp(p)) == -2 and "single mesh" in _lib.last_error(h)
        one = np.empty(CELLS[0])
        assert lib.psm_solve(h, dp(np.ascontiguousarray(ens.array(0))), CELLS[0], 0, dp(one)) == 0
        check_against_oracle(one, ens.array(0), ens.ref(0))


def _checksum(p):
    return int(np.ascontiguousarray(p).view(np.uint64).sum(dtype=np.uint64))


@pytest.mark.gpu
def test_solver_ensemble_and_the_cpp_example(ens, tmp_path):
    """SolverEnsemble('native') (psm_init_geometry_cases) reproduces the C-ABI results on the natively built tables bit for
    bit; examples/ensemble_batched_host.cpp, three cases for two steps, prints the checksums of the same pressures."""
    order = (0, 1, 2)
    se = SolverEnsemble(ens.model, ens.maxs, 4, geometry="native")
    assert se.init_func(*zip(*[ens.mesh[k] for k in order])) == 0
    assert se.cell_off == [0, 16021, 32186, 48024]
    got = [se.py_func([ens.array(k, step) for k in order]) for step in (0, 1)]
    se.py_func_begin([ens.array(k) for k in order])
    for a, b in zip(se.py_func_end(), got[0]):
        np.testing.assert_array_equal(a, b)
    with case_set(ens, order) as sur:
        for step in (0, 1):
            for a, b in zip(split(solve_cases(sur, pack(ens, order, step)), order), got[step]):
                np.testing.assert_array_equal(a, b)
    se._sur.close()

    exe = str(tmp_path / "ensemble_batched_host")
    r = _build_example(exe)
    assert r.returncode == 0, r.stderr[-2000:]
    model = ens.model
    with open(tmp_path / "ensemble.bin", "wb") as f:
        f.write(struct.pack("<5i", model.p_in, model.p_out, len(model.weights), len(order), 2))
        for a in (model.comp_in, model.mean_in, model.comp_out, model.mean_out, np.array([model.in_a, model.out_a]), np.array(ens.maxs)):
            f.write(np.ascontiguousarray(a, "<f8").tobytes())
        for W, b in model.weights:
            f.write(struct.pack("<2i", *W.shape))
            f.write(np.ascontiguousarray(W, "<f4").tobytes()); f.write(np.ascontiguousarray(b, "<f4").tobytes())
        for k in order:
            a, t, o = ens.mesh[k]
            f.write(struct.pack("<3i", len(a), len(t), len(o)))
            for x in (t, o, a, ens.array(k, 1)):
                f.write(np.ascontiguousarray(x, "<f8").tobytes())
    run = subprocess.run([exe, str(tmp_path / "ensemble.bin")], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout, run.stderr)
    sums = {(int(s), int(c)): int(x, 16) for s, c, x in re.findall(r"step (\d+) case (\d+) cells \d+ checksum ([0-9a-f]{16})", run.stdout)}
    assert sums == {(step, i): _checksum(got[step][i]) for step in (0, 1) for i in range(3)}


@pytest.mark.gpu
def test_solver_ensemble_checks_its_input(ens):
    """The argument checks of the Python mirror."""
    se = SolverEnsemble(ens.model, ens.maxs, 2, geometry="native")
    with pytest.raises(RuntimeError):
        se.py_func([ens.array(0)])
    with pytest.raises(ValueError):
        se.init_func(*zip(*[ens.mesh[k] for k in (0, 1, 2)]))           # more than max_cases
    se.init_func(*zip(*[ens.mesh[k] for k in (0, 1)]))
    with pytest.raises(ValueError):
        se.py_func([ens.array(0)])                                       # one array per case
    with pytest.raises(ValueError):
        se.py_func([ens.array(1), ens.array(0)])                         # cell counts of init_func
    with pytest.raises(ValueError):
        SolverEnsemble(ens.model, ens.maxs, 2, geometry="qhull")
    se._sur.close()
