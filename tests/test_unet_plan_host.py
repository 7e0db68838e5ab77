"""The conv path's planner (csrc/psm_unet_plan.cpp) against tests/golden/unet_plan_matrix.txt, the table of per-layer decision records
the planner produced while it still lived inside psm_unet_api.cpp: on the host under AddressSanitizer / UBSan (no device, a stand-alone
program), and once through the built library's psm_unet_plan_detail on the GPU (planning only, no forward pass)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "solving-poisson-s-equation-through-dl-for-cfd-apllications_amd", "csrc")
FIXTURE = os.path.join(ROOT, "tests", "golden", "unet_plan_matrix.txt")
# plan_detail field -> column of a fixture row (after `row NAME PRECISION LAYER`; the header of the fixture names them)
_COLUMNS = {"arrangement": 7, "nct": 8, "ksplit": 11, "kw": 12, "x6": 17, "pair": 18, "pair_kind": 19, "src": 25, "stem": 26,
            "in_bf": 15, "out_bf": 16, "fuse_head": 14, "km": 27, "one": 28}


def _fixture():
    """{name: (settings of the config line, {precision: [row columns per layer]})}"""
    configs = {}
    with open(FIXTURE) as f:
        for line in f:
            t = line.split()
            if t and t[0] == "config":
                configs[t[1]] = (dict(kv.split("=", 1) for kv in t[2:]), {"f32": [], "bf16": []})
            elif t and t[0] == "row":
                configs[t[1]][1][t[2]].append([int(v) for v in t[4:]])
    return configs


_CONFIGS = _fixture()
_ON_GPU = [name for name, (s, _) in _CONFIGS.items() if int(s["ny"]) * int(s["nx"]) * int(s["n"]) <= 1 << 20]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_planner_matches_the_recorded_matrix_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "unet_plan_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
           os.path.join(ROOT, "tests", "native", "unet_plan_host.cpp"), os.path.join(CSRC, "psm_unet_plan.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe, FIXTURE], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert f"configurations: {len(_CONFIGS)}, rows: {sum(len(r) for _, p in _CONFIGS.values() for r in p.values())}, failures: 0" in r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("name", _ON_GPU)
def test_gpu_library_plans_the_recorded_matrix(name, monkeypatch):
    """psm_unet_plan of the built library (plan only, zero weights) gives the fixture's plan_detail columns: library, host planner and
    the recording are one table."""
    from psm_amd import UNetSurrogate
    s, rows = _CONFIGS[name]
    for var in os.environ:
        if var.startswith("PSM_UNET_"):
            monkeypatch.delenv(var)
    if s["env"] != "-":
        for kv in s["env"].split(";"):
            monkeypatch.setenv(*kv.split("=", 1))
    widths = tuple(int(w) for w in s["widths"].split(","))
    c_in, c_out, ny, nx, n = (int(s[k]) for k in ("c_in", "c_out", "ny", "nx", "n"))
    choices = None if s["choices"] == "-" else [[int(v) for v in layer.split(":")] for layer in s["choices"].split(",")]
    cins = [c_in if l == 0 else widths[l - 1] for l in range(len(widths))]
    shapes = [sh for l, w in enumerate(widths) for sh in ((3, cins[l], w), (3, w, w))]
    shapes += [sh for l in range(len(widths) - 2, -1, -1) for sh in ((3, widths[l + 1] + widths[l], widths[l]), (3, widths[l], widths[l]))]
    shapes.append((1, widths[0], c_out))
    weights = [(np.zeros((k, k, ci, co), np.float32), np.zeros(co, np.float32)) for k, ci, co in shapes]
    for precision in ("f32", "bf16"):
        with UNetSurrogate(weights, ny, nx, c_in=c_in, c_out=c_out, widths=widths, max_cases=n, precision=precision, choices=choices) as net:
            got = [net.plan_detail(i) for i in range(len(shapes))]
        assert len(got) == len(rows[precision])
        for i, (d, row) in enumerate(zip(got, rows[precision])):
            assert [k for k, col in _COLUMNS.items() if d[k] != row[col]] == [], (name, precision, i, d, row)
            assert (d["keep"], d["bf16"]) == (0, int(precision == "bf16"))
