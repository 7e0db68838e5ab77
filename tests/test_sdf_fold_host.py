"""Host side of the SDF fold (csrc/psm_fold.cpp: the packed basis over the velocity channels and the SDF channel's constant share of
the coefficients) as a stand-alone program under AddressSanitizer / UBSan: S = 128, c_in 3 and 4, 33 components (not a multiple
of the 32-component tile), 6 blocks.  CPU build only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "solving-poisson-s-equation-through-dl-for-cfd-apllications_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_fold_host_routines_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "sdf_fold_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
           os.path.join(ROOT, "tests", "native", "sdf_fold_host.cpp"), os.path.join(CSRC, "psm_fold.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "sdf fold host routines: ok" in r.stdout
