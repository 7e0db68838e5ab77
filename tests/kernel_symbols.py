"""Kernel symbols in the gfx950 code objects of the built library: the .hip_fatbin section (llvm-objcopy), one offload bundle
per translation unit, each unbundled (clang-offload-bundler), the function symbols read demangled (llvm-readelf).  Shared by
the kernel tables of test_unet_layer_oracle.py and test_pca_stage_oracle.py."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

KERNEL_RE = re.compile(r"(psm_\w+_kernel)(<[^>]*>)?\(")


def library_kernels(lib_path, pattern=KERNEL_RE):
    """{name + template arguments without spaces} of every function symbol `pattern` matches (group 1 name, group 2 args)."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    tools = {}
    for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"):
        p = os.path.join(rocm, "llvm", "bin", t)
        tools[t] = p if os.path.exists(p) else shutil.which(t)
        if tools[t] is None:
            pytest.skip(f"{t} not found")
    names = set()
    with tempfile.TemporaryDirectory() as td:
        fb = os.path.join(td, "fatbin")
        subprocess.run([tools["llvm-objcopy"], f"--dump-section=.hip_fatbin={fb}", lib_path, os.path.join(td, "stripped")],
                       check=True, capture_output=True)
        data = open(fb, "rb").read()
        magic = b"__CLANG_OFFLOAD_BUNDLE__"
        starts = [m.start() for m in re.finditer(re.escape(magic), data)] + [len(data)]
        assert len(starts) > 1, "no offload bundle in .hip_fatbin"
        for k in range(len(starts) - 1):
            b, co = os.path.join(td, f"b{k}"), os.path.join(td, f"c{k}.o")
            open(b, "wb").write(data[starts[k]:starts[k + 1]])
            subprocess.run([tools["clang-offload-bundler"], "--unbundle", "--type=o", f"--input={b}",
                            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True, capture_output=True)
            sym = subprocess.run([tools["llvm-readelf"], "-s", "--demangle", "--wide", co], check=True, capture_output=True,
                                 text=True).stdout
            for line in sym.splitlines():
                f = line.split(None, 7)
                if len(f) == 8 and f[3] == "FUNC":
                    m = pattern.search(f[7])
                    if m:
                        names.add(m.group(1) + (m.group(2) or "").replace(" ", ""))
    return names
