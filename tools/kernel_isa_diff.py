#!/usr/bin/env python3
"""Do two source trees compile to the same gfx950 kernels?  For a refactor that moves kernels between files.

    python tools/kernel_isa_diff.py OLD_CSRC NEW_CSRC [--exclude psm_unet.hip ...] [--keep DIR] [-j N]

Every *.hip of each csrc directory (minus --exclude) is compiled on its own with the flags of
the shipped library plus --cuda-device-only -S.  The listing is cut into one text per kernel symbol, from the symbol's
label to its .Lfunc_end, which takes in the .amdhsa_kernel descriptor block.  What depends on file layout rather than on code
is dropped: comments, .file / .loc / .ident lines, and the numbering of local .L labels (renumbered in order of appearance).
For the kernels of both trees it requires: the same set of symbols, identical text, identical .amdhsa_ resource lines
(next_free_vgpr, next_free_sgpr, accum_offset, group_segment_fixed_size, private_segment_fixed_size) and identical
.vgpr_spill_count in the metadata.  Exit status 0 only if all of that holds.  Needs hipcc; no GPU."""
import argparse
import concurrent.futures
import difflib
import os
import re
import subprocess
import sys
import tempfile

FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-x", "hip", "--cuda-device-only", "-S"]
RESOURCES = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "group_segment_fixed_size", "private_segment_fixed_size")
LOCAL_LABEL = re.compile(r"\.L[A-Za-z_$.]*\d+(?:_\d+)*")


def units(csrc, exclude):
    """The *.hip files of a tree, each a translation unit of its own."""
    return [f for f in sorted(os.listdir(csrc)) if f.endswith(".hip") and f not in exclude]


def compile_unit(hipcc, csrc, name, out_dir):
    out = os.path.join(out_dir, name[:-4] + ".s")
    subprocess.run([hipcc] + FLAGS + [name, "-o", out], cwd=csrc, check=True, capture_output=True)
    return out


def kernels_of(listing):
    """{symbol: (normalised text, {resource: value}, vgpr spills)} of one device listing."""
    lines = open(listing).read().split("\n")
    spills, name = {}, None
    for ln in lines:                                    # metadata: one YAML block per kernel, keys in alphabetical order
        m = re.match(r"\s+(?:- )?\.(name|vgpr_spill_count):\s+(\S+)", ln)
        if m and m.group(1) == "name":
            name = m.group(2)
        elif m and name:
            spills[name], name = int(m.group(2)), None
    found = {}
    for sym in (ln.split()[1] for ln in lines if ln.strip().startswith(".amdhsa_kernel ")):
        start = next(i for i, ln in enumerate(lines) if ln.startswith(sym + ":"))
        text, labels, res = [], {}, {}
        for ln in lines[start:]:
            ln = ln.split(";", 1)[0].rstrip()
            if not ln.strip() or re.match(r"\s*\.(file|loc|ident)\b", ln):
                continue
            end = re.match(r"\.Lfunc_end\d+:", ln)
            text.append(LOCAL_LABEL.sub(lambda m: labels.setdefault(m.group(0), ".L%d" % len(labels)), ln))
            m = re.match(r"\s*\.amdhsa_(\w+)\s+(\S+)", ln)
            if m and m.group(1) in RESOURCES:
                res[m.group(1)] = m.group(2)
            if end:
                break
        found[sym] = ("\n".join(text), res, spills.get(sym))
    return found


def tree_kernels(hipcc, csrc, exclude, out_dir, jobs):
    os.makedirs(out_dir, exist_ok=True)
    names = units(csrc, exclude)
    with concurrent.futures.ThreadPoolExecutor(jobs) as ex:
        listings = list(ex.map(lambda n: compile_unit(hipcc, csrc, n, out_dir), names))
    found = {}
    for name, listing in zip(names, listings):
        for sym, k in kernels_of(listing).items():
            assert sym not in found, f"{sym} is defined twice in {csrc} (second time in {name})"
            found[sym] = k + (name,)
    return found


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old"), ap.add_argument("new")
    ap.add_argument("--exclude", nargs="*", default=[], help="file names left out on both sides")
    ap.add_argument("--keep", help="directory for the listings (default: a temporary one)")
    ap.add_argument("-j", type=int, default=8)
    a = ap.parse_args()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as td:
        base = a.keep or td
        old = tree_kernels(hipcc, a.old, set(a.exclude), os.path.join(base, "old"), a.j)
        new = tree_kernels(hipcc, a.new, set(a.exclude), os.path.join(base, "new"), a.j)
    bad = 0
    for sym in sorted(set(old) ^ set(new)):
        print("only in", "old" if sym in old else "new", ":", sym)
        bad += 1
    both = sorted(set(old) & set(new))
    same = 0
    for sym in both:
        (t0, r0, s0, f0), (t1, r1, s1, f1) = old[sym], new[sym]
        assert len(r0) == len(RESOURCES) and s0 is not None, f"{sym}: descriptor or metadata not found in {f0}"
        if t0 == t1 and r0 == r1 and s0 == s1:
            same += 1
            continue
        bad += 1
        print(f"DIFFERENT {sym}  ({f0} -> {f1})  resources {r0} spills {s0} -> {r1} spills {s1}")
        for ln in list(difflib.unified_diff(t0.split("\n"), t1.split("\n"), f0, f1, lineterm="", n=1))[:40]:
            print("   ", ln)
    print(f"{len(both)} kernels compared, {same} identical (text, {', '.join(RESOURCES)}, vgpr_spill_count); "
          f"{len(old)} old, {len(new)} new")
    return 1 if bad or not both else 0


if __name__ == "__main__":
    sys.exit(main())
