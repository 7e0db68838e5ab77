#!/usr/bin/env python3
"""Do two source trees compile to the same gfx950 kernels?  For a refactor that moves kernels between files.

    python tools/kernel_isa_diff.py OLD_CSRC NEW_CSRC [--exclude psm_unet.hip ...] [--same-work NAME ...] [--keep DIR] [-j N]

Every *.hip of each csrc directory (minus --exclude) is compiled on its own with the flags of
the shipped library plus --cuda-device-only -S.  The listing is cut into one text per kernel symbol, from the symbol's
label to its .Lfunc_end, which takes in the .amdhsa_kernel descriptor block.  What depends on file layout rather than on code
is dropped: comments, .file / .loc / .ident lines, and the numbering of local .L labels (renumbered in order of appearance).
For the kernels of both trees it requires: the same set of symbols, identical text, identical .amdhsa_ resource lines
(next_free_vgpr, next_free_sgpr, accum_offset, group_segment_fixed_size, private_segment_fixed_size) and identical
.vgpr_spill_count in the metadata.  Exit status 0 only if all of that holds.  Needs hipcc; no GPU.

--same-work NAME ...: kernels whose symbol contains one of the names now call a body they share with another kernel, so the
compiler may schedule them and compute their addresses differently.  Where such a kernel's text differs it passes if it does the
same work in the same budget: the same multiset of vector floating-point, convert, LDS and global / buffer / flat memory instructions (counted by
mnemonic, like tools/isa_mix.py counts classes), the same group_segment_fixed_size, private_segment_fixed_size 0 and no spills,
next_free_vgpr not above the old one.  A next_free_sgpr in a higher allocation granule (SGPR_GRANULE = 16 registers) than the old one is
printed as "sgpr granule rose" and counted apart, for the change to explain; it does not fail the run."""
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


def work_of(text):
    """The multiset of the instructions that are the kernel's work rather than its bookkeeping, as {mnemonic: count}."""
    work = {}
    for ln in text.split("\n"):
        op = ln.split()[0] if ln.split() else ""
        if (op.startswith("v_") and (re.search(r"_(f|bf)(16|32|64)\b|_f\d+_|_pk_f", op) or op.startswith("v_cvt_"))) or \
                op.startswith(("ds_", "global_", "buffer_", "flat_")):
            work[op] = work.get(op, 0) + 1
    return work


def same_work(old, new):
    """None if `new` = (text, resources, spills) passes the --same-work rule against `old`, else what it misses."""
    (t0, r0, s0), (t1, r1, s1) = old, new
    w0, w1 = work_of(t0), work_of(t1)
    if w0 != w1:
        return "instruction multiset: " + ", ".join(f"{op} {w0.get(op, 0)} -> {w1.get(op, 0)}" for op in sorted(set(w0) | set(w1)) if w0.get(op) != w1.get(op))
    if r0["group_segment_fixed_size"] != r1["group_segment_fixed_size"]:
        return "group_segment_fixed_size"
    if int(r1["private_segment_fixed_size"]) != 0 or s1 != 0:
        return "scratch or spills"
    if int(r1["next_free_vgpr"]) > int(r0["next_free_vgpr"]):
        return "next_free_vgpr rose"
    return None


# SGPRs are allocated to a wave in blocks of 16 on GFX9-family targets, gfx950 among them (LLVM AMDGPUUsage, "SGPR allocation
# granule": 16 for GFX9; the kernel descriptor's GRANULATED_WAVEFRONT_SGPR_COUNT is 2 * ((n_sgprs / 16) - 1))
SGPR_GRANULE = 16


def sgpr_granule_rose(r0, r1):
    return -(-int(r1["next_free_sgpr"]) // SGPR_GRANULE) > -(-int(r0["next_free_sgpr"]) // SGPR_GRANULE)


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
    ap.add_argument("--same-work", nargs="*", default=[], metavar="NAME", help="symbols containing NAME may differ in text if they do the same work")
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
    same = relaxed = rose = 0
    for sym in both:
        (t0, r0, s0, f0), (t1, r1, s1, f1) = old[sym], new[sym]
        assert len(r0) == len(RESOURCES) and s0 is not None, f"{sym}: descriptor or metadata not found in {f0}"
        if t0 == t1 and r0 == r1 and s0 == s1:
            same += 1
            continue
        n_ins = [sum(1 for ln in t.split("\n") if ln.startswith("\t") and not ln.lstrip().startswith(".")) for t in (t0, t1)]
        miss = same_work((t0, r0, s0), (t1, r1, s1)) if any(n in sym for n in a.same_work) else "not named by --same-work"
        if miss is None:
            relaxed += 1
            rose += sgpr_granule_rose(r0, r1)
            print(f"SAME WORK {sym}  instructions {n_ins[0]} -> {n_ins[1]}  vgpr {r0['next_free_vgpr']} -> {r1['next_free_vgpr']}  "
                  f"sgpr {r0['next_free_sgpr']} -> {r1['next_free_sgpr']}  lds {r1['group_segment_fixed_size']}  scratch 0  spills 0" + ("  sgpr granule rose" if sgpr_granule_rose(r0, r1) else ""))
            continue
        bad += 1
        print(f"DIFFERENT {sym}  [{miss}]  ({f0} -> {f1})  resources {r0} spills {s0} -> {r1} spills {s1}")
        for ln in list(difflib.unified_diff(t0.split("\n"), t1.split("\n"), f0, f1, lineterm="", n=1))[:40]:
            print("   ", ln)
    print(f"{len(both)} kernels compared, {same} identical (text, {', '.join(RESOURCES)}, vgpr_spill_count), "
          f"{relaxed} same work (--same-work; sgpr granule rose in {rose}); {len(old)} old, {len(new)} new")
    return 1 if bad or not both else 0


if __name__ == "__main__":
    sys.exit(main())
