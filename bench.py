#!/usr/bin/env python3
"""bench.py -- pressure-solves/sec of the surrogate hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W [--full] [--dump-outputs DIR]

A plain run measures the headline only: set-up, an untimed settling pass (>= 200 solves), W warm-up steps, the K timed
steps, the fields of the last timed step written to DIR/fields.npy when ``--dump-outputs`` is given, and the result line
(contract keys and the workload's config).  ``--full`` adds everything described below the workload paragraph: the
roofline and per-kernel passes, the per-solve quantiles, the end-to-end / solver-boundary / case-stream rates, the case
batch, the other legs, the CPU baselines and the oracle and golden comparisons.

``--gpus N`` with no torchrun environment starts the N ranks itself (fresh child processes, one per GPU, before this
process touches the GPU; every child is supervised: the first rank that fails ends the job within seconds, each rank's
stderr is kept in bench_rank<r>.err); under ``python -m torch.distributed.run --nproc-per-node N bench.py --gpus N`` the
environment's ranks are used.  The world size reported by the process group must equal ``--gpus`` and every rank must
sit on its own GPU (PCI bus ids on the line).

Workload of ``value`` at every N (weak scaling: the per-GPU work is fixed): BASELINE.json configs[1] -- 256x256
channel-with-obstacle U_to_gradP inference, batch 1, fp32, P_i = P_o = 128, MLP 3x512 (SURVEY.md §8 d config 1;
synthetic seeded input, seeded random-init weights of that architecture).  One step = one solve
(grid[256,256,3] -> fields[256,256,2]) through the C-ABI with the input already resident in HBM (the bench contract:
the PCIe-inclusive rate is never ``value``; it is ``value_end_to_end`` on the --full line); steps are issued back to back
on one stream, K steps are timed between barrier + synchronize on both sides, MAX over ranks.  Each rank drives its own
GPU with its own independent case stream (no data-path collective); RCCL carries the model broadcast (outside the timed
region), the barrier and the max-reduction of the time.

The ONE line on stdout is a summary shorter than 4096 characters (compact_line: contract keys, roofline and cpu_baseline
of the headline, a few numbers per extra leg); the full record described below -- per-kernel tables, per-launch stamps,
planner dumps -- is written to bench_detail.json (PSM_BENCH_LOGDIR, default: next to this script).

Objects of the full record of a --full run (the line carries their summary):
  value_end_to_end / end_to_end   SURVEY §8(d)'s solve INCLUDING the H2D copy of the grid and the D2H copy of the field
               (host buffers in, host buffers out), measured by a C++ loop inside the library through the public C-ABI
               (psm_bench_host): the pinned ring on caller-registered memory, next to the synchronous psm_solve_grid,
               the ring on pageable memory and the zero-copy slot form.
  case_batch   BASELINE configs[3]: random-obstacle 256x256 deltaU_to_deltaP cases, 8 per GPU per step (64 over 8 GPUs),
               one geometry per case slot, aggregate solves/s over all ranks + one all-gather of the result shards
               (outside the timed region); roofline of its dominant kernel against the f32 matrix peak.
  legs         (N = 1) every other BASELINE config and the convolutional path with the same protocol at a smaller K:
               configs[2], configs[4] (PCA-MLP, bf16 operands, 512x512), unet (UNet-S f32 batch 1), unet8 (f32, 8 cases per
               step: the x6 arithmetic's regime), unet8_bf16, unet512_bf16 (configs[4] as BASELINE.json words it) -- each with ms_per_step, l2_vs_oracle, roofline and,
               for the conv legs, the NumPy U-Net as cpu_baseline.
  roofline     the kernel with the largest measured time in this run: every dispatch of K instrumented solves carries
               its own begin / end stamps (hipExtLaunchKernelGGL events, psm_time_kernels); achieved = that kernel's
               algorithmic bytes per launch / its average duration.  "traffic" = HBM-side bytes per launch from the
               committed PMC run of the same kernel (profiles/archive/r04_pmc.json; null when the kernel source has changed
               since that run).
  cpu_baseline the C / OpenMP port of the reference's algorithm (float64 PCA + float32 MLP like the reference) timed on
               the host cores, rank 0, N=1; the NumPy oracle beside it.
"""
import argparse
import hashlib
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
# The host-buffer ring keeps several tickets in flight on their own streams: this PROGRAM asks the HIP runtime for enough
# hardware queues for them (read when the runtime initialises, i.e. before torch touches the GPU).  Measured: 50 us per
# end-to-end solve with 8 queues against 35 with 16.  The library itself never changes the
# environment; end_to_end.hw_queues reports what this process asked for and whether that was before HIP came up.


def _cpu_share():
    """CPUs this process may use: min(affinity, cgroup quota) -- the GPU boxes show 256 CPUs with a quota of 16."""
    n = os.cpu_count() or 1
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except Exception:
        pass
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            n = min(n, max(1, -(-int(q) // int(per))))
    except Exception:
        pass
    return max(1, n)


# BLAS / OpenMP pools of the CPU-baseline legs sized to that share BEFORE NumPy loads its BLAS: a pool of 256 spinning
# threads inside a 16-CPU quota gets the whole process throttled, launch thread included (measured: the f32 U-Net leg,
# 18 launches per step, at 364 us per step instead of 168 after an oracle call with the default pool).
for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ.setdefault(_v, str(_cpu_share()))
_HWQ_PRESET = os.environ.get("GPU_MAX_HW_QUEUES")
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")

P = 128
HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: HBM3E 8 TB/s (spec)
MFMA_F32_PEAK_TFLOPS = 157.3   # MI355X_MICROARCH.md: dense f32 matrix peak (256 CUs x 4 SIMDs x 64 FLOP/clk x 2.4 GHz)
MFMA_BF16_PEAK_TFLOPS = 2516.6   # dense bf16 matrix peak (16x the f32 rate)
PMC_FILE = "profiles/r06_pmc.json"
UNET_PMC_FILE = "profiles/r06_unet_pmc.json"

# BASELINE.json configs as (variant, Ny, Nx, cases per step per GPU, precision, description)
WORKLOADS = {
    "config1": ("gradp", 256, 256, 1, "f32", "BASELINE configs[1]: 256x256 channel+obstacle U_to_gradP, batch 1, fp32, "
                "B=30 blocks of 128x128x3, P_i=P_o=128, MLP 3x512, one independent case stream per GPU"),
    "config2": ("deltas", 256, 256, 1, "f32", "BASELINE configs[2]: 256x256 deltaU_to_deltaP, sequential solves (PISO correctors), "
                "B=9 blocks, P=128, MLP 3x512"),
    "config3": ("deltas", 256, 256, 8, "f32", "BASELINE configs[3]: random-obstacle 256x256 cases, 8 per GPU per step, "
                "B=9 blocks per case, P=128, MLP 3x512"),
    "config4": ("deltas", 512, 512, 1, "bf16", "BASELINE configs[4] (PCA-MLP form): 512x512 high-Re cylinder, bf16 operands / f32 accumulate, "
                "B=30 blocks, P=128, MLP 3x512"),
}
UNET_WORKLOADS = {           # the convolutional path (SURVEY.md section 8 row a-conv, parity unpinned) -- not the headline
    "unet": (256, 256, 1, "UNet-S (build-defined: 3x3 convs x2 per level, widths 16-32-64-128-256, max-pool, nearest "
             "upsample + skip concat, 1x1 head), 256x256x3 -> 256x256x1, batch 1, fp32, 7.0 GFLOP per solve"),
    "unet8": (256, 256, 8, "UNet-S, 256x256x3 -> 256x256x1, 8 cases per step per GPU, fp32 (wide layers: float32 products as six bf16 MFMA terms of exactly split operands)"),
    "unet_bf16": (256, 256, 1, "UNet-S, 256x256x3 -> 256x256x1, batch 1, bf16 operands / f32 accumulate"),
    "unet8_bf16": (256, 256, 8, "UNet-S, 256x256x3 -> 256x256x1, 8 cases per step per GPU, bf16 operands / f32 accumulate"),
    "unet512_bf16": (512, 512, 1, "UNet-S, 512x512x3 -> 512x512x1 (BASELINE configs[4] as worded: bf16 MFMA conv path), batch 1, "
                     "bf16 operands / f32 accumulate"),
    # configs[3]'s 64 cases on the conv path: 8x the work per launch of unet8_bf16 -- separates what the kernels sustain from what
    # the chain of 14 dependent launches costs (round-5 verdict, item 1a)
    "unet64_bf16": (256, 256, 64, "UNet-S, 256x256x3 -> 256x256x1, 64 cases per step on one GPU (BASELINE configs[3]'s batch on the conv path), "
                    "bf16 operands / f32 accumulate"),
}
DEFAULT_LEGS = ("config2", "config4", "unet", "unet8", "unet8_bf16", "unet512_bf16", "unet64_bf16")


# ----------------------------------------------------------------------------------------------------------------
# launcher: --gpus N without a torchrun environment
# ----------------------------------------------------------------------------------------------------------------
def _tail(path, n=1500):
    try:
        with open(path, "rb") as f:
            f.seek(0, 2)
            f.seek(max(0, f.tell() - n))
            return f.read().decode(errors="replace")
    except OSError:
        return ""


def spawn_ranks(n: int) -> int:
    """Start n fresh rank processes of this script (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set), supervise ALL of them
    and relay rank 0's JSON line.  The first rank that exits non-zero ends the job: the other children (exactly the ones
    started here) are terminated and its exit code is returned within seconds, with the tail of its stderr; every rank's
    stderr stays in bench_rank<r>.err (PSM_BENCH_LOGDIR, default: the working directory).  PSM_BENCH_TIMEOUT (seconds,
    default 1500) bounds the whole job.  Called before anything in this process has touched the GPU; nothing is ever
    re-exec'd."""
    import signal
    deadline = time.time() + float(os.environ.get("PSM_BENCH_TIMEOUT", "1500"))
    logdir = os.environ.get("PSM_BENCH_LOGDIR", os.getcwd())
    live = []                                         # the children of the current attempt, for the signal handler

    def on_signal(signum, _frame):
        # SIGTERM / SIGINT to the launcher (e.g. an outer `timeout`): stop exactly our children, then leave non-zero --
        # a rank parked in an RCCL barrier must not outlive the job and keep its GPU
        for p in live:
            if p.poll() is None:
                p.terminate()
        t_end = time.time() + 5.0
        for p in live:
            try:
                p.wait(timeout=max(0.1, t_end - time.time()))
            except subprocess.TimeoutExpired:
                p.kill()
        sys.stderr.write(f"bench.py --gpus {n}: launcher got signal {signum}; the ranks were stopped\n")
        os._exit(128 + signum)
    for sg in (signal.SIGTERM, signal.SIGINT, signal.SIGHUP):
        signal.signal(sg, on_signal)
    os.makedirs(logdir, exist_ok=True)
    out0 = os.path.join(logdir, "bench_rank0.out")
    for attempt in range(3):
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()                                     # rank 0 binds it next; a lost race shows as EADDRINUSE -> retried below
        procs, files = [], []
        for r in range(n):
            env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                       MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), PSM_BENCH_SPAWNED="1")
            env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
            ferr = open(os.path.join(logdir, f"bench_rank{r}.err"), "wb")
            fout = open(out0, "wb") if r == 0 else subprocess.DEVNULL
            files += [ferr] + ([fout] if r == 0 else [])
            procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env, stdout=fout, stderr=ferr))
        live[:] = procs

        def stop_all():
            for p in procs:
                if p.poll() is None:
                    p.terminate()                     # exactly the children this launcher started
            t_end = time.time() + 5.0
            for p in procs:
                try:
                    p.wait(timeout=max(0.1, t_end - time.time()))
                except subprocess.TimeoutExpired:
                    p.kill()
                    p.wait()

        rc_job, failed = 0, None
        while True:
            rcs = [p.poll() for p in procs]
            bad = [(r, rc) for r, rc in enumerate(rcs) if rc not in (None, 0)]
            if bad:
                failed, rc_job = bad[0]
                stop_all()
                break
            if all(rc == 0 for rc in rcs):
                break
            if time.time() > deadline:
                stop_all()
                failed, rc_job = -1, 124
                break
            time.sleep(0.05)
        for f in files:
            f.close()
        if rc_job == 0:
            with open(out0) as f:
                sys.stdout.write(f.read())
            sys.stdout.flush()
            return 0
        err = _tail(os.path.join(logdir, f"bench_rank{max(failed, 0)}.err"))
        if failed == 0 and attempt < 2 and ("EADDRINUSE" in err or "ddress already in use" in err):
            continue                                  # another process took the rendezvous port: new port, new ranks
        what = "deadline PSM_BENCH_TIMEOUT passed" if failed < 0 else f"rank {failed} exited with {rc_job}"
        sys.stderr.write(f"bench.py --gpus {n}: {what}; the other ranks were stopped.  Its stderr ({logdir}/bench_rank{max(failed, 0)}.err) ends:\n{err}\n")
        return rc_job if rc_job > 0 else 1
    return 1


# ----------------------------------------------------------------------------------------------------------------
# algorithmic work
# ----------------------------------------------------------------------------------------------------------------
def to_device(torch, arr):
    """NumPy -> device through a PINNED host tensor: hipMemcpy from ordinary memory makes the runtime pin the caller's pages on
    the fly; the library never does that (csrc/psm_alloc.h) and the bench does not either."""
    return torch.from_numpy(arr).pin_memory().cuda()


def to_host(torch, t):
    """device tensor -> NumPy through a pinned host tensor (see to_device)."""
    h = torch.empty(tuple(t.shape), dtype=t.dtype, pin_memory=True)
    h.copy_(t)
    return h.numpy().copy()


def algorithmic_bytes(model, ny, nx, wbytes=4):
    """SURVEY.md §8(d) BYTES formula, split per kernel group (float32 = 4 B)."""
    S2 = model.S ** 2
    enc = 4 * (ny * nx * model.c_in + S2 * model.c_in) + wbytes * S2 * model.c_in * model.p_in
    dec = 4 * (S2 * model.c_out + ny * nx * model.c_out) + wbytes * S2 * model.c_out * model.p_out
    layers = [wbytes * W.size + 4 * b.size for W, b in model.weights]
    return {"encode": enc, "decode": dec, "mlp": sum(layers), "layers": layers, "total": enc + dec + sum(layers)}


def algorithmic_flops(model, M):
    """SURVEY.md §8(d) FLOP formula for M block rows, split per kernel group."""
    S2 = model.S ** 2
    layers = [2 * M * W.shape[0] * W.shape[1] for W, _ in model.weights]
    enc, dec = 2 * M * S2 * model.c_in * model.p_in, 2 * M * model.p_out * S2 * model.c_out
    return {"encode": enc, "decode": dec, "layers": layers, "total": enc + dec + sum(layers)}


def kernel_algorithmic(name, table, launches_per_solve):
    """Algorithmic bytes (or flops) one launch of kernel `name` accounts for (None for kernels whose traffic is an
    artefact of the launch structure: slab sums, strip sums, chain)."""
    nl = len(table["layers"])
    if "encode" in name:
        return table["encode"]
    if "decode" in name:
        return table["decode"]
    if "reduce_dense1" in name:
        return table["layers"][0]
    if "#layer" in name:                       # psm_time_kernels lists every Dense layer by itself
        return table["layers"][int(name.rsplit("#layer", 1)[1])]
    if "dense" in name:
        # the remaining layers share this kernel: average over the layers it ran
        rest = table["layers"][1:] if launches_per_solve < nl else table["layers"]
        return sum(rest) / max(len(rest), 1)
    return None


def arithmetic_note(precision, kernels):
    """Which matrix pipe the PCA GEMMs of this run used, from the names of the kernels that were launched (x6 = a float32
    operand as three bf16 planes, six v_mfma_f32_32x32x16_bf16 terms, float32-grade error)."""
    if precision == "bf16":
        return "bf16 operands / f32 accumulate (bf16 MFMA) in encode, MLP and decode"
    form = {}
    for k in kernels:
        for part in ("encode", "decode"):
            if part in k["name"]:
                form[part] = "x6 split-bf16" if kernel_peak_tflops(k["name"], precision) != MFMA_F32_PEAK_TFLOPS else "f32 MFMA"
    return (f"{form.get('encode', '?')} encode / f32 MFMA MLP / {form.get('decode', '?')} decode"
            " (x6: 3 bf16 planes per f32 operand, 6 MFMA terms, f32-grade error)")


def kernel_peak_tflops(name, precision):
    """Matrix peak of the pipe a launch runs on: x6 launches issue six bf16 MFMA flops per algorithmic flop, so their
    ceiling is the bf16 peak / 6; bf16 handles the bf16 peak; everything else the f32 MFMA peak.  A fraction priced this
    way cannot exceed 1."""
    if precision == "bf16":
        return MFMA_BF16_PEAK_TFLOPS
    base = name.split("#")[0].strip()
    if "x6" in base or (base.startswith("psm_decode_paste") and base.rstrip(">").rstrip().endswith(", 2")):
        return MFMA_BF16_PEAK_TFLOPS / 6.0
    return MFMA_F32_PEAK_TFLOPS


def kernel_source_hash():
    h = hashlib.sha256()
    for f in ("psm_kernels.hip", "psm_bf16.hip", "psm_kernels.h"):
        p = os.path.join(ROOT, "solving-poisson-s-equation-through-dl-for-cfd-apllications_amd", "csrc", f)
        if os.path.exists(p):
            h.update(open(p, "rb").read())
    return h.hexdigest()[:16]


def committed_traffic(kernel, workload):
    """HBM-side bytes per launch of `kernel` from the committed PMC passes (tools/pmc_summary.py), only while the
    kernel sources are the ones that were profiled."""
    f = os.path.join(ROOT, PMC_FILE)
    try:
        d = json.load(open(f))
    except Exception:
        return None, None
    if d.get("workload") != workload:
        return None, None                                   # the committed counter passes are of the headline workload only
    if d.get("kernel_source_hash") != kernel_source_hash():
        return None, PMC_FILE + " is from other kernel sources: not used"
    v = d.get("kernels", {}).get(kernel.split("#layer")[0])          # rocprofv3 names the symbol, not the layer
    return (v, PMC_FILE + " (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes; 2*FETCH + WRITE KiB, gfx950 correction)") if v else (None, None)


def unet_source_hash():
    h = hashlib.sha256()
    for f in ("psm_unet.hip", "psm_unet_pair.hip", "psm_unet.h", "psm_unet_api.cpp"):
        p = os.path.join(ROOT, "solving-poisson-s-equation-through-dl-for-cfd-apllications_amd", "csrc", f)
        if os.path.exists(p):
            h.update(open(p, "rb").read())
    return h.hexdigest()[:16]


def unet_launch_key(net, first, kname, wgs):
    """What identifies a launch of the conv path in a rocprofv3 trace (tools/unet_hbm_summary.py writes the same keys): the generic
    kernel by tile rows, channel tiles, source transform and grid size; a fused pair by its template instantiation."""
    base = kname.strip("() ").split("(")[0]
    if not base.startswith("psm_conv3x3_kernel"):
        return "pair|" + base.replace(" ", "")
    th, nct, _, role = net.plan_info(first)[:4]
    n = len(net.shapes)
    L = (n + 1) // 4
    src = 2 if (0 < first < 2 * L and first % 2 == 0) else (1 if (2 * L <= first < n - 1 and (first - 2 * L) % 2 == 0) else 0)
    return f"conv3x3|{th}|{nct}|{src}|{int(wgs[first]) * (512 if role & 8 else 256)}"                # (eight-wave workgroups with the in-workgroup K split)


def committed_unet_traffic(workload, key):
    """HBM-side bytes per launch of a conv-path launch from the committed counter passes (tools/unet_hbm.sh), while the conv
    sources are the ones that were profiled."""
    try:
        d = json.load(open(os.path.join(ROOT, UNET_PMC_FILE)))
    except Exception:
        return None, None
    if d.get("unet_source_hash") != unet_source_hash():
        return None, UNET_PMC_FILE + ": other conv sources, not used"
    v = (d.get("workloads", {}).get(workload) or {}).get(key)
    return (v, UNET_PMC_FILE + " (rocprofv3 --pmc, 2*FETCH+WRITE KiB)") if v else (None, None)


def oracle_model(model):
    from oracle import psm_oracle as orc
    sc = orc.Scaler(model.scaler_kind, model.in_a, model.in_b, model.out_a, model.out_b)
    return orc.Model(model.variant, model.c_in, model.c_out, model.comp_in, model.mean_in, model.comp_out,
                     model.mean_out, model.weights, sc, model.out_scale, model.S, model.ov, model.sdf_ch, getattr(model, "conv1d", ()), getattr(model, "attention", None))


def cpu_baseline(model, grid, precision="f32", budget_s=12.0, max_solves=4000):
    """Time the CPU restatements on the host cores (bounded sample of the same workload): the C / OpenMP port
    (oracle/psm_cpu.c, "CPU back-end A" of BASELINE.md) is the reported baseline, the NumPy oracle -- the reference-style
    number -- is timed beside it; the fields for l2_vs_oracle come from the NumPy oracle."""
    import numpy as np
    from oracle import psm_oracle as orc
    from psm_amd import hostinfo
    cores = hostinfo.available_cpus()            # CPU share of this process (affinity / cgroup quota)
    _limit = hostinfo.limit_blas_threads(cores)  # BLAS pool = the threads actually used
    om = oracle_model(model)
    g = grid.astype(np.float64)
    orc.solve_grid(g, om, precision=precision)  # warm-up (BLAS threads, page faults)
    n, t0 = 0, time.perf_counter()
    while n < max_solves and (time.perf_counter() - t0) < budget_s / 2:
        sol = orc.solve_grid(g, om, precision=precision)
        n += 1
    dt = time.perf_counter() - t0
    numpy_rate = n / dt
    out = {"value": numpy_rate, "unit": "solves/s", "cores": int(cores), "kind": "port",
           "sample": f"{n} sequential {grid.shape[0]}x{grid.shape[1]} {model.variant} solves of the NumPy oracle "
                     f"(float64 PCA/reassembly, float32 MLP) in {dt:.1f} s"}
    if precision == "f32":
        try:
            from oracle import psm_cpu
            cm = psm_cpu.CpuModel(om)
            f = psm_cpu.solve_grid(g, cm, threads=int(cores))
            agree = float(np.abs(f - sol.fields).max() / np.abs(sol.fields).max())
            n, t0 = 0, time.perf_counter()
            while n < max_solves and (time.perf_counter() - t0) < budget_s / 2:
                psm_cpu.solve_grid(g, cm, threads=int(cores))
                n += 1
            dt = time.perf_counter() - t0
            out = {"value": n / dt, "unit": "solves/s", "cores": int(cores), "kind": "port",
                   "sample": f"{n} sequential {grid.shape[0]}x{grid.shape[1]} {model.variant} solves of the C / OpenMP port oracle/psm_cpu.c "
                             f"(float64 PCA/reassembly, float32 MLP, {int(cores)} threads) in {dt:.1f} s",
                   "numpy_oracle_solves_per_s": numpy_rate, "max_rel_diff_vs_numpy_oracle": agree}
        except Exception as e:                   # no compiler on the box: the NumPy oracle stays the baseline
            out["c_port"] = f"not available: {e!r}"[:200]
    return out, sol


def degenerate_note(variant, ny, nx, S=128):
    """BASELINE configs whose last block row duplicates the previous one: the reference itself is undefined there."""
    stride = 32 if variant == "gradp" else (96 if variant == "deltas" else None)
    if stride is None or (ny - S) % stride != 0:
        return None
    where = ("UGP:340 -> UGP:359 (mean of an empty slice: NaN dp/dx field, NaN rows in dp/dy; tests/golden/gradp_degenerate_256x256.npz)" if variant == "gradp"
             else "SMD:335 (broadcast error; tests/golden/deltas_degenerate_512x512.npz)")
    return ("build-defined skip: reference undefined on this grid (p_i == 0; " + where.split(" (")[0] + "); strict_degenerate=1 reproduces its NaN/error; goldens use other grids. "
            "In full: p_i == 0 on this grid, where the reference itself is undefined (" + where + "); the duplicate "
            "last block row is encoded / decoded but left out of the reassembly, and l2_vs_oracle compares with the "
            "oracle's same skip mode (strict_degenerate=1 reproduces the reference's NaN / error; the golden vectors of "
            "the parity claim use non-degenerate grids)")


def die_with_parent():
    """A rank started by spawn_ranks asks the kernel for SIGTERM when its parent dies: a launcher killed with SIGKILL cannot
    stop its ranks itself.  Linux prctl(PR_SET_PDEATHSIG); silently skipped elsewhere."""
    if os.environ.get("PSM_BENCH_SPAWNED") != "1":            # only ranks started by spawn_ranks (its main thread outlives them); the
        return                                                # death signal follows the parent THREAD: not under other launchers
    try:
        import ctypes
        import signal
        ctypes.CDLL(None, use_errno=True).prctl(1, int(signal.SIGTERM), 0, 0, 0)       # PR_SET_PDEATHSIG = 1
    except Exception:
        pass


_REAL_STDOUT = None


def own_stdout():
    """The driver reads ONE JSON line from stdout, but gloo and RCCL print banners there ("[Gloo] Rank 0 is connected ...",
    "RCCL version : ...").  From here on file descriptor 1 of this process points to stderr; the JSON line goes to the
    original stdout through emit()."""
    global _REAL_STDOUT
    if _REAL_STDOUT is None:
        sys.stdout.flush()
        _REAL_STDOUT = os.fdopen(os.dup(1), "w")
        os.dup2(2, 1)


def emit(obj):
    line = json.dumps(obj) + "\n"
    if _REAL_STDOUT is not None:
        _REAL_STDOUT.write(line)
        _REAL_STDOUT.flush()
    else:
        sys.stdout.write(line)
        sys.stdout.flush()


Q_CHUNK = 50                 # solves per sample of the quantile pass (value_p50 / p10 / p90)
LINE_LIMIT = 4096            # the driver keeps about 8 KB of stdout: the line must stay well inside it (tests assert < 4096)
DETAIL_FILE = "bench_detail.json"


def _sig(x, n=6):
    """Floats at n significant digits (the line is a summary; bench_detail.json keeps full precision)."""
    if isinstance(x, bool) or not isinstance(x, float):
        return x
    if x != x or x in (float("inf"), float("-inf")):
        return None
    return float(f"{x:.{n}g}")


def _clip(s, n):
    s = str(s)
    return s if len(s) <= n else s[:n - 3] + "..."


def _compact_roofline(r):
    keep = ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "algorithmic_bytes", "avg_launch_us")
    out = {k: _sig(r.get(k)) for k in keep}
    out["kernel"] = _clip(out["kernel"], 100)
    if r.get("traffic_source"):
        out["traffic_source"] = _clip(r["traffic_source"], 48)
    return out


def _compact_leg(leg):
    r = leg.get("roofline", {})
    out = {"value": _sig(leg.get("value")), "ms_per_step": _sig(leg.get("ms_per_step")), "dtype": leg.get("dtype"),
           "l2_vs_oracle": _sig(leg.get("l2_vs_oracle"), 3), "bound": r.get("bound"), "frac": _sig(r.get("frac"), 4)}
    wp = r.get("whole_pass") or r.get("whole_solve") or {}
    if wp.get("frac") is not None:
        out["frac_pass"] = _sig(wp["frac"], 4)           # whole pass against the time-weighted ceiling of its launches
    cb = leg.get("cpu_baseline")
    out["cpu"] = _sig(cb["value"], 4) if cb else None
    return out


def compact_line(d):
    """The ONE JSON line the driver parses: the contract keys, `roofline` and `cpu_baseline` of the headline workload and a
    few numbers per extra leg.  Everything else (per-kernel tables, per-launch stamps, planner dumps, prose) is in
    bench_detail.json and on stderr.  Always shorter than LINE_LIMIT characters (tests/test_bench_contract.py)."""
    c = d.get("config", {})
    out = {k: d.get(k) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                                 "scaling", "vs_baseline", "dtype", "data")}
    out["config"] = {"workload": _clip(c.get("workload", ""), 160)}
    for k, n in (("arithmetic", 120), ("parallelism", 120), ("geometry", 100), ("value_is", 140), ("degenerate", 160), ("parity", 120)):
        if c.get(k) is not None:
            out["config"][k] = _clip(c[k], n)
    for k in ("grid", "blocks", "cases_per_step_per_gpu", "guard_trips"):
        if k in c:
            out["config"][k] = c[k]
    if "roofline" in d:
        out["roofline"] = _compact_roofline(d["roofline"])
    if "cpu_baseline" in d:
        cb = d["cpu_baseline"]
        out["cpu_baseline"] = {"value": _sig(cb.get("value")), "unit": cb.get("unit"), "cores": cb.get("cores"), "kind": cb.get("kind"),
                               "sample": _clip(cb.get("sample", ""), 120)}
    for k in ("l2_vs_oracle", "gpu_over_cpu", "value_end_to_end", "value_p50", "value_p10", "value_p90"):
        if k in d:
            out[k] = _sig(d[k])
    if "frac_pass" in d:
        out["frac_pass"] = _sig(d["frac_pass"], 4)          # whole solve against its (time-weighted) ceiling, as every leg reports it
    if isinstance(d.get("shipped_case"), dict):             # the reference's deployment shape in ITS unit (DLPoissonFoam.C:111: ms per call)
        sc = d["shipped_case"]
        out["shipped_case"] = ({"error": _clip(sc["error"], 80)} if "error" in sc else
                               {"ms_per_call": _sig(sc.get("ms_per_call"), 4), "p10": _sig(sc.get("ms_per_call_p10"), 4), "p90": _sig(sc.get("ms_per_call_p90"), 4),
                                "cells": sc.get("cells"), "grid": sc.get("grid"), "blocks": sc.get("blocks"),
                                "cpu_ms": _sig((sc.get("cpu_baseline") or {}).get("value"), 4)})
    if isinstance(d.get("case_streams"), dict) and d["case_streams"].get("value") is not None:     # 4 independent batch-1 streams on the card
        out["case_streams4"] = _sig(d["case_streams"]["value"])
    if isinstance(d.get("l2_vs_reference_goldens"), dict):   # reference-run golden vectors (one per block layout)
        out["l2_vs_reference_goldens"] = {_clip(k, 24): (_sig(v, 3) if isinstance(v, float) else _clip(v, 60)) for k, v in list(d["l2_vs_reference_goldens"].items())[:4]}
    for k in ("world_size_reported", "dry_run"):
        if k in d:
            out[k] = d[k]
    if "devices" in d:
        out["devices"] = [_clip(x, 16) for x in d["devices"][:8]]
    if "case_batch" in d:
        cb = d["case_batch"]
        out["case_batch"] = dict(_compact_leg(cb), total_cases=cb.get("total_cases"), cases_per_step_per_gpu=cb.get("cases_per_step_per_gpu"),
                                 guard_trips=cb.get("guard_trips"))
        x64 = cb.get("all_64_cases_on_one_gpu") or {}
        if x64.get("value") is not None:            # configs[3]'s 64 cases per step on one card
            out["case_batch"]["x64_one_gpu"] = _sig(x64["value"])
        if "shards" in cb:                          # dry run: (first, count) of every rank's contiguous shard
            out["case_batch"]["shards"] = cb["shards"][:16]
    if "legs" in d:
        out["legs"] = {name: _compact_leg(leg) for name, leg in d["legs"].items()}
    out["detail"] = DETAIL_FILE
    line = json.dumps(out, separators=(",", ":"))
    if len(line) >= LINE_LIMIT:                      # never hand the driver a line it cannot keep: drop the optional parts
        for k in ("legs", "devices", "case_batch"):
            out.pop(k, None)
            line = json.dumps(out, separators=(",", ":"))
            if len(line) < LINE_LIMIT:
                break
    assert len(line) < LINE_LIMIT, len(line)
    return line


def emit_result(detail):
    """Rank 0: full record -> bench_detail.json (PSM_BENCH_LOGDIR, default next to this script) and stderr; compact line -> stdout."""
    logdir = os.environ.get("PSM_BENCH_LOGDIR", ROOT)
    try:
        os.makedirs(logdir, exist_ok=True)
        with open(os.path.join(logdir, DETAIL_FILE), "w") as f:
            json.dump(detail, f, indent=1)
    except OSError as e:
        sys.stderr.write(f"bench.py: could not write {DETAIL_FILE}: {e}\n")
    # stderr: a SHORT per-kernel table of the headline (the driver keeps only the tail of the output, so the full record
    # goes to the file; PSM_BENCH_VERBOSE=1 dumps it to stderr as well), written BEFORE the stdout line
    if os.environ.get("PSM_BENCH_VERBOSE"):
        sys.stderr.write("bench detail: " + json.dumps(detail) + "\n")
    rows = []
    for k in (detail.get("roofline") or {}).get("kernels", [])[:12]:
        gb = f"{k['achieved_GBs']:.0f} GB/s" if k.get("achieved_GBs") else "-"
        rows.append(f"  {k['name'][:60]:<60} {k['avg_us']:7.2f} us  {gb}")
    if rows:
        sys.stderr.write(("kernels of one solve (dispatch stamps):\n" + "\n".join(rows) + "\n")[:2000])
    sys.stderr.write(f"bench detail -> {os.path.join(logdir, DETAIL_FILE)}\n")
    sys.stderr.flush()
    line = compact_line(detail) + "\n"
    w = _REAL_STDOUT if _REAL_STDOUT is not None else sys.stdout
    w.write(line)
    w.flush()



DUMP_LIMIT = 64 << 20        # bytes of --dump-outputs in all


def dump_outputs(dirpath, arrays):
    """--dump-outputs: {name: host array} -> dirpath/<name>.npy in float32 (float64 kept).  The inputs are seeded, so two builds
    run with the same arguments can be compared array for array."""
    import numpy as np
    arrays = {k: np.ascontiguousarray(v, np.float64 if v.dtype == np.float64 else np.float32) for k, v in arrays.items()}
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_LIMIT:
        raise SystemExit(f"bench.py: --dump-outputs would write {total} bytes (limit {DUMP_LIMIT})")
    os.makedirs(dirpath, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(dirpath, k + ".npy"), a)


def finish(pdist_mod=None):
    try:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            dist.destroy_process_group()
    except Exception:
        pass


def main_dry(args):
    """Launcher / process-group plumbing only (CPU tests): no GPU work, value is null."""
    from psm_amd import dist as pdist
    import torch.distributed as dist
    rank, world, _ = pdist.env_world()
    if os.environ.get("PSM_BENCH_FAIL_RANK") == str(rank):          # supervision test: this rank dies before the rendezvous
        sys.stderr.write(f"rank {rank}: PSM_BENCH_FAIL_RANK set, exiting with 3\n")
        sys.exit(3)
    if os.environ.get("PSM_BENCH_DRY_SLEEP"):                       # supervision test: ranks that outlast the launcher's SIGTERM
        with open(os.path.join(os.environ.get("PSM_BENCH_LOGDIR", "."), "rank_pids"), "a") as f:
            f.write(f"{os.getpid()}\n")
        time.sleep(float(os.environ["PSM_BENCH_DRY_SLEEP"]))
    pdist.init(os.environ.get("PSM_BENCH_BACKEND", "gloo"))
    if world != args.gpus:
        raise SystemExit(f"world size {world} != --gpus {args.gpus}")
    dt = pdist.timed_region(lambda i: time.sleep(1e-4), args.steps, args.warmup)
    reported = dist.get_world_size() if dist.is_initialized() else 1
    # BASELINE configs[3]: the contiguous shard of the case batch every rank would own (8 cases per GPU), gathered
    nc3 = WORKLOADS["config3"][3]
    total_cases = nc3 * world
    mine = list(pdist.shard_cases(total_cases, world, rank))
    shards = [None] * world
    if dist.is_initialized():
        dist.all_gather_object(shards, mine)
    else:
        shards = [mine]
    if rank == 0:
        emit_result({"metric": "pressure-solves/sec (256x256 U->p inference)", "value": None, "unit": "solves/s",
                     "n_gpus": world, "world_size_reported": reported, "steps": args.steps, "warmup": args.warmup,
                     "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
                     "dtype": WORKLOADS[args.workload][4] if args.workload in WORKLOADS else None, "dry_run": True,
                     "data": "none (dry run: launcher and process-group plumbing only)",
                     "config": {"workload": WORKLOADS[args.workload][5] if args.workload in WORKLOADS else args.workload,
                                "parallelism": f"case-sharded x{world} (no data-path collective)"},
                     "devices": [f"dry:{r}" for r in range(world)],
                     "case_batch": {"total_cases": total_cases, "cases_per_step_per_gpu": nc3, "shards": shards}})
    finish()


# ----------------------------------------------------------------------------------------------------------------
# GPU helpers
# ----------------------------------------------------------------------------------------------------------------
def device_identity(torch, local_rank):
    pr = torch.cuda.get_device_properties(local_rank)
    if all(hasattr(pr, a) for a in ("pci_domain_id", "pci_bus_id", "pci_device_id")):
        return f"{pr.pci_domain_id:04x}:{pr.pci_bus_id:02x}:{pr.pci_device_id:02x}"
    return str(getattr(pr, "uuid", f"ordinal{local_rank}"))


def gather_devices(torch, local_rank, world):
    """PCI bus id of every rank's GPU; under RCCL the ranks must sit on distinct cards."""
    import torch.distributed as dist
    me = device_identity(torch, local_rank)
    if not (dist.is_available() and dist.is_initialized()) or world == 1:
        return [me]
    got = [None] * world
    dist.all_gather_object(got, me)
    return got


def guard_trips_after(sur, what):
    """The bound-geometry contract is checked by guard waves on the device; a raised flag only reaches the host counter
    through psm_synchronize (torch.cuda.synchronize does not look at it).  Called after every timed region on a bound
    handle: a trip (PSM_ERR_GEOMETRY) means the timed solves produced NaN fields -- a failed run, not a bench line."""
    try:
        sur.synchronize()
    except Exception as e:
        raise SystemExit(f"bench.py: {what}: the device-side geometry guard tripped during the timed region: {e}")
    n = sur.guard_trips
    if n:
        raise SystemExit(f"bench.py: {what}: guard_trips = {n} after the timed region")
    return n


def golden_parity(psm_amd, device):
    """BASELINE configs[1] itself has p_i == 0, where the reference defines no answer (config.degenerate); the parity claim
    rests on the golden vectors -- outputs of the reference's OWN statements run on seeded inputs (tests/golden/make_golden.py).
    One per block layout, solved here through the C-ABI: relative L2 of the assembled field against the reference-run field."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import cases
    out = {}
    for name in ("gradp_272x288", "deltas_256x256", "chapter5_300x400"):
        grid, model = cases.build(name)
        ref = cases.load_golden(name)["fields"]
        with psm_amd.GridSurrogate(model, grid.shape[0], grid.shape[1], device=device) as sur:
            f = sur.solve(grid.astype(np.float32), out_scale=[model.out_scale] if model.variant == "deltas" else None)[0]
        out[name] = float(np.linalg.norm(f - ref) / np.linalg.norm(ref))
    return out


def solver_boundary_leg(synthetic, device, steps):
    """psm_solve as DLPoissonFoam calls it (PythonComm.H:1-37): the solver's persistent cells[N,5] / p[N] float64 arrays,
    registered once (psm_pin_buffers), one synchronous call per time step -- mesh -> grid, the surrogate, grid -> mesh on the
    GPU.  16 k-cell channel mesh, 138 x 300 grid, Chapter-5 layout (the shape of tests/measure/mesh_bench.py)."""
    import numpy as np
    from psm_amd import SolverModule
    array, top, obst = synthetic.channel_mesh()
    model = synthetic.make_model("chapter5", p_in=32, p_out=32, seed_pca=4321, seed_w=11)
    sm = SolverModule(model, (1.0, 0.536133, 0.999023, 0.510742), device=device, geometry="native")   # no SciPy needed on the box
    sm.init_func(array, top, obst)
    cells, p = np.ascontiguousarray(array, np.float64).copy(), np.empty(array.shape[0], np.float64)
    sm.pin(cells, p)
    for _ in range(50):
        sm.py_func(cells, out=p)
    t0 = time.perf_counter()
    for _ in range(steps):
        sm.py_func(cells, out=p)
    dt = (time.perf_counter() - t0) / steps
    sm.unpin()
    return {"psm_solve_us": dt * 1e6, "solves_per_s": 1.0 / dt, "cells": int(array.shape[0]), "grid": [int(sm._sur.ny), int(sm._sur.nx)],
            "steps": steps, "finite": bool(np.isfinite(p).all()),
            "what": "psm_solve on registered buffers (psm_pin_buffers), synchronous, Python call overhead included"}


def case_streams_leg(torch, psm_amd, synthetic, model, ny, nx, precision, device, n_streams, steps):
    """Independent batch-1 case streams sharing ONE GPU (the north star's "ensemble of geometries / timesteps" on a single card, without
    batching them into one call): n_streams handles, each on its own HIP stream with its own bound geometry and its own input, solves
    issued round-robin from one host thread.  A single stream leaves the card idle between its six dependent launches; this is what the
    card delivers when other cases fill those gaps.  Device-resident like `value`; NOT the headline (one PISO run is one sequential stream)."""
    import numpy as np
    surs = [psm_amd.GridSurrogate(model, ny, nx, max_cases=1, device=device, precision=precision) for _ in range(n_streams)]
    streams = [torch.cuda.Stream() for _ in range(n_streams)]
    d_in = [to_device(torch, synthetic.channel_grid(ny, nx, seed=101 + 7 * k).astype(np.float32)[None]) for k in range(n_streams)]
    d_out = [torch.empty((1, ny, nx, model.c_out), dtype=torch.float32, device="cuda") for _ in range(n_streams)]
    try:
        bound = all(bool(surs[k].bind_geometry(d_in[k].data_ptr(), on_device=True)) for k in range(n_streams))

        def step(i):
            k = i % n_streams
            surs[k].solve_device(d_in[k].data_ptr(), 1, d_out[k].data_ptr(), streams[k].cuda_stream)
        for i in range(40 * n_streams):
            step(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            step(i)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        finite = all(bool(torch.isfinite(o).all().item()) for o in d_out)
        trips = sum(int(s_.guard_trips) for s_ in surs)
    finally:
        for s_ in surs:
            s_.close()
    return {"value": steps / dt, "unit": "solves/s", "streams": n_streams, "steps": steps, "us_per_solve": dt / steps * 1e6,
            "geometry": "one bound geometry per stream" if bound else "general path", "guard_trips": trips, "finite": finite,
            "what": "independent batch-1 case streams on one GPU, one handle + HIP stream each, round-robin from one host thread, inputs resident in HBM"}


def shipped_case_leg(synthetic, device, steps, with_cpu):
    """The reference's one real deployment shape, in the unit its solver prints (DLPoissonFoam.C:106-111, "DL pressure prediction &
    data transport: %.2f ms"): ONE synchronous psm_solve per PISO step on the shipped case's shape -- 400 x 3000 grid (15 x 2 m at
    delta 0.005), Chapter-5 layout = 104 blocks, the shipped weights.h5 network (45 -> 512 x 3 -> 48; tests/golden/chapter5_weights.npz),
    a channel mesh of ~31 k cells (the shipped meshes: 31 k - 207 k) -- cells[N,5] float64 in, p[N] float64 out, the solver's arrays
    registered (psm_pin_buffers).  Beside it the C port of the grid solve on the same grid (no mesh interpolation on the CPU side)."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import cases
    from psm_amd import SolverModule
    W, maxs4, maxs_pca = cases.real_chapter5_weights()
    model = synthetic.make_model("chapter5", p_in=45, p_out=48, weights=W)
    model.in_a, model.out_a = float(maxs_pca[0]), float(maxs_pca[1])
    array, top, obst = synthetic.shipped_case_mesh()
    sm = SolverModule(model, tuple(float(v) for v in maxs4), device=device, geometry="native")
    t0 = time.perf_counter()
    sm.init_func(array, top, obst)
    t_init = time.perf_counter() - t0
    cells, p = np.ascontiguousarray(array, np.float64).copy(), np.empty(array.shape[0], np.float64)
    sm.pin(cells, p)
    for _ in range(20):
        sm.py_func(cells, out=p)
    per = []
    for _ in range(steps):
        t0 = time.perf_counter()
        sm.py_func(cells, out=p)
        per.append(time.perf_counter() - t0)
    per.sort()
    sm.unpin()
    leg = {"what": "one synchronous psm_solve per call on the reference's shipped case shape (DLPoissonFoam.C:106-111 prints this time in ms)",
           "ms_per_call": per[len(per) // 2] * 1e3, "ms_per_call_p10": per[len(per) // 10] * 1e3, "ms_per_call_p90": per[(len(per) * 9) // 10] * 1e3,
           "calls": steps, "cells": int(array.shape[0]), "grid": [int(sm._sur.ny), int(sm._sur.nx)], "blocks": int(sm._sur.B),
           "components": [45, 48], "geometry_bound": bool(sm._sur.geometry_bound), "init_func_s": t_init,
           "finite": bool(np.isfinite(p).all()), "unit": "ms per psm_solve call (registered buffers, Python call overhead included)"}
    if with_cpu:
        try:
            from oracle import psm_cpu                       # checker / cpu_baseline leg only
            from psm_amd import hostinfo
            cores = hostinfo.available_cpus()
            om = oracle_model(model)
            g = synthetic.channel_grid(int(sm._sur.ny), int(sm._sur.nx), seed=1).astype(np.float64)
            cm = psm_cpu.CpuModel(om)
            psm_cpu.solve_grid(g, cm, threads=int(cores))
            n, t0 = 0, time.perf_counter()
            while n < 20 and (n == 0 or time.perf_counter() - t0 < 6.0):
                psm_cpu.solve_grid(g, cm, threads=int(cores))
                n += 1
            dt = (time.perf_counter() - t0) / n
            leg["cpu_baseline"] = {"value": dt * 1e3, "unit": "ms per grid solve", "cores": int(cores), "kind": "port",
                                   "sample": f"{n} solves of the C / OpenMP port oracle/psm_cpu.c on the same {g.shape[0]}x{g.shape[1]} grid "
                                             f"(grid in, field out: no mesh interpolation), {int(cores)} threads"}
        except Exception as e:
            leg["cpu_baseline"] = {"error": repr(e)[:200]}
    return leg


def host_rates(sur, grids, n_cases, steps, warmup, modes):
    """psm_bench_host (C++ loop through the public C-ABI): {mode name: (solves/s per rank, last field)}."""
    import ctypes as C
    import numpy as np
    host = np.ascontiguousarray(np.stack(grids))                     # [n_inputs][n_cases, ny, nx, c_in]
    out = {}
    names = {0: "sync_pageable", 1: "ring_pageable", 2: "ring_registered", 3: "ring_zero_copy"}
    for mode, depth in modes:
        last = np.empty((n_cases, sur.ny, sur.nx, sur.model.c_out), np.float32)
        sec = C.c_double()
        sur._chk(sur.lib.psm_bench_host(sur.h, host.ctypes.data_as(C.POINTER(C.c_float)), host.shape[0], n_cases, mode, depth,
                                        steps, warmup, C.byref(sec), last.ctypes.data_as(C.POINTER(C.c_float))))
        out[names[mode] + (f"_depth{depth}" if mode else "")] = (n_cases * steps / sec.value, last)
    return out


def time_kernels(sur, d_grid, n_cases, d_fields, steps, quantiles=False):
    """psm_time_kernels_q -> [(name, MEDIAN us of the kernel's dispatches, launches)] in launch order; with ``quantiles`` a fourth
    element (p10 us, p90 us).  Median, not mean: one slow dispatch among a few hundred must not pick the dominant kernel."""
    import ctypes as C
    cap = 32
    names = C.create_string_buffer(cap * 64)
    med, p10, p90 = (C.c_double * cap)(), (C.c_double * cap)(), (C.c_double * cap)()
    cnt = (C.c_int64 * cap)()
    nk = C.c_int32()
    sur._chk(sur.lib.psm_time_kernels_q(sur.h, C.c_void_p(d_grid), n_cases, C.c_void_p(d_fields), steps, names, med, p10, p90, cnt, cap, C.byref(nk)))
    out = []
    for k in range(min(nk.value, cap)):
        nm = names.raw[k * 64:(k + 1) * 64].split(b"\0", 1)[0].decode()
        rec = (nm, float(med[k]), int(cnt[k]))
        out.append(rec + ((float(p10[k]), float(p90[k])),) if quantiles else rec)
    return out


def pca_roofline(sur, model, ny, nx, n_cases, precision, d_grid, d_fields, steps, dt_step, workload, bound_path, kt=None):
    """Roofline of the kernel with the largest measured time: every dispatch of an instrumented pass over `steps` solves
    carries its own begin / end stamps.  Both ceilings are priced -- algorithmic bytes against the HBM peak, algorithmic
    flops against the f32 / bf16 matrix peak -- and the kernel is bound by the one it sits closer to."""
    wb = 2 if precision == "bf16" else 4
    ab = algorithmic_bytes(model, ny, nx, wb)
    ab_batch = dict(ab, encode=ab["encode"] + (n_cases - 1) * 4 * ny * nx * model.c_in,
                    decode=ab["decode"] + (n_cases - 1) * 4 * ny * nx * model.c_out)       # bases read once, fields per case
    af = algorithmic_flops(model, n_cases * sur.B)
    if kt is None:
        kt = time_kernels(sur, d_grid, n_cases, d_fields, steps, quantiles=True)
    per_solve = {rec[0]: rec[2] / steps for rec in kt}
    kernels = []
    for rec in kt:
        nm, us, n = rec[:3]
        q10, q90 = rec[3] if len(rec) > 3 else (None, None)
        b, f = kernel_algorithmic(nm, ab_batch, per_solve[nm]), kernel_algorithmic(nm, af, per_solve[nm])
        kernels.append({"name": nm, "avg_us": us, "p10_us": q10, "p90_us": q90,      # avg_us = MEDIAN of this run's dispatch stamps (name kept from round 3)
                        "launches_per_solve": per_solve[nm], "algorithmic_bytes": b, "algorithmic_flops": f,
                        "peak_TFLOPs": kernel_peak_tflops(nm, precision),      # the pipe THIS launch runs on (x6: bf16 peak / 6)
                        "achieved_GBs": (b / (us * 1e-6) / 1e9) if b else None,
                        "achieved_TFLOPs": (f / (us * 1e-6) / 1e12) if f else None})
    # the dominant launch = the longest among those that carry a non-trivial share (>= 5 %) of the solve's algorithmic bytes or flops:
    # a launch-bound 0.26 MB layer that happens to be the longest says nothing about a ceiling (configs[4]'s PCA-bf16 leg, rounds 4-5)
    tot_b, tot_f = ab_batch["total"], af["total"]
    heavy = [k for k in kernels if (k["algorithmic_bytes"] or 0) >= 0.05 * tot_b or (k["algorithmic_flops"] or 0) >= 0.05 * tot_f]
    dom = max(heavy or kernels, key=lambda k: k["avg_us"] * k["launches_per_solve"])
    peak_f = dom["peak_TFLOPs"]
    gbs, tfl = dom["achieved_GBs"] or 0.0, dom["achieved_TFLOPs"] or 0.0
    f_hbm, f_mfma = gbs / HBM_PEAK_GBS, tfl / peak_f
    # whole solve: flops against the time-weighted matrix ceiling of its launches (sum of t_i * peak_i), bytes against HBM
    t_sum = sum(k["avg_us"] * k["launches_per_solve"] for k in kernels)
    ceil_f = sum(k["avg_us"] * k["launches_per_solve"] * k["peak_TFLOPs"] for k in kernels) / max(t_sum, 1e-12)
    traffic, traffic_src = committed_traffic(dom["name"], workload) if bound_path else (None, None)
    roof = {"kernel": dom["name"], "bound": "mfma" if f_mfma > f_hbm else "hbm"}
    if roof["bound"] == "hbm":
        roof.update(achieved=gbs, peak=HBM_PEAK_GBS, unit="GB/s", frac=f_hbm)
    else:
        roof.update(achieved=tfl, peak=peak_f, unit="TFLOP/s", frac=f_mfma)
    roof.update(traffic=traffic, traffic_source=traffic_src, algorithmic_bytes=dom["algorithmic_bytes"], algorithmic_flops=dom["algorithmic_flops"],
                avg_launch_us=dom["avg_us"], launches=int(dom["launches_per_solve"] * steps), frac_hbm=f_hbm, frac_mfma=f_mfma,
                selection="largest MEDIAN dispatch time per solve among the launches of the instrumented pass that carry >= 5 % of the solve's "
                          "algorithmic bytes or flops (every Dense layer is its own "
                          "entry: the two hidden layers run the same template instantiation, which rocprofv3 lists as one kernel "
                          "with two calls per solve); bound = the ceiling it sits closer to",
                whole_solve={"algorithmic_bytes": tot_b, "algorithmic_flops": af["total"],
                             "achieved_GBs": tot_b / dt_step / 1e9, "frac_hbm": tot_b / dt_step / 1e9 / HBM_PEAK_GBS,
                             "achieved_TFLOPs": af["total"] / dt_step / 1e12, "ceiling_TFLOPs_time_weighted": ceil_f,
                             "frac_mfma": af["total"] / dt_step / 1e12 / ceil_f,
                             "frac": max(tot_b / dt_step / 1e9 / HBM_PEAK_GBS, af["total"] / dt_step / 1e12 / ceil_f)},
                kernels=kernels)
    return roof


def unet_leg(name, args, torch, pdist, rank, world, local_rank, backend, steps, warmup, with_cpu, cpu_budget_s=4.0, full=True, dump_dir=None):
    """The convolutional path with the bench protocol: K forward passes back to back, input resident in HBM.  ``full``: the
    per-launch roofline pass and (``with_cpu``) the NumPy U-Net as cpu_baseline after the timed region; ``dump_dir``: the
    fields of the last timed pass are written there (dump_outputs)."""
    import numpy as np
    from psm_amd import UNetSurrogate, synthetic
    NY, NX, NC, desc = UNET_WORKLOADS[name]
    W = synthetic.unet_he_weights(seed=7)
    prec = "bf16" if name.endswith("bf16") else "f32"
    peak = MFMA_BF16_PEAK_TFLOPS if prec == "bf16" else MFMA_F32_PEAK_TFLOPS
    net = UNetSurrogate(W, NY, NX, max_cases=NC, device=local_rank, precision=prec, autotune=True)   # plan-time, outside the timed region
    n_in = min(args.inputs, 2 if (NY > 256 or NC > 8) else args.inputs)
    grids = [np.stack([synthetic.channel_grid(NY, NX, seed=1 + 1000 * rank + 10 * i + k, noise=0.05 if NY > 256 else 0.02).astype(np.float32)
                       for k in range(NC)]) for i in range(n_in)]
    d_in = [to_device(torch, g) for g in grids]
    d_out = [torch.empty((NC, NY, NX, 1), dtype=torch.float32, device="cuda") for _ in grids]
    stream = torch.cuda.current_stream().cuda_stream

    def step(i):
        k = i % len(d_in)
        net.forward_device(d_in[k].data_ptr(), NC, d_out[k].data_ptr(), stream)
    dt_max = pdist.timed_region(step, steps, warmup, torch.cuda.synchronize, "cuda" if backend == "nccl" else "cpu")
    torch.cuda.synchronize()
    if dump_dir:
        dump_outputs(dump_dir, {"fields": to_host(torch, d_out[(steps - 1) % len(d_in)])})       # [NC, NY, NX, 1]
    leg = {"workload": desc, "value": pdist.aggregate_throughput(NC, steps, world, dt_max), "unit": "solves/s", "steps": steps, "warmup": warmup,
           "ms_per_step": dt_max / steps * 1e3, "dtype": prec, "cases_per_step_per_gpu": NC, "grid": [NY, NX],
           "parity": "unpinned (no reference network): l2_vs_oracle is against the build-defined NumPy U-Net with the same rounding points",
           "planner": {"autotuned_split_k": net.autotuned}}
    if not full:
        net.close()
        return leg
    got = to_host(torch, d_out[0][0])
    flops = net.flops * NC
    achieved = flops * steps / dt_max / 1e12
    # every launch of the forward pass with its own dispatch stamps: flops and activation / weight bytes of the convolutions it covers
    ab, wbts = (2, 2) if prec == "bf16" else (4, 4)
    launches = []
    wgs_all = net.profile(d_in[0].data_ptr(), NC, d_out[0].data_ptr())[1]
    for first, convs, kname, us in net.time_kernels(d_in[0].data_ptr(), NC, d_out[0].data_ptr(), steps=max(5, min(20, steps))):
        fl = sum(net.conv_flops(c) for c in convs) * NC
        # a fused launch (level pair, fused 1x1 head) reads the first convolution's input and writes the last one's output
        by = (net.conv_bytes(convs[0], ab, wbts)[0] + net.conv_bytes(convs[-1], ab, wbts)[1]) * NC + sum(net.conv_bytes(c, ab, wbts)[2] for c in convs)
        # float32 mode: a layer planned with the x6 arithmetic issues SIX bf16 MFMA flops per algorithmic flop, so its ceiling is
        # the bf16 matrix peak / 6 (419 TFLOP/s of float32-accurate products), not the f32 MFMA peak
        x6 = prec == "f32" and bool(net.plan_info(first)[3] & 4)
        pk = MFMA_BF16_PEAK_TFLOPS / 6.0 if x6 else peak
        launches.append({"convs": convs, "kernel": kname, "key": unet_launch_key(net, first, kname, wgs_all), "avg_us": us, "flops": fl, "algorithmic_bytes": by,
                         "arithmetic": "x6 (3 bf16 planes per operand, 6 MFMA terms)" if x6 else ("bf16 MFMA" if prec == "bf16" else "f32 MFMA"),
                         "peak_TFLOPs": pk, "achieved_TFLOPs": fl / (us * 1e-6) / 1e12, "achieved_GBs": by / (us * 1e-6) / 1e9})
    dom = max(launches, key=lambda l: l["avg_us"])
    ceil_pass = sum(l["avg_us"] * l["peak_TFLOPs"] for l in launches) / max(sum(l["avg_us"] for l in launches), 1e-12)
    f_mfma, f_hbm = dom["achieved_TFLOPs"] / dom["peak_TFLOPs"], dom["achieved_GBs"] / HBM_PEAK_GBS
    roof = {"kernel": f"{dom['kernel']} (convolutions {dom['convs']})", "bound": "mfma" if f_mfma > f_hbm else "hbm"}
    if roof["bound"] == "mfma":
        roof.update(achieved=dom["achieved_TFLOPs"], peak=dom["peak_TFLOPs"], unit="TFLOP/s", frac=f_mfma, arithmetic=dom["arithmetic"])
    else:
        roof.update(achieved=dom["achieved_GBs"], peak=HBM_PEAK_GBS, unit="GB/s", frac=f_hbm)
    traffic, traffic_src = committed_unet_traffic(name, dom["key"])
    for l in launches:
        l["traffic"] = committed_unet_traffic(name, l["key"])[0]
    roof.update(traffic=traffic, traffic_source=traffic_src, avg_launch_us=dom["avg_us"], algorithmic_flops=dom["flops"], algorithmic_bytes=dom["algorithmic_bytes"],
                frac_mfma=f_mfma, frac_hbm=f_hbm, selection="the launch of the forward pass with the largest MEDIAN dispatch-stamped duration",
                whole_pass={"algorithmic_flops": flops, "achieved_TFLOPs": achieved,
                            # every launch against the pipe it runs on: ceiling = sum(t_i * peak_i) / sum(t_i); a pass whose launches
                            # are each below their own peak cannot exceed 1
                            "ceiling_TFLOPs_time_weighted": ceil_pass, "frac": achieved / ceil_pass, "frac_mfma": achieved / ceil_pass,
                            "frac_mfma_priced_against": "time-weighted ceiling of the launches (x6 launches: bf16 peak / 6 = 419.4; f32 MFMA 157.3; bf16 2516.6 TFLOP/s)",
                            "sum_of_launches_us": sum(l["avg_us"] for l in launches), "n_launches": len(launches)},
                launches=launches)
    leg["roofline"] = roof
    if with_cpu:
        from oracle import unet_oracle as uo           # checker + cpu_baseline leg only
        from psm_amd import hostinfo
        cores = hostinfo.available_cpus()
        hostinfo.limit_blas_threads(cores)
        g0 = grids[0][0]
        n, t0 = 0, time.perf_counter()
        while n < 50 and (n == 0 or time.perf_counter() - t0 < cpu_budget_s):
            ref = uo.unet_forward(g0, W, precision=prec)
            n += 1
        dt = time.perf_counter() - t0
        leg["cpu_baseline"] = {"value": n / dt, "unit": "solves/s", "cores": int(cores), "kind": "port",
                               "sample": f"{n} UNet-S {NY}x{NX} forward pass(es) of the NumPy oracle (float64 accumulation, BLAS on {int(cores)} threads) in {dt:.1f} s"}
        leg["l2_vs_oracle"] = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
    net.close()
    return leg


def main_unet(args):
    import torch
    from psm_amd import dist as pdist
    rank, world, local_rank = pdist.env_world()
    backend = os.environ.get("PSM_BENCH_BACKEND", "nccl")
    local_rank = int(os.environ.get("PSM_BENCH_DEVICE", local_rank))
    torch.cuda.set_device(local_rank)
    pdist.init(backend, torch.device("cuda", local_rank))
    leg = unet_leg(args.workload, args, torch, pdist, rank, world, local_rank, backend, args.steps, args.warmup,
                   args.full and rank == 0 and world == 1 and not args.no_cpu_baseline, cpu_budget_s=12.0, full=args.full,
                   dump_dir=args.dump_outputs if rank == 0 else None)
    out = {"metric": "pressure-solves/sec (256x256 U->p inference)", "value": leg["value"], "unit": "solves/s", "n_gpus": world,
           "steps": args.steps, "warmup": args.warmup, "ms_per_step": leg["ms_per_step"], "higher_is_better": True, "scaling": "weak",
           "vs_baseline": None, "dtype": leg["dtype"], "data": "synthetic",
           "config": {"workload": leg["workload"], "grid": leg["grid"], "cases_per_step_per_gpu": leg["cases_per_step_per_gpu"],
                      "parallelism": f"case-sharded x{world} (no data-path collective)", "parity": leg["parity"], "planner": leg["planner"],
                      "arithmetic": ("bf16 operands / f32 accumulate (bf16 MFMA)" if leg["dtype"] == "bf16" else
                                     "f32 MFMA; layers with c_in >= 64 on 8-row tiles as x6 split-bf16 (6 bf16 MFMA terms, f32-grade error)")}}
    for k in ("roofline", "cpu_baseline", "l2_vs_oracle"):
        if k in leg:
            out[k] = leg[k]
    if rank == 0:
        emit_result(out)
    finish()


def pca_leg(name, model, args, torch, pdist, psm_amd, synthetic, rank, world, local_rank, red_dev, steps, warmup, with_oracle):
    """One BASELINE config of the PCA-MLP path with the bench protocol (device-resident steps, geometry bound once)."""
    import numpy as np
    variant, NY, NX, NC, precision, desc = WORKLOADS[name]
    sur = psm_amd.GridSurrogate(model, NY, NX, max_cases=NC, device=local_rank, precision=precision)
    if name == "config2":        # sequential delta-U fields of one simulation: phase-shifted frames on one geometry
        base = synthetic.channel_grid(NY, NX, seed=1 + 1000 * rank).astype(np.float32)
        grids = []
        for i in range(args.inputs):
            g = synthetic.delta_grid(NY, NX, seed=2 + 1000 * rank, step=i).astype(np.float32)
            g[..., model.sdf_ch] = base[..., model.sdf_ch]
            g[..., :model.sdf_ch] *= (base[..., model.sdf_ch:model.sdf_ch + 1] != 0)
            grids.append(g[None])
    else:
        grids = [synthetic.channel_grid(NY, NX, seed=4 + 1000 * rank + i, noise=0.05 if NY > 256 else 0.02).astype(np.float32)[None]
                 for i in range(args.inputs)]
    d_in = [to_device(torch, g) for g in grids]
    d_out = [torch.empty((NC, NY, NX, model.c_out), dtype=torch.float32, device="cuda") for _ in grids]
    stream = torch.cuda.current_stream().cuda_stream
    masks = [g[..., model.sdf_ch] != 0 for g in grids]
    bound = (not args.no_bind) and all(np.array_equal(masks[0], m) for m in masks[1:]) and sur.bind_geometry(d_in[0].data_ptr(), on_device=True, n_cases=NC)

    def step(i):
        k = i % len(d_in)
        sur.solve_device(d_in[k].data_ptr(), NC, d_out[k].data_ptr(), stream)
    dt = pdist.timed_region(step, steps, warmup, torch.cuda.synchronize, red_dev)
    torch.cuda.synchronize()
    trips = guard_trips_after(sur, name)
    got = to_host(torch, d_out[0])[0]
    leg = {"workload": desc, "value": pdist.aggregate_throughput(NC, steps, world, dt), "unit": "solves/s", "steps": steps, "warmup": warmup,
           "ms_per_step": dt / steps * 1e3, "dtype": precision, "grid": [NY, NX], "blocks": sur.B,
           "geometry": "bound once per case stream" if bound else "general path", "guard_trips": trips,
           "degenerate": degenerate_note(variant, NY, NX),
           "roofline": pca_roofline(sur, model, NY, NX, NC, precision, d_in[0].data_ptr(), d_out[0].data_ptr(), steps, dt / steps, name, bound)}
    if with_oracle:
        from oracle import psm_oracle as orc
        t0 = time.perf_counter()
        ref = orc.solve_grid(grids[0][0].astype(np.float64), oracle_model(model), precision=precision).fields
        leg["l2_vs_oracle"] = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
        leg["oracle"] = ("NumPy oracle with the same bf16 rounding points (the reference has no bf16 path)" if precision == "bf16"
                         else "NumPy oracle (float64 PCA / reassembly, float32 MLP)") + f", one solve in {time.perf_counter() - t0:.2f} s"
    sur.close()
    return leg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--inputs", type=int, default=4, help="distinct input grids rotated through (all resident in HBM)")
    ap.add_argument("--no-bind", action="store_true", help="do not bind the geometry: general 8-launch path")
    ap.add_argument("--no-extras", action="store_true", help="skip the end-to-end, case-batch and other legs")
    ap.add_argument("--no-shipped-case", action="store_true", help="skip the shipped_case leg (psm_solve on the reference's 400 x 3000 / 104-block shape)")
    ap.add_argument("--legs", default=",".join(DEFAULT_LEGS), help="comma-separated extra legs at N = 1 (BASELINE configs and conv path); 'none' skips them")
    ap.add_argument("--leg-budget-s", type=float, default=240.0, help="wall-clock budget of the optional legs: legs that would start after it are skipped and say so")
    ap.add_argument("--dry-run", action="store_true", help="launcher / process-group plumbing only (no GPU work)")
    ap.add_argument("--workload", default="config1", choices=sorted(WORKLOADS) + sorted(UNET_WORKLOADS),
                    help="BASELINE.json config to run as the headline (default: configs[1], the one the metric is quoted on)")
    ap.add_argument("--full", action="store_true",
                    help="beside the headline: roofline and per-kernel passes, per-solve quantiles, end-to-end and solver-boundary "
                         "rates, case batch, the other legs, CPU baselines and oracle / golden comparisons (a plain run times the headline only)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write the arrays the last timed step returned (rank 0) as DIR/<name>.npy")
    args = ap.parse_args()
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    # N ranks asked for and no launcher environment: start them ourselves, before this process touches the GPU
    if args.gpus > 1 and "RANK" not in os.environ and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(args.gpus))
    die_with_parent()
    own_stdout()
    if args.dry_run:
        return main_dry(args)
    if args.workload in UNET_WORKLOADS:
        return main_unet(args)

    import numpy as np
    import torch
    hip_up_before = torch.cuda.is_initialized()
    import psm_amd
    from psm_amd import dist as pdist, synthetic
    rank, world, local_rank = pdist.env_world()
    if world != args.gpus:
        raise SystemExit(f"WORLD_SIZE={world} but --gpus {args.gpus}: launch with --nproc-per-node {args.gpus} or without a launcher")
    # Rehearsal switches (not used by the driver): several ranks on ONE card need the gloo backend and a
    # forced device index, e.g. PSM_BENCH_BACKEND=gloo PSM_BENCH_DEVICE=0 python bench.py --gpus 2
    backend = os.environ.get("PSM_BENCH_BACKEND", "nccl")
    shared_card = "PSM_BENCH_DEVICE" in os.environ
    local_rank = int(os.environ.get("PSM_BENCH_DEVICE", local_rank))
    if local_rank >= torch.cuda.device_count():
        raise SystemExit(f"rank {rank}: LOCAL_RANK {local_rank} but only {torch.cuda.device_count()} GPU(s) visible")
    torch.cuda.set_device(local_rank)
    pdist.init(backend, torch.device("cuda", local_rank))
    red_dev = "cuda" if backend == "nccl" else "cpu"
    import torch.distributed as dist
    world_reported = dist.get_world_size() if dist.is_initialized() else 1
    if world_reported != args.gpus:
        raise SystemExit(f"process group reports {world_reported} ranks, --gpus {args.gpus}")
    devices = gather_devices(torch, local_rank, world)
    if world > 1 and not shared_card and len(set(devices)) != world:
        raise SystemExit(f"ranks share a GPU: {devices}")

    variant, NY, NX, NC, precision, wl_desc = WORKLOADS[args.workload]
    # rank 0 builds the artefacts, every other rank receives them over RCCL (one byte broadcast, outside the timed region)
    t_b = time.perf_counter()
    model = synthetic.make_model(variant, p_in=P, p_out=P) if rank == 0 else None
    model = pdist.broadcast_model(model, 0, red_dev)
    broadcast_s = time.perf_counter() - t_b
    sur = psm_amd.GridSurrogate(model, NY, NX, max_cases=NC, device=local_rank, precision=precision)
    # independent cases per rank (different seeds), all resident in HBM before timing
    if NC == 1:
        grids = [synthetic.channel_grid(NY, NX, seed=1 + 1000 * rank + i, noise=0.05 if NY > 256 else 0.02).astype(np.float32)[None]
                 for i in range(args.inputs)]
    else:
        # an ensemble of NC geometries per rank, each advancing in time: the rotated inputs are the same cases with other
        # velocity fields (the SDF channel -- the geometry -- stays)
        base = synthetic.random_obstacle_cases(NC, NY, NX, seed=3 + 1000 * rank).astype(np.float32)
        grids = []
        for i in range(args.inputs):
            g = base.copy()
            g[..., :model.sdf_ch] *= np.float32(1.0 + 0.05 * i)
            grids.append(g)
    d_in = [to_device(torch, g) for g in grids]
    d_out = [torch.empty((NC, NY, NX, model.c_out), dtype=torch.float32, device="cuda") for _ in grids]
    stream = torch.cuda.current_stream().cuda_stream

    # One case stream per GPU = one simulation: its geometry (the flow-cell pattern of the SDF channel) is bound once,
    # outside the timed region, like the reference's computeOnlyOnce / init_func; the rotated inputs differ in the
    # velocity channels only (checked here, and on the device at every solve: guard_trips stays 0).  --no-bind times the
    # general path, which takes any geometry per call.
    bound = False
    if not args.no_bind:
        masks = [g[..., model.sdf_ch] != 0 for g in grids]
        if all(np.array_equal(masks[0], m) for m in masks[1:]):
            bound = sur.bind_geometry(d_in[0].data_ptr(), on_device=True, n_cases=NC)

    def step(i):
        k = i % len(d_in)
        sur.solve_device(d_in[k].data_ptr(), NC, d_out[k].data_ptr(), stream)

    # Before the contract's W warm-up steps and K timed steps, at least 200 untimed solves leave clocks, caches and the runtime's
    # kernel objects warm, so that a short driver run (K = 20) measures the same steady state as the default K = 2000.  With --full
    # that pass is the roofline's instrumented one (every dispatch stamped); a plain run issues up to 2000 of the same solves unstamped.
    if args.full:
        kt_steps = max(args.steps, 200)
        kt_head = time_kernels(sur, d_in[0].data_ptr(), NC, d_out[0].data_ptr(), kt_steps, quantiles=True)
        kt_head = [(nm, us, n * args.steps // kt_steps, q) for nm, us, n, q in kt_head]    # launches per `steps` solves, as pca_roofline counts them
    else:
        for i in range(max(200, min(args.steps, 2000))):
            step(i)
    torch.cuda.synchronize()

    dt_max = pdist.timed_region(step, args.steps, args.warmup, torch.cuda.synchronize, red_dev)
    torch.cuda.synchronize()
    trips = guard_trips_after(sur, args.workload)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"fields": to_host(torch, d_out[(args.steps - 1) % len(d_in)])})    # [NC, NY, NX, c_out]
    value = pdist.aggregate_throughput(NC, args.steps, world, dt_max)
    out = {
        "metric": "pressure-solves/sec (256x256 U->p inference)",
        "value": value, "value_device_resident": value,
        "unit": "solves/s", "n_gpus": world, "world_size_reported": world_reported, "devices": devices,
        "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": dt_max / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": precision, "data": "synthetic",
        "config": {"workload": wl_desc,
                   "grid": [NY, NX], "blocks": sur.B, "p_in": P, "p_out": P, "cases_per_step_per_gpu": NC,
                   "parallelism": f"case-sharded x{world} (no data-path collective; model broadcast from rank 0 over "
                                  f"{'RCCL' if backend == 'nccl' else backend} before the timed region: {broadcast_s * 1e3:.0f} ms)",
                   "value_is": "device-resident rate: the input grid is already in HBM when the timed region starts and the "
                               "field stays in HBM (the bench contract: the PCIe-inclusive rate is never `value`); the solve of "
                               "SURVEY section 8(d) / BASELINE.md:4 -- host grid in, host field out, H2D and D2H included -- is "
                               "value_end_to_end on the --full line",
                   "degenerate": degenerate_note(variant, NY, NX),
                   "geometry": ("bound once per case stream (psm_bind_geometry = the reference's computeOnlyOnce / init_func split): "
                                "6 launches per solve, 7 for case batches; the contract is checked on the device at every solve") if bound
                               else "general path (any geometry per call): 8 launches per solve (9 for case batches)",
                   "guard_trips": trips},
    }
    if not args.full:
        if rank == 0:
            emit_result(out)
        sur.close()
        finish()
        return

    got_dev = to_host(torch, d_out[0])
    roofline = pca_roofline(sur, model, NY, NX, NC, precision, d_in[0].data_ptr(), d_out[0].data_ptr(), args.steps, dt_max / args.steps,
                            args.workload, bound, kt=kt_head)
    # BASELINE.md section 2's protocol beside the contract's K-step mean: >= 200 timed samples, median and 10th / 90th percentile.
    # A sample = the DEVICE time between two events recorded Q_CHUNK solves apart on the solve stream, per solve; the stream is
    # never drained between samples, so the samples are the steady state `value` averages over.  (Two other forms were tried and
    # dropped: an event pair around every single solve makes the pass host-bound -- 31 us of submission per solve; wall-clocked
    # chunks between device synchronisations restart from an idle GPU every 1.6 ms and read 5-20 % slow depending on how fast the
    # box drops its clocks: 32.4-39.8 us per solve between boxes for the same build.)
    n_q = 20 if args.no_extras else 200                      # (profiling passes run with --no-extras: keep their traces small)
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(n_q + 1)]
    q_stream = torch.cuda.Stream()                           # (stream 0 of `step` means "the handle's own stream", which torch cannot record on)
    def step_q(i):
        k = i % len(d_in)
        sur.solve_device(d_in[k].data_ptr(), NC, d_out[k].data_ptr(), q_stream.cuda_stream)
    torch.cuda.synchronize()
    for j in range(Q_CHUNK):                                 # a filled pipeline in front of the first event
        step_q(j)
    evs[0].record(q_stream)
    for i in range(n_q):
        for j in range(Q_CHUNK):
            step_q(i * Q_CHUNK + j)
        evs[i + 1].record(q_stream)
    torch.cuda.synchronize()
    per_ms = [evs[i].elapsed_time(evs[i + 1]) / Q_CHUNK for i in range(n_q)]
    per_ms.sort()
    q_ms = {"p50": per_ms[n_q // 2], "p10": per_ms[n_q // 10], "p90": per_ms[(n_q * 9) // 10]}

    out.update({
        # rates at the median / 90th / 10th percentile of the per-solve time of n_q event-separated samples on this rank (x world: case-
        # sharded, no collective): value_p10 is computed from ms_p90, the SLOW decile of the times (the low rate), value_p90 from ms_p10
        "value_p50": NC * world / (q_ms["p50"] * 1e-3), "value_p10": NC * world / (q_ms["p90"] * 1e-3), "value_p90": NC * world / (q_ms["p10"] * 1e-3),
        "per_solve_quantiles": {"solves": n_q * Q_CHUNK, "samples": n_q, "solves_per_sample": Q_CHUNK, "ms_p50": q_ms["p50"], "ms_p10": q_ms["p10"], "ms_p90": q_ms["p90"],
                                "what": "a sample = device time between two events recorded solves_per_sample solves apart on a stream that is never "
                                        "drained, per solve; value_p10 / value_p90 = rate at the slow / fast decile of the times"},
        "frac_pass": roofline["whole_solve"]["frac"],
        # a timed region starts on a drained stream (the contract's synchronise): its first solve waits for the host's first launches
        # (~25 us of pipeline fill).  At K = 2000 that is 0.04 % of the region, at the driver's K = 20 it is 3-4 %: the round-4 driver line
        # (27.8 k) against the builder's K = 2000 lines (29.2 k) on equal boxes; value_p50 (chunks of 50) sits between the two.
        "pipeline_fill_note": f"K={args.steps}: one fill of ~25 us = {25.0 / (dt_max / args.steps * 1e6 * args.steps) * 100:.1f} % of the timed region",
        "roofline": roofline,
    })
    out["config"]["arithmetic"] = arithmetic_note(precision, roofline["kernels"])

    # ---- one solve = host grid in, host field out (H2D + D2H included)
    if not args.no_extras:
        n_e2e = max(200, min(args.steps, 3000))
        modes = [(2, 4)] if world > 1 else [(0, 1), (1, 4), (2, 1), (2, 2), (2, 4), (3, 4)]
        pdist.barrier(torch.cuda.synchronize)
        wu_e2e = min(args.warmup, 100)
        rates = host_rates(sur, grids, NC, n_e2e, wu_e2e, modes)
        key = "ring_registered_depth4"
        last_in = (wu_e2e + n_e2e - 1) % len(grids)                          # input of the last end-to-end solve
        slow = pdist.max_over_ranks(1.0 / rates[key][0], red_dev)            # slowest rank bounds the job
        out["value_end_to_end"] = world * 1.0 / slow
        out["end_to_end"] = {
            "what": "host buffers in, host buffers out: H2D of the grid and D2H of the field included (SURVEY section 8(d)); "
                    "C++ loop inside the library through the public C-ABI (psm_bench_host); ring slots with their own "
                    "stream and scratch: DMA copy in, one hipGraph replay of the kernels, DMA copy out per ticket",
            "value_is": key + " (psm_submit_grid_io / psm_wait_grid on caller-registered memory, 4 tickets in flight)",
            "hw_queues": {"GPU_MAX_HW_QUEUES": os.environ.get("GPU_MAX_HW_QUEUES"), "set_by": "the caller's environment" if _HWQ_PRESET else "bench.py (the library never sets it)",
                          "hip_initialised_before_it_was_set": bool(hip_up_before)},
            "steps": n_e2e, "solves_per_s_per_rank": {k: v[0] for k, v in rates.items()},
            "matches_device_resident_result": bool(np.array_equal(rates[key][1], to_host(torch, d_out[last_in])))}

    # ---- the solver boundary (psm_solve = py_func of PythonComm.H: cells[N,5] float64 in, p[N] float64 out), registered buffers
    if not args.no_extras and world == 1 and args.workload == "config1" and "end_to_end" in out:
        try:
            out["end_to_end"]["psm_solve"] = solver_boundary_leg(synthetic, local_rank, max(200, min(args.steps, 2000)))
        except Exception as e:                                # reported, not fatal for the headline
            out["end_to_end"]["psm_solve"] = {"error": repr(e)[:200]}

    # ---- independent batch-1 case streams on the one card (N = 1 default run only; never the headline)
    if not args.no_extras and world == 1 and args.workload == "config1" and not args.no_bind:
        try:
            out["case_streams"] = case_streams_leg(torch, psm_amd, synthetic, model, NY, NX, precision, local_rank, 4, max(1000, min(args.steps, 4000)))
        except Exception as e:                                # reported, not fatal for the headline
            out["case_streams"] = {"error": repr(e)[:200]}

    # ---- the reference's deployment shape in its own unit (ms per call), N = 1 default run only
    if not args.no_extras and world == 1 and args.workload == "config1" and not args.no_shipped_case:
        try:
            out["shipped_case"] = shipped_case_leg(synthetic, local_rank, 200, rank == 0 and not args.no_cpu_baseline)
        except Exception as e:                                # reported, not fatal for the headline
            out["shipped_case"] = {"error": repr(e)[:200]}

    # ---- parity against the reference-run golden vectors (non-degenerate grids), on the line beside l2_vs_oracle
    if not args.no_extras and rank == 0 and world == 1 and args.workload == "config1" and not args.no_cpu_baseline:
        try:
            out["l2_vs_reference_goldens"] = golden_parity(psm_amd, local_rank)
        except Exception as e:                                # fixtures not shipped with this copy: reported, not fatal
            out["l2_vs_reference_goldens"] = {"error": repr(e)[:200]}

    # ---- BASELINE configs[3]: the case batch, 8 random-obstacle cases per GPU per step
    m3 = None
    if not args.no_extras and args.workload == "config1":
        v3, ny3, nx3, nc3, prec3, desc3 = WORKLOADS["config3"]
        m3 = synthetic.make_model(v3, p_in=P, p_out=P) if rank == 0 else None
        m3 = pdist.broadcast_model(m3, 0, red_dev)
        total_cases = nc3 * world
        first, count = pdist.shard_cases(total_cases, world, rank)           # contiguous shard of the case batch
        allc = synthetic.random_obstacle_cases(count, ny3, nx3, seed=3 + 1000 * rank).astype(np.float32)
        sur3 = psm_amd.GridSurrogate(m3, ny3, nx3, max_cases=count, device=local_rank, precision=prec3)
        g3 = []
        for i in range(args.inputs):
            g = allc.copy()
            g[..., :m3.sdf_ch] *= np.float32(1.0 + 0.05 * i)
            g3.append(to_device(torch, g))
        o3 = [torch.empty((count, ny3, nx3, m3.c_out), dtype=torch.float32, device="cuda") for _ in g3]
        b3 = sur3.bind_geometry(g3[0].data_ptr(), on_device=True, n_cases=count) if not args.no_bind else False

        def step3(i):
            k = i % len(g3)
            sur3.solve_device(g3[k].data_ptr(), count, o3[k].data_ptr(), stream)
        k3 = max(300, args.steps // 4)                     # (legs are not under the K contract: long enough that one pipeline fill is < 1 % of the region)
        dt3 = pdist.timed_region(step3, k3, max(10, args.warmup // 4), torch.cuda.synchronize, red_dev)
        torch.cuda.synchronize()
        trips3 = guard_trips_after(sur3, "config3")
        whole = pdist.gather_cases(o3[0] if red_dev == "cuda" else torch.from_numpy(to_host(torch, o3[0])), total_cases)     # one all-gather, untimed
        out["case_batch"] = {"workload": desc3, "value": total_cases * k3 / dt3, "unit": "solves/s", "steps": k3,
                             "ms_per_step": dt3 / k3 * 1e3, "dtype": prec3, "cases_per_step_per_gpu": count, "total_cases": total_cases,
                             "geometry": "one bound geometry per case slot (6 launches per step up to 128 block rows, 7 beyond)" if b3 else "general path (8-9 launches per step)",
                             "guard_trips": trips3, "gathered_shape": list(whole.shape),
                             "roofline": pca_roofline(sur3, m3, ny3, nx3, count, prec3, g3[0].data_ptr(), o3[0].data_ptr(), k3, dt3 / k3, "config3", bool(b3))}
        if rank == 0 and world == 1 and not args.no_cpu_baseline:
            from oracle import psm_oracle as orc
            c = count - 1
            ref = orc.solve_grid(allc[c].astype(np.float64), oracle_model(m3)).fields
            gotc = to_host(torch, o3[0][c])
            out["case_batch"]["l2_vs_oracle"] = float(np.linalg.norm(gotc - ref) / np.linalg.norm(ref))
        sur3.close()
        # the whole batch of configs[3] -- 64 cases -- per step on ONE GPU (N = 1 only): what a single card does with the batch the
        # eight-GPU job shards; same protocol, fewer steps (asked for by round 3's verdict; detail file + one number on the line)
        if world == 1 and not args.no_bind:
            try:
                n64 = 64
                all64 = synthetic.random_obstacle_cases(n64, ny3, nx3, seed=3).astype(np.float32)
                sur64 = psm_amd.GridSurrogate(m3, ny3, nx3, max_cases=n64, device=local_rank, precision=prec3)
                g64 = to_device(torch, all64)
                o64 = torch.empty((n64, ny3, nx3, m3.c_out), dtype=torch.float32, device="cuda")
                b64 = sur64.bind_geometry(g64.data_ptr(), on_device=True, n_cases=n64)
                k64 = max(300, min(400, args.steps // 10))       # (40 untimed steps first: with 10 the leg read 7-8 % under the back-to-back rate of tools/kernel_times.py -- clocks and caches still settling)
                dt64 = pdist.timed_region(lambda i: sur64.solve_device(g64.data_ptr(), n64, o64.data_ptr(), stream), k64, 40,
                                          torch.cuda.synchronize, red_dev)
                torch.cuda.synchronize()
                trips64 = guard_trips_after(sur64, "config3 x64")
                out["case_batch"]["all_64_cases_on_one_gpu"] = {
                    "value": n64 * k64 / dt64, "unit": "solves/s", "ms_per_step": dt64 / k64 * 1e3, "steps": k64, "cases_per_step": n64,
                    "geometry": "one bound geometry per case slot" if b64 else "general path", "guard_trips": trips64,
                    "finite": bool(torch.isfinite(o64).all().item())}
                sur64.close()
                del g64, o64
            except Exception as e:                            # reported, not fatal for the headline
                out["case_batch"]["all_64_cases_on_one_gpu"] = {"error": repr(e)[:200]}

    # ---- the other BASELINE configs and the convolutional path (N = 1): same protocol, smaller K
    legs = [] if (args.no_extras or world > 1 or args.workload != "config1" or args.legs in ("", "none")) else [l for l in args.legs.split(",") if l]
    if legs:
        out["legs"] = {}
        k_leg, w_leg = max(300, args.steps // 4), max(20, args.warmup // 4)
        with_oracle = rank == 0 and not args.no_cpu_baseline
        t_legs = time.perf_counter()
        for name in legs:
            t0 = time.perf_counter()
            if t0 - t_legs > args.leg_budget_s:                      # a slow box must not cost the driver its line: the rest is skipped, loudly
                out["legs"][name] = {"skipped": f"leg budget of {args.leg_budget_s:.0f} s spent"}
                continue
            if name in WORKLOADS:
                if m3 is None:
                    m3 = synthetic.make_model("deltas", p_in=P, p_out=P)
                mdl = m3 if WORKLOADS[name][0] == "deltas" else model
                leg = pca_leg(name, mdl, args, torch, pdist, psm_amd, synthetic, rank, world, local_rank, red_dev, k_leg, w_leg, with_oracle)
            elif name in UNET_WORKLOADS:
                big = UNET_WORKLOADS[name][2] > 8                    # 64 cases: 0.8 ms per step; the CPU oracle is timed by the other legs
                # 400 timed steps behind 100 untimed ones (64 cases: 100 behind 30): with 100-200 behind 25 the bf16 legs read 2 % above the same workload run on its
                # own (K = 2000) on the same box -- clocks still settling behind the plan-time autotune, as for the 64-case PCA leg above
                ku, wu = (100, 30) if big else (max(100, min(k_leg, 400)), max(100, w_leg // 2))
                leg = unet_leg(name, args, torch, pdist, rank, world, local_rank, backend, ku, wu, with_oracle,
                               cpu_budget_s=0.0 if big else 4.0)
            else:
                raise SystemExit(f"unknown leg {name!r}")
            leg["leg_wall_s"] = time.perf_counter() - t0
            out["legs"][name] = leg

    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        cb, sol = cpu_baseline(model, grids[0][0], precision)
        out["cpu_baseline"] = cb
        ref = sol.fields
        out["l2_vs_oracle"] = float(np.linalg.norm(got_dev[0] - ref) / np.linalg.norm(ref))
        out["gpu_over_cpu"] = out["value"] / cb["value"]
    if rank == 0:
        emit_result(out)
    sur.close()
    finish()


if __name__ == "__main__":
    main()
