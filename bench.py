"""bench.py — HR frames/s of the PFNL forward hot path on N MI355X GPUs (one process per GPU).

    python bench.py [--gpus N] [--steps K] [--warmup W]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W
    python bench.py ... --dump-outputs DIR      # + the last timed step's SR frames as DIR/<name>.npy (float32)
    python bench.py ... --full                  # + everything below that takes runs of its own

Workload = BASELINE.json configs[1]: PFNL 4xSR, 7 LR frames 128x128 -> one 512x512 HR frame per clip,
batch 4 clips per GPU, fp32, synthetic U[0,1) clips and seeded Xavier weights (no checkpoint/dataset
can be fetched).  A "step" = one pfnl_forward over the rank's batch with the input already resident in
HBM.  Clips are independent, so ranks share nothing on the data path (weak scaling: 4 clips per GPU);
RCCL carries the weight replica (pfnl_comm_bcast_weights), the barriers and the max-over-ranks time only.

A plain run sets up, warms up, times the K steps, writes --dump-outputs and prints ONE JSON line (rank 0) with the contract fields plus
`roofline` (it rides in the timed steps).  `--full` adds what costs runs of its own: the per-class breakdown pass (`roofline_nl`,
`roofline_hbm_classes`, the whole of `kernel_ms_per_step`; the small shapes' `roofline`), `sustained`, `secondary` and `cpu_baseline`.
  roofline      dominant kernel class (the 3x3 64->64 convolutions), timed live with HIP events on the launch stream INSIDE the timed
                steps (the launches of one of the 20 identical progressive-fusion blocks: 3 events per forward; the per-class
                breakdown of the whole forward comes from a separate untimed pass: --full);
                frac = ALGORITHMIC work (bytes or FLOPs the reference graph needs, shared-base split) / time / the binding peak;
                what the kernel executes on the matrix pipe (3 f16 MFMAs per product block) is in mfma_executed_*, next to the
                ceiling the chip sustains on that instruction stream under its power cap (tools/ubench/conv_core)
  sustained     (--full) >= 2 s of back-to-back steps (no events): ms/step, so clock droop is visible
  secondary     (--full) measured in the same process after the headline: configs[3] (1080p bf16), one Vid4 window, configs[0], configs[4]
                (2x, T=5, 64x64) and the HOST-pointer configs[1] path (H2D + D2H inside, what the reference's
                sess.run timing covers, model/pfnl.py:249-253)
  cpu_baseline  (--full, N=1) the torch-CPU fp32 oracle = the stand-in for the reference's TF1 CPU path, on a bounded sample.
"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_F32_MFMA_TFLOPS = 157.3      # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense, no xf32 on gfx950
PEAK_F16_MFMA_TFLOPS = 2500.0     # dense bf16 / f16 MFMA (no sparsity)
PEAK_HBM_GBS = 8000.0
# what 256 CUs sustain on the split-f16 kernels' own MFMA + LDS-operand core with random operands, nothing else running:
# 1.27 - 1.52 PFLOP/s at a 1.33 - 1.57 GHz shader clock (power cap; tools/ubench/conv_core.hip, profiles/r03_ubench_conv_core.txt)
SUSTAINED_F16_MFMA_TFLOPS = 1500.0
# what 256 CUs move when one 512-thread workgroup per CU (the launches' residency) does NOTHING but a tile's byte streams - halo by LDS-DMA,
# residual lines, output lines: 5.5 - 5.8 TB/s of compulsory bytes, ~11 B per clock and CU (tools/ubench/cu_stream_mix.hip,
# profiles/r04_ubench_cu_stream_mix.txt).  Context next to `frac` (which is priced on the 8 TB/s spec), not a substitute for it.
STREAM_MIX_CEILING_GBS = 5600.0
# the package power cap as a roofline (tools/ubench/energy_mix.hip, profiles/r06_ubench_energy_mix.txt): a launch that runs f16 MFMAs on data-like
# operands next to an HBM stream takes t = a F + b B - the matrix pipe alone sustains 1 / a = 1.67 - 1.74 PFLOP/s at 1.7 GHz under the 1 400 W
# cap, and every HBM byte costs the time of ~210 MFMA FLOPs on top (NOT max(t_mfma, t_bytes): at the trunk's mixes that would be 1.4 - 1.6x less)
POWER_CAP_MS_PER_TFLOP = 0.587
POWER_CAP_MS_PER_TFLOP_16 = 0.49                                    # the same for v_mfma_f32_16x16x32_* (2 030 - 2 060 TFLOP/s back to back: tools/ubench/mfma_shape_power.hip)
POWER_CAP_US_PER_GB = 123.0
CU_PORT_B_PER_CLK = 11.2                                           # what a CU's memory port moved per shader clock with nothing else to do (ibid.)
PREWARM_S = 0.3                                                    # untimed steps in front of the warm-up: the clock ramp of an idle chip
T = 7

# BASELINE.json configs, as `--workload`.  clips = per GPU under weak scaling (the config's own batch); strong = the fixed global
# batch of `--strong` (configs[2]: 32 clips over 8 GPUs; the others: 8 x their batch so that 8 ranks still hold a clip each)
WORKLOADS = {
    "cfg2": {"clips": 4, "H": 128, "W": 128, "T": 7, "scale": 4, "strong": 32, "config": "configs[1]",
             "label": "PFNL 4xSR, 7 frames, 128x128->512x512, batch=%d %s per MI355X (BASELINE.json configs[1]%s)"},
    "cfg0": {"clips": 1, "H": 32, "W": 32, "T": 7, "scale": 4, "strong": 8, "config": "configs[0]",
             "label": "PFNL 4xSR, 7 frames, 32x32->128x128, batch=%d %s per MI355X (BASELINE.json configs[0]%s)"},
    "cfg4": {"clips": 1, "H": 270, "W": 480, "T": 7, "scale": 4, "strong": 8, "config": "configs[3]",
             "label": "PFNL 4xSR, 7 frames, 270x480->1080x1920 (1080p), batch=%d %s per MI355X (BASELINE.json configs[3]%s)"},
    "cfg5": {"clips": 1, "H": 64, "W": 64, "T": 5, "scale": 2, "strong": 8, "config": "configs[4]",
             "label": "PFNL 2xSR, 5 frames, 64x64->128x128, batch=%d %s per MI355X (BASELINE.json configs[4]%s)"},
}

CONV3X3_KERNELS = {
    "winograd": ("conv_wino_ws_kernel<*> (fused Winograd F(2x2,3x3) 64->64, f32 MFMA, persistent wave-specialised)",
                 ["conv_wino_ws.hip", "wino_geom.h"]),
    "winograd_tile": ("conv_wino_kernel<*> (fused Winograd F(2x2,3x3) 64->64, f32 MFMA, one workgroup per tile)",
                      ["conv_wino.hip", "wino_geom.h"]),
    "direct": ("conv_mfma_kernel<3,16,*> (3x3 64->64 f32 MFMA implicit GEMM)", ["conv_mfma.hip"]),
    "split16": ("conv3x3_c1c10_kernel (conv1_i + conv10_i in one launch: the frame tiles leave as split-format lines through LDS, where conv10_i takes them "
                "as MFMA operands) + conv3x3_sf_chain16_kernel / conv3x3_sf_chain_kernel (the whole of conv2_i on v_mfma_f32_16x16x32_f16 / 32x32x16 - pfnl_plan mfma: split-format input and weights by LDS-DMA, shared half "
                "in registers): direct 3x3 64->64 on f16 MFMA with exactly split fp32 operands, 3 MFMAs per product block, fp32 accumulation",
                ["conv_split16.hip", "conv_sf.hip"]),
    "small": ("conv_small_kernel<3,R> (small-shape trunk: conv1_i and the whole of conv2_i, 4 waves per R x 32-pixel tile, split-f16 MFMA, weights "
              "streamed as B operands)", ["conv_small.hip"]),
    "bf16": ("conv3x3_bf16_v3_kernel<2 / 1> (conv1_i + conv10_i, the per-frame half of conv2_i: halo by LDS-DMA, the two halves of the workgroup "
             "half a tile period apart) + conv3x3_bf16_v2_kernel<0> (the shared half of conv2_i): direct 3x3 64->64, bf16 MFMA, fp32 "
             "accumulation, persistent", ["conv_bf16.hip", "conv_bf16_v2.hip", "conv_bf16_v3.hip"]),
}


def power_cap_model(executed_flops, moved_bytes, avg_ms, share16=0.0):
    """What a launch with this many executed MFMA FLOPs and HBM bytes takes on the power cap according to the micro-benchmark's fit (no LDS
    operand reads, no VALU, no launch ramp: a floor), next to what it took.  share16: the part of the FLOPs issued as v_mfma_f32_16x16x32_*
    (pfnl_plan mfma=16: the bf16 trunk's chained launches; the fp32 chain launch of conv2_i), which cost 14 % less."""
    a = POWER_CAP_MS_PER_TFLOP * (1.0 - share16) + POWER_CAP_MS_PER_TFLOP_16 * share16
    t = a * executed_flops / 1e12 + POWER_CAP_US_PER_GB * 1e-3 * moved_bytes / 1e9
    return {"model_ms_per_launch": round(t, 4), "measured_ms_per_launch": round(avg_ms, 4), "model_over_measured": round(t / avg_ms, 4),
            "ms_per_tflop": round(a, 4), "us_per_gb": POWER_CAP_US_PER_GB, "flop_share_on_16x16x32": round(share16, 3),
            "note": "t = a F + b B under the 1 400 W package cap, a and b measured by tools/ubench/energy_mix.hip (profiles/r06_ubench_energy_mix.txt): "
                    "MFMAs on data-like operands + an HBM stream, nothing else; model_over_measured near 1 = the launch is at the chip's power roofline"}


def kernel_source_sha(files):
    """sha256 over the sources of a kernel: `roofline.traffic` (PMC bytes measured offline) is only reported while the
    kernel it was measured on is the kernel that is being timed."""
    h = hashlib.sha256()
    for f in files:
        with open(os.path.join(ROOT, "pfnl_amd", "csrc", f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


class PowerSampler:
    """`rocm-smi --showpower --showclocks --showmaxpower` polled on a thread while the sustained steps run: the split-f16 kernels are
    bound by the package power cap, so the line carries what the chip drew and the clock it settled at.  Best effort:
    no rocm-smi, nothing reported."""

    def __init__(self, device):
        import threading
        self.samples, self.cap, self._stop = [], None, threading.Event()
        self.device = int(device)
        self._t = threading.Thread(target=self._run, daemon=True)
        self._t.start()

    def _run(self):
        import re
        import shutil
        import subprocess
        exe = shutil.which("rocm-smi") or "/opt/rocm/bin/rocm-smi"
        while not self._stop.is_set():
            try:
                out = subprocess.run([exe, "-d", str(self.device), "--showpower", "--showclocks", "--showmaxpower"], capture_output=True,
                                     text=True, timeout=10).stdout
            except Exception:
                return
            pw = re.search(r"(?:Current Socket|Average) Graphics Package Power \(W\): ([0-9.]+)", out)
            ck = re.search(r"sclk clock level: \S+ \(([0-9]+)Mhz\)", out)
            cap = re.search(r"Max Graphics Package Power \(W\): ([0-9.]+)", out)
            if cap:
                self.cap = float(cap.group(1))
            if pw and ck and not self._stop.is_set():
                self.samples.append((float(pw.group(1)), int(ck.group(1))))

    def stop(self):
        self._stop.set()
        self._t.join(timeout=15)
        s = [x for x in self.samples if x[0] > 0]
        if not s:
            return None
        top = max(x[0] for x in s)
        s = [x for x in s if x[0] >= 0.7 * top]                         # (a sample taken before the first step landed reads idle power)
        return {"package_w": round(sum(x[0] for x in s) / len(s), 1), "package_w_max": max(x[0] for x in s), "cap_w": self.cap,
                "sclk_mhz": round(sum(x[1] for x in s) / len(s)), "samples": len(s),
                "source": "rocm-smi polled during the sustained run (the first samples may precede it)"}


def cpu_baseline(weights, sample_clips, H, W, budget_s=20.0):
    """Times oracle/pfnl_fast.py (the CPU port of the reference graph) on this host: SURVEY.md 8(d).  A BOUNDED sample (~20 s): the thread
    count that is best on most hosts (16) runs the GPU line's whole batch - 1 warm-up + max-fps of 3 runs, mirroring model/pfnl.py:262 -,
    n = 8 and all physical cores (BASELINE.md asks for both) run the batch's first clip twice after a warm-up; `clips_timed` and
    `runs_per_thread_count` say what each figure is."""
    import numpy as np
    import torch
    from oracle import pfnl_fast
    t_begin = time.time()

    def run(threads, sample, runs, deadline):
        torch.set_num_threads(threads)
        fo = pfnl_fast.FastOracle(weights)
        fo.forward(sample_clips[:1])                  # warm-up, discarded (reference model/pfnl.py:262)
        fps = []
        while len(fps) < runs:
            t0 = time.time()
            fo.forward(sample)
            dt = time.time() - t0
            fps.append(sample.shape[0] / dt)
            if time.time() > deadline and len(fps) >= 1:     # a host slower than expected: what has been measured is reported
                break
            if dt > 4.0 and sample.shape[0] > 1:
                sample = sample_clips[:1]
        return max(fps), float(np.mean(fps)), len(fps), int(sample.shape[0])

    ncpu = os.cpu_count() or 1
    phys = physical_cores() or ncpu
    default_thr = torch.get_num_threads()
    cands = sorted({c for c in (8, 16, phys) if 1 <= c <= max(ncpu, 1)})   # n = 8 and all physical cores (+ 16: the best on most hosts)
    primary = 16 if 16 in cands else cands[0]
    results = {primary: run(primary, sample_clips, 3, t_begin + 0.6 * budget_s)}
    others = [c for c in cands if c != primary]
    for i, c in enumerate(others):                    # oversubscription hurts oneDNN: report the best
        results[c] = run(c, sample_clips[:1], 2, t_begin + budget_s * (0.6 + 0.4 * (i + 1) / len(others)))
    torch.set_num_threads(default_thr)
    best = max(results, key=lambda c: results[c][0])
    return {"value": round(results[best][0], 4), "unit": "HR frames/s", "cores": best, "kind": "port",
            "sample": "oracle/pfnl_fast.py (torch-CPU, oneDNN) on 7x%dx%d->%dx%d fp32 clips of the GPU line's batch: %d threads run all %d clips "
                      "(1 warm-up + max of 3 runs), the other thread counts the first clip (1 warm-up + max of 2 runs); best thread count "
                      "reported, n = 8 and all physical cores in by_threads; bounded to ~%d s" % (H, W, 4 * H, 4 * W, primary, sample_clips.shape[0], int(budget_s)),
            "threads_used": best, "host_physical_cores": phys,
            "mean_value": round(results[best][1], 4), "host_logical_cpus": ncpu,
            "value_8_threads": round(results[8][0], 4) if 8 in results else None,
            "value_all_physical_cores": round(results[phys][0], 4) if phys in results else None,
            "runs_per_thread_count": {str(c): v[2] for c, v in results.items()},
            "clips_timed": {str(c): v[3] for c, v in results.items()},
            "by_threads": {str(c): round(v[0], 4) for c, v in results.items()},
            "elapsed_s": round(time.time() - t_begin, 1)}


def physical_cores():
    """(socket, core) pairs of /proc/cpuinfo; None when it cannot be read."""
    try:
        pairs, phys, core = set(), None, None
        for ln in open("/proc/cpuinfo"):
            if ln.startswith("physical id"):
                phys = ln.split(":")[1].strip()
            elif ln.startswith("core id"):
                core = ln.split(":")[1].strip()
            elif not ln.strip():
                if phys is not None and core is not None:
                    pairs.add((phys, core))
                phys = core = None
        return len(pairs) or None
    except OSError:
        return None


class stdout_to_stderr:
    """RCCL prints a version banner on stdout when a communicator is created; the contract is ONE JSON line there."""
    def __enter__(self):
        sys.stdout.flush()
        self._saved = os.dup(1)
        os.dup2(2, 1)

    def __exit__(self, *exc):
        sys.stdout.flush()
        os.dup2(self._saved, 1)
        os.close(self._saved)


def blocks_sampled(nb):
    """PF blocks that carry events in sampled profiling (pfnl_amd/csrc/capi.hip, prof_sampled): blocks 3, 13, ... from ten blocks
    up, every 4th below."""
    return len([i for i in range(nb) if (i % 10 == 3 if nb >= 10 else i % 4 == 0)]) or 1


DUMP_LIMIT_BYTES = 64 << 20                                        # --dump-outputs: all ranks' files together


def dump_output(out, dump_dir, name, budget):
    """Writes the forward's output [B,1,sH,sW,3] (float32) as dump_dir/<name>.npy.  An output larger than `budget` bytes is cut
    to a fixed, seeded choice of whole clips (in clip order); the record says which clips were kept."""
    import numpy as np
    a = out.detach().float().cpu().numpy()
    per_clip = a[0].nbytes if a.shape[0] else 1
    keep = list(range(a.shape[0]))
    if a.nbytes > budget:
        n = max(1, int(budget // per_clip))
        keep = sorted(np.random.default_rng(0).choice(a.shape[0], size=n, replace=False).tolist())
        a = a[keep]
        if a.nbytes > budget:                                          # one clip alone is over the budget: a seeded sample of its values
            flat = a.reshape(-1)
            idx = np.sort(np.random.default_rng(0).choice(flat.size, size=int(budget // 4), replace=False))
            a = flat[idx]
    os.makedirs(dump_dir, exist_ok=True)
    np.save(os.path.join(dump_dir, name + ".npy"), np.ascontiguousarray(a, dtype=np.float32))
    return {"file": name + ".npy", "shape": list(a.shape), "dtype": "float32", "full_shape": list(out.shape), "clips": keep}


def timed_steps(step, fence, steps):
    fence()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    fence()
    return time.perf_counter() - t0


def conv3x3_roofline(geom, prof, B, H, W, plan, workload):
    """`roofline` of the dominant kernel class from the live HIP-event timing (k = prof["conv3x3"]).  `plan` = PFNLEngine.plan(B, H, W)
    (pfnl_plan): the launch structure that ran - structure name, launches per block, c10_fused / chain / sf0 - is READ there, not re-derived."""
    k = prof["conv3x3"]
    if not k["launches"]:
        return None
    bf16 = plan.get("precision") == "bf16"
    algo = plan_algo(plan)
    P, F = H * W, B * geom.num_frames
    avg_ms = k["ms"] / k["launches"]                                   # over the launches that were timed
    flops3 = geom.num_block * (2 * F + B) * P * 9 * 64 * 64 * 2.0      # direct-convolution FLOPs, shared-base split
    if bf16:
        # bf16 trunk: the 3x3 launches are bound by HBM, not by the matrix pipe: algorithmic bytes
        # per PF block of the IMPLEMENTED launch structure = conv1_i + conv10_i in one launch (read F, write F + B tiles of 128 B per
        # pixel) + shared half (read B, write B) + per-frame half (read F + residual F + addend B, write F), over 3 launches
        launches_per_step = 3 * geom.num_block                              # (conv10_i as its own launch - bf16_4 / bf16_mid4 - is the conv1x1 class)
        bytes_per_launch = P * 128.0 * (5 * F + 4 * B) / 3.0
        gbs = bytes_per_launch / (avg_ms * 1e-3) / 1e9
        name, files = CONV3X3_KERNELS["bf16"]
        traffic = stamped_traffic("traffic_bf16.json", files, workload)
        return {"bound": "hbm", "achieved": round(gbs, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": round(gbs / PEAK_HBM_GBS, 4),
                "traffic": traffic, "kernel": name, "avg_launch_ms": round(avg_ms, 4), "launches_timed": k["launches"],
                "launches_per_step": launches_per_step, "mbytes_per_launch": round(bytes_per_launch / 1e6, 2), "tiles_per_block": "5F+4B",
                "stream_mix_ceiling_gbs": STREAM_MIX_CEILING_GBS, "hbm_vs_stream_mix_ceiling": round(gbs / STREAM_MIX_CEILING_GBS, 4),
                "mfma_tflops": round(flops3 / launches_per_step / (avg_ms * 1e-3) / 1e12, 1), "mfma_peak_bf16_tflops": PEAK_F16_MFMA_TFLOPS,
                "power_cap_model": power_cap_model((flops3 + geom.num_block * F * P * 64 * 64 * 2.0) / launches_per_step, bytes_per_launch, avg_ms,
                                                   share16=(2.0 * F / (2.0 * F + B)) * flops3 / (flops3 + geom.num_block * F * P * 64 * 64 * 2.0) if plan.get("mfma") == 16 else 0.0)}
    # fp32: conv1_i + conv2_i; the default kernel runs the whole of conv2_i as one grouped launch, the others launch its
    # shared half and its per-frame half separately
    # launches of the class per PF block: 2 with conv2_i as one launch (Winograd's grouped mode; the split-f16 chain kernel), else 3
    chain, c10, sf0 = bool(plan.get("chain")), bool(plan.get("c10_fused")), bool(plan.get("sf0"))
    # launches of THIS class per block: the plan's, minus conv10_i's own launch (class conv1x1) where it is not fused into conv1_i's
    c1x1 = plan["c1x1"] if "c1x1" in plan else (0 if (c10 or plan["structure"].startswith("small2")) else 1)
    launches_per_step = (plan["launches_per_block"] - c1x1) * geom.num_block
    # conv10_i rides in the conv1_i launch of the default path (conv3x3_c1c10_kernel): its work belongs to this class then
    if c10:
        flops3 += geom.num_block * F * P * 64 * 64 * 2.0
    flops_per_launch = flops3 / launches_per_step
    direct_tflops = flops_per_launch / (avg_ms * 1e-3) / 1e12
    if algo == "split16":
        # fp32 tensors in HBM (256 B per pixel), 3 f16 MFMAs per product block: between the f16 matrix roof (3x the direct
        # FLOPs against 2.5 PFLOP/s) and the HBM roof (conv1_i: read F + write F; shared half: read B + write B; per-frame
        # half: read F + addend B + residual F, write F - over 3 launches) - both fractions are reported, the larger binds
        name, files = CONV3X3_KERNELS[algo]
        # ALGORITHMIC bytes of the fusion level that is IMPLEMENTED: what the launches of this class must move when
        # each reads its inputs once and writes its outputs once, in tiles of P x 256 B (F frame tiles, B clip tiles per block):
        #   conv1_i alone            read F, write F                          conv1_i + conv10_i (one launch)  read F, write F + B
        #   conv2_i as a chain       read F (inp1) + B (base) + F (residual), write F
        #   conv2_i as two launches  shared half: read B, write B (pb);  per-frame half: read F + B (pb) + F (residual), write F
        # default since round 3 (c1c10 + chain, 2 launches): 5F + 2B.  (Round 3 still charged the un-fused graph's 5F + 3B + F + B
        # here, which put `frac` above what the kernels move: VERDICT r3.)
        tiles_block = ((2 * F + B) if c10 else 2 * F) + ((3 * F + B) if chain else (2 * B + 3 * F + B))
        bytes_per_launch = P * 256.0 * tiles_block * geom.num_block / launches_per_step
        gbs = bytes_per_launch / (avg_ms * 1e-3) / 1e9
        ex = 3.0 * direct_tflops
        # frac = ALGORITHMIC work / time / peak: the reference graph's bytes (layer-granular, shared-base split) against HBM, its
        # FLOPs (once, not the 3 MFMAs a product costs here) against the dense f16 MFMA peak; the larger fraction names the bound
        f_m, f_h = direct_tflops / PEAK_F16_MFMA_TFLOPS, gbs / PEAK_HBM_GBS
        rec = {"bound": "hbm" if f_h >= f_m else "mfma"}
        if f_h >= f_m:
            rec.update({"achieved": round(gbs, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": round(f_h, 4)})
        else:
            rec.update({"achieved": round(direct_tflops, 1), "peak": PEAK_F16_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": round(f_m, 4)})
        # chain2_sf0: blocks 0 .. nb-2 write their output a second time in the split format (F tiles) - REDUNDANT bytes: they stay out of the
        # algorithmic figure `frac` is priced on and must show up as traffic / algorithmic ~ 1.19 instead
        nb = geom.num_block
        sf_copy = P * 256.0 * F * (nb - 1) / float(launches_per_step) if sf0 else 0.0
        if sf0:
            rec["sf_copy"] = {"redundant_mbytes_per_launch": round(sf_copy / 1e6, 2), "moved_mbytes_per_launch": round((bytes_per_launch + sf_copy) / 1e6, 2),
                              "expected_traffic_over_algorithmic": round((bytes_per_launch + sf_copy) / bytes_per_launch, 3),
                              "moved_gbs": round((bytes_per_launch + sf_copy) / (avg_ms * 1e-3) / 1e9, 1)}
        # what passes through a CU's memory port besides the compulsory bytes: the split weight pack does not fit next to the halo buffers
        # (147 KB), so every 8 x 32-pixel tile replaces one channel half of it from L2 (73 728 B; conv_split16.hip / conv_sf.hip) - bytes
        # that never reach HBM but share the port's ~11 B per clock and CU (tools/ubench/cu_stream_mix) with the ones that do
        tiles_item = ((H + 7) // 8) * ((W + 31) // 32)
        wstream = 73728.0 * tiles_item * (2 * F + B) * nb / launches_per_step
        traffic = stamped_traffic("traffic_split16.json", files, (algo, workload))
        if traffic is not None and traffic < 0.95 * bytes_per_launch:
            # counter bytes below the compulsory bytes: the byte model and the launch structure that ran disagree - say so instead
            # of printing a fraction that does not follow (tests/test_host.py asserts the committed profile against this model)
            rec["traffic_inconsistent"] = {"pmc_bytes_per_launch": traffic, "algorithmic_bytes_per_launch": round(bytes_per_launch)}
            traffic = None
        rec.update({"traffic": traffic, "kernel": name,
                    "avg_launch_ms": round(avg_ms, 4), "launches_timed": k["launches"], "launches_per_step": launches_per_step,
                    "mbytes_per_launch": round(bytes_per_launch / 1e6, 2),
                    "tiles_per_block": "5F+%dB" % ((1 if c10 else 0) + (1 if chain else 3)), "plan": plan["structure"],
                    "stream_mix_ceiling_gbs": STREAM_MIX_CEILING_GBS, "hbm_vs_stream_mix_ceiling": round(gbs / STREAM_MIX_CEILING_GBS, 4),
                    "cu_port": {"l2_weight_stream_mbytes_per_launch": round(wstream / 1e6, 2),
                                "mbytes_per_launch": round((bytes_per_launch + sf_copy + wstream) / 1e6, 2),
                                "gbs": round((bytes_per_launch + sf_copy + wstream) / (avg_ms * 1e-3) / 1e9, 1),
                                "ceiling_b_per_clk_cu": CU_PORT_B_PER_CLK,
                                "note": "compulsory bytes + the weight halves a tile re-reads from L2; b_per_clk_cu / frac are filled in "
                                        "from the shader clock of the sustained run (power.sclk_mhz) when rocm-smi reports it"},
                    "hbm_gbs": round(gbs, 1), "hbm_frac": round(f_h, 4),
                    "algorithmic_direct_tflops": round(direct_tflops, 2), "algorithmic_mfma_frac": round(f_m, 4),
                    "mfma_executed_tflops": round(ex, 1), "mfma_executed_frac": round(ex / PEAK_F16_MFMA_TFLOPS, 4),
                    "mfma_sustained_ceiling_tflops": SUSTAINED_F16_MFMA_TFLOPS,
                    "mfma_executed_vs_sustained_ceiling": round(ex / SUSTAINED_F16_MFMA_TFLOPS, 4),
                    "algorithmic_vs_f32_mfma_roof": round(direct_tflops / PEAK_F32_MFMA_TFLOPS, 4),
                    # (mfma=16: the chain launch of conv2_i = (F + B) of the (2F + B) 3x3 tile-layers of a block; conv1_i and conv10_i stay on 32x32x16)
                    "power_cap_model": power_cap_model(3.0 * flops_per_launch, bytes_per_launch + sf_copy, avg_ms,
                                                       share16=((F + B) * 9.0 / ((2 * F + B) * 9.0 + (F if c10 else 0))) if (plan.get("mfma") == 16 and chain) else 0.0),
                    "note": "frac = algorithmic bytes (or FLOPs) / time / peak.  mfma_executed_* counts the 3 f16 MFMAs a product block costs; "
                            "mfma_sustained_ceiling = what the chip sustains on this kernel's MFMA + LDS core alone under its power cap "
                            "(shader clock 1.3 - 1.6 GHz; profiles/r03_ubench_conv_core.txt)"})
        return rec
    if algo == "small":
        # small shapes: conv1_i (+ conv10_i's per-frame partials since round 4) + the WHOLE of conv2_i (3x3 over concat([base, f]): the
        # reference graph's FLOPs, no shared-base split), 2 launches per block; latency-bound: the fraction of the f16 MFMA
        # peak is what it is
        launches_per_step = 2 * geom.num_block
        flops_ref3 = geom.num_block * 3 * F * P * 9 * 64 * 64 * 2.0
        t = flops_ref3 / launches_per_step / (avg_ms * 1e-3) / 1e12
        name, files = CONV3X3_KERNELS[algo]
        return {"bound": "mfma", "achieved": round(t, 2), "peak": PEAK_F16_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": round(t / PEAK_F16_MFMA_TFLOPS, 4),
                "traffic": None, "kernel": name, "avg_launch_ms": round(avg_ms, 4), "launches_timed": k["launches"],
                "launches_per_step": launches_per_step, "mfma_executed_tflops": round(3 * t, 2),
                "mfma_executed_frac": round(3 * t / PEAK_F16_MFMA_TFLOPS, 4),
                "note": "latency-bound launches of 4 - 15 us (dispatch of ~220 workgroups, one round trip for the halo, a K loop of 54 - 324 MFMAs "
                        "per wave, meeting of the K halves): tools/cm_timing.py has the phase timeline"}
    wino = algo.startswith("winograd")
    executed = direct_tflops / 2.25 if wino else direct_tflops          # F(2x2,3x3): 16 multiplies instead of 36 per 2x2 outputs
    name, files = CONV3X3_KERNELS[algo]
    return {"bound": "mfma", "achieved": round(executed, 2), "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s",
            "frac": round(executed / PEAK_F32_MFMA_TFLOPS, 4),
            "traffic": stamped_traffic("traffic.json", files, (algo, workload)),
            "kernel": name, "avg_launch_ms": round(avg_ms, 4), "launches_timed": k["launches"],
            "launches_per_step": launches_per_step,
            "gflop_per_launch_executed": round(flops_per_launch / (2.25 if wino else 1.0) / 1e9, 3),
            "gflop_per_launch_direct": round(flops_per_launch / 1e9, 3),
            "algorithmic_direct_tflops": round(direct_tflops, 2),
            "algorithmic_vs_direct_roof": round(direct_tflops / PEAK_F32_MFMA_TFLOPS, 4),
            "note": ("achieved = matrix-pipe FLOPs the kernel executes (Winograd F(2x2,3x3): direct-conv FLOPs / 2.25) / time, "
                     "against the dense f32 MFMA peak; algorithmic_* = the direct convolution's FLOPs / time, which a Winograd "
                     "kernel can take past the direct algorithm's roof") if wino else "achieved = executed = algorithmic (direct convolution)"}


def nl_sources_sha():
    return kernel_source_sha(["nonlocal_f16.hip", "nonlocal.hip"])


def nonlocal_roofline(geom, kernel_ms, B, H, W, bf16, plan=None):
    """`roofline_nl`: the affinity matmul + softmax class (reference utils.py:53-64) against the dense f16 MFMA peak.  Algorithmic FLOPs
    = SURVEY.md 8(a)-C: 4 N^2 C + 4 N C^2 per clip (S = X X^T and Y = P X, then the folded 1x1 pair); executed = what the kernel's MFMAs
    do: channels padded to CP = 32 ceil(C / 32), three f16 MFMAs per product block in the fp32 path (exactly split operands), one under
    precision=bf16 (hi parts only).  kernel_ms = the class's HIP-event time per step (pack + attention + merge launches)."""
    ms = kernel_ms.get("nl_attn")
    if not ms:
        return None
    N = (H // 2) * (W // 2)
    C = 4 * 3 * geom.num_frames
    CP = 32 * ((C + 31) // 32)
    alg = B * (4.0 * N * N * C + 4.0 * N * C * C)
    fam = (plan or {}).get("nl", "f16" if bf16 else "split16")      # pfnl_plan: the kernel family that ran
    mult = {"f16": 1, "split16": 3}.get(fam, 1)                      # f16 MFMAs per product block (the f32-MFMA kernels: one f32 MFMA, priced against the f16 peak all the same)
    ex = B * (4.0 * N * N * CP * mult + 4.0 * N * CP * CP)
    t = ms * 1e-3
    rec = {"bound": "mfma", "achieved": round(alg / t / 1e12, 2), "peak": PEAK_F16_MFMA_TFLOPS, "unit": "TFLOP/s",
           "frac": round(alg / t / 1e12 / PEAK_F16_MFMA_TFLOPS, 4), "class_ms_per_step": round(ms, 4),
           "algorithmic_gflop_per_step": round(alg / 1e9, 3), "keys": N, "channels": C, "channels_padded": CP,
           "mfma_per_product": mult, "mfma_executed_tflops": round(ex / t / 1e12, 1),
           "mfma_executed_frac": round(ex / t / 1e12 / PEAK_F16_MFMA_TFLOPS, 4),
           "kernel": ("nl_attn_f16_sw_kernel<C, %s> (+ nl_merge in the class time)" % ("false" if fam == "f16" else "true")) if fam in ("f16", "split16")
                     else "nl_attn_kernel<C> (f32 MFMA: small key counts / strict_fp32 / the general form of the block)", "family": fam,
           "matrix_pipe_busy": None,
           "note": "frac = algorithmic FLOPs / class time / 2.5 PFLOP/s; the class time includes the pack and merge launches around the attention kernel"}
    import glob
    cands = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_pmc_nl.json")))
    if cands:
        pj = json.load(open(cands[-1]))
        key = "%dx%d_%s" % (H, W, "bf16" if bf16 else "fp32")
        if pj.get("kernel_src_sha") == nl_sources_sha() and key in pj.get("matrix_pipe_busy", {}):
            rec["matrix_pipe_busy"] = pj["matrix_pipe_busy"][key]         # SQ_VALU_MFMA_BUSY_CYCLES / (SIMDs x GRBM_GUI_ACTIVE / XCDs), PMC pass
            rec["matrix_pipe_busy_source"] = os.path.basename(cands[-1])
    return rec


def hbm_class_rooflines(geom, kernel_ms, B, H, W, merge_stride=64, plan=None):
    """Achieved GB/s of the bandwidth-class kernels (gather / scatter / tail / bicubic) against 8 TB/s: the
    ALGORITHMIC bytes each class must move (inputs read once, outputs written once) over its HIP-event time per step."""
    T, sc = geom.num_frames, geom.scale
    P, N = H * W, (H // 2) * (W // 2)
    C = 4 * 3 * T
    CP = 32 * ((C + 31) // 32)
    out = {}
    model = {
        # x [B,T,H,W,3] fp32 -> X [B,N,CP] fp32 (space_to_depth of the stacked frames, model/pfnl.py:55-57)
        # (+ the binary16 K / V^T operands - hi and lo' parts, keys padded to 32 + 64 - when the one fused pack launch writes them too: pfnl_plan)
        "nl_pack": B * (T * P * 3 * 4.0 + N * CP * 4.0 + (4.0 * 96 * ((N + 31) // 32 * 32 + 64) * 2.0 if (plan or {}).get("nl_pack_fused") else 0.0)),
        # Xo [B,N,CP] (+ the LR frames' residual already inside) -> conv 5x5 3->64 + lrelu -> inp0 [B*T,H,W,64] fp32 (model/pfnl.py:61-62)
        "conv0": B * (N * CP * 4.0 + T * P * 64 * 4.0),
        # convmerge1: reads the trunk [B*T,H,W,64], writes merge [B,H,W,merge_stride] (model/pfnl.py:73-74)
        "merge1": B * (T * P * 64 * 4.0 + P * merge_stride * 4.0),
        # tail: merge (48 channels used) + the centre LR frame (bicubic) -> out [B,1,sH,sW,3] (model/pfnl.py:63,76-80)
        "tail": B * (P * 48 * 4.0 + P * 3 * 4.0 + sc * sc * P * 3 * 4.0),
    }
    for k, nbytes in model.items():
        ms = kernel_ms.get(k)
        if ms:
            gbs = nbytes / (ms * 1e-3) / 1e9
            out[k] = {"ms_per_step": round(ms, 4), "algorithmic_mbytes_per_step": round(nbytes / 1e6, 3), "gbs": round(gbs, 1),
                      "frac_of_hbm_peak": round(gbs / PEAK_HBM_GBS, 4)}
    out["note"] = ("launch-latency-class kernels at these sizes (10 - 100 us each): merge1 is an MFMA kernel (convmerge1 448 -> 48), listed with its "
                   "bytes for completeness; peak = 8 TB/s")
    return out


def plan_algo(plan):
    """The key of CONV3X3_KERNELS / conv3x3_roofline for a launch plan (PFNLEngine.plan = pfnl_plan: the rule itself lives in capi.hip's
    trunk_plan and nowhere else)."""
    return "bf16" if plan.get("precision") == "bf16" else plan["conv3x3"]


def stamped_traffic(suffix, files, key):
    """HBM bytes per launch from the rocprofv3 --pmc passes kept under profiles/ (the newest r<NN>_<suffix>), or None when
    the kernel sources have changed since they were measured (the file records the sha of the sources it was measured on)."""
    import glob
    cands = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_" + suffix)))
    if not cands:
        return None
    tj = json.load(open(cands[-1]))
    if tj.get("kernel_src_sha") != kernel_source_sha(files):
        return None
    v = tj.get("hbm_bytes_per_launch_avg")
    if isinstance(v, dict):                                # per workload (the bf16 file)
        return v.get(key)
    if isinstance(key, tuple):                             # (algo, workload): a single figure measured on one workload
        return v if (tj.get("algo"), tj.get("workload", "cfg2")) == key else None
    return v if tj.get("algo", key) == key else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--full", action="store_true",
                    help="also run what the headline figure does not need: the untimed per-class breakdown pass (roofline_nl, "
                         "roofline_hbm_classes, the whole kernel_ms_per_step; the small shapes' roofline), the sustained run with the "
                         "power sampler, the secondary workloads and the CPU baseline.  Off by default: a plain run warms up, times "
                         "the steps, writes --dump-outputs and prints its line")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-secondary", action="store_true", help="with --full: skip the secondary workloads and the sustained run")
    ap.add_argument("--conv3x3", choices=["auto", "split16", "winograd", "winograd_tile", "direct"], default=None,
                    help="override the 3x3 conv algorithm (default auto: split16 for launches of >= 200 tiles, the small-shape kernels below)")
    ap.add_argument("--conv1x1", choices=["split16", "stream", "tiled"], default=None, help="override the conv10_i algorithm")
    ap.add_argument("--precision", choices=["fp32", "bf16"], default="fp32",
                    help="trunk arithmetic: fp32 = the reference's (the judged line); bf16 = BASELINE.json configs[3]'s")
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="cfg2",
                    help="cfg2 = configs[1] 4x7x128x128 per GPU (default, the metric's config); cfg0 = configs[0] 1x7x32x32 (north_star's "
                         "second size); cfg4 = configs[3] 1x7x270x480 (1080p); cfg5 = configs[4] 2x, 1x5x64x64")
    ap.add_argument("--clips-per-gpu", type=int, default=0, help="override the workload's clips per GPU (weak scaling); stated in config")
    ap.add_argument("--strong", action="store_true",
                    help="strong scaling (SURVEY.md 8(e)): a FIXED global batch (--global-batch, default configs[2]'s 32 clips for cfg2) in "
                         "contiguous shards over the N ranks instead of a fixed batch per GPU; the line says scaling = strong")
    ap.add_argument("--global-batch", type=int, default=0, help="global batch of --strong (default: the workload's)")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"],
                    help="collective backend for --gpus > 1 (nccl = RCCL over xGMI; gloo only to exercise the N>1 plumbing on a 1-GPU box)")
    ap.add_argument("--comm", default="pfnl", choices=["pfnl", "torch"],
                    help="--gpus > 1 with nccl: who carries the weight replica and the max-over-ranks time - the library's own RCCL "
                         "communicator (pfnl_comm_*, include/pfnl_hip.h; falls back to torch.distributed if it cannot be created on "
                         "every rank) or torch.distributed")
    ap.add_argument("--require-comm", action="store_true",
                    help="with --comm pfnl: no fallback to torch.distributed - a rank whose pfnl_comm (RCCL) does not come up fails the run")
    ap.add_argument("--full-profile", action="store_true",
                    help="HIP events around every launch of the timed steps (default: the launches of one of the twenty progressive-fusion "
                         "blocks; the whole-forward breakdown from an untimed pass)")
    ap.add_argument("--no-profile", action="store_true", help="do not bracket kernels with HIP events (no roofline object)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last of them computed (the SR frames a caller of the forward receives) "
                         "as DIR/output.npy (DIR/output_rank<r>.npy with N > 1), float32, at most 64 MB over all ranks")
    args = ap.parse_args()
    if args.steps < 1:
        raise SystemExit("--steps must be at least 1")
    wl = WORKLOADS[args.workload]
    H, W, T_WL = wl["H"], wl["W"], wl["T"]

    import numpy as np
    import torch
    from pfnl_amd import dist as pd
    from pfnl_amd import synth
    from pfnl_amd.engine import PFNLEngine
    from pfnl_amd.spec import PFNLGeometry

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if "WORLD_SIZE" in os.environ or "RANK" in os.environ:
            raise SystemExit("bench.py --gpus %d was launched with WORLD_SIZE=%d" % (args.gpus, world))
        # not under a launcher: spawn one rank per GPU ourselves (the command the driver uses) and relay rank 0's line
        import socket
        import subprocess
        sk = socket.socket()
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
        sk.close()
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        raise SystemExit(subprocess.call(cmd, env=env))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device: the product path has no CPU fallback")
    ndev = torch.cuda.device_count()
    if args.backend == "nccl" and local_rank >= ndev:
        raise SystemExit("rank %d has no GPU (%d visible)" % (local_rank, ndev))
    local_dev = local_rank % ndev                      # gloo test mode may stack ranks on one GPU
    torch.cuda.set_device(local_dev)
    dev = "cuda:%d" % local_dev
    geom = PFNLGeometry(num_frames=T_WL, scale=wl["scale"])
    if args.strong:
        GB = args.global_batch or wl["strong"]
        if GB < world:
            raise SystemExit("--strong: a global batch of %d clips cannot be split over %d ranks" % (GB, world))
        lo, hi = pd.shard_range(GB, rank, world)                      # contiguous shards, sizes differ by at most one clip
        B_PER_GPU = hi - lo
    else:
        B_PER_GPU = args.clips_per_gpu or wl["clips"]
        GB = world * B_PER_GPU

    use_dist = world > 1 or bool(os.environ.get("PFNL_BENCH_FORCE_DIST"))   # (the env: run the N>1 code path with one rank - tests)
    comm = None
    comm_hung = False
    eng = PFNLEngine(geom, device=local_dev)
    if use_dist:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if args.backend == "nccl":
            # torch.distributed is the launcher (rendezvous + the contract's barrier); the weight replica and the
            # max-over-ranks time go through the library's own RCCL communicator (pfnl_comm_*, include/pfnl_hip.h)
            from pfnl_amd.comm import Comm
            with stdout_to_stderr():
                dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device(dev))
                dist.barrier()                                         # creates torch's communicator now, not inside the timed region
                if args.comm == "pfnl":
                    # ncclCommInitRank is a collective: a rank that cannot join would hang the others.  It runs under a
                    # watchdog so that a node where the second communicator does not come up still produces its bench line
                    # (through torch's group) instead of running into the driver's timeout.
                    import threading
                    box = {}

                    def _init():
                        try:
                            torch.cuda.set_device(local_dev)           # (the current device is per thread)
                            box["comm"] = Comm.from_torch_distributed(local_dev)
                        except Exception as e:                         # (RCCL not loadable, id exchange failed ...)
                            box["err"] = e

                    th = threading.Thread(target=_init, daemon=True)
                    th.start()
                    th.join(timeout=float(os.environ.get("PFNL_COMM_INIT_TIMEOUT", "120")))
                    if th.is_alive():
                        print("pfnl_comm init timed out on rank %d: falling back to torch.distributed" % rank, file=sys.stderr)
                        comm_hung = True
                    elif "err" in box:
                        print("pfnl_comm unavailable on rank %d (%s)" % (rank, box["err"]), file=sys.stderr)
                    comm = box.get("comm") if not th.is_alive() else None
                    # every rank must take the same road: agree through the launcher's group
                    ok = torch.tensor([1 if comm is not None else 0], device=dev)
                    dist.all_reduce(ok, op=dist.ReduceOp.MIN)
                    if int(ok[0]) == 0 and args.require_comm:
                        raise SystemExit("--require-comm: pfnl_comm (RCCL) did not come up on every rank (rank %d: %s)"
                                         % (rank, "ok" if comm is not None else box.get("err", "timed out")))
                    if int(ok[0]) == 0 and comm is not None:
                        comm.close()
                        comm = None
                weights = synth.synthetic_weights(geom, seed=0) if rank == 0 else None
                if comm is not None:
                    if rank == 0:
                        eng.load_weights(weights)
                    comm.bcast_weights(eng, root=0)                    # ncclBroadcast of the packed device blobs, once
                else:
                    weights = pd.broadcast_weights(geom, weights, src=0, device=dev)   # the same 12 MB through torch's RCCL group
                    eng.load_weights(weights)
        else:
            dist.init_process_group("gloo", rank=rank, world_size=world)
            weights = pd.broadcast_weights(geom, synth.synthetic_weights(geom, seed=0) if rank == 0 else None, src=0)
            eng.load_weights(weights)
    else:
        weights = synth.synthetic_weights(geom, seed=0)
        eng.load_weights(weights)

    comm_nranks = comm_rank = None
    if comm is not None:                                                # what RCCL itself reports (pfnl_comm_rank): the line proves N ranks were seen
        comm_rank, comm_nranks = comm.rank_and_size()
        if comm_nranks != world or comm_rank != rank:
            raise SystemExit("pfnl_comm reports rank %d of %d, the launcher rank %d of %d" % (comm_rank, comm_nranks, rank, world))
    if args.conv3x3:
        eng.set_option("conv3x3", args.conv3x3)
    if args.conv1x1:
        eng.set_option("conv1x1", args.conv1x1)
    bf16 = args.precision == "bf16"
    if bf16:
        eng.set_option("precision", "bf16")
    for kv in os.environ.get("BENCH_OPTIONS", "").split(","):         # same-box A/B runs (tools/ab_r06.sh): engine options by name
        if "=" in kv:
            eng.set_option(*kv.split("=", 1))
    plan = eng.plan(B_PER_GPU, H, W)                                   # the launch structure that will run (pfnl_plan: the one statement of the rule)
    x = torch.from_numpy(synth.uniform_clips(B_PER_GPU, T_WL, H, W, seed=1234 + rank)).to(dev)   # resident in HBM
    out = torch.empty(eng.out_shape(B_PER_GPU, H, W), dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def step():
        eng.forward_device(x.data_ptr(), out.data_ptr(), B_PER_GPU, H, W, stream)

    def fence():
        torch.cuda.synchronize()
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()

    # clock ramp: a chip that has been idle runs its first ~50 ms of work below the clock it settles at (measured: 865 fps over the
    # first 10 steps after 2, 877-879 after 50 or over 100 steps).  PREWARM_S seconds of untimed steps bring it there before the W
    # warm-up steps and the K timed steps of the contract are run; the figure is in the line (`prewarm_s`).
    t_pre = time.perf_counter()
    while time.perf_counter() - t_pre < PREWARM_S:
        for _ in range(8):
            step()
        torch.cuda.synchronize()
    for _ in range(args.warmup):
        step()
    fence()
    eng.profile_reset()
    # HIP events on the launch stream: the TIMED steps carry them around the launches of ONE of the 20 identical PF blocks only (the
    # dominant class: `roofline` is measured live in the timed region, at 3 events per forward); the per-class breakdown of the whole
    # forward comes from a separate, untimed pass with events on two blocks and on everything outside the blocks (--full-profile: the
    # timed steps carry events around every launch instead - an event costs the stream 2 us and more where it splits back-to-back launches)
    prof_mode = 0 if args.no_profile else (1 if args.full_profile else 3)
    small_shape = plan["structure"].startswith("small")
    if small_shape and prof_mode == 3:
        # launch-bound shapes (~47 launches of 5 - 15 us): even three events move the step; the timed steps carry none and the
        # breakdown pass below runs in "class runs" mode (one event per change of kernel class: pfnl_profile_enable(4))
        prof_mode = 0
    eng.profile(prof_mode)
    elapsed = timed_steps(step, fence, args.steps)
    eng.profile(False)
    dumped = None
    if args.dump_outputs:                                              # the last timed step's result, before anything else writes `out`
        dumped = dump_output(out, args.dump_outputs, "output" if world == 1 else "output_rank%d" % rank, DUMP_LIMIT_BYTES // world)
    prof = eng.profile_read()
    prof_all, n_all = None, 0
    if args.full and (prof_mode == 3 or (small_shape and not args.no_profile and not args.full_profile)):
        n_all = max(3, args.steps // 2)
        eng.profile_reset()
        eng.profile(4 if small_shape else 2)
        timed_steps(step, fence, n_all)                                  # (not part of `value`)
        eng.profile(False)
        prof_all = eng.profile_read()
        if small_shape:
            prof = prof_all                                              # (the roofline's launch average comes from this pass)

    if use_dist:
        if comm is not None:
            elapsed = float(comm.allreduce([elapsed], "max")[0])
        else:
            t = torch.tensor([elapsed], dtype=torch.float64, device=dev if args.backend == "nccl" else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            elapsed = float(t[0])
    assert torch.isfinite(out).all().item(), "non-finite output"

    clips_total = GB * args.steps                                     # all ranks' clips (weak: world x clips per GPU; strong: the fixed batch)
    value = clips_total / elapsed                                     # 1 HR frame per clip
    ms_per_step = 1e3 * elapsed / args.steps

    algo = plan_algo(plan)
    roof = conv3x3_roofline(geom, prof, B_PER_GPU, H, W, plan, args.workload)
    f_ref = geom.flops_per_clip(H, W) * B_PER_GPU
    f_exec = geom.flops_per_clip(H, W, shared_base=True) * B_PER_GPU
    # sampled mode: the two classes inside the PF blocks were timed in ceil(nb/4) of the nb blocks
    nb = geom.num_block
    scale_blk = nb / float(blocks_sampled(nb)) if prof_mode == 2 and nb else 1.0
    if prof_all is None and prof_mode == 3:
        # a plain run: the one block of the timed steps (x nb) is all that carried events - the other classes are --full's
        breakdown = {n: round(v["ms"] / args.steps * nb, 4) for n, v in prof.items() if v["launches"]}
    elif prof_all is None:
        breakdown = {n: round(v["ms"] / args.steps * (scale_blk if n in ("conv3x3", "conv1x1") else 1.0), 4)
                     for n, v in prof.items()}
    else:
        # in-block classes: live, from the one block of the timed steps (x nb); the rest: from the untimed pass
        sc_all = nb / float(blocks_sampled(nb)) if nb else 1.0
        breakdown = {}
        for n, v in prof.items():
            if small_shape:                                              # class runs: whole-forward intervals, nothing to scale
                breakdown[n] = round(prof_all[n]["ms"] / n_all, 4)
            elif v["launches"]:
                breakdown[n] = round(v["ms"] / args.steps * nb, 4)
            else:
                breakdown[n] = round(prof_all[n]["ms"] / n_all * (sc_all if n in ("conv3x3", "conv1x1") else 1.0), 4)

    res = {
        "metric": "HR frames/sec at %dxSR, %d-frame %dx%d->%dx%d" % (wl["scale"], T_WL, H, W, wl["scale"] * H, wl["scale"] * W),
        "value": round(value, 3), "unit": "HR frames/s",
        "n_gpus": world, "full": bool(args.full), "steps": args.steps, "warmup": args.warmup, "prewarm_s": PREWARM_S, "ms_per_step": round(ms_per_step, 4),
        "higher_is_better": True, "scaling": "strong" if args.strong else "weak", "vs_baseline": None, "dtype": "bf16" if bf16 else "f32",
        "data": "synthetic",
        "config": {"workload": wl["label"] % (B_PER_GPU, "bf16 trunk" if bf16 else "fp32",
                                              (": the fixed global batch of %d clips in contiguous shards, this is rank 0's" % GB) if args.strong else ""),
                   "clips_per_gpu": B_PER_GPU, "global_batch": GB, "parallelism": "dp%d" % world, "backend": (args.backend if use_dist else None),
                   "comm": (("pfnl_comm (RCCL)" if comm is not None else "torch.distributed") if use_dist else None),
                   "comm_nranks": comm_nranks, "comm_required": bool(args.require_comm),
                   "weights": "synthetic Xavier (seed 0)", "input": "resident in HBM", "conv3x3": algo, "plan": plan["structure"], "mfma": plan.get("mfma")},
        "roofline": roof,
        "roofline_nl": nonlocal_roofline(geom, breakdown, B_PER_GPU, H, W, bf16, plan),
        "roofline_hbm_classes": hbm_class_rooflines(geom, breakdown, B_PER_GPU, H, W, plan=plan) if (args.full or prof_mode == 1) else None,
        "whole_forward": {"tflops_ref_graph": round(f_ref / (ms_per_step * 1e-3) / 1e12, 2),
                          "tflops_direct_shared_base": round(f_exec / (ms_per_step * 1e-3) / 1e12, 2),
                          "kernel_ms_per_step": breakdown},
    }
    if dumped is not None:
        res["dump_outputs"] = dict(dumped, dir=os.path.abspath(args.dump_outputs))

    if args.full and not args.no_secondary:
        # ---- sustained: >= 2 s of back-to-back steps, no events (clock droop shows up as ms/step above the headline's)
        n_sus = max(args.steps, int(2.2e3 / max(ms_per_step, 1e-3)) + 1)
        sampler = PowerSampler(local_dev) if rank == 0 else None       # package power / shader clock while the sustained run is under way
        el = timed_steps(step, fence, n_sus)
        if sampler is not None:
            power = sampler.stop()
            if power:
                res["power"] = power
                port = (res.get("roofline") or {}).get("cu_port")
                if port and power.get("sclk_mhz"):                  # per shader clock and CU: the unit the port's ceiling was measured in
                    n_cu = torch.cuda.get_device_properties(local_dev).multi_processor_count
                    port["b_per_clk_cu"] = round(port["gbs"] * 1e9 / (n_cu * power["sclk_mhz"] * 1e6), 2)
                    port["frac"] = round(port["b_per_clk_cu"] / CU_PORT_B_PER_CLK, 3)
        if use_dist:
            if comm is not None:
                el = float(comm.allreduce([el], "max")[0])
            else:
                t = torch.tensor([el], dtype=torch.float64, device=dev if args.backend == "nccl" else "cpu")
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                el = float(t[0])
        res["sustained"] = {"steps": n_sus, "seconds": round(el, 3), "ms_per_step": round(1e3 * el / n_sus, 4),
                            "value": round(GB * n_sus / el, 3)}
        if res.get("power") and world == 1:
            # energy per HR frame = package power x time per step / clips per step, both from the sustained run: the split-f16 launches sit on
            # the package power cap, so a kernel change is a change of THIS number or it is nothing
            res["joules_per_frame"] = round(res["power"]["package_w"] * (el / n_sus) / B_PER_GPU, 4)
    if rank == 0 and world == 1 and args.full and not args.no_secondary and args.workload == "cfg2" and not bf16 and not args.strong and not args.clips_per_gpu:
        res["secondary"] = secondary_workloads(eng, geom, weights, local_dev, dev, x, out)
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline and args.workload in ("cfg2", "cfg0"):   # (the 1080p oracle needs minutes per pass; configs[4] is build-defined)
        sample = synth.uniform_clips(B_PER_GPU, T, H, W, seed=1234)     # the GPU line's batch (same seed: the same clips)
        res["cpu_baseline"] = cpu_baseline(weights, sample, H, W)
        res["gpu_over_cpu"] = round(value / res["cpu_baseline"]["value"], 1)
    if rank == 0:
        print(json.dumps(res), flush=True)
    if comm is not None:
        comm.close()
    if comm_hung:                                                     # a stuck ncclCommInitRank thread would block a clean exit
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(0)
    if use_dist:
        dist.destroy_process_group()


def secondary_workloads(eng, geom, weights, local_dev, dev, x_cfg2, out_cfg2):
    """The other BASELINE.json configurations and the host-pointer path, each: 2 warm-up + K timed steps bracketed by
    synchronize WITHOUT profiling events (an event costs the stream ~2 us: a fifth of a small-shape forward), then a second
    pass of the same K steps with the sampled HIP-event breakdown for `kernel_ms_per_step` and `roofline`; N=1 only.
    Not the judged `value` - driver-visible evidence."""
    import numpy as np
    import torch
    from pfnl_amd import synth
    from pfnl_amd.engine import PFNLEngine
    from pfnl_amd.spec import PFNLGeometry

    def sync():
        torch.cuda.synchronize()

    def run(e, g, B, H, W, steps, seed, bf16=False, label="", small=False):
        xs = torch.from_numpy(synth.uniform_clips(B, g.num_frames, H, W, seed=seed)).to(dev)
        o = torch.empty(e.out_shape(B, H, W), dtype=torch.float32, device=dev)
        st = torch.cuda.current_stream().cuda_stream
        fwd = lambda: e.forward_device(xs.data_ptr(), o.data_ptr(), B, H, W, st)    # noqa: E731
        for _ in range(2):
            fwd()
        sync()
        el = timed_steps(fwd, sync, steps)                           # the line's ms_per_step / value: no events
        e.profile_reset()
        e.profile(4 if small else 2)                                 # the breakdown: sampled events (small shapes: one per class run)
        timed_steps(fwd, sync, steps)
        e.profile(False)
        prof = e.profile_read()
        nb = g.num_block
        sc = 1.0 if small else (nb / float(blocks_sampled(nb)) if nb else 1.0)
        ms = 1e3 * el / steps
        rec = {"workload": label, "dtype": "bf16" if bf16 else "f32", "clips": B, "steps": steps, "ms_per_step": round(ms, 4),
               "value": round(B * steps / el, 3), "unit": "HR frames/s", "input": "resident in HBM",
               "kernel_ms_per_step": {n: round(v["ms"] / steps * (sc if n in ("conv3x3", "conv1x1") else 1.0), 4) for n, v in prof.items()}}
        assert torch.isfinite(o).all().item(), "non-finite output (%s)" % label
        rec["roofline_nl"] = nonlocal_roofline(g, rec["kernel_ms_per_step"], B, H, W, bf16, e.plan(B, H, W))
        return rec, prof

    out = []
    # configs[3]: 1080p, bf16 trunk
    eng.set_option("precision", "bf16")
    rec, prof = run(eng, geom, 1, 270, 480, 10, 4040, bf16=True, label="BASELINE.json configs[3]: 4xSR 7x270x480 -> 1080x1920, batch 1, bf16 trunk")
    rec["roofline"] = conv3x3_roofline(geom, prof, 1, 270, 480, eng.plan(1, 270, 480), "cfg4")
    out.append(rec)
    rec["plan"] = eng.plan(1, 270, 480)["structure"]
    eng.set_option("precision", "fp32")
    # configs[3] geometry in fp32 (the reference's arithmetic at 1080p)
    rec, prof = run(eng, geom, 1, 270, 480, 5, 4040, label="configs[3] geometry in fp32: 7x270x480 -> 1080x1920, batch 1")
    rec["roofline"] = conv3x3_roofline(geom, prof, 1, 270, 480, eng.plan(1, 270, 480), "cfg4")
    rec["plan"] = eng.plan(1, 270, 480)["structure"]
    out.append(rec)
    # one window at the reference harness's Vid4 geometry (model/pfnl.py:236-247 batches `part` windows; a caller's own forward(x) of one
    # clip is this): 108 (clip, tile) chains - below 136 the block runs as four per-tile launches, so the two-launch
    # byte model of `roofline` does not describe it: timing and the per-class breakdown only
    rec, prof = run(eng, geom, 1, 144, 180, 20, 77, label="reference harness geometry: one Vid4 window 7x144x180 -> 576x720, batch 1, fp32 (mid shapes: four per-tile launches per block)")
    rec["roofline"] = conv3x3_roofline(geom, prof, 1, 144, 180, eng.plan(1, 144, 180), "vid4")   # (mid4: conv1_i, shared half, per-frame half = 5F + 3B over 3 launches of this class)
    rec["plan"] = eng.plan(1, 144, 180)["structure"]
    out.append(rec)
    # configs[0]: 7x32x32, batch 1 (the reference's CPU-runnable plumbing case; latency-bound on a GPU)
    rec, prof = run(eng, geom, 1, 32, 32, 100, 1234, label="BASELINE.json configs[0]: 4xSR 7x32x32 -> 128x128, batch 1, fp32", small=True)
    rec["roofline"] = conv3x3_roofline(geom, prof, 1, 32, 32, eng.plan(1, 32, 32), "cfg1")
    rec["plan"] = eng.plan(1, 32, 32)["structure"]
    out.append(rec)
    # configs[4]: 2x, 5 frames, 64x64 (build-defined tail; 20 blocks)
    g5 = PFNLGeometry(num_frames=5, scale=2, num_block=20)
    e5 = PFNLEngine(g5, device=local_dev)
    e5.load_weights(synth.synthetic_weights(g5, seed=0))
    rec, prof = run(e5, g5, 1, 64, 64, 100, 55, label="BASELINE.json configs[4]: 2xSR 5x64x64 -> 128x128, batch 1, fp32", small=True)
    rec["roofline"] = conv3x3_roofline(g5, prof, 1, 64, 64, e5.plan(1, 64, 64), "cfg5")
    rec["plan"] = e5.plan(1, 64, 64)["structure"]
    out.append(rec)
    e5.close()
    # configs[1] on the EXACT f32-MFMA kernels (option strict_fp32: Winograd / streaming 1x1 / f32 non-local / VALU conv0 - v_mfma_f32_32x32x2_f32 and
    # fp32 FMAs only): the pure-fp32 figure beside the headline, whose "f32" means fp32 tensors + fp32 accumulation + products taken from two
    # binary16 halves (>= 22 mantissa bits; include/pfnl_hip.h "strict_fp32")
    Bs, Hs, Ws = int(x_cfg2.shape[0]), int(x_cfg2.shape[2]), int(x_cfg2.shape[3])
    eng.set_option("strict_fp32", "on")
    rec, prof = run(eng, geom, Bs, Hs, Ws, 5, 1234, label="BASELINE.json configs[1] with strict_fp32=on: every product an exact fp32 FMA (f32 MFMA 32x32x2, "
                    "Winograd F(2x2,3x3) for the 3x3s) - the pure-fp32 figure beside the split-f16 headline")
    rec["roofline"] = conv3x3_roofline(geom, prof, Bs, Hs, Ws, eng.plan(Bs, Hs, Ws), "cfg2")
    rec["plan"] = eng.plan(Bs, Hs, Ws)["structure"]
    eng.set_option("strict_fp32", "off")
    out.append(rec)
    # configs[1] through HOST pointers: numpy in -> numpy out, H2D + kernels + D2H inside pfnl_forward
    xh = np.ascontiguousarray(x_cfg2.cpu().numpy())
    for _ in range(2):
        eng.forward(xh)
    sync()
    steps = 10
    t0 = time.perf_counter()
    for _ in range(steps):
        yh = eng.forward(xh)
    el = time.perf_counter() - t0
    assert np.isfinite(yh).all()
    eng.profile_reset()
    eng.profile(2)
    for _ in range(3):
        eng.forward(xh)
    eng.profile(False)
    prof_h = eng.profile_read()
    Bh, Hh, Wh = int(xh.shape[0]), int(xh.shape[2]), int(xh.shape[3])          # [B, T, H, W, 3]
    rf_h = conv3x3_roofline(geom, prof_h, Bh, Hh, Wh, eng.plan(Bh, Hh, Wh), "cfg2")
    out.append({"roofline": rf_h, "pcie_mbytes_per_step": round((xh.nbytes + yh.nbytes) / 1e6, 2),
                "workload": "BASELINE.json configs[1] through HOST pointers (pageable numpy in/out: 5.5 MB H2D + 12.6 MB D2H inside pfnl_forward; "
                            "what the reference's sess.run timing covers, model/pfnl.py:249-253)",
                "host_output": PFNLEngine.host_output_mode(),
                "dtype": "f32", "clips": int(xh.shape[0]), "steps": steps, "ms_per_step": round(1e3 * el / steps, 4),
                "value": round(xh.shape[0] * steps / el, 3), "unit": "HR frames/s", "input": "host memory (PCIe-inclusive)"})
    return out


if __name__ == "__main__":
    main()
