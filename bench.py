"""Headline benchmark: ViT-B/16 224 training step, bs=256 per GPU, bf16 (BASELINE.json configs[1]).

One step = forward + mean cross-entropy + backward + fused SGD (lr 0.1, momentum
0.9, wd 1e-4) on one synthetic batch already resident in HBM (VIT:132-147 minus
the data loader).  N>1: one process per GPU, 256 images per rank (weak scaling),
gradients averaged with RCCL all-reduces issued block by block during the
backward (DDP in the reference, VIT:287).  Prints ONE JSON line on rank 0.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--batch B] [--graph] [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times the K steps and prints the headline line, nothing else.
``--dump-outputs DIR`` also writes what the last timed step computed (its loss, its logits and a
fixed seeded sample of the updated parameters) as ``DIR/<name>.npy``; the seeds are fixed, so two
builds run with the same arguments see the same weights and batch and can be compared array by array.

``--full`` adds every other measurement, each of which costs GPU or host time of its own: the GPU's
clock / power telemetry and the HIP events around the weight-gradient and optimizer launches in the
timed steps, the standalone weight-gradient leg and the ``roofline`` key, the CPU baseline
(``--no-cpu`` drops it) and, at N=1, the ``c3`` key (``--no-c3`` drops it): the CLIP-HBA step
(BASELINE configs[2]) timed in fp32, the reference's precision, and in the bf16 opt-in -- an extra
key, not the headline value.

``--gpus N`` without a torchrun environment launches its own N ranks (one
process per GPU, ``torch.distributed.run`` on 127.0.0.1, as the reference's
``torchrun --nproc_per_node`` does: VSLURM:47) before anything touches the GPU.
``--dry`` runs the same launcher and gradient-averaging path on CPU (gloo) with a
stand-in gradient buffer: the multi-rank plumbing test (tests/test_bench_cli.py).
"""
from __future__ import annotations

import argparse
import json
import math
import os
import socket
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "vit-project_amd"))

FWD_FLOP_PER_IMG = 35.128e9          # SURVEY §8d (oracle.vit_flops_per_image)
STEP_FLOP_PER_IMG = 3 * FWD_FLOP_PER_IMG
# gfx950 dense bf16 MFMA: 256 CU x 4 SIMD x 1024 FLOP/clk (16x16x32: 16384 FLOP / 16 clk) x 2.4 GHz
PEAK_BF16_TFLOPS = 256 * 4 * 1024 * 2.4e9 / 1e12


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--graph", action="store_true",
                    help="replay one captured HIP graph per step (ROCm replays graph branches serially, so the "
                         "two-stream overlap is lost; eager is faster with overlap on)")
    ap.add_argument("--full", action="store_true",
                    help="also run what the headline figure does not need: GPU telemetry, per-launch HIP events, "
                         "the standalone weight-gradient leg / roofline, the C3 legs and the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's loss, logits and a seeded sample of the updated parameters "
                         "as DIR/<name>.npy (float32)")
    ap.add_argument("--cpu-seconds", type=float, default=12.0, help="CPU baseline sample budget")
    ap.add_argument("--no-cpu", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-overlap", action="store_true", help="weight gradients inline instead of on a side stream")
    ap.add_argument("--no-probe", action="store_true", help="with --full: no HIP events around the weight-gradient launches")
    ap.add_argument("--no-c3", action="store_true", help="with --full: skip the CLIP-HBA (config C3) leg")
    ap.add_argument("--dry", action="store_true", help="CPU/gloo launcher + gradient-averaging check, no GPU")
    return ap.parse_args(argv)


# ----------------------------------------------------------------------------
# rank launcher (before any GPU call)
# ----------------------------------------------------------------------------

def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch_ranks(n: int, argv) -> int:
    """Start N ranks of this script under torch.distributed.run as child processes (never an
    exec: the parent has not touched the GPU, and exits with the launcher's code)."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__), *argv]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "1")
    return subprocess.call(cmd, env=env)


# ----------------------------------------------------------------------------
# CPU baseline
# ----------------------------------------------------------------------------

def host_cpus():
    """(threads usable by this process, os.cpu_count(), lscpu model name).  On the GPU box
    os.cpu_count() reports the whole machine; the process's share is its affinity mask,
    further capped by a cgroup CPU quota when one is set."""
    total = os.cpu_count() or 1
    try:
        usable = len(os.sched_getaffinity(0))
    except AttributeError:
        usable = total
    for f in ("/sys/fs/cgroup/cpu.max",):
        try:
            q, per = open(f).read().split()[:2]
            if q != "max":
                usable = min(usable, max(1, math.ceil(int(q) / int(per))))
        except (OSError, ValueError):
            pass
    model = None
    try:
        out = subprocess.run(["lscpu"], capture_output=True, text=True, timeout=10).stdout
        for line in out.splitlines():
            if line.startswith("Model name:"):
                model = line.split(":", 1)[1].strip()
                break
    except (OSError, subprocess.SubprocessError):
        pass
    return usable, total, model


def cpu_baseline(seconds: float):
    """The oracle's fp32 ViT-B/16 train step (bs=4, configs[0]) on the host cores."""
    import torch
    from oracle import vit_ref as R
    threads, total, model = host_cpus()
    torch.set_num_threads(threads)
    cfg = R.VIT_B16
    p = R.init_params(cfg, seed=0)
    bufs = {}
    g = torch.Generator().manual_seed(0)
    B = 4
    x = torch.randn(B, 3, 224, 224, generator=g)
    y = torch.randint(0, 1000, (B,), generator=g)
    R.train_step(p, bufs, x, y, lr=0.1, cfg=cfg)  # warmup
    n, t0 = 0, time.perf_counter()
    while True:
        R.train_step(p, bufs, x, y, lr=0.1, cfg=cfg)
        n += 1
        el = time.perf_counter() - t0
        if el >= seconds or n >= 50:
            break
    return {"value": round(n * B / el, 3), "unit": "images/s", "cores": threads, "kind": "port",
            "host_cpu_count": total, "cpu_model": model,
            "sample": f"{n} fp32 ViT-B/16 train steps (bs=4, fwd+CE+bwd+SGD) of oracle/vit_ref.py, "
                      f"{el:.1f} s, torch CPU {threads} threads (the process's CPU share of {total})"}


# the sources the weight-gradient kernel is built from: a committed counter file records their hash
# (tools/pmc_traffic.py / tools/pmc_step_classes.py --src-sha), so the bench line can say whether the
# counters it quotes were taken on the kernel that ran
WGRAD_SOURCES = ("vit-project_amd/csrc/gemm.hip", "vit-project_amd/csrc/gemm_lds.hpp", "vit-project_amd/csrc/gemm_w4.inc",
                 "vit-project_amd/csrc/gemm_epi.hpp")


def wgrad_src_sha():
    import hashlib
    h = hashlib.sha256()
    for f in WGRAD_SOURCES:
        with open(os.path.join(ROOT, f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def _latest_counter_file(pattern):
    import glob
    return sorted(glob.glob(os.path.join(ROOT, "profiles", "r0*", pattern)), reverse=True)


def _pmc_mfma_busy():
    """MFMA-busy fraction of the weight-gradient class from the latest committed step counter
    passes (profiles/r0N/pmc_step_classes*.json, tools/pmc_step_classes.py), its source file and
    source hash (None when the file predates the hash), or Nones."""
    for f in _latest_counter_file("pmc_step_classes*.json"):
        try:
            with open(f) as fh:
                d = json.load(fh)
            return d["classes"]["gemm wgrad"].get("mfma_busy"), os.path.relpath(f, ROOT), d.get("src_sha")
        except (OSError, KeyError, ValueError):
            continue
    return None, None, None


def _pmc_traffic(name):
    """HBM bytes per launch of a kernel from the latest committed counter passes (tools/pmc_traffic.py;
    FETCH_SIZE doubled per the gfx950 correction), its file and source hash, or Nones."""
    for f in _latest_counter_file(name):
        try:
            with open(f) as fh:
                d = json.load(fh)
            return int(d["traffic_bytes_per_launch"]), os.path.relpath(f, ROOT), d.get("src_sha")
        except (OSError, KeyError, ValueError):
            continue
    return None, None, None


# ----------------------------------------------------------------------------
# config C3 leg: CLIP-HBA ViT-L/14 + DoRA train step, in both dtypes
# ----------------------------------------------------------------------------

PEAK_F32_TFLOPS = 256 * 4 * 64 * 2.4e9 / 1e12  # v_mfma_f32_16x16x4_f32: 64 FLOP/clk/SIMD


def _block_flops(tokens, width, seq):
    """forward FLOPs of one pre-LN transformer block (qkv, attention, out_proj, MLP 4x)."""
    return 2 * tokens * width * (3 * width + width + 8 * width) + 4 * tokens * seq * width


def c3_step_flop(batch):
    """Analytic FLOPs of one C3 step, counting exactly the GEMM / attention work the kernels do
    (DESIGN.md §4.6b).  Forward: the visual tower (24 blocks + patch embedding) and the last text
    block (66 prompts x 77 tokens; blocks 0-10 are a cached frozen prefix).  Backward, as
    ``_BlockFn.backward`` runs it under ``needs_input_grad`` (clip.py module docstring):
      * visual block 23 (its input feeds block 22's DoRA gradient): fc2 and fc1 input gradients
        (8 + 8 TD^2), out_proj weight and input gradients (2 + 2), attention backward (dP, dV, dQ,
        dK: 8 TND; the kernels' recompute of S is not counted), qkv input gradient (6) = 26 TD^2;
      * visual block 22 and text block 11 (nothing upstream trains): fc2, fc1 input gradients and
        the DoRA out_proj weight gradient only = 18 TD^2.
    LayerNorm / DoRA-weight / head backward work is not GEMM work and is left out."""
    T, D, N = batch * 257, 1024, 257
    Tt, Dt = 66 * 77, 768
    vis = _block_flops(T, D, N)
    txt = _block_flops(Tt, Dt, 77)
    fwd = 24 * vis + 2 * batch * 256 * 588 * 1024 + txt
    bwd = 26 * T * D * D + 8 * T * N * D + 18 * T * D * D + 18 * Tt * Dt * Dt
    return fwd + bwd


def c3_leg(dev, dtype="f32", batch=64, steps=10, warmup=3):
    """One C3 step rate (BASELINE configs[2]): CLIPHBA ViT-L/14, DoRA r=32 on the last 2 visual
    blocks and the last text out_proj (NEWP:484-544), MSE on 66-D targets, fused AdamW
    (NEWP:994-1001, 1181).  Random-init weights and synthetic images (OpenAI weights and THINGS
    images are absent offline).  f32 = the reference's precision (NEWP:274), bf16 the opt-in."""
    import torch
    import vit_amd
    T = torch.float32 if dtype == "f32" else torch.bfloat16
    torch.manual_seed(0)
    m = vit_amd.CLIPHBA(["class%d" % i for i in range(66)], "ViT-L/14", pos_embedding=True, compute_dtype=T)
    vit_amd.apply_dora_to_ViT(m, n_vision_layers=2, n_transformer_layers=1, r=32)
    vit_amd.switch_dora_layers(m, freeze_all=True, dora_state=True)
    m = m.to(dev)
    opt = vit_amd.FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=3e-4)
    x = torch.randn(batch, 3, 224, 224, device=dev)
    y = torch.randn(batch, 66, device=dev) * 0.5 + 1.0

    def step():
        opt.zero_grad(set_to_none=True)
        loss = vit_amd.mse_loss(m(x), y)
        loss.backward()
        opt.step()
        return loss

    for _ in range(warmup):
        loss = step()
    torch.cuda.synchronize(dev)
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    t0 = time.perf_counter()
    marks[0].record()
    for i in range(steps):
        loss = step()
        marks[i + 1].record()
    torch.cuda.synchronize(dev)
    el = time.perf_counter() - t0
    med = statistics.median(marks[i].elapsed_time(marks[i + 1]) for i in range(steps))
    fl = c3_step_flop(batch)
    tf = fl * steps / el / 1e12
    peak = PEAK_F32_TFLOPS if dtype == "f32" else PEAK_BF16_TFLOPS
    out = {"value": round(batch * steps / el, 2), "unit": "images/s", "ms_per_step": round(el / steps * 1e3, 3),
           "ms_per_step_median": round(med, 3), "batch": batch, "steps": steps, "warmup": warmup, "dtype": dtype,
           "step_tflop": round(fl / 1e12, 3), "achieved_tflops": round(tf, 1), "peak_tflops": round(peak, 1),
           "frac_of_peak": round(tf / peak, 4), "final_loss": round(float(loss.item()), 4)}
    del m, opt, x, y, loss
    torch.cuda.empty_cache()
    return out


# ----------------------------------------------------------------------------
# dry run: launcher + gradient averaging on CPU (gloo)
# ----------------------------------------------------------------------------

def dry_main(a):
    import torch
    import torch.distributed as dist
    from vit_amd import parallel
    rank, world, _ = parallel.init_from_env("gloo")
    n = 1 << 16
    flat = torch.full((n,), float(rank + 1)) + torch.arange(n, dtype=torch.float32) * 1e-3
    t0 = time.perf_counter()
    for _ in range(max(1, a.steps)):
        g = flat.clone()
        parallel.allreduce_flat(g, bucket_mb=0.0625)
    el = time.perf_counter() - t0
    expect = torch.full((n,), (world + 1) / 2.0) + torch.arange(n, dtype=torch.float32) * 1e-3
    ok = torch.allclose(g, expect, rtol=0, atol=1e-5)
    oks = [None] * world if world > 1 else [ok]
    if world > 1:
        dist.all_gather_object(oks, ok)
    if rank == 0:
        print(json.dumps({"metric": "dry", "n_gpus": world, "ranks_ok": oks, "grad_avg_ok": all(oks),
                          "steps": a.steps, "ms_per_step": round(el / max(1, a.steps) * 1e3, 3), "dry": True}),
              flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return 0 if all(oks) else 1


# ----------------------------------------------------------------------------
# the benchmark
class GpuTelemetry:
    """The GPU's clocks, power and temperature across the timed region (amdsmi gpu metrics, sampled on a
    thread every `interval` s), so a bench line from one box can be read against another's: a driver run
    and a builder run of the same tree differ by the box's sustained clock.  Every
    field is None when amdsmi or the metric is unavailable; nothing here touches the GPU's queues."""

    KEYS = ("current_gfxclk", "current_gfxclks", "average_gfxclk_frequency", "current_uclk", "current_socket_power",
            "average_socket_power", "temperature_hotspot", "temperature_mem", "average_gfx_activity",
            "average_umc_activity")

    def __init__(self, dev_index, interval=0.05):
        self.interval, self.samples, self.handle, self.bdf, self.err = interval, [], None, None, None
        try:
            import amdsmi
            import torch
            self.smi = amdsmi
            amdsmi.amdsmi_init()
            pr = torch.cuda.get_device_properties(dev_index)
            want = (int(pr.pci_domain_id), int(pr.pci_bus_id), int(pr.pci_device_id))
            for h in amdsmi.amdsmi_get_processor_handles():
                bdf = amdsmi.amdsmi_get_gpu_device_bdf(h)
                dom, bus, rest = bdf.split(":")
                if (int(dom, 16), int(bus, 16), int(rest.split(".")[0], 16)) == want:
                    self.handle, self.bdf = h, bdf
                    break
        except Exception as ex:  # noqa: BLE001
            self.err = str(ex)[:120]

    def _sample(self):
        m = self.smi.amdsmi_get_gpu_metrics_info(self.handle)
        out = {}
        for k in self.KEYS:
            v = m.get(k)
            vals = v if isinstance(v, (list, tuple)) else [v]
            vals = [float(x) for x in vals if isinstance(x, (int, float)) and 0 < x < 65535]
            if vals:
                out[k] = sum(vals) / len(vals)
        return out

    def start(self):
        import threading
        if self.handle is None:
            return self
        self._stop = threading.Event()

        def run():
            while not self._stop.is_set():
                try:
                    self.samples.append(self._sample())
                except Exception as ex:  # noqa: BLE001
                    self.err = str(ex)[:120]
                    return
                self._stop.wait(self.interval)
        self._t = threading.Thread(target=run, daemon=True)
        self._t.start()
        return self

    def stop(self):
        if self.handle is not None and hasattr(self, "_t"):
            self._stop.set()
            self._t.join()
        out = {"source": "amdsmi_get_gpu_metrics_info", "bdf": self.bdf, "samples": len(self.samples)}
        for k in self.KEYS:
            vals = [s[k] for s in self.samples if k in s]
            if vals:
                out[k] = {"mean": round(sum(vals) / len(vals), 1), "min": round(min(vals), 1), "max": round(max(vals), 1)}
        if self.err:
            out["error"] = self.err
        return out


# ----------------------------------------------------------------------------

PARAM_SAMPLE = 1 << 22  # elements of the flattened parameters written by --dump-outputs (16 MiB as float32)


def dump_outputs(out_dir, loss, logits, model):
    """What a caller of the timed step holds after its last call, as float32 .npy files: the step's
    loss (``loss``), its logits (``logits``, [B, classes]) and the parameters the optimizer left
    (``params_sample``: PARAM_SAMPLE elements of the parameters flattened in ``named_parameters()``
    order, at indices drawn once from a CPU generator with a fixed seed; all 86.6 M would be 346 MB)."""
    import numpy as np
    import torch
    os.makedirs(out_dir, exist_ok=True)
    flat = torch.cat([p.detach().float().reshape(-1) for _, p in model.named_parameters()])
    idx = torch.randint(0, flat.numel(), (PARAM_SAMPLE,), generator=torch.Generator().manual_seed(4321))
    arrays = {"loss": loss.detach().float().reshape(1), "logits": logits.detach().float(),
              "params_sample": flat[idx.to(flat.device)]}
    for name, t in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), t.cpu().numpy())


def roofline_leg(dev, main_stream, B, wg):
    """--full: the ``roofline`` key.  Times the weight-gradient kernel standalone and joins it with the
    in-step figures of the probe (``wg``, or None) and the committed counter files."""
    import torch
    from vit_amd import ops
    # --- standalone leg of the same kernel as the step runs it: the MLP weight-gradient pair
    #     (dW2 = dy^T act, M = B*197, 768 x 3072, and dW1 = dpre^T h2, 3072 x 768) as one grouped
    #     launch at the step's split, then its split-K slab sums (the block's reduction launch),
    #     alone on the GPU, HIP events on its stream; both launches count in the time
    M = B * 197
    bf = torch.bfloat16
    dy2, act = torch.randn(M, 768, device=dev).to(bf), torch.randn(M, 3072, device=dev).to(bf)
    dpre, h2 = torch.randn(M, 3072, device=dev).to(bf), torch.randn(M, 768, device=dev).to(bf)
    dw2, dw1 = torch.empty(768, 3072, device=dev), torch.empty(3072, 768, device=dev)

    def pair_step():
        cb = ops.ColBatch()
        ops.linear_wgrad_pair((dy2, act, dw2), (dpre, h2, dw1), cb)
        cb.launch()

    with torch.cuda.stream(main_stream):
        for _ in range(10):
            pair_step()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = 20
        e0.record()
        for _ in range(reps):
            pair_step()
        e1.record()
        torch.cuda.synchronize(dev)
    k_ms = e0.elapsed_time(e1) / reps
    k_flop = 2.0 * 2.0 * M * 3072 * 768
    k_tflops = k_flop / (k_ms * 1e-3) / 1e12
    traffic, traffic_src, traffic_sha = _pmc_traffic("pmc_traffic_wgrad_pair.json")
    mfma_busy, busy_src, busy_sha = _pmc_mfma_busy()
    src_sha = wgrad_src_sha()
    if wg is not None:
        roof = {"bound": "mfma", "kernel": "big::pp_kernel2 / pp_kernel (split-K weight-gradient GEMM, 256x256x32 "
                                           "ping-pong; fc2+fc1 and proj+qkv as grouped pairs; VIT_GEMM_WGRAD=11 selects "
                                           "the w4 kernel): every bf16 dW = dY^T X of the step",
                "achieved": wg["tflops"], "peak": round(PEAK_BF16_TFLOPS, 1), "unit": "TFLOP/s",
                "frac": round(wg["tflops"] / PEAK_BF16_TFLOPS, 4), "traffic": traffic,
                "measured": "in-step: HIP events around each launch on the side stream it runs on, over the timed "
                            "steps (its CUs are shared with the caller stream's kernels); the split-K slab sums run "
                            "in each block's single reduction launch, which the standalone leg includes",
                "launches_per_step": wg["launches_per_step"], "ms_per_step": wg["ms_per_step"],
                "avg_launch_ms": wg["avg_launch_ms"], "flop_per_step": wg["flop_per_step"],
                "standalone": {"shape": "MLP pair dW2 (768x3072) + dW1 (3072x768), M=%d, grouped launch + slab-sum "
                                        "launch" % M, "ms": round(k_ms, 4),
                               "achieved": round(k_tflops, 1), "frac": round(k_tflops / PEAK_BF16_TFLOPS, 4),
                               "flop_per_launch": k_flop},
                "traffic_unit": "HBM bytes per standalone pair (grouped launch + its slab sums; FETCH_SIZE x2 + "
                                "WRITE_SIZE, rocprofv3 --pmc passes, %s)" % traffic_src,
                "mfma_busy": mfma_busy,
                "mfma_busy_unit": "SQ_VALU_MFMA_BUSY_CYCLES / (1024 SIMDs x GRBM_GUI_ACTIVE/8) of the weight-gradient "
                                  "launches in the step's counter passes (dispatches serialized; %s)" % busy_src,
                # the counter files record the hash of the kernel sources they were taken on
                "counters_src_sha": {"kernel_sources": src_sha, "traffic": traffic_sha, "mfma_busy": busy_sha},
                "counters_match_kernel": traffic_sha == src_sha and busy_sha == src_sha}
    else:
        roof = {"bound": "mfma", "kernel": "MLP weight-gradient pair (ping-pong kernel), standalone",
                "achieved": round(k_tflops, 1), "peak": round(PEAK_BF16_TFLOPS, 1), "unit": "TFLOP/s",
                "frac": round(k_tflops / PEAK_BF16_TFLOPS, 4), "traffic": traffic, "kernel_ms": round(k_ms, 4),
                "flop_per_launch": k_flop}
    return roof


def main(a):
    import torch
    import torch.distributed as dist
    import vit_amd
    from vit_amd import parallel, ops

    rank, world, local = parallel.init_from_env("nccl")
    if world != a.gpus:
        print(f"warning: --gpus {a.gpus} but WORLD_SIZE {world}", file=sys.stderr)
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    torch.manual_seed(1234 + rank)

    B = a.batch
    model = vit_amd.create_model("vit_base_patch16_224", num_classes=1000, compute_dtype=torch.bfloat16).to(dev)
    flat = model.use_flat_grads(True)
    model.set_deferred_grad_join(True)  # gradients are read only after backward() returns
    vit_amd.set_wgrad_overlap(not a.no_overlap)
    opt = vit_amd.FusedSGD(model.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-4)
    x = torch.randn(B, 3, 224, 224, device=dev)
    y = torch.randint(0, 1000, (B,), device=dev)

    # world > 1: gradients averaged block by block during the backward (RCCL beside compute);
    # VIT_DDP_OVERLAP=0 falls back to bucketed all-reduces after the backward
    reducer = None
    if world > 1 and os.environ.get("VIT_DDP_OVERLAP", "1") != "0":
        reducer = parallel.OverlappedGradReduce(model)
    main_stream = torch.cuda.Stream(device=dev)
    red_events = []
    sgd_events = []  # HIP events around the optimizer's one launch in the timed steps (a kernel no round changes)

    last = {}  # --dump-outputs: the logits of the last timed step

    def step(record=False, sgd=False, keep=False):
        logits = model(x)
        if keep:
            last["logits"] = logits
        loss = vit_amd.cross_entropy(logits, y)
        del logits
        loss.backward()
        if world > 1:
            if record:
                r0 = torch.cuda.Event(enable_timing=True)
                r0.record()
            if reducer is not None:
                reducer.finish()
            else:
                parallel.allreduce_flat(flat, bucket_mb=64.0)
            if record:
                r1 = torch.cuda.Event(enable_timing=True)
                r1.record()
                red_events.append((r0, r1))
        if sgd:
            s0 = torch.cuda.Event(enable_timing=True)
            s0.record()
        opt.step()
        if sgd:
            s1 = torch.cuda.Event(enable_timing=True)
            s1.record()
            sgd_events.append((s0, s1))
        opt.zero_grad(set_to_none=True)
        return loss

    use_graph = a.graph and world == 1
    with torch.cuda.stream(main_stream):
        main_stream.wait_stream(torch.cuda.default_stream(dev))
        for _ in range(max(1, a.warmup)):
            loss = step()
        torch.cuda.synchronize(dev)
        warm_loss = float(loss.item())
        del loss
        graph = None
        if use_graph:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                gloss = step(keep=a.dump_outputs is not None)
            graph.replay()  # one untimed replay
            torch.cuda.synchronize(dev)

        # --- timed region: exactly K steps, barrier + synchronize on both sides.  HIP events on
        #     the caller's stream between steps give per-step times (median); with --full, HIP
        #     events around every weight-gradient launch (on the side stream it runs on) give that
        #     kernel's live in-step duration for the roofline line.
        probe = [] if (a.full and not a.no_probe and graph is None) else None
        ops.WGRAD_PROBE[0] = probe
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(a.steps + 1)]
        telem = GpuTelemetry(local) if a.full else None
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize(dev)
        if telem is not None:
            telem.start()
        t0 = time.perf_counter()
        marks[0].record()
        for i in range(a.steps):
            if graph is not None:
                graph.replay()
            else:
                tloss = step(record=a.full and world > 1, sgd=a.full,
                             keep=a.dump_outputs is not None and i == a.steps - 1)
            marks[i + 1].record()
        torch.cuda.synchronize(dev)
        if world > 1:
            dist.barrier()
        el = time.perf_counter() - t0
        box = telem.stop() if telem is not None else None
        ops.WGRAD_PROBE[0] = None
        if a.dump_outputs is not None and rank == 0 and a.steps > 0:
            dump_outputs(a.dump_outputs, gloss if graph is not None else tloss, last["logits"], model)
    step_ms = [marks[i].elapsed_time(marks[i + 1]) for i in range(a.steps)]
    el_rank = el
    per_rank = [el_rank]
    if world > 1:
        t = torch.tensor([el], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        el = float(t.item())
        per_rank = [None] * world
        dist.all_gather_object(per_rank, el_rank)
    final_loss = float(gloss.item()) if graph is not None else warm_loss

    # --- weight-gradient GEMMs (the step's dominant kernel class) in the timed steps
    wg = None
    if probe:
        durs = [(e0.elapsed_time(e1), fl) for e0, e1, fl, mfma in probe if mfma]
        per_step = len(durs) / a.steps
        tot_ms = sum(d for d, _ in durs) / a.steps
        tot_fl = sum(f for _, f in durs) / a.steps
        wg = {"launches_per_step": per_step, "ms_per_step": round(tot_ms, 3),
              "avg_launch_ms": round(tot_ms / per_step, 4), "flop_per_step": tot_fl,
              "tflops": round(tot_fl / (tot_ms * 1e-3) / 1e12, 1)}

    roof = roofline_leg(dev, main_stream, B, wg) if a.full else None
    red_ms = None
    if red_events:
        torch.cuda.synchronize(dev)
        red_ms = statistics.median(r0.elapsed_time(r1) for r0, r1 in red_events)
    if sgd_events:
        box["sgd_kernel_ms_median"] = round(statistics.median(s0.elapsed_time(s1) for s0, s1 in sgd_events), 4)
        box["sgd_kernel_note"] = ("the one FusedSGD launch per step (86.6 M params, 1.9 GB of HBM traffic), HIP events "
                                  "on the caller stream in the timed steps: unchanged code since round 1, so its "
                                  "time tracks the box's HBM clock")

    if rank != 0:
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        return 0
    imgs = world * B * a.steps
    value = imgs / el
    ms = el / a.steps * 1e3
    step_tflops = value / world * STEP_FLOP_PER_IMG / 1e12
    out = {
        "metric": "images/sec ViT-B/16 224 train step bs=256 (whole job)",
        "value": round(value, 2),
        "unit": "images/s",
        "n_gpus": world,
        "steps": a.steps,
        "warmup": a.warmup,
        "ms_per_step": round(ms, 3),
        "ms_per_step_median": round(statistics.median(step_ms), 3),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "bf16",
        "data": "synthetic randn images [256,3,224,224] f32 + randint labels, resident in HBM; random-init ViT-B/16",
        "config": {"workload": "ViT-B/16 224 train step (fwd+CE+bwd+SGD), BASELINE configs[1]",
                   "model": "vit_base_patch16_224", "global_batch": world * B, "per_gpu_batch": B,
                   "seq_len": 197, "parallelism": f"dp{world}", "launch": "hipgraph" if graph is not None else "eager",
                   "final_loss": round(final_loss, 4)},
        "step_mfma": {"achieved_tflops": round(step_tflops, 1), "frac": round(step_tflops / PEAK_BF16_TFLOPS, 4),
                      "flop_per_img": STEP_FLOP_PER_IMG},
    }
    if a.full:
        out["roofline"] = roof
        out["box"] = box
    if world > 1:
        out["per_rank_s"] = [round(v, 4) for v in per_rank]
        out["allreduce_exposed_ms_median"] = None if red_ms is None else round(red_ms, 3)
        out["allreduce"] = "overlapped per block (side stream)" if reducer is not None else "bucketed after backward"
    if a.full and world == 1 and not a.no_c3:
        # extra key, not the headline: BASELINE configs[2] (C3) at the reference's fp32 and the bf16 opt-in
        out["c3"] = {"workload": "CLIP-HBA ViT-L/14 + DoRA train step (fwd+MSE+bwd+AdamW), BASELINE configs[2]",
                     "metric": "images/sec", "data": "synthetic images [64,3,224,224] + 66-D targets; random-init "
                                                     "weights (OpenAI weights absent offline)",
                     "f32": c3_leg(dev, "f32"), "bf16": c3_leg(dev, "bf16")}
    if a.full and world == 1 and not a.no_cpu:
        out["cpu_baseline"] = cpu_baseline(a.cpu_seconds)
    print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(args.gpus, sys.argv[1:]))
    sys.exit(dry_main(args) if args.dry else main(args))
