"""Config C3 with the frozen visual prefix cached against the same step uncached.

CLIP-HBA ViT-L/14, DoRA r = 32 on the last two visual blocks and the last text block, MSE, AdamW, bs = 64
(config C3), in fp32 and bf16.  Per dtype, in one process, cached and uncached alternate over --rounds
rounds (>= 3); the record holds every round, the medians, the round-to-round spread and the ratio:

  * the training step over shuffled batches of a --train image set (the cached step: ``cache.take(idx)`` +
    ``forward(visual_prefix=...)``; the uncached one: ``images[idx]`` + ``forward(images)``),
  * ``sweep.evaluate`` over 362 test images and ``sweep.behavioral_rsa`` over 48 inference images,
  * the cache build itself.

A third leg times the gather alone on one [n, 257, 1024] f32 tensor, 64 rows a call: ``take()`` (host index
check and the index's copy included), and with the index already on the device ``vit_gather_blocks``,
``vit_gather_rows`` and ``torch.index_select``.

Without --leg this is a driver: every leg runs as a child process of its own under a time limit, the first
failure stops the run, and the GPU clocks ``rocm-smi --showclocks`` reports are recorded before and after.
Records go to --out (one JSON file per leg).

    python tools/bench_clip_cached.py [--out profiles/r13] [--rounds 3] [--steps 8] [--leg f32|bf16|gather]
                                      [--adapter dora|lora]

``--cls-tail`` adds the visual tower's class-token tail (``CLIP.set_cls_tail``): every round runs
uncached and cached with the tail off and then on, on the same model in the same process; the record gains the
``*_tail`` series, ``cls_tail_speedup`` for the cached and the uncached pass and the on-against-off relative
difference of a batch's predictions; the records are named ``bench_clip_cached_clstail_{dtype}.json``.

``--eot-tail`` does the same for the text tower's EOT tail (``CLIP.set_eot_tail``): the ``*_tail``
series and ``eot_tail_speedup`` are then that switch's; given together with ``--cls-tail`` the class-token tail
stays on throughout and the EOT tail alone alternates.  Records: ``bench_clip_cached_eottail[_clstail]_{dtype}.json``.

``--f32-matmul highest|high`` sets the fp32 GEMM arithmetic of the whole run (``vit_amd.set_float32_matmul_precision``;
``high`` = bf16x3).  ``--f32-ab`` alternates the two instead, as the tails are alternated (the
``*_tail`` series are then the ``high`` passes, on prefix caches built in ``high``; ``--cls-tail`` keeps that tail
on throughout): ``f32_high_speedup``, records ``bench_clip_cached_f32high[_clstail]_{dtype}.json``.

``--f32-attention highest|high`` sets the fp32 attention arithmetic of the whole run
(``vit_amd.set_float32_attention_precision``) and ``--f32-attention-ab`` alternates the two the way
``--f32-ab`` alternates the GEMM mode, the GEMMs staying at ``--f32-matmul``: ``f32_attention_high_speedup``, records
``bench_clip_cached[_f32high]_f32attnhigh[_clstail]_{dtype}.json``.

``--f32-presplit`` (with ``--f32-matmul high``) keeps pre-split images of the frozen fp32 weights for the whole run
(``set_float32_matmul_precision("high", presplit_weights=True)``); ``--f32-presplit-ab`` alternates
in-loop ``high`` (the plain series) and pre-split ``high`` (the ``*_tail`` series) on the same prefix caches, which
both read as hits: ``f32_presplit_speedup``, ``weight_image_bytes``, records
``bench_clip_cached_f32high_presplit[_clstail]_{dtype}.json``.
``--f32-attention-presplit`` (with ``--f32-attention high``) carries pre-split images through attention in the
forward-only blocks; ``--f32-attention-presplit-ab`` alternates attention ``high`` without and with them,
the GEMMs as the ``--f32-matmul`` flags say (the baseline: ``--f32-matmul high --f32-presplit --f32-presplit-act``), on
one set of caches: ``f32_attention_presplit_speedup``, ``cache_build_seconds_ab``.
``--f32-presplit-act`` (with ``--f32-matmul high --f32-presplit``) adds pre-split activation images in the forward-only
blocks; ``--f32-presplit-act-ab`` (with ``--f32-matmul high``) alternates pre-split weights and
pre-split weights + activations, one set of caches again, and times the prefix-cache build itself in either mode,
alternating: ``f32_presplit_act_speedup``, ``cache_build_seconds_ab``, records
``bench_clip_cached_f32high_presplitact[_clstail]_{dtype}.json``.

``--adapter lora`` puts the reference's LoRA pair (NEWP:339-404) where DoRA stands; its records are named
``bench_clip_cached_lora_{dtype}.json``.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "vit-project_amd"))

LEGS = ("f32", "bf16", "gather")
LEG_TIMEOUT = {"f32": 420, "bf16": 300, "gather": 120}  # seconds, each child's own limit


def _summary(vals):
    med = statistics.median(vals)
    return {"rounds": [round(v, 4) for v in vals], "median": round(med, 4),
            "spread": round((max(vals) - min(vals)) / med, 4)}


def _timed(fn, sync):
    sync()
    t0 = time.perf_counter()
    out = fn()
    sync()
    return time.perf_counter() - t0, out


def model_leg(a, dtype_name):
    import numpy as np
    import torch
    import vit_amd
    from vit_amd import sweep as S
    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    dtype = {"f32": torch.float32, "bf16": torch.bfloat16}[dtype_name]
    torch.manual_seed(0)
    m = vit_amd.CLIPHBA([f"c{i}" for i in range(66)], "ViT-L/14", pos_embedding=True, compute_dtype=dtype)
    if a.adapter == "lora":
        vit_amd.apply_lora_to_ViT(m, n_vision_layers=2, n_transformer_layers=1, r=32)
        vit_amd.unfreeze_lora_layers(m, freeze_all=True)
    else:
        vit_amd.apply_dora_to_ViT(m, n_vision_layers=2, n_transformer_layers=1, r=32)
        vit_amd.switch_dora_layers(m, freeze_all=True, dora_state=True)
    m = m.to(dev)
    opt = vit_amd.FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=3e-4)
    crit = vit_amd.MSELoss()
    g = torch.Generator().manual_seed(1)
    mk = lambda n: (torch.randn(n, 3, 224, 224, generator=g).to(dev),
                    (torch.randn(n, 66, generator=g) * 0.5 + 1.0).to(dev))
    data = dict(train=mk(a.train), test=mk(362), inference=mk(48)[0])
    r = np.random.default_rng(0).random((48, 48))
    data["reference_rdm"] = (r + r.T) / 2
    tr_x, tr_y = data["train"]
    te_x, te_y = data["test"]

    t_build, caches = _timed(lambda: S.prefix_caches_for(m, data, None, a.batch), sync)
    rows = sum(c.x.shape[0] for c in caches.values())
    order = torch.Generator().manual_seed(2)
    # a shuffled batch's predictions, from the cache (built in order, in chunks) against the images themselves:
    # other GEMM row counts in the frozen blocks, so equal to rounding, not bit for bit, in f32 (stream-K)
    with torch.no_grad():
        idx = torch.randperm(a.train, generator=torch.Generator().manual_seed(4))[:a.batch]
        pu, pc = m(tr_x[idx]).double(), m(visual_prefix=caches["train"].take(idx)).double()
        pred_diff = float((pc - pu).abs().max() / pu.abs().max())

    fixed = caches["train"].take(torch.arange(a.batch))
    ab = (a.f32_ab or a.f32_attention_ab or a.f32_presplit_ab or a.f32_presplit_act_ab
          or a.f32_attention_presplit_ab)  # an fp32 mode alternates
    tails = (False, True) if (a.cls_tail or a.eot_tail or ab) else (False,)
    # the switch that alternates: the EOT tail if asked for (the class-token tail then stays as --cls-tail says)
    set_tail = m.clip_model.set_eot_tail if a.eot_tail else m.clip_model.set_cls_tail
    tail_key = "eot_tail" if a.eot_tail else "cls_tail"
    if a.eot_tail or ab:
        m.clip_model.set_cls_tail(a.cls_tail)
    if ab:  # the fp32 GEMM (or attention) mode alternates; each mode reads the prefix caches built in it
        set_mode = (vit_amd.set_float32_attention_precision if a.f32_attention_ab
                    else vit_amd.set_float32_matmul_precision)
        if a.f32_attention_presplit_ab:  # attention "high" throughout, images through it off and on: the same bits
            set_mode = lambda mode: vit_amd.set_float32_attention_precision("high", presplit=mode == "high")
            by_mode = {False: caches, True: caches}
        elif a.f32_presplit_act_ab:  # weight images throughout, activation images off and on: the same bits again
            set_mode = lambda mode: vit_amd.set_float32_matmul_precision("high", presplit_weights=True,
                                                                         presplit_activations=mode == "high")
            by_mode = {False: caches, True: caches}
        elif a.f32_presplit_ab:  # in-loop "high" against pre-split "high": the same bits, so the same caches
            set_mode = lambda mode: vit_amd.set_float32_matmul_precision("high", presplit_weights=mode == "high")
            by_mode = {False: caches, True: caches}
        else:
            set_mode("high")
            by_mode = {False: caches, True: S.prefix_caches_for(m, data, None, a.batch)}
        set_mode("highest")
        tail_key = ("f32_attention_presplit" if a.f32_attention_presplit_ab else
                    "f32_presplit_act" if a.f32_presplit_act_ab else "f32_presplit" if a.f32_presplit_ab
                    else "f32_attention_high" if a.f32_attention_ab else "f32_high")

        def set_tail(on):
            nonlocal caches
            set_mode("high" if on else "highest")
            caches = by_mode[on]
    vname = lambda c, t: ("cached" if c else "uncached") + ("_tail" if t else "")
    tail_diff = None
    if len(tails) > 1:  # the same batch's predictions with the tail on against off (cached pass)
        with torch.no_grad():
            p0 = m(visual_prefix=caches["train"].take(idx)).double()
            set_tail(True)
            pt = m(visual_prefix=caches["train"].take(idx)).double()
            set_tail(False)
        tail_diff = float((pt - p0).abs().max() / p0.abs().max())

    def steps(cached, n):
        m.train()
        loss = None
        for _ in range(n):
            idx = torch.randperm(a.train, generator=order)[:a.batch]
            x, y = tr_x[idx], tr_y[idx]  # as sweep._batches: the batch exists before the step is queued
            opt.zero_grad(set_to_none=True)
            if cached == "fixed":  # the cached step less its gather: one batch's rows, taken once
                pred = m(visual_prefix=fixed)
            else:
                pred = m(visual_prefix=caches["train"].take(idx)) if cached else m(x)
            loss = crit(pred, y)
            loss.backward()
            opt.step()
        return loss

    passes = {
        "train_step_images_per_sec": None,
        "evaluate_362_seconds": lambda c: S.evaluate(m, te_x, te_y, a.batch, crit,
                                                     cache_visual_prefix=caches["test"] if c else False),
        "rsa_48_seconds": lambda c: S.behavioral_rsa(m, data["inference"], data["reference_rdm"],
                                                     cache_visual_prefix=caches["inference"] if c else False),
    }
    for t in tails:  # every shape of the timed windows, once
        set_tail(t)
        for c in (False, True):
            steps(c, a.warmup)
            passes["evaluate_362_seconds"](c)
            passes["rsa_48_seconds"](c)
    res = {k: {vname(c, t): [] for t in tails for c in (False, True)} for k in passes}
    host_ms = {"uncached": [], "cached": []}
    no_gather = []
    for _ in range(a.rounds):
        for t in tails:
            set_tail(t)
            for c in (False, True):
                name = vname(c, t)
                dt, loss = _timed(lambda: steps(c, a.steps), sync)
                assert torch.isfinite(loss)
                res["train_step_images_per_sec"][name].append(a.batch * a.steps / dt)
                for k in ("evaluate_362_seconds", "rsa_48_seconds"):
                    dt, _ = _timed(lambda: passes[k](c), sync)
                    res[k][name].append(dt)
        set_tail(False)
        dt, _ = _timed(lambda: steps("fixed", a.steps), sync)
        no_gather.append(a.batch * a.steps / dt)
    # the host's cost of queueing one step, the GPU idle when it starts (inside the windows above the index
    # copy at the head of a step waits for the stream, so host time there is wall time): where this is
    # close to the step's wall time the step is bound by the launches, not by the kernels
    for name, c in (("uncached", False), ("cached", True)):
        for _ in range(7):
            sync()
            t0 = time.perf_counter()
            steps(c, 1)
            host_ms[name].append((time.perf_counter() - t0) * 1e3)
            sync()
    # the clocks while the uncached step keeps the GPU busy (rocm-smi in a thread, steps until it returns)
    import threading
    load_clocks = []
    th = threading.Thread(target=lambda: load_clocks.extend(_clocks()))
    th.start()
    while th.is_alive():
        steps(False, 2)
    th.join()
    sync()
    rec = {"metric": f"CLIP-HBA ViT-L/14 + {'LoRA' if a.adapter == 'lora' else 'DoRA'} (config C3), frozen visual "
                     "prefix cached vs uncached, one process", "adapter": a.adapter,
           "clocks_under_load": load_clocks,
           "dtype": dtype_name, "batch": a.batch, "steps_per_round": a.steps, "rounds": a.rounds,
           "train_images": a.train, "cache_rows": rows, "cache_gib": round(sum(c.nbytes for c in caches.values()) / 2 ** 30, 3),
           "cache_build_seconds": round(t_build, 3), "shuffled_batch_prediction_rel_diff": pred_diff,
           "cache_counters": {k: dict(hits=c.hits, bypassed=c.bypassed, builds=c.builds) for k, c in caches.items()},
           "peak_mem_gib": round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 2)}
    rec["train_step_ms"] = {n: round(1e3 * a.batch / statistics.median(res["train_step_images_per_sec"][n]), 3)
                            for n in host_ms}
    rec["train_step_host_enqueue_ms"] = {n: _summary(v) for n, v in host_ms.items()}
    for k, v in res.items():
        u, c = _summary(v["uncached"]), _summary(v["cached"])
        ratio = c["median"] / u["median"] if k.endswith("per_sec") else u["median"] / c["median"]
        rec[k] = {"uncached": u, "cached": c, "cached_speedup": round(ratio, 3)}
        if len(tails) > 1:
            gain = {}
            for base in ("uncached", "cached"):
                rec[k][base + "_tail"] = s = _summary(v[base + "_tail"])
                b = rec[k][base]["median"]
                gain[base] = round(s["median"] / b if k.endswith("per_sec") else b / s["median"], 4)
            rec[k][tail_key + "_speedup"] = gain
    if ab:  # the 48 images' RSA correlation in either mode, on the parameters as the timed steps left them
        rho = {}
        for t in tails:
            set_tail(t)
            rho[("attnimg" if t else "attn") if a.f32_attention_presplit_ab else ("act" if t else "presplit") if a.f32_presplit_act_ab else ("presplit" if t else "high") if a.f32_presplit_ab else ("high" if t else "highest")] = float(S.behavioral_rsa(m, data["inference"], data["reference_rdm"])[0])
        set_tail(False)
        rec[tail_key + "_rsa_rho"] = rho
    if len(tails) > 1:
        rec[tail_key + "_prediction_rel_diff"] = tail_diff
        rec[tail_key + "_prediction_bound"] = 1e-3 if dtype_name == "f32" else 3e-2
        rec["cls_tail_throughout"] = bool((a.eot_tail or ab) and a.cls_tail)
    if a.f32_presplit_act_ab or a.f32_attention_presplit_ab:  # the prefix-cache build itself, off against on
        bk = ("attn", "attnimg") if a.f32_attention_presplit_ab else ("presplit", "act")
        builds = {k: [] for k in bk}
        for _ in range(a.rounds):
            for t in tails:
                set_tail(t)
                dt, fresh = _timed(lambda: S.prefix_caches_for(m, data, None, a.batch), sync)
                builds[bk[t]].append(dt)
        set_tail(False)
        rec["cache_build_seconds_ab"] = {k: _summary(v) for k, v in builds.items()}
        rec["cache_build_rows_bit_equal"] = bool(torch.equal(fresh["train"].take(idx), caches["train"].take(idx)))
    if a.f32_presplit_ab or a.f32_presplit_act_ab:
        set_tail(True)
        with torch.no_grad():
            m(visual_prefix=caches["train"].take(idx))
        rec["weight_image_bytes"] = vit_amd.weight_image_bytes(m)
        set_tail(False)
    rec["f32_presplit"] = "ab" if a.f32_presplit_ab else vit_amd.get_float32_matmul_presplit()
    rec["f32_presplit_act"] = "ab" if a.f32_presplit_act_ab else vit_amd.get_float32_matmul_presplit_activations()
    rec["f32_matmul"], rec["f32_attention"] = (vit_amd.get_float32_matmul_precision(),
                                               "ab" if a.f32_attention_ab else vit_amd.get_float32_attention_precision())
    rec["f32_attention_presplit"] = "ab" if a.f32_attention_presplit_ab else vit_amd.get_float32_attention_presplit()
    rec["train_step_images_per_sec"]["cached_without_gather"] = _summary(no_gather)
    return rec


def gather_leg(a):
    import torch
    from vit_amd import _lib as L
    from vit_amd import ops
    from vit_amd.prefix_cache import VisualPrefixCache
    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    n, N, W, b = a.gather_rows, 257, 1024, a.batch
    cache = VisualPrefixCache()
    cache.x = torch.randn(n, N, W, device=dev)
    g = torch.Generator().manual_seed(3)
    idxs = [torch.randperm(n, generator=g)[:b] for _ in range(a.gather_calls)]
    didxs = [i.to(dev) for i in idxs]
    out = torch.empty(b, N, W, device=dev)
    src2, out2 = cache.x.view(n, N * W), out.view(b, N * W)
    st = L.stream_ptr(dev)
    variants = {
        "take_cpu_index": lambda k: cache.take(idxs[k]),
        "vit_gather_blocks": lambda k: L.call("vit_gather_blocks", b, N * W, L.ptr(cache.x), L.ptr(didxs[k]), L.ptr(out), st),
        "vit_gather_rows": lambda k: ops.gather_rows(src2, didxs[k], out=out2),
        "torch_index_select": lambda k: torch.index_select(cache.x, 0, didxs[k], out=out),
    }
    want = torch.index_select(cache.x, 0, didxs[0])
    for name, fn in variants.items():
        got = fn(0)
        got = out if got is None else got
        assert torch.equal(got.view(b, N, W), want), name
    us = {k: [] for k in variants}
    for _ in range(max(a.rounds, 5)):
        for name, fn in variants.items():
            dt, _ = _timed(lambda: [fn(k) for k in range(a.gather_calls)], sync)
            us[name].append(dt / a.gather_calls * 1e6)
    moved = 2 * b * N * W * 4
    rec = {"metric": "gather of 64 cached [257, 1024] f32 rows, microseconds per call (calls queued back to back, one "
                     "synchronise per round)", "source_rows": n, "rows_per_call": b, "calls_per_round": a.gather_calls,
           "bytes_moved_per_call": moved}
    for k, v in us.items():
        s = _summary(v)
        s["gb_per_sec_at_median"] = round(moved / s["median"] / 1e3, 1)
        rec[k] = s
    return rec


def _clocks():
    try:
        p = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30)
        return [ln.strip() for ln in p.stdout.splitlines() if "clk" in ln.lower()][:16] or ["not reported"]
    except (OSError, subprocess.SubprocessError) as e:
        return [f"not available: {type(e).__name__}"]


def driver(a):
    os.makedirs(a.out, exist_ok=True)
    clocks = {"before": _clocks()}
    for leg in a.legs.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--out", a.out, "--rounds", str(a.rounds),
               "--steps", str(a.steps), "--warmup", str(a.warmup), "--batch", str(a.batch), "--train", str(a.train),
               "--gather-rows", str(a.gather_rows), "--gather-calls", str(a.gather_calls), "--adapter", a.adapter]
        if a.cls_tail:
            cmd.append("--cls-tail")
        if a.eot_tail:
            cmd.append("--eot-tail")
        if a.f32_ab:
            cmd.append("--f32-ab")
        if a.f32_matmul:
            cmd += ["--f32-matmul", a.f32_matmul]
        if a.f32_presplit:
            cmd.append("--f32-presplit")
        if a.f32_presplit_ab:
            cmd.append("--f32-presplit-ab")
        if a.f32_presplit_act:
            cmd.append("--f32-presplit-act")
        if a.f32_presplit_act_ab:
            cmd.append("--f32-presplit-act-ab")
        if a.f32_attention_ab:
            cmd.append("--f32-attention-ab")
        if a.f32_attention:
            cmd += ["--f32-attention", a.f32_attention]
        if a.f32_attention_presplit:
            cmd.append("--f32-attention-presplit")
        if a.f32_attention_presplit_ab:
            cmd.append("--f32-attention-presplit-ab")
        print("leg", leg, flush=True)
        rc = subprocess.run(cmd, timeout=LEG_TIMEOUT[leg] * a.timeout_scale * (2 if (a.cls_tail or a.eot_tail or a.f32_ab or a.f32_attention_ab or a.f32_presplit_ab or a.f32_presplit_act_ab or a.f32_attention_presplit_ab) else 1)).returncode  # TimeoutExpired ends the run
        if rc != 0:
            print(f"leg {leg} failed with exit code {rc}: stopping", flush=True)
            return rc
    clocks["after"] = _clocks()
    with open(os.path.join(a.out, "clocks.json"), "w") as fh:
        json.dump(clocks, fh, indent=1)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=LEGS)
    ap.add_argument("--legs", default=",".join(LEGS), help="the driver's legs, in order")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13"))
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--train", type=int, default=256, help="training images (1444 in the sweep; the step sees 64 a time)")
    ap.add_argument("--gather-rows", type=int, default=512)
    ap.add_argument("--gather-calls", type=int, default=100)
    ap.add_argument("--timeout-scale", type=float, default=1.0)
    ap.add_argument("--adapter", choices=["dora", "lora"], default="dora",
                    help="the adapter on the three out_proj layers: DoRA (config C3) or the reference's LoRA pair")
    ap.add_argument("--cls-tail", action="store_true",
                    help="also run every pass with the visual tower's class-token tail on, alternated with off")
    ap.add_argument("--eot-tail", action="store_true",
                    help="also run every pass with the text tower's EOT tail on, alternated with off (with --cls-tail: "
                         "that tail on throughout)")
    ap.add_argument("--f32-matmul", choices=["highest", "high"], default=None,
                    help="fp32 GEMM arithmetic of the whole run (high = bf16x3)")
    ap.add_argument("--f32-ab", action="store_true",
                    help="alternate the fp32 GEMM modes highest and high (with --cls-tail: that tail on throughout)")
    ap.add_argument("--f32-presplit", action="store_true",
                    help="with --f32-matmul high: pre-split images of the frozen fp32 weights for the whole run")
    ap.add_argument("--f32-presplit-act", action="store_true",
                    help="with --f32-matmul high --f32-presplit: pre-split activation images in forward-only blocks")
    ap.add_argument("--f32-presplit-act-ab", action="store_true",
                    help="with --f32-matmul high: alternate pre-split weights and pre-split weights + activations")
    ap.add_argument("--f32-presplit-ab", action="store_true",
                    help="with --f32-matmul high: alternate in-loop high and pre-split high (with --cls-tail: that tail "
                         "on throughout)")
    ap.add_argument("--f32-attention", choices=["highest", "high"], default=None,
                    help="fp32 attention arithmetic of the whole run (high = bf16x3 in the resident f32 kernels)")
    ap.add_argument("--f32-attention-ab", action="store_true",
                    help="alternate the fp32 attention modes highest and high, the GEMMs as --f32-matmul says (with "
                         "--cls-tail: that tail on throughout)")
    ap.add_argument("--f32-attention-presplit", action="store_true",
                    help="with --f32-attention high: pre-split images through attention in forward-only blocks")
    ap.add_argument("--f32-attention-presplit-ab", action="store_true",
                    help="alternate attention high without and with images through attention, the GEMMs as the "
                         "--f32-matmul flags say")
    a = ap.parse_args()
    if a.f32_attention_presplit and a.f32_attention != "high":
        ap.error("--f32-attention-presplit needs --f32-attention high")
    if a.f32_attention_presplit_ab and (a.eot_tail or a.f32_ab or a.f32_attention_ab or a.f32_presplit_ab
                                        or a.f32_presplit_act_ab or a.f32_attention == "highest"):
        ap.error("--f32-attention-presplit-ab alternates the images through attention alone, attention at high")
    if a.rounds < 3:
        ap.error("--rounds must be at least 3: the spread is part of the record")
    if a.f32_ab and (a.eot_tail or a.f32_matmul):
        ap.error("--f32-ab alternates the fp32 GEMM mode alone")
    if a.f32_attention_ab and (a.eot_tail or a.f32_ab or a.f32_attention):
        ap.error("--f32-attention-ab alternates the fp32 attention mode alone")
    if (a.f32_presplit or a.f32_presplit_ab) and a.f32_matmul != "high":
        ap.error("--f32-presplit / --f32-presplit-ab need --f32-matmul high")
    if a.f32_presplit_ab and (a.eot_tail or a.f32_ab or a.f32_attention_ab or a.f32_presplit):
        ap.error("--f32-presplit-ab alternates pre-splitting alone")
    if (a.f32_presplit_act and not a.f32_presplit) or (a.f32_presplit_act_ab and a.f32_matmul != "high"):
        ap.error("--f32-presplit-act needs --f32-matmul high --f32-presplit; --f32-presplit-act-ab --f32-matmul high")
    if a.f32_presplit_act_ab and (a.eot_tail or a.f32_ab or a.f32_attention_ab or a.f32_presplit_ab or a.f32_presplit
                                  or a.f32_presplit_act):
        ap.error("--f32-presplit-act-ab alternates the activation images alone")
    if a.leg is None:
        sys.exit(driver(a))
    if a.f32_matmul:
        import vit_amd
        vit_amd.set_float32_matmul_precision(a.f32_matmul, presplit_weights=a.f32_presplit or a.f32_presplit_act_ab,
                                             presplit_activations=a.f32_presplit_act)
    if a.f32_attention:
        import vit_amd
        vit_amd.set_float32_attention_precision(a.f32_attention, presplit=a.f32_attention_presplit)
    rec = gather_leg(a) if a.leg == "gather" else model_leg(a, a.leg)
    os.makedirs(a.out, exist_ok=True)
    tag = (("" if a.adapter == "dora" else f"_{a.adapter}") + ("_eottail" if a.eot_tail else "")
           + ("_f32high" if (a.f32_ab or a.f32_matmul == "high") else "")
           + ("_presplitact" if (a.f32_presplit_act or a.f32_presplit_act_ab) else
              "_presplit" if (a.f32_presplit or a.f32_presplit_ab) else "")
           + ("_f32attnhigh" if (a.f32_attention_ab or a.f32_attention == "high") else "")
           + ("_attnpresplit" if (a.f32_attention_presplit or a.f32_attention_presplit_ab) else "")
           + ("_clstail" if a.cls_tail else ""))
    name = "gather_blocks.json" if a.leg == "gather" else f"bench_clip_cached{tag}_{a.leg}.json"
    with open(os.path.join(a.out, name), "w") as fh:
        json.dump(rec, fh, indent=1)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
