"""CLIP-HBA ViT-L/14@336px + DoRA fp32 train step (config C3's recipe -- r = 32 on the last two visual blocks
and the last text block, MSE, AdamW -- on the 336-pixel tower: 577 visual tokens), with attention past 288
tokens on the streamed f32 kernels against the generic ones (vit_sdpa_long_config(1) / (0)), alternated over
--rounds rounds in one process.  Prints one JSON line: the median images/s of each variant and their ratio.

    python tools/bench_clip_long.py [--batch 16] [--steps 5] [--warmup 2] [--rounds 3] [--steps-generic 2]
                                    [--f32-matmul highest|high] [--f32-ab] [--f32-presplit] [--f32-presplit-ab]
                                    [--f32-presplit-act] [--f32-presplit-act-ab]
                                    [--f32-attention highest|high] [--f32-attention-ab] [--f32-attention-long]
                                    [--f32-attention-presplit] [--f32-attention-presplit-ab]

``--f32-matmul`` sets the fp32 GEMM arithmetic of the run (``high`` = bf16x3); ``--f32-ab``
alternates ``highest`` and ``high`` instead, both on the streamed attention kernels.  ``--f32-attention`` and
``--f32-attention-ab`` do the same with the fp32 attention mode: at 577 tokens only the text
tower's 77-token attention takes the bf16x3 kernels, the visual tower's streamed f32 kernels stay exact --
unless ``--f32-attention-long`` is given too: then ``high`` means
``set_float32_attention_precision("high", long_sequences=True)`` and the visual tower's streamed attention takes
the bf16x3 kernels as well.  With ``--f32-attention-ab`` the record then also holds ``pred_distance``, the largest
difference between the two modes' predictions on the batch over the largest prediction, taken before the first step.
``--f32-presplit`` (with ``--f32-matmul high``) keeps pre-split images of the frozen fp32 weights;
``--f32-presplit-ab`` alternates in-loop ``high`` and pre-split ``high`` (sides ``high`` / ``presplit``), the
attention as ``--f32-attention`` says, and records whether the two sides' predictions are the same bits.
``--f32-attention-presplit`` (with ``--f32-attention high``) carries pre-split images through attention
in the forward-only blocks; ``--f32-attention-presplit-ab`` alternates attention ``high`` without and with them (sides
``attn`` / ``attnimg``), ``long_sequences`` as ``--f32-attention-long`` says on both sides and the GEMMs as the
``--f32-matmul`` flags say (the baseline: ``--f32-matmul high --f32-presplit --f32-presplit-act --f32-attention-long``),
and records whether the two sides' predictions are the same bits.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "vit-project_amd"))

import torch  # noqa: E402

import vit_amd  # noqa: E402
from vit_amd import _lib as L  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--steps-generic", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--prompts", type=int, default=66)
    ap.add_argument("--f32-matmul", choices=["highest", "high"], default=None)
    ap.add_argument("--f32-ab", action="store_true")
    ap.add_argument("--f32-presplit", action="store_true", help="with --f32-matmul high: pre-split weight images")
    ap.add_argument("--f32-presplit-ab", action="store_true", help="alternate in-loop high and pre-split high")
    ap.add_argument("--f32-presplit-act", action="store_true",
                    help="with --f32-matmul high --f32-presplit: pre-split activation images (DESIGN 4.26)")
    ap.add_argument("--f32-presplit-act-ab", action="store_true",
                    help="alternate pre-split weights and pre-split weights + activations")
    ap.add_argument("--f32-attention", choices=["highest", "high"], default=None)
    ap.add_argument("--f32-attention-ab", action="store_true")
    ap.add_argument("--f32-attention-long", action="store_true",
                    help="with --f32-attention high or --f32-attention-ab: high also covers streamed attention")
    ap.add_argument("--f32-attention-presplit", action="store_true",
                    help="with --f32-attention high: pre-split images through attention (DESIGN 4.27)")
    ap.add_argument("--f32-attention-presplit-ab", action="store_true",
                    help="alternate attention high without and with images through attention")
    a = ap.parse_args()
    if a.f32_ab + a.f32_attention_ab + a.f32_presplit_ab + a.f32_presplit_act_ab + a.f32_attention_presplit_ab > 1:
        ap.error("one switch alternates at a time")
    if a.f32_attention_presplit and a.f32_attention != "high":
        ap.error("--f32-attention-presplit needs --f32-attention high")
    if a.f32_attention_presplit_ab and a.f32_attention not in (None, "high"):
        ap.error("--f32-attention-presplit-ab runs attention high on both sides")
    if a.f32_presplit and a.f32_matmul != "high":
        ap.error("--f32-presplit needs --f32-matmul high")
    if a.f32_presplit_act and not a.f32_presplit:
        ap.error("--f32-presplit-act needs --f32-matmul high --f32-presplit")
    if a.f32_attention_long and not (a.f32_attention == "high" or a.f32_attention_ab or a.f32_attention_presplit_ab):
        ap.error("--f32-attention-long needs --f32-attention high, --f32-attention-ab or --f32-attention-presplit-ab")

    def set_attention(mode, presplit=None):
        high = mode == "high"
        vit_amd.set_float32_attention_precision(
            mode, long_sequences=a.f32_attention_long and high,
            presplit=high and (a.f32_attention_presplit if presplit is None else presplit))
    if a.f32_matmul:
        vit_amd.set_float32_matmul_precision(a.f32_matmul, presplit_weights=a.f32_presplit,
                                             presplit_activations=a.f32_presplit_act)
    if a.f32_attention:
        set_attention(a.f32_attention)
    set_mode = set_attention if a.f32_attention_ab else vit_amd.set_float32_matmul_precision
    sides = ("highest", "high")
    if a.f32_presplit_ab:
        sides = ("high", "presplit")
        set_mode = lambda name: vit_amd.set_float32_matmul_precision("highest" if name == "highest" else "high",
                                                                     presplit_weights=name == "presplit")
    if a.f32_presplit_act_ab:
        sides = ("presplit", "act")
        set_mode = lambda name: vit_amd.set_float32_matmul_precision(
            "highest" if name == "highest" else "high", presplit_weights=name != "highest",
            presplit_activations=name == "act")
    if a.f32_attention_presplit_ab:  # attention high (+ long as asked) on both sides, the images off and on
        sides = ("attn", "attnimg")
        set_mode = lambda name: set_attention("highest" if name == "highest" else "high", presplit=name == "attnimg")
    dev = torch.device("cuda", 0)
    lib = L.lib()
    torch.manual_seed(0)
    m = vit_amd.CLIPHBA([f"c{i}" for i in range(a.prompts)], "ViT-L/14@336px", pos_embedding=True)
    vit_amd.apply_dora_to_ViT(m, n_vision_layers=2, n_transformer_layers=1, r=32)
    vit_amd.switch_dora_layers(m, freeze_all=True, dora_state=True)
    m = m.to(dev)
    opt = vit_amd.FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=3e-4)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(a.batch, 3, 336, 336, generator=g).to(dev)
    y = (torch.randn(a.batch, a.prompts, generator=g) * 0.5 + 1.0).to(dev)

    def step():
        opt.zero_grad(set_to_none=True)
        loss = vit_amd.mse_loss(m(x), y)
        loss.backward()
        opt.step()
        return loss

    def run(mode, steps, warmup):
        lib.vit_sdpa_long_config(mode)
        for _ in range(warmup):
            step()
        torch.cuda.synchronize()
        c0 = lib.vit_sdpa_long_f32_count(0)
        t0 = time.perf_counter()
        for _ in range(steps):
            loss = step()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert torch.isfinite(loss)
        return a.batch * steps / dt, lib.vit_sdpa_long_f32_count(0) - c0

    if a.f32_ab or a.f32_attention_ab or a.f32_presplit_ab or a.f32_presplit_act_ab or a.f32_attention_presplit_ab:
        ips = {k: [] for k in sides}
        extra = {}
        try:
            if a.f32_presplit_ab or a.f32_presplit_act_ab:
                count = lib.vit_gemm_f32_presplit_act_count if a.f32_presplit_act_ab else lib.vit_gemm_f32_presplit_count
                lib.vit_sdpa_long_config(1)
                with torch.no_grad():  # (a process's first forward registers the stream-K workspace after its patch
                    m(x)               # embedding has run: its bits are not a later forward's in either form)
                preds = {}
                for name in ips:
                    set_mode(name)
                    c0 = count(0)
                    with torch.no_grad():
                        preds[name] = m(x)
                    assert (count(0) > c0) == (name == sides[1]), name
                    if name == "presplit":
                        extra["weight_image_bytes"] = vit_amd.weight_image_bytes(m)
                extra["predictions_bit_equal"] = bool(torch.equal(preds[sides[0]], preds[sides[1]]))
            if a.f32_attention_presplit_ab:
                lib.vit_sdpa_long_config(1)
                with torch.no_grad():  # (the first forward of a process: see above)
                    m(x)
                preds = {}
                for name in ips:
                    set_mode(name)
                    c0 = lib.vit_sdpa_f32_image_count(0)
                    with torch.no_grad():
                        preds[name] = m(x)
                    extra["image_launches_" + name] = lib.vit_sdpa_f32_image_count(0) - c0
                assert extra["image_launches_attn"] == 0, extra
                extra["predictions_bit_equal"] = bool(torch.equal(preds["attn"], preds["attnimg"]))
                extra["f32_attention_long"] = bool(a.f32_attention_long)
            if a.f32_attention_ab and a.f32_attention_long:
                lib.vit_sdpa_long_config(1)
                preds = {}
                for name in ips:
                    set_mode(name)
                    c0 = lib.vit_sdpa_long_f32_split_count(0)
                    with torch.no_grad():
                        preds[name] = m(x).double()
                    assert (lib.vit_sdpa_long_f32_split_count(0) > c0) == (name == "high"), name
                extra["pred_distance"] = float((preds["high"] - preds["highest"]).abs().max()
                                               / preds["highest"].abs().max())
                extra["f32_attention_long"] = True
            for rnd in range(a.rounds):
                for name in ips:
                    set_mode(name)
                    ips[name].append(round(run(1, a.steps, a.warmup if rnd == 0 else 1)[0], 2))
        finally:
            lib.vit_sdpa_long_config(-1)
            set_mode("highest")
        med = {k: statistics.median(v) for k, v in ips.items()}
        print(json.dumps({"metric": "images/sec CLIP-HBA ViT-L/14@336px + DoRA fp32 train step", "batch": a.batch,
                          "steps": a.steps, "rounds": a.rounds, "images_per_sec": ips, "median": med,
                          "alternated": ("f32_attention_presplit" if a.f32_attention_presplit_ab else
                                         "f32_presplit_act" if a.f32_presplit_act_ab else
                                         "f32_presplit" if a.f32_presplit_ab else
                                         "f32_attention" if a.f32_attention_ab else "f32_matmul"),
                          "f32_matmul": "ab" if a.f32_ab else "high" if (a.f32_presplit_ab or a.f32_presplit_act_ab) else (a.f32_matmul or "highest"),
                          "spread": {k: round((max(v) - min(v)) / med[k], 4) for k, v in ips.items()},
                          f"{sides[1]}_over_{sides[0]}": round(med[sides[1]] / med[sides[0]], 3), **extra}), flush=True)
        return
    ips = {"streamed": [], "generic": []}
    try:
        for rnd in range(a.rounds):
            for name, mode, steps in (("streamed", 1, a.steps), ("generic", 0, a.steps_generic)):
                r, calls = run(mode, steps, a.warmup if rnd == 0 and mode else 1)
                assert (calls > 0) == bool(mode), (name, calls)
                ips[name].append(round(r, 2))
    finally:
        lib.vit_sdpa_long_config(-1)
    med = {k: statistics.median(v) for k, v in ips.items()}
    print(json.dumps({"metric": "images/sec CLIP-HBA ViT-L/14@336px + DoRA fp32 train step", "batch": a.batch,
                      "steps": a.steps, "steps_generic": a.steps_generic, "rounds": a.rounds, "images_per_sec": ips,
                      "median": med, "streamed_over_generic": round(med["streamed"] / med["generic"], 2),
                      "peak_mem_gib": round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 2)}), flush=True)


if __name__ == "__main__":
    main()
