"""Config C3 step rate alone: CLIP-HBA ViT-L/14 + DoRA train step (bench.py's ``c3`` leg, which
the default bench line carries in both dtypes).  Prints one JSON line.

    python tools/bench_clip.py [--batch 64] [--steps 10] [--warmup 3] [--dtype f32|bf16] [--adapter dora|lora]

``--adapter lora`` times the same step with the reference's LoRA pair (``apply_lora_to_ViT`` /
``unfreeze_lora_layers``, NEWP:339-404) in place of the DoRA pair; ``dora`` (the default) is bench.py's leg itself.

``--cls-tail`` times the step with the visual tower's class-token tail (``CLIP.set_cls_tail``) off
and on, alternated on one model in one process over ``--rounds`` rounds (>= 3): medians, the round-to-round
spread ``(max - min) / median``, the ratio, and the on-against-off relative difference of the predictions.

``--eot-tail`` does the same for the text tower's EOT tail (``CLIP.set_eot_tail``); given together
with ``--cls-tail`` the class-token tail stays on throughout and the EOT tail alone alternates.

``--f32-attention highest|high`` sets the fp32 attention arithmetic of the whole run
(``vit_amd.set_float32_attention_precision``); ``--f32-attention-ab`` alternates the two in one process
the way ``--f32-ab`` alternates the GEMM mode, the GEMMs staying at ``--f32-matmul``.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def lora_leg(dev, dtype, batch, steps, warmup):
    """bench.c3_leg with LoRA r = 32 on the same three out_proj layers: same data, step and timing."""
    import statistics
    import time
    import torch
    import vit_amd
    T = torch.float32 if dtype == "f32" else torch.bfloat16
    torch.manual_seed(0)
    m = vit_amd.CLIPHBA(["class%d" % i for i in range(66)], "ViT-L/14", pos_embedding=True, compute_dtype=T)
    vit_amd.apply_lora_to_ViT(m, n_vision_layers=2, n_transformer_layers=1, r=32)
    vit_amd.unfreeze_lora_layers(m, freeze_all=True)
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
    return {"value": round(batch * steps / el, 2), "unit": "images/s", "ms_per_step": round(el / steps * 1e3, 3),
            "ms_per_step_median": round(med, 3), "batch": batch, "steps": steps, "warmup": warmup, "dtype": dtype,
            "final_loss": round(float(loss.item()), 4)}


def cls_tail_leg(dev, dtype, batch, steps, warmup, adapter, rounds, which="cls", cls_fixed=False):
    """The C3 step (bench.c3_leg's model, data and optimizer) with the class-token tail (``which`` = "cls") or the
    EOT tail ("eot"; ``cls_fixed``: the class-token tail on throughout) off and on, alternated."""
    import statistics
    import torch
    import vit_amd
    T = torch.float32 if dtype == "f32" else torch.bfloat16
    torch.manual_seed(0)
    m = vit_amd.CLIPHBA(["class%d" % i for i in range(66)], "ViT-L/14", pos_embedding=True, compute_dtype=T)
    if adapter == "lora":
        vit_amd.apply_lora_to_ViT(m, n_vision_layers=2, n_transformer_layers=1, r=32)
        vit_amd.unfreeze_lora_layers(m, freeze_all=True)
    else:
        vit_amd.apply_dora_to_ViT(m, n_vision_layers=2, n_transformer_layers=1, r=32)
        vit_amd.switch_dora_layers(m, freeze_all=True, dora_state=True)
    m = m.to(dev)
    opt = vit_amd.FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=3e-4)
    x = torch.randn(batch, 3, 224, 224, device=dev)
    y = torch.randn(batch, 66, device=dev) * 0.5 + 1.0
    if which == "f32":  # the fp32 GEMM mode ("high" = bf16x3) off and on, the class-token tail as cls_fixed says
        switch = lambda on: vit_amd.set_float32_matmul_precision("high" if on else "highest")
    elif which == "f32pre":  # "high" throughout; pre-split weight images off and on
        switch = lambda on: vit_amd.set_float32_matmul_precision("high", presplit_weights=on)
    elif which == "f32act":  # "high" with weight images throughout; activation images off and on
        switch = lambda on: vit_amd.set_float32_matmul_precision("high", presplit_weights=True, presplit_activations=on)
    elif which == "f32attnimg":  # attention "high" throughout; images through attention off and on
        switch = lambda on: vit_amd.set_float32_attention_precision("high", presplit=on)
    elif which == "f32attn":  # the fp32 attention mode off and on, the GEMM mode as --f32-matmul says
        switch = lambda on: vit_amd.set_float32_attention_precision("high" if on else "highest")
    else:
        switch = m.clip_model.set_cls_tail if which == "cls" else m.clip_model.set_eot_tail
    if which in ("eot", "f32", "f32attn", "f32attnimg", "f32pre", "f32act"):
        m.clip_model.set_cls_tail(cls_fixed)
    key = {"f32": "f32_high", "f32attn": "f32_attention_high", "f32pre": "f32_presplit",
           "f32act": "f32_presplit_act", "f32attnimg": "f32_attention_presplit"}.get(which, which + "_tail")

    def window(n):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(n):
            opt.zero_grad(set_to_none=True)
            loss = vit_amd.mse_loss(m(x), y)
            loss.backward()
            opt.step()
        ev[1].record()
        torch.cuda.synchronize(dev)
        assert torch.isfinite(loss)
        return ev[0].elapsed_time(ev[1]) / n

    preds = {}
    for on in (False, True):  # the same parameters: before any step moves them
        switch(on)
        with torch.no_grad():
            preds[on] = m(x).double()
    for on in (False, True):
        switch(on)
        window(warmup)
    ms = {False: [], True: []}
    for _ in range(rounds):
        for on in (False, True):
            switch(on)
            ms[on].append(window(steps))
    held = vit_amd.weight_image_bytes(m)
    switch(False)

    def summary(v):
        med = statistics.median(v)
        return {"rounds": [round(t, 3) for t in v], "median": round(med, 3), "spread": round((max(v) - min(v)) / med, 4)}

    off, on = summary(ms[False]), summary(ms[True])
    return {"ms_per_step": {key + "_off": off, key + "_on": on}, key + "_speedup": round(off["median"] / on["median"], 4),
            "images_per_sec": {key + "_off": round(batch / off["median"] * 1e3, 2),
                               key + "_on": round(batch / on["median"] * 1e3, 2)},
            "cls_tail_throughout": bool(which in ("eot", "f32", "f32attn", "f32attnimg", "f32pre", "f32act") and cls_fixed),
            "weight_image_bytes": held,
            "predictions_bit_equal": bool(torch.equal(preds[True], preds[False])),
            "prediction_rel_diff_on_vs_off": float((preds[True] - preds[False]).abs().max() / preds[False].abs().max()),
            "prediction_rms_rel_diff_on_vs_off": float(((preds[True] - preds[False]).pow(2).mean()
                                                        / preds[False].pow(2).mean()).sqrt()),
            "prediction_bound": 1e-3 if dtype == "f32" else 3e-2,
            "batch": batch, "steps": steps, "warmup": warmup, "rounds": rounds, "dtype": dtype}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtype", choices=["f32", "bf16"], default="f32",
                    help="compute dtype: f32 = the reference's precision (NEWP:274), bf16 opt-in")
    ap.add_argument("--adapter", choices=["dora", "lora"], default="dora")
    ap.add_argument("--cls-tail", action="store_true",
                    help="alternate the visual tower's class-token tail off and on in one process")
    ap.add_argument("--eot-tail", action="store_true",
                    help="alternate the text tower's EOT tail off and on in one process (with --cls-tail: that tail on "
                         "throughout)")
    ap.add_argument("--rounds", type=int, default=3, help="rounds of the --cls-tail / --eot-tail alternation (>= 3)")
    ap.add_argument("--f32-matmul", choices=["highest", "high"], default=None,
                    help="fp32 GEMM arithmetic of the whole run (vit_amd.set_float32_matmul_precision; high = bf16x3)")
    ap.add_argument("--f32-ab", action="store_true",
                    help="alternate --f32-matmul highest and high in one process (with --cls-tail: that tail on throughout)")
    ap.add_argument("--f32-presplit", action="store_true",
                    help="with --f32-matmul high: keep pre-split hi / lo images of the frozen fp32 weights "
                         "(set_float32_matmul_precision('high', presplit_weights=True))")
    ap.add_argument("--f32-presplit-ab", action="store_true",
                    help="alternate in-loop 'high' and pre-split 'high' in one process (with --cls-tail: that tail on "
                         "throughout)")
    ap.add_argument("--f32-presplit-act", action="store_true",
                    help="with --f32-matmul high --f32-presplit: forward-only blocks hand pre-split activation images "
                         "from producer to GEMM (presplit_activations=True)")
    ap.add_argument("--f32-presplit-act-ab", action="store_true",
                    help="alternate pre-split weights and pre-split weights + activations in one process (with "
                         "--cls-tail: that tail on throughout)")
    ap.add_argument("--f32-attention", choices=["highest", "high"], default=None,
                    help="fp32 attention arithmetic of the whole run (vit_amd.set_float32_attention_precision; high = "
                         "bf16x3 in the resident f32 kernels)")
    ap.add_argument("--f32-attention-ab", action="store_true",
                    help="alternate --f32-attention highest and high in one process, the GEMMs as --f32-matmul says "
                         "(with --cls-tail: that tail on throughout)")
    ap.add_argument("--f32-attention-presplit", action="store_true",
                    help="with --f32-attention high: forward-only blocks carry pre-split images through attention "
                         "(set_float32_attention_precision('high', presplit=True); needs the --f32-presplit-act chain)")
    ap.add_argument("--f32-attention-presplit-ab", action="store_true",
                    help="alternate attention high without and with images through attention in one process, the GEMMs "
                         "as the --f32-matmul flags say (the baseline: --f32-matmul high --f32-presplit "
                         "--f32-presplit-act)")
    a = ap.parse_args()
    import torch
    if a.f32_attention_presplit and a.f32_attention != "high":
        ap.error("--f32-attention-presplit needs --f32-attention high")
    if a.f32_matmul:
        import vit_amd
        if a.f32_presplit_act and not a.f32_presplit:
            ap.error("--f32-presplit-act needs --f32-presplit")
        vit_amd.set_float32_matmul_precision(a.f32_matmul, presplit_weights=a.f32_presplit,
                                             presplit_activations=a.f32_presplit_act)
    elif a.f32_presplit or a.f32_presplit_act:
        ap.error("--f32-presplit / --f32-presplit-act need --f32-matmul high")
    if a.f32_attention:
        import vit_amd
        vit_amd.set_float32_attention_precision(a.f32_attention, presplit=a.f32_attention_presplit)
    if (a.cls_tail or a.eot_tail or a.f32_ab or a.f32_attention_ab or a.f32_presplit_ab or a.f32_presplit_act_ab
            or a.f32_attention_presplit_ab):
        if a.rounds < 3:
            ap.error("--rounds must be at least 3: the spread is part of the record")
        r = cls_tail_leg(torch.device("cuda", 0), a.dtype, a.batch, a.steps, a.warmup, a.adapter, a.rounds,
                         "f32attnimg" if a.f32_attention_presplit_ab else "f32act" if a.f32_presplit_act_ab else "f32pre" if a.f32_presplit_ab else "f32attn" if a.f32_attention_ab else "f32" if a.f32_ab else "eot" if a.eot_tail else "cls",
                         a.cls_tail)
    else:
        leg = bench.c3_leg if a.adapter == "dora" else lora_leg
        r = leg(torch.device("cuda", 0), a.dtype, a.batch, a.steps, a.warmup)
    r["metric"] = f"images/sec CLIP-HBA ViT-L/14 + {'DoRA' if a.adapter == 'dora' else 'LoRA'} train step (config C3)"
    r["adapter"] = a.adapter
    if a.f32_matmul:
        r["f32_matmul"] = a.f32_matmul
        # what ran: a flag given for the whole run, or "ab" for the switch that alternated (weight images are on
        # throughout when the activation images alternate)
        r["f32_presplit"] = "ab" if a.f32_presplit_ab else bool(a.f32_presplit or a.f32_presplit_act_ab)
        r["f32_presplit_act"] = "ab" if a.f32_presplit_act_ab else bool(a.f32_presplit_act)
    if a.f32_attention:
        r["f32_attention"] = a.f32_attention
    if a.f32_attention_presplit or a.f32_attention_presplit_ab:
        r["f32_attention_presplit"] = "ab" if a.f32_attention_presplit_ab else True
    print(json.dumps(r))


if __name__ == "__main__":
    main()
