"""Config C3 step rate alone: CLIP-HBA ViT-L/14 + DoRA train step (bench.py's ``c3`` leg, which
the default bench line carries in both dtypes).  Prints one JSON line.

    python tools/bench_clip.py [--batch 64] [--steps 10] [--warmup 3] [--dtype f32|bf16] [--adapter dora|lora]

``--adapter lora`` times the same step with the reference's LoRA pair (``apply_lora_to_ViT`` /
``unfreeze_lora_layers``, NEWP:339-404) in place of the DoRA pair; ``dora`` (the default) is bench.py's leg itself.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtype", choices=["f32", "bf16"], default="f32",
                    help="compute dtype: f32 = the reference's precision (NEWP:274), bf16 opt-in")
    ap.add_argument("--adapter", choices=["dora", "lora"], default="dora")
    a = ap.parse_args()
    import torch
    leg = bench.c3_leg if a.adapter == "dora" else lora_leg
    r = leg(torch.device("cuda", 0), a.dtype, a.batch, a.steps, a.warmup)
    r["metric"] = f"images/sec CLIP-HBA ViT-L/14 + {'DoRA' if a.adapter == 'dora' else 'LoRA'} train step (config C3)"
    r["adapter"] = a.adapter
    print(json.dumps(r))


if __name__ == "__main__":
    main()
