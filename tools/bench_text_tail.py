"""The CLIP text tower's live part alone with the EOT tail (``CLIP.set_eot_tail``) off and on: what the
C3 step can gain from it at most.

CLIP-HBA ViT-L/14, DoRA r = 32 on the last text block, 66 prompts of unequal lengths; the frozen text blocks'
output is cached as in a step, so ``encode_text`` is the last block and the pool head.  Two passes, each with the
switch alternated in one process over --rounds rounds (>= 3), device events around windows of --calls calls:
``encode_text`` + backward of a sum (the step's share), and ``encode_text`` under ``no_grad`` (``evaluate`` /
``behavioral_rsa``'s share).  Medians, the round-to-round spread (max - min) / median, the ratio.  One JSON line
per dtype; --out also writes them.

    python tools/bench_text_tail.py [--calls 50] [--rounds 5] [--out profiles/r18/bench_text_tail.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-project_amd"))


def _summary(v):
    med = statistics.median(v)
    return {"rounds": [round(t, 4) for t in v], "median": round(med, 4), "spread": round((max(v) - min(v)) / med, 4)}


def leg(dtype_name, calls, rounds):
    import torch
    import vit_amd
    dev = torch.device("cuda", 0)
    T = {"f32": torch.float32, "bf16": torch.bfloat16}[dtype_name]
    torch.manual_seed(0)
    names = ["c" * (1 + (7 * i) % 40) for i in range(66)]  # prompts of 3 .. 42 tokens
    m = vit_amd.CLIPHBA(names, "ViT-L/14", pos_embedding=True, compute_dtype=T)
    vit_amd.apply_dora_to_ViT(m, n_vision_layers=2, n_transformer_layers=1, r=32)
    vit_amd.switch_dora_layers(m, freeze_all=True, dora_state=True)
    m = m.to(dev)
    cm = m.clip_model
    text = m.tokenized_prompts.to(dev)
    w = torch.randn(66, 768, device=dev)
    trainable = [p for p in m.parameters() if p.requires_grad]

    def train_call():
        for p in trainable:
            p.grad = None
        (cm.encode_text(text) * w).sum().backward()

    def eval_call():
        with torch.no_grad():
            cm.encode_text(text)

    def window(fn, n):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(n):
            fn()
        ev[1].record()
        torch.cuda.synchronize(dev)
        return ev[0].elapsed_time(ev[1]) / n

    rec = {"dtype": dtype_name, "prompts": 66, "context_length": 77, "calls_per_window": calls, "rounds": rounds}
    for name, fn in (("encode_text_fwd_bwd_ms", train_call), ("encode_text_no_grad_ms", eval_call)):
        for on in (False, True):
            cm.set_eot_tail(on)
            window(fn, 5)
        ms = {False: [], True: []}
        for _ in range(rounds):
            for on in (False, True):
                cm.set_eot_tail(on)
                ms[on].append(window(fn, calls))
        off, on_ = _summary(ms[False]), _summary(ms[True])
        rec[name] = {"eot_tail_off": off, "eot_tail_on": on_, "ratio": round(off["median"] / on_["median"], 3),
                     "saved_ms": round(off["median"] - on_["median"], 4)}
    cm.set_eot_tail(False)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.rounds < 3:
        ap.error("--rounds must be at least 3: the spread is part of the record")
    lines = []
    for dt in ("f32", "bf16"):
        lines.append(json.dumps(leg(dt, a.calls, a.rounds)))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
