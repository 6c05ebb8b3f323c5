"""The one-query attention forward at a row per sequence (vit_sdpa_row1_fwd) alone, against the kernel
the CLIP text tower's last block runs without it: vit_sdpa_fwd(causal=1) over all rows.

Shape: S = 66 prompts, H = 12, N = 77 (CLIP ViT-L/14's text tower), f32 and bf16; the EOT positions are drawn
between 3 and 76, as prompts of unequal lengths have them.  Device events around back-to-back calls on warmed
shapes, as many calls as fill --window-ms (at least --calls), --rounds windows (>= 3); per kernel the median time
of a call and the round-to-round spread (max - min) / median.  The whole qkv tensor is 14 MB in f32: both kernels
read it from the Infinity Cache here, as they do in a step, where the qkv GEMM has just written it.

Prints one JSON line per dtype; --out also writes them.

    python tools/bench_attn_row1.py [--window-ms 100] [--rounds 5] [--out profiles/r18/bench_attn_row1.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-project_amd"))

SHAPES = [(66, 12, 77, "f32"), (66, 12, 77, "bf16")]


def _summary(vals):
    med = statistics.median(vals)
    return {"us": round(med * 1e3, 2), "spread": round((max(vals) - min(vals)) / med, 4)}


def shape_leg(B, H, N, dtype_name, calls, rounds, window_ms):
    import torch
    from vit_amd import ops
    dev = torch.device("cuda", 0)
    T = {"f32": torch.float32, "bf16": torch.bfloat16}[dtype_name]
    D = H * 64
    g = torch.Generator().manual_seed(N)
    qkv = (torch.randn(B * N, 3 * D, generator=g) * 1.5).to(T).to(dev)
    qrow = torch.randint(3, N, (B,), generator=g).to(dev)
    o1, lse1 = ops.sdpa_row1_fwd(qkv, qrow, B, H, N, causal=True)
    o, lse = ops.sdpa_fwd(qkv, B, H, N, causal=True)
    kernels = {
        "row1_fwd": lambda: ops.sdpa_row1_fwd(qkv, qrow, B, H, N, causal=True, o=o1, lse=lse1),
        "fwd_causal": lambda: ops.sdpa_fwd(qkv, B, H, N, o=o, lse=lse, causal=True),
    }

    def window(fn, n):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(n):
            fn()
        ev[1].record()
        torch.cuda.synchronize(dev)
        return ev[0].elapsed_time(ev[1]) / n

    ncalls = {}
    for name, fn in kernels.items():  # warm both, and size the window from a first look
        window(fn, 8)
        ncalls[name] = max(calls, int(window_ms / window(fn, 8)))
    # the two routes agree (rounding): what the timed kernels compute is the same thing
    rows = torch.arange(B, device=dev) * N + qrow
    want = o.index_select(0, rows).double()
    agree = float((o1.double() - want).abs().max() / want.abs().max())
    ms = {k: [] for k in kernels}
    for _ in range(rounds):
        for name, fn in kernels.items():
            ms[name].append(window(fn, ncalls[name]))
    rec = {"B": B, "H": H, "N": N, "dtype": dtype_name, "calls_per_window": ncalls, "rounds": rounds,
           "agreement_rel_o": agree}
    for name, v in ms.items():
        rec[name] = _summary(v)
    rec["speedup_vs_fwd_causal"] = round(rec["fwd_causal"]["us"] / rec["row1_fwd"]["us"], 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50, help="least calls per timed window")
    ap.add_argument("--window-ms", type=float, default=100.0, help="device time a timed window should fill")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.rounds < 3:
        ap.error("--rounds must be at least 3: the spread is part of the record")
    lines = []
    for B, H, N, dt in SHAPES:
        lines.append(json.dumps(shape_leg(B, H, N, dt, a.calls, a.rounds, a.window_ms)))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
