"""The resident f32 attention forward and backward alone, in both fp32 attention modes ("highest" = f32 MFMA, "high"
= bf16x3), alternated in one process.  Default shapes: the CLIP ViT-L/14 visual tower's (B = 64,
H = 16, N = 257) and the text tower's (B = 66, H = 12, N = 77, causal).  Per shape, kernel and mode: the median over
``--pairs`` alternating pairs of a window of ``--reps`` back-to-back calls, the spread (max - min) / median, the
ratio of the medians and whether it counts (past twice the larger spread).  Prints one JSON line per shape.

    python tools/bench_attn_f32.py [--pairs 3] [--reps 20] [--shape B,H,N,causal ...]

``--image``: the "high" forward on f32 qkv / o against the image forward (qkv and o as pre-split images,
``vit_sdpa_fwd_image``), alternated the same way; past 288 tokens both sides run the streamed kernels
(``long_sequences=True``).  The o image must equal the image of the f32 o and lse must be equal, bit for bit, before
anything is timed.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "vit-project_amd"))

import torch  # noqa: E402

from vit_amd import _lib as L  # noqa: E402
from vit_amd import ops  # noqa: E402

MODES = ("highest", "high")


def window(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps * 1e3  # microseconds per call


def summary(v):
    med = statistics.median(v)
    return {"us": [round(t, 1) for t in v], "median_us": round(med, 1), "spread": round((max(v) - min(v)) / med, 4)}


def shape_leg(B, H, N, causal, pairs, reps):
    D = H * 64
    g = torch.Generator().manual_seed(0)
    qkv = (torch.randn(B * N, 3 * D, generator=g) * 1.5).cuda()
    do = torch.randn(B * N, D, generator=g).cuda()
    o, lse = ops.sdpa_fwd(qkv, B, H, N, causal=causal)
    dq = torch.empty_like(qkv)
    calls = {"fwd": lambda: ops.sdpa_fwd(qkv, B, H, N, o=o, lse=lse, causal=causal),
             "bwd": lambda: ops.sdpa_bwd(qkv, o, do, lse, B, H, N, dqkv=dq, causal=causal)}
    us = {k: {m: [] for m in MODES} for k in calls}
    lib = L.lib()
    try:
        for m in MODES:  # warm both modes, and check which kernels each takes
            ops.set_float32_attention_precision(m)
            c0 = lib.vit_sdpa_f32_split_count(0)
            for fn in calls.values():
                window(fn, 3)
            took = lib.vit_sdpa_f32_split_count(0) - c0
            assert took == (6 if m == "high" else 0), (m, took)
        for _ in range(pairs):
            for m in MODES:
                ops.set_float32_attention_precision(m)
                for k, fn in calls.items():
                    us[k][m].append(window(fn, reps))
    finally:
        ops.set_float32_attention_precision("highest")
    rec = {"B": B, "H": H, "N": N, "causal": bool(causal), "pairs": pairs, "reps": reps}
    fl = 4.0 * B * H * N * N * 64 * (0.5 if causal else 1.0)
    for k in calls:
        s = {m: summary(us[k][m]) for m in MODES}
        ratio = s["highest"]["median_us"] / s["high"]["median_us"]
        noise = 2 * max(s[m]["spread"] for m in MODES)
        s["high_speedup"] = round(ratio, 3)
        s["counts"] = bool(abs(ratio - 1) > noise)
        s["high_tflops_of_the_f32_product"] = round((1.0 if k == "fwd" else 2.5) * fl / s["high"]["median_us"] / 1e6, 1)
        rec[k] = s
    return rec


def image_leg(B, H, N, causal, pairs, reps):
    """f32 "high" forward against the image forward of the same values."""
    D = H * 64
    g = torch.Generator().manual_seed(0)
    qkv = (torch.randn(B * N, 3 * D, generator=g) * 1.5).cuda()
    lib = L.lib()
    sides = ("f32", "image")
    us = {m: [] for m in sides}
    try:
        ops.set_float32_attention_precision("high", long_sequences=N > 288, presplit=True)
        qimg = ops.weight_image_raw(qkv)   # an activation image is the row-by-row image of the matrix
        o, lse = ops.sdpa_fwd(qkv, B, H, N, causal=causal)
        oi, lsei = torch.empty_like(o), torch.empty_like(lse)
        assert ops.sdpa_fwd_takes_image(qimg, B, H, N, oi, lsei, causal=causal)
        calls = {"f32": lambda: ops.sdpa_fwd(qkv, B, H, N, o=o, lse=lse, causal=causal),
                 "image": lambda: ops.sdpa_fwd(qimg, B, H, N, o=oi, lse=lsei, causal=causal, image=True)}
        c0 = lib.vit_sdpa_f32_image_count(0)
        for fn in calls.values():
            window(fn, 3)
        assert lib.vit_sdpa_f32_image_count(0) - c0 == 3
        assert torch.equal(oi.view(torch.int32), ops.weight_image_raw(o).view(torch.int32)), "o image != image of o"
        assert torch.equal(lsei.view(torch.int32), lse.view(torch.int32)), "lse differs"
        for _ in range(pairs):
            for m in sides:
                us[m].append(window(calls[m], reps))
    finally:
        ops.set_float32_attention_precision("highest")
    rec = {"B": B, "H": H, "N": N, "causal": bool(causal), "pairs": pairs, "reps": reps, "bits_equal": True}
    s = {m: summary(us[m]) for m in sides}
    ratio = s["f32"]["median_us"] / s["image"]["median_us"]
    fl = 4.0 * B * H * N * N * 64 * (0.5 if causal else 1.0)
    rec["fwd"] = dict(s, image_speedup=round(ratio, 3),
                      counts=bool(abs(ratio - 1) > 2 * max(s[m]["spread"] for m in sides)),
                      image_tflops_of_the_f32_product=round(fl / s["image"]["median_us"] / 1e6, 1))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=3, help="alternating (highest, high) pairs, at least 3")
    ap.add_argument("--reps", type=int, default=20, help="calls per timed window")
    ap.add_argument("--shape", action="append", default=None, help="B,H,N,causal (0 / 1); may be given more than once")
    ap.add_argument("--image", action="store_true", help='the "high" forward on f32 tensors against the image forward')
    a = ap.parse_args()
    if a.pairs < 3:
        ap.error("--pairs must be at least 3: the spread is part of the record")
    shapes = [tuple(int(x) for x in s.split(",")) for s in a.shape] if a.shape else [(64, 16, 257, 0), (66, 12, 77, 1)]
    for B, H, N, causal in shapes:
        print(json.dumps((image_leg if a.image else shape_leg)(B, H, N, causal, a.pairs, a.reps)), flush=True)


if __name__ == "__main__":
    main()
