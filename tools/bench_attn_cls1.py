"""The one-query attention kernels (vit_sdpa_cls1_fwd / vit_sdpa_cls1_bwd) alone, against the kernels
the class-token tail runs without them: vit_sdpa_fwd_cls (bf16 up to 288 tokens: query tile 0 of the resident
kernel) or vit_sdpa_fwd, and vit_sdpa_bwd on a dense dO that is zero except row 0 of every image.

Shapes: B = 64, H = 16 (CLIP ViT-L/14 at bs = 64), N = 257 and 577 (ViT-L/14@336px), f32 and bf16.  Device events
around back-to-back calls on warmed shapes, as many calls as fill --window-ms (at least --calls), --rounds windows
(>= 3); per kernel the median time of a call, the round-to-round spread (max - min) / median, and for the
one-query kernels the bytes they must move, counted from the shapes -- K + V for the forward, plus the dqkv write
for the backward (N = 257, f32: 135 MB and 337 MB) -- as TB/s and as a share of the 8 TB/s HBM peak.

Calls on one buffer re-read what the 256 MiB Infinity Cache may still hold (in a step the qkv GEMM has just written
it, so this is the nearer picture of the two).  The ``*_rot`` series rotate over --rotate qkv / dqkv buffers, whose
footprint between two uses of a line is past the cache: the figure against HBM alone.

Prints one JSON line per shape; --out also writes them.

    python tools/bench_attn_cls1.py [--window-ms 200] [--rounds 5] [--rotate 4] [--out profiles/r16/bench_attn_cls1.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-project_amd"))

HBM_PEAK = 8.0e12  # bytes / s
SHAPES = [(64, 16, 257, "f32"), (64, 16, 257, "bf16"), (64, 16, 577, "f32"), (64, 16, 577, "bf16")]


def _summary(vals):
    med = statistics.median(vals)
    return {"us": round(med * 1e3, 2), "spread": round((max(vals) - min(vals)) / med, 4)}


def shape_leg(B, H, N, dtype_name, calls, rounds, window_ms, rotate):
    import torch
    from vit_amd import ops
    dev = torch.device("cuda", 0)
    T = {"f32": torch.float32, "bf16": torch.bfloat16}[dtype_name]
    es = 4 if T == torch.float32 else 2
    D = H * 64
    g = torch.Generator().manual_seed(N)
    qkv = (torch.randn(B * N, 3 * D, generator=g) * 1.5).to(T).to(dev)
    do_cls = torch.randn(B, D, generator=g).to(T).to(dev)
    do_dense = torch.zeros(B * N, D, dtype=T, device=dev)
    do_dense.view(B, N * D)[:, :D].copy_(do_cls)
    o1, lse1 = ops.sdpa_cls1_fwd(qkv, B, H, N)
    o, lse = ops.sdpa_fwd(qkv, B, H, N)
    oc, lsec = ops.sdpa_fwd_cls(qkv, B, H, N)
    dq1 = torch.empty_like(qkv)
    dq = torch.empty_like(qkv)
    rq = [qkv] + [qkv.clone() for _ in range(rotate - 1)]
    rd = [dq1] + [torch.empty_like(qkv) for _ in range(rotate - 1)]
    turn = [0, 0]

    def rot_fwd():
        turn[0] = (turn[0] + 1) % rotate
        ops.sdpa_cls1_fwd(rq[turn[0]], B, H, N, o=o1, lse=lse1)

    def rot_bwd():
        turn[1] = (turn[1] + 1) % rotate
        ops.sdpa_cls1_bwd(rq[turn[1]], o1, do_cls, lse1, B, H, N, dqkv=rd[turn[1]])

    kernels = {
        "cls1_fwd": lambda: ops.sdpa_cls1_fwd(qkv, B, H, N, o=o1, lse=lse1),
        "fwd_cls": lambda: ops.sdpa_fwd_cls(qkv, B, H, N, o=oc, lse=lsec),
        "fwd": lambda: ops.sdpa_fwd(qkv, B, H, N, o=o, lse=lse),
        "cls1_bwd": lambda: ops.sdpa_cls1_bwd(qkv, o1, do_cls, lse1, B, H, N, dqkv=dq1),
        "bwd": lambda: ops.sdpa_bwd(qkv, o, do_dense, lse, B, H, N, dqkv=dq),
        "cls1_fwd_rot": rot_fwd,
        "cls1_bwd_rot": rot_bwd,
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
    for name, fn in kernels.items():  # warm every shape, and size the window from a first look
        window(fn, 2 * rotate)
        ncalls[name] = max(calls, int(window_ms / window(fn, 2 * rotate)))
    # the two routes agree (rounding): what the timed kernels compute is the same thing
    cls_o = o.view(B, N * D)[:, :D].double()
    agree = {"o": float((o1.double() - cls_o).abs().max() / cls_o.abs().max()),
             "dqkv": float((dq1.double() - dq.double()).abs().max() / dq.double().abs().max())}
    ms = {k: [] for k in kernels}
    for _ in range(rounds):
        for name, fn in kernels.items():
            ms[name].append(window(fn, ncalls[name]))
    rec = {"B": B, "H": H, "N": N, "dtype": dtype_name, "calls_per_window": ncalls, "rounds": rounds,
           "rotating_buffers": rotate, "rotating_footprint_mb": round(rotate * qkv.numel() * es / 1e6),
           "agreement_rel": agree}
    moved = {"cls1_fwd": B * N * 2 * D * es, "cls1_bwd": B * N * 2 * D * es + B * N * 3 * D * es}
    moved.update(cls1_fwd_rot=moved["cls1_fwd"], cls1_bwd_rot=moved["cls1_bwd"])
    for name, v in ms.items():
        s = _summary(v)
        if name in moved:
            bps = moved[name] / (s["us"] * 1e-6)
            s.update(bytes_moved=moved[name], tb_per_sec=round(bps / 1e12, 3), hbm_peak_share=round(bps / HBM_PEAK, 3))
        rec[name] = s
    rec["fwd_speedup_vs_fwd_cls"] = round(rec["fwd_cls"]["us"] / rec["cls1_fwd"]["us"], 2)
    rec["fwd_speedup_vs_fwd"] = round(rec["fwd"]["us"] / rec["cls1_fwd"]["us"], 2)
    rec["bwd_speedup_vs_bwd"] = round(rec["bwd"]["us"] / rec["cls1_bwd"]["us"], 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50, help="least calls per timed window")
    ap.add_argument("--window-ms", type=float, default=200.0, help="device time a timed window should fill")
    ap.add_argument("--rotate", type=int, default=4, help="buffers of the *_rot series (footprint past the Infinity Cache)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.rounds < 3:
        ap.error("--rounds must be at least 3: the spread is part of the record")
    if a.rotate < 2:
        ap.error("--rotate must be at least 2")
    lines = []
    for B, H, N, dt in SHAPES:
        lines.append(json.dumps(shape_leg(B, H, N, dt, a.calls, a.rounds, a.window_ms, a.rotate)))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
