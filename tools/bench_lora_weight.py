"""The adapter weight build alone: vit_lora_weight_fwd / _bwd against vit_dora_weight_fwd / _bwd_ws.

Per shape (n, r) -- (1024, 32) and (768, 32), the two out_proj widths of CLIP ViT-L/14 -- every variant is one
C-ABI call on fixed device buffers.  A window is --launches calls queued back to back between two device events;
the variants alternate inside a round, over --rounds rounds, in one process.  The record holds every round's
microseconds per call, the median, the round-to-round spread and, for LoRA, the bytes the call must move (W0 in
and W out; gW in) over the median.  The buffers of a shape (at most 25 MB) stay in the 256 MB Infinity Cache
between launches: these are warm-cache figures, as the step sees them (gW was just written by the weight
gradient GEMM, W is read next by the out_proj GEMM).

    python tools/bench_lora_weight.py [--out profiles/r15] [--launches 2000] [--rounds 9]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-project_amd"))


def _summary(vals):
    med = statistics.median(vals)
    return {"rounds_us": [round(v, 3) for v in vals], "median_us": round(med, 3),
            "spread": round((max(vals) - min(vals)) / med, 4)}


def shape_record(n, r, launches, rounds, graphs):
    import torch
    from vit_amd import _lib as L
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(n + r)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)
    s = 16 / r
    W0, A, Bm, gW = rnd(n, n) * 0.05, rnd(r, n) * 0.3, rnd(n, r) * 0.3, rnd(n, n)
    W, dA, dB = torch.empty(n, n, device=dev), torch.empty(r, n, device=dev), torch.empty(n, r, device=dev)
    ws = torch.empty(L.lib().vit_lora_weight_bwd_ws_floats(n, r), device=dev)
    # DoRA on the same layer: D = W0^T / ||.||_col, m the norms (DoRALayer.__init__)
    Wt = W0.t().contiguous()
    m = torch.norm(Wt, dim=0).contiguous()
    D = (Wt / m).contiguous()
    Wd, nu, DnT = torch.empty(n, n, device=dev), torch.empty(n, device=dev), torch.empty(n, n, device=dev)
    colsq = torch.empty(((n + 63) // 64) * n, device=dev)
    dm, dAd, dBd = torch.empty(n, device=dev), torch.empty(r, n, device=dev), torch.empty(n, r, device=dev)
    slab_floats = 2 * 256 * 1024
    base = -(-n * n // 4) * 4
    wsd = torch.empty(base + slab_floats, device=dev)
    p = L.ptr
    cur = lambda: L.stream_ptr(dev)  # the capture stream while a graph is being recorded
    variants = {
        "lora_weight_fwd": lambda: L.call("vit_lora_weight_fwd", n, r, p(W0), p(A), p(Bm), s, p(W), cur()),
        "dora_weight_fwd": lambda: L.call("vit_dora_weight_fwd", n, n, r, p(m), p(A), p(Bm), p(D), s, None, p(Wd), p(nu),
                                          p(DnT), p(colsq), cur()),
        "lora_weight_bwd": lambda: L.call("vit_lora_weight_bwd", n, r, p(A), p(Bm), p(gW), s, p(dA), p(dB), p(ws), cur()),
        "dora_weight_bwd_ws": lambda: L.call("vit_dora_weight_bwd_ws", n, n, r, p(m), p(A), p(Bm), p(gW), p(DnT), s, p(nu),
                                             p(dm), p(dAd), p(dBd), p(wsd), p(wsd[base:]), slab_floats, None, cur()),
    }
    for fn in variants.values():  # every shape of the timed windows, once (the DoRA backward reads the forward's DnT)
        for _ in range(20):
            fn()
    torch.cuda.synchronize(dev)
    per_graph = 100
    replays = {}
    if graphs:  # 100 calls recorded once and replayed: the host's per-call cost is out of the window
        for name, fn in variants.items():
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                for _ in range(per_graph):
                    fn()
            gr.replay()
            replays[name] = gr
        torch.cuda.synchronize(dev)
    us = {k: [] for k in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            if graphs:
                for _ in range(launches // per_graph):
                    replays[name].replay()
            else:
                for _ in range(launches):
                    fn()
            e1.record()
            e1.synchronize()
            us[name].append(e0.elapsed_time(e1) * 1e3 / (launches // per_graph * per_graph if graphs else launches))
    rec = {"n": n, "r": r, "launches_per_window": launches, "rounds": rounds,
           "queued_by": "graph replay (100 calls a graph)" if graphs else "the host, call by call"}
    for k, v in us.items():
        rec[k] = _summary(v)
    must = {"lora_weight_fwd": 2 * n * n * 4, "lora_weight_bwd": n * n * 4}
    for k, b in must.items():
        rec[k]["bytes_needed"] = b
        rec[k]["gb_per_sec_at_median"] = round(b / rec[k]["median_us"] / 1e3, 1)
    rec["fwd_lora_over_dora"] = round(rec["lora_weight_fwd"]["median_us"] / rec["dora_weight_fwd"]["median_us"], 3)
    rec["bwd_lora_over_dora"] = round(rec["lora_weight_bwd"]["median_us"] / rec["dora_weight_bwd_ws"]["median_us"], 3)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15"))
    ap.add_argument("--launches", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=9)
    a = ap.parse_args()
    if a.rounds < 3:
        ap.error("--rounds must be at least 3: the spread is part of the record")
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_lora_weight.py needs a GPU: nothing is measured without one")
    rec = {"metric": "adapter weight build, microseconds per C-ABI call (device events around back-to-back calls); "
                     "host-queued windows are bound by the host's enqueue rate where that exceeds the kernels, "
                     "graph replays are not",
           "host_queued": [shape_record(n, r, a.launches, a.rounds, False) for n, r in ((1024, 32), (768, 32))],
           "graph_replay": [shape_record(n, r, a.launches, a.rounds, True) for n, r in ((1024, 32), (768, 32))]}
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "lora_weight_build.json"), "w") as fh:
        json.dump(rec, fh, indent=1)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
