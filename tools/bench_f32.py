"""fp32 MFMA GEMM timing at config C3's shapes (CLIP ViT-L/14 visual tower, B=64: M = 64 x 257 rows),
with and without the stream's stream-K workspace (f32m::gemm_sk_kernel vs one tile per workgroup).

    python tools/bench_f32.py [--batch 64] [--reps 20] [--precision highest|high] [--presplit] [--presplit-act]
                              [--pairs N] [--json out.jsonl]

``--precision`` sets the fp32 GEMM arithmetic (vit_amd.set_float32_matmul_precision; "high" = bf16x3, DESIGN
§4.22).  ``--pairs N`` times every case N times in "highest" and "high", alternating, in this one process, and
prints per case the median of each, their ratio and the spread (max - min over median) of each side.  TFLOP/s
count 2 M N R in both modes.  ``sum`` is a float64 checksum of the case's output (to compare two builds).
``--presplit`` gives every case the pre-split image of its weight: alone it times "high" reading the
images; with ``--pairs N`` the two sides are in-loop "high" and pre-split "high" (``high`` / ``presplit``), and each
case's two outputs are compared bit for bit.  It also times the image pass itself (both forms, three shapes) as GB/s
of the 8 bytes per element it moves.
``--presplit-act --pairs N``: pre-split weights (``presplit``) against pre-split weights and activations
(``act``), alternating: the qkv / fc1 / fc2 forwards of the forward-only chain with X (and fc1's output) as images,
and the producers alone -- both LayerNorm entry points and fc1's epilogue writing an image against writing f32, which
move the same bytes.  Consumer outputs are compared bit for bit, produced images against the image of the f32 output.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "vit-project_amd"))

import torch  # noqa: E402

from vit_amd import _lib as L, ops  # noqa: E402

PEAK_F32 = 256 * 4 * 64 * 2.4e9 / 1e12


def timeit(fn, reps):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e-3


def presplit_act_pairs(a, dev, M, D, x, h, w, b, wi):
    """--presplit-act --pairs: weights-only against weights + activations, alternating in this process."""
    ops._streamk(dev)
    lib = L.lib()
    raw = lambda t: t.view(torch.int32)
    ximg, himg = ops.weight_image_raw(x), ops.weight_image_raw(h)
    nw, nb = torch.randn(D, device=dev), torch.randn(D, device=dev)
    r = torch.randn(M, D, device=dev)
    mean, rstd = torch.empty(M, device=dev), torch.empty(M, device=dev)
    y, xs, y4 = torch.empty(M, D, device=dev), torch.empty(M, D, device=dev), torch.empty(M, 4 * D, device=dev)
    y3 = torch.empty(M, 3 * D, device=dev)
    fwd = ops.linear_fwd
    QG = L.EPI_BIAS_QGELU_FWD
    # name -> (weights-only side, weights + activations side, FLOP or None, bytes or None, output is an image)
    cases = {
        "fwd qkv (bias), image X": (
            lambda: fwd(x, w["qkv"], b["qkv"], out=y3, wimg=wi["qkv"]),
            lambda: fwd(ximg, w["qkv"], b["qkv"], out=y3, wimg=wi["qkv"], x_image=True), 2 * M * 3 * D * D, None, False),
        "fwd proj (bias + residual), image X": (   # its X is the attention kernels' o image
            lambda: fwd(x, w["proj"], b["proj"], epi=L.EPI_RESID, resid=r, out=y, wimg=wi["proj"]),
            lambda: fwd(ximg, w["proj"], b["proj"], epi=L.EPI_RESID, resid=r, out=y, wimg=wi["proj"], x_image=True),
            2 * M * D * D, None, False),
        "producer: qkv epilogue, image X, image Y": (   # ... and the qkv GEMM writes attention's operand image
            lambda: fwd(ximg, w["qkv"], b["qkv"], out=y3, wimg=wi["qkv"], x_image=True),
            lambda: fwd(ximg, w["qkv"], b["qkv"], out=y3, wimg=wi["qkv"], x_image=True, out_image=True),
            2 * M * 3 * D * D, None, True),
        "fwd fc1 (bias + QuickGELU act-only), image X, image Y": (
            lambda: fwd(x, w["fc1"], b["fc1"], epi=QG, out=y4, wimg=wi["fc1"]),
            lambda: fwd(ximg, w["fc1"], b["fc1"], epi=QG, out=y4, wimg=wi["fc1"], x_image=True, out_image=True),
            2 * M * 4 * D * D, None, True),
        "fwd fc2 (bias + residual), image X": (
            lambda: fwd(h, w["fc2"], b["fc2"], epi=L.EPI_RESID, resid=r, out=y, wimg=wi["fc2"]),
            lambda: fwd(himg, w["fc2"], b["fc2"], epi=L.EPI_RESID, resid=r, out=y, wimg=wi["fc2"], x_image=True),
            2 * M * 4 * D * D, None, False),
        "producer: fc1 epilogue, f32 X, image Y": (
            lambda: fwd(x, w["fc1"], b["fc1"], epi=QG, out=y4, wimg=wi["fc1"]),
            lambda: fwd(x, w["fc1"], b["fc1"], epi=QG, out=y4, wimg=wi["fc1"], out_image=True),
            2 * M * 4 * D * D, None, True),
        "producer: layer_norm_fwd": (
            lambda: ops.layer_norm_fwd(x, nw, nb, 1e-5, torch.float32, out=y, mean=mean, rstd=rstd)[0],
            lambda: ops.layer_norm_fwd(x, nw, nb, 1e-5, torch.float32, out=y, mean=mean, rstd=rstd, out_image=True)[0],
            None, 8 * M * D, True),
        "producer: add_layer_norm_fwd": (
            lambda: (ops.add_layer_norm_fwd(x, r, xs, nw, nb, 1e-5, out=y, mean=mean, rstd=rstd), y)[1],
            lambda: (ops.add_layer_norm_fwd(x, r, xs, nw, nb, 1e-5, out=y, mean=mean, rstd=rstd, out_image=True), y)[1],
            None, 16 * M * D, True),
    }
    rows = []
    for name, (f0, f1, flop, nbytes, image_out) in cases.items():
        fns = {"presplit": f0, "act": f1}
        t, outs = {"presplit": [], "act": []}, {}
        for _ in range(a.pairs):
            for side in ("presplit", "act"):
                c0 = lib.vit_gemm_f32_presplit_act_count(0)
                t[side].append(timeit(fns[side], a.reps))
                reads = lib.vit_gemm_f32_presplit_act_count(0) > c0
                assert reads == ("image X" in name and (side == "act" or name.startswith("producer: qkv"))), (name, side)
                outs[side] = fns[side]().clone()
        want = ops.weight_image_raw(outs["presplit"]) if image_out else outs["presplit"]
        med = {m: sorted(v)[len(v) // 2] for m, v in t.items()}
        row = {"case": name, "M": M, "pairs": a.pairs, "bit_equal": bool(torch.equal(raw(want), raw(outs["act"])))}
        for m in t:
            row[m + "_us"] = round(med[m] * 1e6, 1)
            if flop:
                row[m + "_tf"] = round(flop / med[m] / 1e12, 1)
            else:
                row[m + "_gbs"] = round(nbytes / med[m] / 1e9, 1)
            row[m + "_spread"] = round((max(t[m]) - min(t[m])) / med[m], 4)
        row["speedup"] = round(med["presplit"] / med["act"], 3)
        row["past_twice_the_larger_spread"] = bool(abs(row["speedup"] - 1) > 2 * max(row["presplit_spread"], row["act_spread"]))
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default="")
    ap.add_argument("--precision", choices=["highest", "high"], default="highest")
    ap.add_argument("--pairs", type=int, default=0)
    ap.add_argument("--presplit", action="store_true")
    ap.add_argument("--presplit-act", action="store_true")
    a = ap.parse_args()
    if a.presplit_act and not a.pairs:
        ap.error("--presplit-act alternates two sides: give --pairs N")
    a.presplit = a.presplit or a.presplit_act
    ops.set_float32_matmul_precision("high" if a.presplit else a.precision)
    dev = torch.device("cuda", 0)
    M, D = a.batch * 257, 1024
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(M, D, device=dev, generator=g)
    h = torch.randn(M, 4 * D, device=dev, generator=g)
    w = {n: torch.randn(o, i, device=dev, generator=g) * 0.03
         for n, (o, i) in {"qkv": (3 * D, D), "proj": (D, D), "fc1": (4 * D, D), "fc2": (D, 4 * D)}.items()}
    b = {n: torch.zeros(t.shape[0], device=dev) for n, t in w.items()}
    dy4 = torch.randn(M, 4 * D, device=dev, generator=g)
    dy1 = torch.randn(M, D, device=dev, generator=g)
    pre = torch.empty(M, 4 * D, device=dev)
    act = torch.empty_like(pre)
    # the weights' images (forward) and their transposes' (input gradient); `img` switches the cases between them
    wi = {n: ops.weight_image_raw(t) for n, t in w.items()} if a.presplit else {}
    wt = {n: ops.weight_image_raw(w[n], transposed=True) for n in ("fc1", "fc2")} if a.presplit else {}
    img = {"on": a.presplit}
    I = lambda d, n: d[n] if img["on"] else None
    cases = {
        "fwd qkv (bias)": (lambda: ops.linear_fwd(x, w["qkv"], b["qkv"], wimg=I(wi, "qkv")), 2 * M * 3 * D * D),
        "fwd proj (bias)": (lambda: ops.linear_fwd(x, w["proj"], b["proj"], wimg=I(wi, "proj")), 2 * M * D * D),
        "fwd fc1 (bias + QuickGELU pair)": (lambda: ops.linear_fwd(x, w["fc1"], b["fc1"], epi=L.EPI_BIAS_QGELU,
                                                                   out=pre, act_out=act, wimg=I(wi, "fc1")),
                                            2 * M * 4 * D * D),
        "fwd fc2 (bias)": (lambda: ops.linear_fwd(h, w["fc2"], b["fc2"], wimg=I(wi, "fc2")), 2 * M * 4 * D * D),
        "dgrad fc2 -> dh": (lambda: ops.linear_dgrad(dy1, w["fc2"], out_dtype=torch.float32, wimg=I(wt, "fc2")),
                            2 * M * 4 * D * D),
        "dgrad fc1 -> dx": (lambda: ops.linear_dgrad(dy4, w["fc1"], out_dtype=torch.float32, wimg=I(wt, "fc1")),
                            2 * M * 4 * D * D),
    }
    st = L.stream_ptr(dev)
    out = []
    if a.presplit:
        for N, K in ((1024, 1024), (4096, 1024), (1024, 4096)):
            src = torch.randn(N, K, device=dev, generator=g)
            for tr in (False, True):
                dst = torch.empty((K, N) if tr else (N, K), device=dev)
                t = timeit(lambda: ops.weight_image_raw(src, tr, out=dst), a.reps)
                row = {"case": f"image pass [{N},{K}]" + (" transposed" if tr else ""), "us": round(t * 1e6, 1),
                       "gbs": round(8 * N * K / t / 1e9, 1)}
                print(json.dumps(row), flush=True)
                out.append(row)
    if a.pairs and a.presplit_act:
        out += presplit_act_pairs(a, dev, M, D, x, h, w, b, wi)
        cases = {}
        ops.set_float32_matmul_precision("highest")
    elif a.pairs and a.presplit:
        ops._SK.pop(st, None)
        ops._streamk(dev)
        lib = L.lib()
        for name, (fn, flop) in cases.items():
            t, outs = {"high": [], "presplit": []}, {}
            for _ in range(a.pairs):
                for side in ("high", "presplit"):
                    img["on"] = side == "presplit"
                    c0 = lib.vit_gemm_f32_presplit_count(0)
                    t[side].append(timeit(fn, a.reps))
                    assert (lib.vit_gemm_f32_presplit_count(0) > c0) == img["on"], (name, side)
                    r = fn()
                    outs[side] = (r[0] if isinstance(r, tuple) else r).clone()
            med = {m: sorted(v)[len(v) // 2] for m, v in t.items()}
            row = {"case": name, "M": M, "gflop": round(flop / 1e9, 2), "pairs": a.pairs,
                   "bit_equal": bool(torch.equal(outs["high"].view(torch.int32), outs["presplit"].view(torch.int32)))}
            for m in t:
                row[m + "_us"] = round(med[m] * 1e6, 1)
                row[m + "_tf"] = round(flop / med[m] / 1e12, 1)
                row[m + "_spread"] = round((max(t[m]) - min(t[m])) / med[m], 4)
            row["speedup"] = round(med["high"] / med["presplit"], 3)
            print(json.dumps(row), flush=True)
            out.append(row)
        cases = {}
        ops.set_float32_matmul_precision("highest")
    elif a.pairs:
        ops._SK.pop(st, None)
        ops._streamk(dev)
        for name, (fn, flop) in cases.items():
            t = {"highest": [], "high": []}
            for _ in range(a.pairs):
                for mode in ("highest", "high"):
                    ops.set_float32_matmul_precision(mode)
                    t[mode].append(timeit(fn, a.reps))
            ops.set_float32_matmul_precision("highest")
            med = {m: sorted(v)[len(v) // 2] for m, v in t.items()}
            row = {"case": name, "M": M, "gflop": round(flop / 1e9, 2), "pairs": a.pairs}
            for m in t:
                row[m + "_us"] = round(med[m] * 1e6, 1)
                row[m + "_tf"] = round(flop / med[m] / 1e12, 1)
                row[m + "_spread"] = round((max(t[m]) - min(t[m])) / med[m], 4)
            row["speedup"] = round(med["highest"] / med["high"], 3)
            print(json.dumps(row), flush=True)
            out.append(row)
        cases = {}
    for name, (fn, flop) in cases.items():
        row = {"case": name, "M": M, "gflop": round(flop / 1e9, 2),
               "precision": "high, pre-split" if a.presplit else a.precision}
        r = fn()
        row["sum"] = float((r[0] if isinstance(r, tuple) else r).double().sum())
        for mode in ("plain", "streamk"):
            if mode == "plain":  # unregistered, and marked registered so the ops do not register it
                L.lib().vit_gemm_streamk_workspace(st, None, 0, None, 0)
                ops._SK[st] = None
            else:
                ops._SK.pop(st, None)
                ops._streamk(dev)
            t = timeit(fn, a.reps)
            row[mode + "_us"] = round(t * 1e6, 1)
            row[mode + "_tf"] = round(flop / t / 1e12, 1)
        row["frac_streamk"] = round(row["streamk_tf"] / PEAK_F32, 3)
        print(json.dumps(row), flush=True)
        out.append(row)
    if a.json:
        with open(a.json, "w") as f:
            for r in out:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
