"""Attention past 288 tokens: the streamed MFMA kernels against the generic kernels
(vit_sdpa_long_config(1) / (0)) at --n tokens, in bf16 or f32 (--dtype), forward and backward (with the
qkv-bias gradient, as the step runs it), and the resident kernels at --n-resident tokens with the same B and H
for the cost of streaming per score.  The variants alternate over --rounds rounds; the medians and each
variant's round-to-round spread are reported.

    python tools/bench_attn_long.py [--dtype bf16|f32] [--batch 64] [--heads 12] [--n 577] [--n-resident 257]
                                    [--reps 20] [--fp8] [--pairs P]

--fp8 (forward only): the streamed fp8 kernel against the streamed forward of --dtype at --n, and the resident fp8
kernel against the streamed one at --n-resident (<= 320).  At both lengths also the pre-quantised form (DESIGN
§4.20): the pre-pass alone, the consumer alone (on a workspace made beforehand) and the pair as ops.sdpa_fwd runs it
past 320 tokens (workspace from the caching allocator in every call).

--pairs P (--dtype f32, P >= 3): instead, the streamed f32 kernels at --n in both arithmetics -- "highest" (f32 MFMA)
and "high" + long (bf16x3, ``ops.set_float32_attention_precision("high", long_sequences=True)``) --
alternated over P pairs in this one process, as tools/bench_attn_f32.py alternates the resident kernels: per kernel
and mode the median of P windows of --reps back-to-back calls, the spread (max - min) / median, the ratio of the
medians and whether it counts (past twice the larger spread).  One JSON line.

--image (with --dtype f32 --pairs P): the streamed "high" forward on f32 qkv / o against the image
forward (``vit_sdpa_fwd_image``) at --n, alternated the same way (tools/bench_attn_f32.py's image leg: bit equality of
the two sides is asserted before anything is timed).  One JSON line.

Prints one JSON line per (variant, round) and a final summary line.  --no-generic / --no-streamed skip a
variant (a tree without the streamed kernels can still time its resident kernels with --n 0).
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
from tools.bench_kernels import timeit  # noqa: E402


def case(B, H, N, dtype=torch.bfloat16, dev="cuda"):
    D = H * 64
    g = torch.Generator(device=dev).manual_seed(1)
    qkv = torch.randn(B * N, 3 * D, device=dev, generator=g).to(dtype)
    do = torch.randn(B * N, D, device=dev, generator=g).to(dtype)
    o, lse = ops.sdpa_fwd(qkv, B, H, N)
    return dict(B=B, H=H, N=N, qkv=qkv, do=do, o=o, lse=lse, dq=torch.empty_like(qkv),
                dbias=torch.empty(3 * D, device=dev))


def time_case(c, reps):
    B, H, N = c["B"], c["H"], c["N"]
    tf = timeit(lambda: ops.sdpa_fwd(c["qkv"], B, H, N, o=c["o"], lse=c["lse"]), reps)
    tb = timeit(lambda: ops.sdpa_bwd(c["qkv"], c["o"], c["do"], c["lse"], B, H, N, dqkv=c["dq"], dbias=c["dbias"]),
                reps)
    fl = 4.0 * B * H * N * N * 64  # forward: QK^T and PV; the backward has 5 such products
    return {"fwd_ms": round(tf * 1e3, 4), "bwd_ms": round(tb * 1e3, 4), "fwd_tflops": round(fl / tf / 1e12, 1),
            "bwd_tflops": round(2.5 * fl / tb / 1e12, 1),
            "fwd_us_per_head": round(tf * 1e6 / (B * H), 4), "bwd_us_per_head": round(tb * 1e6 / (B * H), 4)}


def main_fp8(a, dtype):
    """--fp8, forward only: at --n the streamed fp8 kernel (ops.sdpa_fwd(fp8=True, fp8_long=True)) against the
    streamed forward of --dtype; at --n-resident the resident fp8 kernel against the streamed one
    (ops.sdpa_fwd_fp8_stream).  At both lengths the pre-quantised form: pre-pass alone, consumer alone, the pair.
    The variants alternate over --rounds rounds in this one process."""
    L.lib().vit_sdpa_long_config(1)
    variants = []

    def pre_variants(c, at):
        """The pre-quantised form on case c: its three timings, names suffixed with `at`."""
        B, H, N = c["B"], c["H"], c["N"]
        ws = ops.sdpa_fp8_quant_kv(c["qkv"], B, H, N)

        def pair():
            w = ops.sdpa_fp8_quant_kv(c["qkv"], B, H, N)  # allocated per call, as ops.sdpa_fwd(fp8_pre=True) does
            return ops.sdpa_fwd_fp8_pre(c["qkv"], w, B, H, N, o=c["o"], lse=c["lse"])
        return [("fp8 pre-pass" + at, c, lambda: ops.sdpa_fp8_quant_kv(c["qkv"], B, H, N, ws=ws)),
                ("fp8 consumer" + at, c, lambda: ops.sdpa_fwd_fp8_pre(c["qkv"], ws, B, H, N, o=c["o"], lse=c["lse"])),
                ("fp8 pre-pass + consumer" + at, c, pair)]

    if a.n:
        c = case(a.batch, a.heads, a.n, dtype)
        fwd = lambda c=c, **kw: ops.sdpa_fwd(c["qkv"], c["B"], c["H"], c["N"], o=c["o"], lse=c["lse"], **kw)
        variants += [(f"streamed {a.dtype}", c, fwd), ("streamed fp8", c, lambda: fwd(fp8=True, fp8_long=True))]
        variants += pre_variants(c, "")
    if a.n_resident:
        r = case(a.batch, a.heads, a.n_resident, dtype)
        variants += [("resident fp8 @ n_resident",  r, lambda: ops.sdpa_fwd(r["qkv"], r["B"], r["H"], r["N"], o=r["o"],
                                                                              lse=r["lse"], fp8=True)),
                     ("streamed fp8 @ n_resident", r, lambda: ops.sdpa_fwd_fp8_stream(r["qkv"], r["B"], r["H"], r["N"],
                                                                                       o=r["o"], lse=r["lse"]))]
        variants += pre_variants(r, " @ n_resident")
    res = {name: [] for name, *_ in variants}
    try:
        for rnd in range(a.rounds):
            for name, vc, f in variants:
                t = timeit(f, a.reps)
                fl = 4.0 * vc["B"] * vc["H"] * vc["N"] * vc["N"] * 64
                row = {"fwd_ms": round(t * 1e3, 4), "fwd_tflops": round(fl / t / 1e12, 1)}
                res[name].append(row)
                print(json.dumps({"variant": name, "dtype": a.dtype, "round": rnd, "N": vc["N"], "batch": a.batch,
                                  "heads": a.heads, **row}), flush=True)
    finally:
        L.lib().vit_sdpa_long_config(-1)
    med = {name: statistics.median(r["fwd_ms"] for r in rs) for name, rs in res.items()}
    spread = {name: round((max(r["fwd_ms"] for r in rs) - min(r["fwd_ms"] for r in rs)) / med[name], 4)
              for name, rs in res.items()}
    out = {"summary": True, "fp8": True, "dtype": a.dtype, "batch": a.batch, "heads": a.heads, "n": a.n,
           "n_resident": a.n_resident, "median_fwd_ms": med, "spread": spread}
    if a.n:
        out[f"streamed_{a.dtype}_over_streamed_fp8"] = round(med[f"streamed {a.dtype}"] / med["streamed fp8"], 3)
        out["pair_over_streamed_fp8"] = round(med["fp8 pre-pass + consumer"] / med["streamed fp8"], 3)
        out[f"pair_over_streamed_{a.dtype}"] = round(med["fp8 pre-pass + consumer"] / med[f"streamed {a.dtype}"], 3)
    if a.n_resident:
        out["streamed_fp8_over_resident_fp8"] = round(med["streamed fp8 @ n_resident"] / med["resident fp8 @ n_resident"], 3)
        out["pair_over_resident_fp8"] = round(med["fp8 pre-pass + consumer @ n_resident"]
                                              / med["resident fp8 @ n_resident"], 3)
    print(json.dumps(out), flush=True)


def main_pairs(a):
    """--pairs: streamed f32 attention at --n, "highest" against "high" + long, alternated."""
    from tools.bench_attn_f32 import summary, window
    B, H, N = a.batch, a.heads, a.n
    lib = L.lib()
    lib.vit_sdpa_long_config(1)
    c = case(B, H, N, torch.float32)
    calls = {"fwd": lambda: ops.sdpa_fwd(c["qkv"], B, H, N, o=c["o"], lse=c["lse"]),
             "bwd": lambda: ops.sdpa_bwd(c["qkv"], c["o"], c["do"], c["lse"], B, H, N, dqkv=c["dq"], dbias=c["dbias"])}
    modes = ("highest", "high+long")
    switch = lambda m: ops.set_float32_attention_precision(m.split("+")[0], long_sequences=m.endswith("+long"))
    us = {k: {m: [] for m in modes} for k in calls}
    try:
        for m in modes:  # warm both modes, and check which kernels each takes
            switch(m)
            c0, s0 = lib.vit_sdpa_long_f32_split_count(0), lib.vit_sdpa_long_f32_count(0)
            for fn in calls.values():
                window(fn, 3)
            took = (lib.vit_sdpa_long_f32_split_count(0) - c0, lib.vit_sdpa_long_f32_count(0) - s0)
            assert took == ((6, 6) if m != "highest" else (0, 6)), (m, took)
        for _ in range(a.pairs):
            for m in modes:
                switch(m)
                for k, fn in calls.items():
                    us[k][m].append(window(fn, a.reps))
    finally:
        ops.set_float32_attention_precision("highest")
        lib.vit_sdpa_long_config(-1)
    rec = {"B": B, "H": H, "N": N, "dtype": "f32", "pairs": a.pairs, "reps": a.reps, "bwd_with_dbias": True}
    fl = 4.0 * B * H * N * N * 64
    for k in calls:
        s = {m: summary(us[k][m]) for m in modes}
        ratio = s["highest"]["median_us"] / s["high+long"]["median_us"]
        s["high_long_speedup"] = round(ratio, 3)
        s["counts"] = bool(abs(ratio - 1) > 2 * max(s[m]["spread"] for m in modes))
        s["high_long_tflops_of_the_f32_product"] = round((1.0 if k == "fwd" else 2.5) * fl
                                                         / s["high+long"]["median_us"] / 1e6, 1)
        rec[k] = s
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fp8", action="store_true", help="forward only: the streamed fp8 kernel against the streamed "
                    "forward of --dtype at --n, and against the resident fp8 kernel at --n-resident")
    ap.add_argument("--dtype", choices=("bf16", "f32"), default="bf16")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--heads", type=int, default=12)
    ap.add_argument("--n", type=int, default=577, help="0: skip the long variants")
    ap.add_argument("--n-resident", type=int, default=257, help="0: skip the resident kernels")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--reps-generic", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-generic", action="store_true")
    ap.add_argument("--no-streamed", action="store_true")
    ap.add_argument("--pairs", type=int, default=0, help="--dtype f32: alternate the streamed kernels' highest and "
                    "high + long arithmetic over this many pairs (at least 3) instead of the variants above")
    ap.add_argument("--image", action="store_true", help="with --dtype f32 --pairs: the streamed high forward on f32 "
                    "tensors against the image forward")
    a = ap.parse_args()
    if a.image and not a.pairs:
        ap.error("--image needs --pairs")
    if a.pairs:
        if a.pairs < 3 or a.dtype != "f32" or a.fp8 or a.n <= 288:
            ap.error("--pairs needs at least 3 pairs, --dtype f32, --n past 288 and no --fp8")
        if a.image:
            from tools.bench_attn_f32 import image_leg
            print(json.dumps(image_leg(a.batch, a.heads, a.n, 0, a.pairs, a.reps)), flush=True)
            return None
        return main_pairs(a)
    lib = L.lib()
    dtype = torch.float32 if a.dtype == "f32" else torch.bfloat16
    if a.fp8:
        return main_fp8(a, dtype)
    variants = []
    if a.n:
        long_case = case(a.batch, a.heads, a.n, dtype)
        if not a.no_streamed:
            variants.append(("streamed", 1, long_case, a.reps))
        if not a.no_generic:
            variants.append(("generic", 0, long_case, a.reps_generic))
    if a.n_resident:
        variants.append(("resident", None, case(a.batch, a.heads, a.n_resident, dtype), a.reps))
    res = {name: [] for name, *_ in variants}
    try:
        for rnd in range(a.rounds):
            for name, mode, c, reps in variants:
                if mode is not None:
                    lib.vit_sdpa_long_config(mode)
                r = time_case(c, reps)
                res[name].append(r)
                print(json.dumps({"variant": name, "dtype": a.dtype, "round": rnd, "N": c["N"], "batch": a.batch,
                                  "heads": a.heads, **r}), flush=True)
    finally:
        if a.n:
            lib.vit_sdpa_long_config(-1)
    med = {name: {k: statistics.median(r[k] for r in rs) for k in ("fwd_ms", "bwd_ms")} for name, rs in res.items()}
    # round-to-round spread of each variant: (max - min) / median over the rounds
    spread = {name: {k: round((max(r[k] for r in rs) - min(r[k] for r in rs)) / med[name][k], 4)
                     for k in ("fwd_ms", "bwd_ms")} for name, rs in res.items()}
    out = {"summary": True, "dtype": a.dtype, "batch": a.batch, "heads": a.heads, "n": a.n,
           "n_resident": a.n_resident, "median_ms": med, "spread": spread}
    if "streamed" in med and "generic" in med:
        out["generic_over_streamed"] = {k: round(med["generic"][k] / med["streamed"][k], 2) for k in ("fwd_ms", "bwd_ms")}
    if "streamed" in med and "resident" in med:
        # same B and H, so the per-(b, h) time ratio is the ratio of the call times
        out["streamed_over_resident"] = {k: round(med["streamed"][k] / med["resident"][k], 2)
                                         for k in ("fwd_ms", "bwd_ms")}
        out["score_work_ratio"] = round((a.n / a.n_resident) ** 2, 2)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
