"""Forward-only path against the training chain, alternated within one process (device events).

    python tools/bench_eval.py [--what fc1,vit] [--repeats 7] [--iters 20] [--batch 256] [--out FILE]

  fc1   the fc1 launch alone: pair epilogue (act' and act written) against the act-only one, at the
        bf16 forward chains' half-batch row counts (27580 / 22852 x 3072 x 768) and at C3's fc1
        (16448 x 4096 x 1024, bf16 with QuickGELU and fp32); bytes written are computed from shapes.
  vit   ViT-B/16 no-grad forward, images/s, set_forward_only(True) against (False).
  vit384fp8  vit_base_patch16_384 no-grad forward (577 tokens), three legs alternated: bf16 attention, the streamed
        fp8 kernel and the pre-quantised fp8 pair (not in the default --what; use --batch 64).

Each pair is warmed up, then timed ``repeats`` times in the order A B A B ..., ``iters`` launches (or
forwards) per timing; the record holds every repeat, the medians, the A/B difference and the repeat
spread ((max - min) / median) next to it.  One JSON line per case on stdout (and in --out).
The C3 step uses tools/bench_clip.py under VIT_FWD_ONLY=1 / =0.
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


def _time(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters  # ms per call


def alternate(fa, fb, repeats, iters, warmup=5):
    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(repeats):
        ta.append(_time(fa, iters))
        tb.append(_time(fb, iters))
    return ta, tb


def summary(ta, tb):
    ma, mb = statistics.median(ta), statistics.median(tb)
    return {"a_ms": [round(t, 4) for t in ta], "b_ms": [round(t, 4) for t in tb],
            "a_median_ms": round(ma, 4), "b_median_ms": round(mb, 4),
            "b_over_a": round(mb / ma, 4),
            "a_spread": round((max(ta) - min(ta)) / ma, 4), "b_spread": round((max(tb) - min(tb)) / mb, 4)}


def bench_fc1(repeats, iters):
    from vit_amd import _lib as L
    from vit_amd import ops
    out = []
    cases = [("vit_b16_fwd_half_a", 27580, 3072, 768, torch.bfloat16, False),
             ("vit_b16_fwd_half_b", 22852, 3072, 768, torch.bfloat16, False),
             ("c3_fc1_bf16", 16448, 4096, 1024, torch.bfloat16, True),
             ("c3_fc1_f32", 16448, 4096, 1024, torch.float32, True)]
    for name, M, N, K, T, quick in cases:
        g = torch.Generator().manual_seed(1)
        x = torch.randn(M, K, generator=g).to(T).cuda()
        w = (torch.randn(N, K, generator=g) * K ** -0.5).to(T).cuda()
        b = torch.randn(N, generator=g).cuda()
        dact, act, only = (torch.empty(M, N, dtype=T, device="cuda") for _ in range(3))
        pair = L.EPI_BIAS_QGELU if quick else L.EPI_BIAS_GELU
        fwd = L.EPI_BIAS_QGELU_FWD if quick else L.EPI_BIAS_GELU_FWD
        fa = lambda: ops.linear_fwd(x, w, b, epi=pair, out=dact, act_out=act)  # noqa: E731
        fb = lambda: ops.linear_fwd(x, w, b, epi=fwd, out=only)  # noqa: E731
        ta, tb = alternate(fa, fb, repeats, iters)
        torch.cuda.synchronize()
        esz = 2 if T == torch.bfloat16 else 4
        r = {"case": "fc1_" + name, "a": "pair epilogue", "b": "act-only epilogue", "M": M, "N": N, "K": K,
             "dtype": str(T)[6:], "act": "quick_gelu" if quick else "gelu", "iters": iters,
             "a_bytes_written": 2 * M * N * esz, "b_bytes_written": M * N * esz,
             "bitwise_equal": bool(torch.equal(act, only))}
        r.update(summary(ta, tb))
        out.append(r)
        del x, w, dact, act, only
    return out


def bench_vit(repeats, iters, batch):
    import vit_amd
    torch.manual_seed(0)
    m = vit_amd.create_model("vit_base_patch16_224", num_classes=1000).cuda().eval()
    x = torch.randn(batch, 3, 224, 224, device="cuda")

    def run(on):
        def f():
            vit_amd.set_forward_only(on)
            with torch.no_grad():
                return m(x)
        return f

    y_off, y_on = run(False)(), run(True)()
    ta, tb = alternate(run(False), run(True), repeats, iters, warmup=3)
    vit_amd.set_forward_only(True)
    r = {"case": "vit_b16_nograd_forward", "a": "set_forward_only(False)", "b": "set_forward_only(True)",
         "batch": batch, "iters": iters, "bitwise_equal": bool(torch.equal(y_off, y_on))}
    r.update(summary(ta, tb))
    r["a_images_per_s"] = round(batch / r["a_median_ms"] * 1e3, 1)
    r["b_images_per_s"] = round(batch / r["b_median_ms"] * 1e3, 1)
    return [r]


def bench_vit384_fp8(repeats, iters, batch):
    """vit_base_patch16_384 (577 tokens, bf16) no-grad forward: bf16 attention against the streamed fp8 kernel
    (set_attention_fp8(True, long_sequences=True)) and the pre-quantised pair (..., prequantize=True)."""
    import vit_amd
    from vit_amd import _lib as L
    torch.manual_seed(0)
    m = vit_amd.create_model("vit_base_patch16_384", num_classes=1000, compute_dtype=torch.bfloat16).cuda().eval()
    x = torch.randn(batch, 3, 384, 384, device="cuda")

    def run(on, pre=False):
        def f():
            m.set_attention_fp8(on, long_sequences=on, prequantize=pre)
            with torch.no_grad():
                return m(x)
        return f

    fa, fb, fc = run(False), run(True), run(True, True)
    c0 = L.lib().vit_sdpa_fp8_stream_count(0)
    y_off, y_on = fa().float(), fb().float()
    streamed = L.lib().vit_sdpa_fp8_stream_count(0) - c0
    p0 = L.lib().vit_sdpa_fp8_pre_count(0)
    y_pre = fc().float()
    pre = L.lib().vit_sdpa_fp8_pre_count(0) - p0
    for _ in range(3):
        fa(), fb(), fc()
    torch.cuda.synchronize()
    ta, tb, tc = [], [], []
    for _ in range(repeats):  # A B C A B C ...
        ta.append(_time(fa, iters))
        tb.append(_time(fb, iters))
        tc.append(_time(fc, iters))
    m.set_attention_fp8(False)
    r = {"case": "vit_b16_384_nograd_forward", "a": "bf16 attention", "b": "streamed fp8 attention",
         "c": "pre-quantised fp8 attention", "batch": batch,
         "iters": iters, "fp8_stream_calls_per_forward": streamed, "fp8_pre_calls_per_forward": pre,
         "logits_max_abs_diff": round((y_on - y_off).abs().max().item(), 5),
         "logits_max_abs": round(y_off.abs().max().item(), 5),
         "c_bitwise_equal_b": bool(torch.equal(y_pre, y_on))}
    r.update(summary(ta, tb))
    mc = statistics.median(tc)
    r.update({"c_ms": [round(t, 4) for t in tc], "c_median_ms": round(mc, 4),
              "c_over_a": round(mc / r["a_median_ms"], 4), "c_over_b": round(mc / r["b_median_ms"], 4),
              "c_spread": round((max(tc) - min(tc)) / mc, 4)})
    for leg in "abc":
        r[leg + "_images_per_s"] = round(batch / r[leg + "_median_ms"] * 1e3, 1)
    return [r]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="fc1,vit", help="fc1, vit, vit384fp8 (comma-separated)")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval.py needs a GPU: nothing is measured without one")
    rows = []
    for what in a.what.split(","):
        if what == "fc1":
            rows += bench_fc1(a.repeats, a.iters)
        elif what == "vit":
            rows += bench_vit(a.repeats, a.iters, a.batch)
        elif what == "vit384fp8":
            rows += bench_vit384_fp8(a.repeats, a.iters, a.batch)
        else:
            raise SystemExit(f"unknown --what {what}")
    text = "\n".join(json.dumps(r) for r in rows)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
