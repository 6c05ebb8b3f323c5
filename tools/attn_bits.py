"""Bit digests of the attention kernels' outputs, to compare two builds of the library (VIT_HIP_LIB selects it):

    VIT_HIP_LIB=<lib a> python tools/attn_bits.py > a.jsonl
    VIT_HIP_LIB=<lib b> python tools/attn_bits.py > b.jsonl        # the two files must be identical

One JSON line per seeded case (inputs as tests/test_gpu_attention_long.py::_case, B = 2, H = 3): SHA-1 of o, lse,
dqkv, delta_ws and dbias; for bf16 also of the [B][3D] bias partials that partial-only mode (dbias == NULL) leaves.
The backward runs from the library's own o and lse.  Cases: the bf16 resident two-kernel backward (N > 224, and
vit_sdpa_bwd_variant(2) below that), the f32 resident kernels, the streamed kernels of both dtypes, the fused
bf16 backward as a control, and last the f32 resident kernels in the "high" mode (vit_sdpa_f32_precision(1), the
bf16x3 kernels; N = 1, 17, 33, 77 causal, 257, 288: one tile, an edge inside a pair's second tile, an odd tile
count, the mask, one workgroup per CU, every tile full) and the f32 streamed kernels in the high + long mode
(vit_sdpa_f32_long_precision(1) as well, the streamed bf16x3 kernels; N = 289, 321, 577; skipped on a library that
lacks the export, whose file then ends three lines earlier).  First come the resident fp8 forward's o and lse (N = 77
causal, 197, 257, 320, both dtypes; ``--fp8-only`` stops after them).
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "vit-project_amd"))

import torch  # noqa: E402

from vit_amd import _lib as L  # noqa: E402
from vit_amd import ops  # noqa: E402
from vit_amd._lib import call, ptr  # noqa: E402

BF16, F32 = torch.bfloat16, torch.float32
B, H = 2, 3
# (kernels, dtype, N, causal, vit_sdpa_bwd_variant)
CASES = ([("bf16 resident two-kernel", BF16, n, False, -1) for n in (240, 257, 288)] +
         [("bf16 resident two-kernel", BF16, 197, False, 2), ("bf16 resident two-kernel", BF16, 77, True, 2)] +
         [("f32 resident", F32, n, c, -1) for n, c in ((50, False), (77, True), (197, False), (257, False), (288, False))] +
         [("streamed", dt, n, False, -1) for dt in (BF16, F32) for n in (289, 320, 577)] +
         [("bf16 fused (control)", BF16, 197, False, -1)])
# f32 resident under vit_sdpa_f32_precision(1): (N, causal)
HIGH_CASES = ((1, False), (17, False), (33, False), (77, True), (257, False), (288, False))
# f32 streamed under vit_sdpa_f32_precision(1) and vit_sdpa_f32_long_precision(1)
HIGH_LONG_CASES = (289, 321, 577)
# the resident fp8 forward (o and lse only), both dtypes; --fp8-only runs these alone
FP8_CASES = ((77, True), (197, False), (257, False), (320, False))


def sha(t):
    t = t.detach().contiguous().cpu()
    if t.dtype == BF16:
        t = t.view(torch.int16)
    return hashlib.sha1(t.numpy().tobytes()).hexdigest()


def run(dtype, N, causal):
    D = H * 64
    g = torch.Generator().manual_seed(34)
    qkv = (torch.randn(B * N, 3 * D, generator=g) * 1.5).to(dtype).cuda()
    do = torch.randn(B * N, D, generator=g).to(dtype).cuda()
    o, lse = ops.sdpa_fwd(qkv, B, H, N, causal=causal)
    nfl = L.lib().vit_sdpa_bwd_partial_floats(B, N, D)
    out = {"o": sha(o), "lse": sha(lse)}
    for mode in ("dbias", "partial-only") if dtype == BF16 else ("dbias",):
        dqkv = torch.zeros_like(qkv)
        delta = torch.zeros(B * H * N, device="cuda")
        dbias = torch.zeros(3 * D, device="cuda")
        part = torch.zeros(nfl, device="cuda")
        call("vit_sdpa_bwd", L.dt(qkv), B, H, N, 64, ptr(qkv), qkv.stride(0), ptr(o), o.stride(0), ptr(do),
             do.stride(0), ptr(lse), ptr(dqkv), dqkv.stride(0), ptr(delta), 0.125, int(causal),
             ptr(dbias) if mode == "dbias" else None, ptr(part), nfl, L.stream_ptr(qkv.device))
        torch.cuda.synchronize()
        if mode == "dbias":
            out.update(dqkv=sha(dqkv), delta_ws=sha(delta), dbias=sha(dbias))
        else:
            out.update(partial_only_dqkv=sha(dqkv), partials=sha(part[:B * 3 * D]))
    return out


def run_fp8(dtype, N, causal):
    """o and lse of the resident fp8 forward (vit_sdpa_fwd_fp8; N <= 320)."""
    D = H * 64
    g = torch.Generator().manual_seed(34)
    qkv = (torch.randn(B * N, 3 * D, generator=g) * 1.5).to(dtype).cuda()
    o, lse = ops.sdpa_fwd(qkv, B, H, N, causal=causal, fp8=True)
    torch.cuda.synchronize()
    return {"o": sha(o), "lse": sha(lse)}


def main():
    # an older build of the library (the parent's, for comparison) lacks the exports added since: bind what it has
    import ctypes
    probe = ctypes.CDLL(L.LIB_PATH)
    for name in [n for n in L.SIGNATURES if not hasattr(probe, n)]:
        del L.SIGNATURES[name]
    L.load()
    lib = L.lib()
    for dtype in (BF16, F32):
        for N, causal in FP8_CASES:
            print(json.dumps({"kernels": "fp8 resident", "dtype": "bf16" if dtype == BF16 else "f32", "N": N,
                              "causal": causal, **run_fp8(dtype, N, causal)}), flush=True)
    if "--fp8-only" in sys.argv[1:]:
        return
    for kernels, dtype, N, causal, variant in CASES:
        lib.vit_sdpa_bwd_variant(variant)
        try:
            r = run(dtype, N, causal)
        finally:
            lib.vit_sdpa_bwd_variant(-1)
        print(json.dumps({"kernels": kernels, "dtype": "bf16" if dtype == BF16 else "f32", "N": N, "causal": causal,
                          "bwd_variant": variant, **r}), flush=True)
    for N, causal in HIGH_CASES:
        lib.vit_sdpa_f32_precision(1)
        try:
            lib.vit_sdpa_f32_split_count(1)  # zero it
            r = run(F32, N, causal)
            took = lib.vit_sdpa_f32_split_count(1)
        finally:
            lib.vit_sdpa_f32_precision(0)
        assert took == 2, ("the forward and the backward must both take the bf16x3 kernels", N, took)
        print(json.dumps({"kernels": "f32 resident high", "dtype": "f32", "N": N, "causal": causal,
                          "bwd_variant": -1, **r}), flush=True)
    if "vit_sdpa_f32_long_precision" not in L.SIGNATURES:  # an older build
        return
    for N in HIGH_LONG_CASES:
        lib.vit_sdpa_f32_precision(1)
        lib.vit_sdpa_f32_long_precision(1)
        try:
            lib.vit_sdpa_long_f32_split_count(1)  # zero it
            r = run(F32, N, False)
            took = lib.vit_sdpa_long_f32_split_count(1)
        finally:
            lib.vit_sdpa_f32_precision(0)
            lib.vit_sdpa_f32_long_precision(0)
        assert took == 2, ("the forward and the backward must both take the streamed bf16x3 kernels", N, took)
        print(json.dumps({"kernels": "f32 streamed high + long", "dtype": "f32", "N": N, "causal": False,
                          "bwd_variant": -1, **r}), flush=True)


if __name__ == "__main__":
    main()
