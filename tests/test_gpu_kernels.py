"""GPU: every HIP kernel against a CPU fp32 reference of the same op.

Tolerances: f32-in/f32-out kernels 1e-5 relative to the output scale; bf16
inputs are rounded to bf16 before the CPU reference so only accumulation order
and the output rounding differ (bf16 out: 1e-2 of scale; f32 out: 1e-5).
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from vit_amd import _lib as L  # noqa: E402
from vit_amd import ops  # noqa: E402

DEV = "cuda"


def _close(got, ref, rel, what=""):
    got = got.detach().float().cpu()
    ref = ref.detach().float().cpu()
    scale = ref.abs().max().item() + 1e-12
    err = (got - ref).abs().max().item()
    assert err <= rel * scale, f"{what}: max err {err:.3e} > {rel:.1e} * scale {scale:.3e}"


def _gelu_grad(x):
    """d/dx of exact-erf GELU."""
    return 0.5 * (1 + torch.erf(x / 2 ** 0.5)) + x * torch.exp(-0.5 * x * x) / (2 * torch.pi) ** 0.5


def _rnd(*shape, dtype=torch.float32, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    L.load()


# ---------------------------------------------------------------------------- GEMM

@pytest.mark.parametrize("M,N,K", [(256, 384, 192), (1024, 768, 768), (384, 256, 3072)])
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
def test_linear_fwd_fast_bf16(M, N, K, out_dtype):
    x = _rnd(M, K, seed=1, dtype=torch.bfloat16)
    w = _rnd(N, K, seed=2, scale=0.05, dtype=torch.bfloat16)
    b = _rnd(N, seed=3)
    ref = x.float() @ w.float().T + b
    y = ops.linear_fwd(x.to(DEV), w.to(DEV), b.to(DEV), out_dtype=out_dtype)
    _close(y, ref, 1e-5 if out_dtype == torch.float32 else 8e-3, "fwd")


def test_linear_fwd_asymmetric_identity():
    # A = I with an asymmetric B catches a transposed C write (guide §3)
    n = 256
    x = torch.eye(n, dtype=torch.bfloat16)
    w = (torch.arange(n * n, dtype=torch.float32).reshape(n, n) % 97).to(torch.bfloat16)
    y = ops.linear_fwd(x.to(DEV), w.to(DEV), None, out_dtype=torch.float32)
    assert torch.equal(y.cpu(), w.float().T.contiguous())


def test_linear_epilogues_bf16():
    M, N, K = 512, 384, 256
    x = _rnd(M, K, seed=4, dtype=torch.bfloat16)
    w = _rnd(N, K, seed=5, scale=0.06, dtype=torch.bfloat16)
    b = _rnd(N, seed=6, scale=0.1)
    acc = x.float() @ w.float().T + b
    dact, act = ops.linear_fwd(x.to(DEV), w.to(DEV), b.to(DEV), epi=L.EPI_BIAS_GELU)
    _close(act, torch.nn.functional.gelu(acc), 8e-3, "gelu")
    _close(dact, _gelu_grad(acc), 8e-3, "gelu'")
    resid = _rnd(M, N, seed=7)
    out = ops.linear_fwd(x.to(DEV), w.to(DEV), b.to(DEV), epi=L.EPI_RESID, resid=resid.to(DEV))
    _close(out, resid + acc, 1e-5, "resid")
    # in-place residual (out aliases resid)
    r2 = resid.to(DEV)
    ops.linear_fwd(x.to(DEV), w.to(DEV), b.to(DEV), epi=L.EPI_RESID, resid=r2, out=r2)
    _close(r2, resid + acc, 1e-5, "resid inplace")
    # quick gelu
    dq, act_q = ops.linear_fwd(x.to(DEV), w.to(DEV), b.to(DEV), epi=L.EPI_BIAS_QGELU)
    s = torch.sigmoid(1.702 * acc)
    _close(act_q, acc * s, 8e-3, "qgelu")
    _close(dq, s + 1.702 * acc * s * (1 - s), 8e-3, "qgelu'")


def test_linear_dgrad_and_gelu_bwd():
    M, N, K = 512, 256, 384
    dy = _rnd(M, N, seed=8, dtype=torch.bfloat16)
    w = _rnd(N, K, seed=9, scale=0.05, dtype=torch.bfloat16)
    ref = dy.float() @ w.float()
    dx = ops.linear_dgrad(dy.to(DEV), w.to(DEV), out_dtype=torch.float32)
    _close(dx, ref, 1e-5, "dgrad")
    pre = _rnd(M, K, seed=10, dtype=torch.bfloat16)
    pf = pre.float().requires_grad_(True)
    torch.nn.functional.gelu(pf).backward(ref)
    db = torch.empty(K, device=DEV)
    # the forward epilogue saves gelu'(pre); the dgrad epilogue multiplies by it
    dact = _gelu_grad(pre.float()).to(torch.bfloat16)
    d = ops.linear_dgrad(dy.to(DEV), w.to(DEV), out_dtype=torch.bfloat16, epi=L.EPI_GELU_BWD, pre=dact.to(DEV),
                         dbias=db)
    _close(d, pf.grad, 8e-3, "gelu bwd")
    # the kernel multiplies by the bf16-rounded gelu' the forward stored: sum exactly that
    _close(db, (ref * dact.float()).sum(0), 1e-3, "fused bias grad (MFMA epilogue)")


@pytest.mark.parametrize("M,N,K,dtype", [(197 * 3, 640, 448, torch.bfloat16), (300, 96, 72, torch.float32),
                                         (70, 64, 40, torch.bfloat16)])
def test_linear_dgrad_fused_bias(M, N, K, dtype):
    """dbias = column sums of dX, fused (MFMA path, ragged M) or after the generic kernel."""
    dy = _rnd(M, N, seed=50, dtype=dtype)
    w = _rnd(N, K, seed=51, scale=0.05, dtype=dtype)
    ref = dy.float() @ w.float()
    db = torch.full((K,), 3.0, device=DEV)
    dx = ops.linear_dgrad(dy.to(DEV), w.to(DEV), out_dtype=torch.float32, dbias=db)
    _close(dx, ref, 1e-5, "dgrad")
    _close(db, ref.sum(0), 1e-5, "dbias")


def test_gemm_rc_operand_past_4gib_is_chunked():
    """An RC operand whose staging offsets pass 2^32 bytes (a [M, 1024]-strided bf16 view over
    4.3 GB) runs as row chunks with every row-indexed operand shifted: forward and
    GELU' dgrad with fused bias sums, checked around the chunk seam and in total."""
    M, LD, K, N = (1 << 21) + 768, 1024, 64, 256
    assert L.lib().vit_gemm_rc_chunk_rows(M, LD) == 1 << 21
    g = torch.Generator(device=DEV).manual_seed(3)
    buf = torch.randn(M, LD, device=DEV, generator=g).to(torch.bfloat16)
    x = buf[:, :K]
    w = (torch.randn(N, K, device=DEV, generator=g) * 0.1).to(torch.bfloat16)
    b = torch.randn(N, device=DEV, generator=g)
    y = ops.linear_fwd(x, w, b, out_dtype=torch.bfloat16)
    for r0, r1 in ((0, 512), ((1 << 21) - 512, (1 << 21) + 512), (M - 300, M)):
        ref = x[r0:r1].float() @ w.float().T + b
        _close(y[r0:r1], ref, 8e-3, f"fwd rows {r0}:{r1}")
    del y
    wd = (torch.randn(K, N, device=DEV, generator=g) * 0.1).to(torch.bfloat16)  # dX[M, N] = dY[M, K] W[K, N]
    pre = torch.randn(M, N, device=DEV, generator=g).to(torch.bfloat16)
    db = torch.empty(N, device=DEV)
    d = ops.linear_dgrad(x, wd, out_dtype=torch.bfloat16, epi=L.EPI_GELU_BWD, pre=pre, dbias=db)
    ref_sum = torch.zeros(N, device=DEV, dtype=torch.float64)
    for r0 in range(0, M, 1 << 19):
        r1 = min(M, r0 + (1 << 19))
        ref = (x[r0:r1].float() @ wd.float()) * pre[r0:r1].float()
        if r0 <= (1 << 21) < r1 or r1 == M:
            _close(d[r0:r1], ref, 8e-3, f"gelu' dgrad rows {r0}:{r1}")
        ref_sum += ref.double().sum(0)
    _close(db, ref_sum.float(), 1e-3, "fused bias sums across chunks")


@pytest.mark.parametrize("M,N,K,split", [(1024, 256, 384, 1), (4096, 384, 256, 4), (6336, 256, 128, 7), (6304, 256, 128, 3)])
def test_linear_wgrad(M, N, K, split):
    dy = _rnd(M, N, seed=11, dtype=torch.bfloat16)
    x = _rnd(M, K, seed=12, dtype=torch.bfloat16)
    ref = dy.float().T @ x.float()
    dw = ops.linear_wgrad(dy.to(DEV), x.to(DEV), split=split)
    _close(dw, ref, 2e-5, "wgrad")


@pytest.mark.parametrize("M,N,K,split,dtype", [(6336, 256, 128, 7, torch.bfloat16), (6304 + 19, 256, 384, 3, torch.bfloat16),
                                               (4096, 512, 256, 4, torch.float32), (50, 256, 128, 2, torch.bfloat16)])
def test_linear_wgrad_partials_sum_to_dw(M, N, K, split, dtype):
    """Split-K slabs only (vit_linear_wgrad_partials, reduced later by the block's batch launch):
    their sum is dW, including a ragged M % 32 tail folded into the last slab; through ColBatch
    the result is the immediate path's reduction bit for bit while there are at most 8 slabs (the
    batch's short path adds the slabs in splitk_reduce_kernel's order: slab 0, then += slab z;
    tests/test_gpu_reductions.py pins both orders), and agrees with it to rounding past 8 (the
    tall path sums 64-row chunks wave by wave)."""
    dy = _rnd(M, N, seed=13, dtype=dtype)
    x = _rnd(M, K, seed=14, dtype=dtype)
    ref = dy.float().T @ x.float()
    dyd, xd = dy.to(DEV), x.to(DEV)
    b = ops.ColBatch()
    out = torch.empty(N, K, device=DEV)
    ops.linear_wgrad(dyd, xd, out=out, split=split, reduce_on=b)
    if dtype == torch.bfloat16:
        assert len(b.jobs) == 1 and b.jobs[0][2] == L.lib().vit_linear_wgrad_nslabs(L.dt(dyd), M, N, K, split)
    b.launch()
    torch.cuda.synchronize()
    _close(out, ref, 2e-5, "wgrad via batch")
    imm = ops.linear_wgrad(dyd, xd, split=split)
    _close(out, imm, 1e-6, "batch vs immediate reduction")
    if L.lib().vit_linear_wgrad_nslabs(L.dt(dyd), M, N, K, split) <= 8:
        assert torch.equal(out, imm), "batch vs immediate reduction: not bitwise equal with at most 8 slabs"


@pytest.mark.parametrize("M,tail", [(197 * 32, False), (197 * 32, True), (197 * 3, False)])
def test_linear_wgrad_pair_matches_separate(M, tail):
    """Two weight gradients as one grouped launch (fc2 + fc1 shapes at width 256 / 1024) against each
    computed alone; a ragged M (197 * 3 = 591, M % 32 != 0) takes the one-by-one fallback."""
    dya, xa = _rnd(M, 256, seed=60, dtype=torch.bfloat16), _rnd(M, 1024, seed=61, dtype=torch.bfloat16)
    dyb, xb = _rnd(M, 1024, seed=62, dtype=torch.bfloat16), _rnd(M, 256, seed=63, dtype=torch.bfloat16)
    ra, rb_ = dya.float().T @ xa.float(), dyb.float().T @ xb.float()
    d = [t.to(DEV) for t in (dya, xa, dyb, xb)]
    oa, ob = torch.empty(256, 1024, device=DEV), torch.empty(1024, 256, device=DEV)
    b = ops.ColBatch()
    ops.linear_wgrad_pair((d[0], d[1], oa), (d[2], d[3], ob), b, tail=tail)
    if M % 32 == 0:
        assert len(b.jobs) == 2  # grouped: the two slab sums are batch jobs
    b.launch()
    torch.cuda.synchronize()
    _close(oa, ra, 2e-5, "pair a")
    _close(ob, rb_, 2e-5, "pair b")


@pytest.mark.parametrize("M,N,K,split", [(6304, 256, 128, 3), (197 * 64, 768, 3072, 5), (197 * 32, 2304, 768, 2),
                                         (4096, 640, 448, 1)])
def test_w4_wgrad_bitwise_matches_pingpong(M, N, K, split):
    """The wide-wave weight-gradient kernel (w4, round 5's default: 4 waves of 128x128, asm MFMAs on AGPR
    accumulators) sums every split chunk's k-steps in the same order with the same MFMA as the round-1..4
    ping-pong kernel (variant 8), so the two agree bit for bit -- odd k-step counts (6304 rows in 3 chunks:
    66 / 66 / 65 steps), ragged output tiles (640 x 448) and every ring / load-placement configuration
    (12-15) included; and the pair launch equals two single launches."""
    lib = L.lib()
    dy = _rnd(M, N, seed=70, dtype=torch.bfloat16).to(DEV)
    x = _rnd(M, K, seed=71, dtype=torch.bfloat16).to(DEV)
    outs = {}
    try:
        for v in (8, 11, 12, 13, 14, 15):
            lib.vit_gemm_variant(v)
            outs[v] = ops.linear_wgrad(dy, x, split=split).cpu()
    finally:
        lib.vit_gemm_variant(-1)
    ref = dy.float().cpu().T @ x.float().cpu()
    _close(outs[11], ref, 2e-5, "w4 wgrad")
    for v in (11, 12, 13, 14, 15):
        assert torch.equal(outs[v], outs[8]), f"variant {v} differs from the ping-pong kernel"
    if M % 32 == 0:
        b = ops.ColBatch()
        oa, ob = torch.empty(N, K, device=DEV), torch.empty(K, N, device=DEV)
        ops.linear_wgrad_pair((dy, x, oa), (x, dy, ob), b)
        b.launch()
        torch.cuda.synchronize()
        _close(oa, ref, 2e-5, "pair a")
        _close(ob, ref.T, 2e-5, "pair b")


@pytest.mark.parametrize("group", [1, 3, 8])
def test_gemm_grouped_tile_walk(group):
    """The banded tile walk (vit_gemm_group) is a bijection over the tiles: every output tile is
    written exactly once for bands that divide the row tiles and for ragged last bands."""
    lib = L.lib()
    M, N, K = 197 * 13, 1536, 256       # 11 row tiles of 256 (the last ragged), 6 column tiles
    x = _rnd(M, K, seed=45, dtype=torch.bfloat16)
    w = _rnd(N, K, seed=46, scale=0.05, dtype=torch.bfloat16)
    dy = _rnd(M, N, seed=47, dtype=torch.bfloat16)
    lib.vit_gemm_group(group, group)
    try:
        _close(ops.linear_fwd(x.to(DEV), w.to(DEV), None, out_dtype=torch.float32), x.float() @ w.float().T, 1e-5,
               "fwd grouped")
        _close(ops.linear_dgrad(dy.to(DEV), w.to(DEV)), dy.float() @ w.float(), 1e-5, "dgrad grouped")
    finally:
        lib.vit_gemm_group(-2, -2)  # back to the defaults (forward row-major, input gradients bands of 4)


@pytest.mark.parametrize("variant", [1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 12, 13, 14, 15])
def test_gemm_every_tile_config(variant):
    """Every kept MFMA configuration (forced through vit_gemm_variant) on ragged
    M/N tiles, fwd + bias/GELU/residual epilogues, dgrad, split-K wgrad."""
    lib = L.lib()
    M, N, K = 197 * 3, 640, 448          # M, N not multiples of any tile; K % 64 == 0
    x = _rnd(M, K, seed=40, dtype=torch.bfloat16)
    w = _rnd(N, K, seed=41, scale=0.05, dtype=torch.bfloat16)
    b = _rnd(N, seed=42)
    res = _rnd(M, N, seed=43)
    dy = _rnd(M, N, seed=44, dtype=torch.bfloat16)
    xd, wd, bd, dyd = x.to(DEV), w.to(DEV), b.to(DEV), dy.to(DEV)
    lib.vit_gemm_variant(variant)
    try:
        ref = x.float() @ w.float().T + b
        dact, act = ops.linear_fwd(xd, wd, bd, epi=L.EPI_BIAS_GELU)
        _close(act, torch.nn.functional.gelu(ref), 1e-2, "gelu")
        _close(dact, _gelu_grad(ref), 1e-2, "gelu'")
        out = res.to(DEV).clone()
        ops.linear_fwd(xd, wd, bd, epi=L.EPI_RESID, resid=out, out=out)
        _close(out, ref + res, 1e-5, "resid")
        _close(ops.linear_dgrad(dyd, wd), dy.float() @ w.float(), 1e-5, "dgrad")
        for split in (1, 3):
            _close(ops.linear_wgrad(dyd, xd, split=split), dy.float().T @ x.float(), 2e-5, f"wgrad split {split}")
    finally:
        lib.vit_gemm_variant(-1)


_FORM_SENTINEL = -512.0


def _run_epilogue_forms(M, N, K, seed0):
    """Every bf16 epilogue of an [M, N] output over K products into sentinel-padded [M + 3, N + 8]
    buffers: {name: (C, aux_out or None)}."""
    x = _rnd(M, K, seed=seed0, dtype=torch.bfloat16).to(DEV)
    w = _rnd(N, K, seed=seed0 + 1, scale=K ** -0.5, dtype=torch.bfloat16).to(DEV)   # forward weight [N, K]
    wt = _rnd(K, N, seed=seed0 + 2, scale=K ** -0.5, dtype=torch.bfloat16).to(DEV)  # dgrad weight: dX = dY wt
    b = _rnd(N, seed=seed0 + 3, scale=0.5).to(DEV)
    dactp = torch.zeros(M + 3, N + 8, dtype=torch.bfloat16, device=DEV)             # a saved act', ld = N + 8
    dactp[:M, :N] = _gelu_grad(_rnd(M, N, seed=seed0 + 4)).to(torch.bfloat16).to(DEV)
    s = L.stream_ptr(x.device)

    def buf():
        return torch.full((M + 3, N + 8), _FORM_SENTINEL, dtype=torch.bfloat16, device=DEV)

    out = {}
    for name, epi, bias, two in (("store", L.EPI_STORE, None, False), ("store+bias", L.EPI_STORE, b, False),
                                 ("gelu pair", L.EPI_BIAS_GELU, b, True), ("qgelu pair", L.EPI_BIAS_QGELU, b, True),
                                 ("gelu act", L.EPI_BIAS_GELU_FWD, b, False),
                                 ("qgelu act", L.EPI_BIAS_QGELU_FWD, b, False)):
        c, aux = buf(), (buf() if two else None)
        L.call("vit_linear_fwd", L.BF16, L.BF16, epi, M, N, K, L.ptr(x), x.stride(0), L.ptr(w), L.ptr(bias), L.ptr(c),
               c.stride(0), None, L.ptr(aux), s)
        out[name] = (c, aux)
    c = buf()
    L.call("vit_linear_dgrad", L.BF16, L.BF16, L.EPI_GELU_BWD, M, K, N, L.ptr(x), x.stride(0), L.ptr(wt), L.ptr(c),
           c.stride(0), L.ptr(dactp), None, None, 0, 0, s)
    out["gelu' dgrad"] = (c, None)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("N", [160, 136])
@pytest.mark.parametrize("variant", [1, 2, 3, 5, 6, 7])
def test_gemm_bf16_epilogue_forms_agree_bitwise(variant, N):
    """The bf16 epilogue forms of big::gemm_tile -- MFMA-fragment stores, permlane16 fragment pairs, the f32
    band staging and the bf16 tile image -- all apply the one epilogue definition (epi_vec and its
    per-element core epi_act_pair), so within a tile configuration they write the same bits.  Each form is forced by
    its timing bit (vit_gemm_variant(v + 100 * bits): 8 fragment, 16 permlane pairs, 64 / 128 band staging,
    256 no bf16 image for the plain store); bits 1, 2 and 4 drop loads / barriers / the epilogue and are
    not used.  M = 300 is ragged in every tile height; N = 160 is a multiple of 32 but of no tile width,
    N = 136 a multiple of 8 only, so the permlane form declines and the fall-through runs; K = 128 is two
    k-steps of the BK = 64 tiles.  Column sums are not compared (their summation order differs by form).
    Measured on the commit before the epilogues were folded together: every pair agreed
    (profiles/r08/epilogue_forms_parent.log)."""
    lib = L.lib()
    M, K = 300, 128
    bits = (0, 8, 16, 64, 128, 256) if variant in (1, 2, 3, 5) else (0, 8)
    bad = []
    try:
        ref = None
        for bit in bits:
            lib.vit_gemm_variant(variant + 100 * bit)
            got = _run_epilogue_forms(M, N, K, seed0=60)
            for name, pair in got.items():
                for which, t in zip(("C", "aux_out"), pair):
                    if t is None:
                        continue
                    what = f"variant {variant} bits {bit} {name} {which}"
                    assert bool((t[:M, N:] == _FORM_SENTINEL).all()) and bool((t[M:] == _FORM_SENTINEL).all()), \
                        what + ": wrote outside its [M, N] output"
                    assert torch.isfinite(t[:M, :N].float()).all(), what
                    assert not bool((t[:M, :N] == _FORM_SENTINEL).any()), what + ": output elements left unwritten"
                    if ref is not None:
                        r = ref[name][0 if which == "C" else 1]
                        ndiff = int((t[:M, :N] != r[:M, :N]).sum())
                        print(f"{what}: {ndiff} elements differ from bits 0")
                        if not torch.equal(t[:M, :N], r[:M, :N]):
                            bad.append(f"{what}: {ndiff} elements")
            if ref is None:
                ref = got
    finally:
        lib.vit_gemm_variant(-1)
    assert not bad, "forms that differ from bits 0: " + "; ".join(bad)


@pytest.mark.parametrize("M,N,K", [(197 * 3, 640, 448), (1024, 768, 96), (300, 132, 64)])
def test_f32_mfma_gemm_every_layout_and_epilogue(M, N, K):
    """The fp32 MFMA kernel (v_mfma_f32_16x16x4_f32; the compute_dtype=float32 path and CLIP at
    the reference's precision): forward with bias / GELU / QuickGELU / residual epilogues, dgrad
    with the GELU' epilogue and fused bias column sums, split-K wgrad with a ragged M tail --
    ragged M / N tiles, against float64 CPU references at 1e-5 of scale."""
    x = _rnd(M, K, seed=60)
    w = _rnd(N, K, seed=61, scale=0.05)
    b = _rnd(N, seed=62)
    res = _rnd(M, N, seed=63)
    dy = _rnd(M, N, seed=64)
    xd, wd, bd, dyd = x.to(DEV), w.to(DEV), b.to(DEV), dy.to(DEV)
    ref = (x.double() @ w.double().T + b.double()).float()
    _close(ops.linear_fwd(xd, wd, bd, out_dtype=torch.float32), ref, 1e-5, "fwd")
    dact, act = ops.linear_fwd(xd, wd, bd, epi=L.EPI_BIAS_GELU, out_dtype=torch.float32)
    _close(act, torch.nn.functional.gelu(ref), 1e-5, "gelu")
    _close(dact, _gelu_grad(ref), 1e-5, "gelu'")
    dq, aq = ops.linear_fwd(xd, wd, bd, epi=L.EPI_BIAS_QGELU, out_dtype=torch.float32)
    sg = torch.sigmoid(1.702 * ref)
    _close(aq, ref * sg, 1e-5, "qgelu")
    out = res.to(DEV).clone()
    ops.linear_fwd(xd, wd, bd, epi=L.EPI_RESID, resid=out, out=out)
    _close(out, ref + res, 1e-5, "resid")
    dref = (dy.double() @ w.double()).float()
    _close(ops.linear_dgrad(dyd, wd, out_dtype=torch.float32), dref, 1e-5, "dgrad")
    pre = _rnd(M, K, seed=65)
    db = torch.empty(K, device=DEV)
    d = ops.linear_dgrad(dyd, wd, out_dtype=torch.float32, epi=L.EPI_GELU_BWD, pre=pre.to(DEV), dbias=db)
    _close(d, dref * pre, 1e-5, "gelu bwd")
    _close(db, (dref.double() * pre.double()).sum(0).float(), 1e-5, "fused dbias")
    wref = (dy.double().T @ x.double()).float()
    for split in (1, 3):
        _close(ops.linear_wgrad(dyd, xd, split=split), wref, 1e-5, f"wgrad split {split}")
    tail = M - 5  # ragged reduction tail (M % 32 != 0) through the generic kernel
    _close(ops.linear_wgrad(dyd[:tail], xd[:tail], split=2), (dy[:tail].double().T @ x[:tail].double()).float(),
           1e-5, "wgrad ragged")


@pytest.mark.parametrize("M,N,K", [(64 * 257, 1024, 256), (64 * 257, 3072, 128), (600 * 16, 1024, 96)])
def test_f32_gemm_streamk_matches_reference(M, N, K):
    """fp32 MFMA GEMM in its stream-K form (C3's ragged 128.5-row-tile shapes: 2*CUs persistent
    workgroups, cut tiles combined in-launch): forward with bias, QuickGELU pair, residual, and the
    input gradient with fused bias sums, against float64 references; the same launch without the
    stream's workspace (one tile per workgroup) agrees to rounding; two stream-K runs are bitwise
    equal."""
    from vit_amd import ops as O
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(M, K, device=DEV, generator=g)
    w = torch.randn(N, K, device=DEV, generator=g) * 0.05
    b = torch.randn(N, device=DEV, generator=g)
    ref = (x.double() @ w.double().T + b.double())
    y1 = O.linear_fwd(x, w, b, out_dtype=torch.float32)
    y2 = O.linear_fwd(x, w, b, out_dtype=torch.float32)
    assert torch.equal(y1, y2)
    _close(y1, ref.float(), 1e-5, "sk fwd")
    dq, aq = O.linear_fwd(x, w, b, epi=L.EPI_BIAS_QGELU)
    s = torch.sigmoid(1.702 * ref)
    _close(aq, (ref * s).float(), 1e-5, "sk qgelu")
    r = torch.randn(M, N, device=DEV, generator=g)
    o = O.linear_fwd(x, w, b, epi=L.EPI_RESID, resid=r)
    _close(o, (ref + r.double()).float(), 1e-5, "sk resid")
    dy = torch.randn(M, N, device=DEV, generator=g)
    db = torch.empty(K, device=DEV)
    dx = O.linear_dgrad(dy, w, out_dtype=torch.float32, dbias=db)
    dref = dy.double() @ w.double()
    _close(dx, dref.float(), 1e-5, "sk dgrad")
    _close(db, dref.sum(0).float(), 1e-5, "sk dgrad bias sums")
    # without the stream's workspace: the plain launch
    st = L.stream_ptr(torch.device(DEV))
    L.lib().vit_gemm_streamk_workspace(st, None, 0, None, 0)
    O._SK.pop(st, None)
    try:
        plain = torch.empty_like(y1)
        L.call("vit_linear_fwd", L.F32, L.F32, L.EPI_STORE, M, N, K, x.data_ptr(), K, w.data_ptr(), b.data_ptr(),
               plain.data_ptr(), N, None, None, st)
        torch.cuda.synchronize()
        _close(plain, y1, 1e-6, "plain vs stream-K")
    finally:
        O._streamk(torch.device(DEV))


def test_gemm_cr_rc_layout_fast():
    # the fourth layout combination (P CR, Q RC) through the raw dispatcher
    M, N, R = 256, 128, 192
    P = _rnd(R, M, seed=13, dtype=torch.bfloat16)   # P(i,r) = P[r][i]
    Q = _rnd(N, R, seed=14, dtype=torch.bfloat16)   # Q(j,r) = Q[j][r]
    C = torch.empty(M, N, dtype=torch.float32, device=DEV)
    Pd, Qd = P.to(DEV), Q.to(DEV)
    L.call("vit_gemm", L.BF16, L.F32, L.LAY_CR, L.LAY_RC, L.EPI_STORE, M, N, R, Pd.data_ptr(), M, Qd.data_ptr(), R,
           C.data_ptr(), N, None, None, 0, None, 1, L.stream_ptr())
    _close(C, P.float().T @ Q.float().T, 1e-5, "cr-rc")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_generic_gemm_odd_shapes(dtype):
    M, N, K = 37, 1000, 70
    x = _rnd(M, K, seed=15, dtype=dtype)
    w = _rnd(N, K, seed=16, scale=0.1, dtype=dtype)
    b = _rnd(N, seed=17)
    y = ops.linear_fwd(x.to(DEV), w.to(DEV), b.to(DEV), out_dtype=torch.float32)
    _close(y, x.float() @ w.float().T + b, 1e-5, "generic fwd")
    dy = _rnd(M, N, seed=18, dtype=dtype)
    _close(ops.linear_dgrad(dy.to(DEV), w.to(DEV)), dy.float() @ w.float(), 1e-5, "generic dgrad")
    _close(ops.linear_wgrad(dy.to(DEV), x.to(DEV)), dy.float().T @ x.float(), 1e-5, "generic wgrad")
    _close(ops.linear_wgrad(dy.to(DEV), x.to(DEV), split=3), dy.float().T @ x.float(), 1e-5, "generic wgrad split")


def test_colreduce_batch_matches_sums_and_is_deterministic():
    """vit_colreduce_batch (one launch for a block's bias / LN-affine reductions): every job against
    a float64 column sum, single-chunk and multi-chunk jobs (in-launch ticket combine), accumulate,
    a non-vector job (N % 4 != 0: two-stage fallback), more than 16 jobs (two launches); two runs
    bitwise equal; the ticket counters are left zero."""
    cases = [(1, 768, 0), (50, 768, 1), (64, 2304, 0), (65, 3072, 0), (788, 3072, 1), (1576, 768, 0),
             (256, 2304, 0), (130, 100, 0), (7, 30, 1)] + [(100 + 37 * i, 768, i % 2) for i in range(10)]
    parts, outs, refs = [], [], []
    for i, (S, N, acc) in enumerate(cases):
        p = _rnd(S, N, seed=200 + i).to(DEV)
        o = _rnd(N, seed=300 + i).to(DEV)
        refs.append(p.double().sum(0) + (o.double() if acc else 0))
        parts.append(p)
        outs.append(o)
    res = []
    for rep in range(2):
        b = ops.ColBatch()
        os_ = [o.clone() for o in outs]
        for p, o, (S, N, acc) in zip(parts, os_, cases):
            b.add(p, S, N, o, accumulate=bool(acc))
        b.launch()
        torch.cuda.synchronize()
        res.append(os_)
    for i, (o1, o2, r) in enumerate(zip(res[0], res[1], refs)):
        _close(o1, r.float(), 1e-5, f"job {i} {cases[i]}")
        assert torch.equal(o1, o2), f"job {i} not reproducible"
    assert int(ops._counters("colbatch", 1, DEV).abs().sum()) == 0


def test_colsum():
    for dtype in (torch.float32, torch.bfloat16):
        x = _rnd(3001, 768, seed=19, dtype=dtype)
        _close(ops.colsum(x.to(DEV)), x.float().sum(0), 1e-5, "colsum")


# ---------------------------------------------------------------------------- patch embed

def test_patch_embed_fwd_and_unfold():
    B, D = 3, 256
    img = _rnd(B, 3, 64, 48, seed=20)
    w = _rnd(D, 3, 16, 16, seed=21, scale=0.02)
    b = _rnd(D, seed=22)
    np_ = (64 // 16) * (48 // 16)
    pos = _rnd(1, np_ + 1, D, seed=23)
    cls = _rnd(1, 1, D, seed=24)
    for dt, rel in ((torch.float32, 1e-5), (torch.bfloat16, 1e-2)):
        U = ops.patch_unfold(img.to(DEV), 16, dt)
        ref_u = img.unfold(2, 16, 16).unfold(3, 16, 16).permute(0, 2, 3, 1, 4, 5).reshape(B * np_, -1)
        assert torch.equal(U.cpu(), ref_u.to(dt))
        x = ops.patch_embed_fwd(U, w.reshape(D, -1).to(dt).to(DEV), b.to(DEV), pos.reshape(-1, D).to(DEV),
                                cls.reshape(-1).to(DEV), B, np_)
        y = torch.nn.functional.conv2d(img, w.to(dt).float(), b, stride=16).flatten(2).transpose(1, 2)
        ref = torch.cat([cls.expand(B, -1, -1), y], 1) + pos
        _close(x, ref, rel if dt == torch.float32 else 2e-3, f"patch {dt}")


def test_patch_embed_padded_reduction_on_mfma_path():
    """CLIP ViT-L/14's patch embedding (ps = 14: 588 columns) with U and the weight zero-padded to
    608 columns (vit_patch_unfold_ld / vit_copy_rows_padded, ABI 7), so the GEMM takes the MFMA
    path: the padded U rows hold the unfolded patch plus exact zeros, and the output matches a
    torch fp32 conv (f32: 1e-5 of scale; bf16 operands: 2e-3).  M = 2 x 256 patches x 2 images."""
    B, D, ps = 2, 1024, 14
    img = _rnd(B, 3, 224, 224, seed=30)
    w = _rnd(D, 3, ps, ps, seed=31, scale=0.02)
    pos = _rnd(1, 257, D, seed=33)
    cls = _rnd(1, 1, D, seed=34)
    np_ = 256
    K, Kp = 3 * ps * ps, 608
    for dt, rel in ((torch.float32, 1e-5), (torch.bfloat16, 2e-3)):
        U = ops.patch_unfold(img.to(DEV), ps, dt, ld=Kp)
        assert U.shape == (B * np_, Kp)
        ref_u = img.unfold(2, ps, ps).unfold(3, ps, ps).permute(0, 2, 3, 1, 4, 5).reshape(B * np_, -1)
        assert torch.equal(U[:, :K].cpu(), ref_u.to(dt))
        assert not U[:, K:].float().abs().any().item()
        wp = ops.pad_cols(w.reshape(D, -1).to(dt).to(DEV), Kp)
        assert torch.equal(wp[:, :K].cpu(), w.reshape(D, -1).to(dt)) and not wp[:, K:].float().abs().any().item()
        x = ops.patch_embed_fwd(U, wp, None, pos.reshape(-1, D).to(DEV), cls.reshape(-1).to(DEV), B, np_)
        y = torch.nn.functional.conv2d(img, w.to(dt).float(), None, stride=ps).flatten(2).transpose(1, 2)
        ref = torch.cat([cls.expand(B, -1, -1), y], 1) + pos
        _close(x, ref, rel, f"padded patch {dt}")


def test_f32_streamk_graph_replay_matches_eager():
    """an f32 GEMM captured on a stream registered before capture (ops.register_capture_stream)
    takes the same stream-K form as the eager launch on that stream, so graph replay and eager agree bit
    for bit (C3's 64 x 257-row shapes: 1032 tiles of 128 x 128 on 512 slots, a ragged last round)."""
    M, N, K = 64 * 257, 1024, 1024
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(M, K, device=DEV, generator=g)
    w = torch.randn(N, K, device=DEV, generator=g) * 0.05
    s = torch.cuda.Stream()
    ops.register_capture_stream(s)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        eager = ops.linear_fwd(x, w, None, out_dtype=torch.float32)
        out = torch.empty_like(eager)
        ops.linear_fwd(x, w, None, out=out)  # warm-up of the captured call's exact arguments
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        ops.linear_fwd(x, w, None, out=out)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    _close(out, (x.double() @ w.double().T).float(), 1e-5, "stream-K replay")


@pytest.mark.parametrize("M,N,R", [(64, 66, 768), (32, 1024, 4096), (1024, 32, 1024), (64, 768, 1024)])
def test_gemm_splitk_matches_reference(M, N, R):
    """vit_gemm_splitk (round 4: DoRA factor gradients, CLIP-HBA head GEMMs): every layout pair against a
    float64 product at 1e-5 of scale, two runs bit-identical (slab sum in a fixed order), and the
    unsplit fallback (no slab room) within the same bound."""
    lib = L.lib()
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(M + N + R)
    slabs = torch.empty(2 * 256 * 1024, device=DEV)
    for pl in (L.LAY_RC, L.LAY_CR):
        for ql in (L.LAY_RC, L.LAY_CR):
            Pm = torch.randn(M, R, generator=g)  # P(i, r)
            Qm = torch.randn(N, R, generator=g)
            Pd = (Pm if pl == L.LAY_RC else Pm.t()).contiguous().to(DEV)
            Qd = (Qm if ql == L.LAY_RC else Qm.t()).contiguous().to(DEV)
            ref = (Pm.double() @ Qm.double().t()).float()
            outs = []
            for room in (slabs.numel(), slabs.numel(), 0):
                c = torch.empty(M, N, device=DEV)
                rc = lib.vit_gemm_splitk(pl, ql, M, N, R, Pd.data_ptr(), Pd.stride(0), Qd.data_ptr(), Qd.stride(0),
                                         c.data_ptr(), slabs.data_ptr() if room else None, room, st)
                assert rc == 0, rc
                torch.cuda.synchronize()
                outs.append(c.cpu())
            _close(outs[0], ref, 1e-5, f"splitk {pl}{ql}")
            _close(outs[2], ref, 1e-5, f"unsplit {pl}{ql}")
            assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("R", [1025, 1100, 2047])
def test_gemm_splitk_slab_room_exact(R):
    """a reduction that is not a multiple of split * 64 with exactly split * M * N floats of slab
    room (M = N = 32: one tile, split min(256, R / 128) = 8).  The kernel must write at most `split` slabs
    (chunks of ceil(R / split) rows), so a guard region right after the room stays untouched."""
    lib = L.lib()
    st = torch.cuda.current_stream().cuda_stream
    M = N = 32
    split = min(256, R // 128)
    room = split * M * N
    g = torch.Generator().manual_seed(R)
    Pm, Qm = torch.randn(M, R, generator=g), torch.randn(N, R, generator=g)
    buf = torch.full((room + 4096,), 12345.0, device=DEV)
    c = torch.empty(M, N, device=DEV)
    Pd, Qd = Pm.to(DEV), Qm.to(DEV)
    rc = lib.vit_gemm_splitk(L.LAY_RC, L.LAY_RC, M, N, R, Pd.data_ptr(), R, Qd.data_ptr(), R, c.data_ptr(),
                             buf.data_ptr(), room, st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert bool((buf[room:] == 12345.0).all()), "split-K slabs overran slab_floats"
    _close(c.cpu(), (Pm.double() @ Qm.double().t()).float(), 1e-5, f"splitk R={R}")


def _g4_pair(x, w, b, dy, variant=-1):
    """(forward + bias, input gradient) through ops with GEMM variant `variant` forced (-1 = default)."""
    lib = L.lib()
    lib.vit_gemm_variant(variant)
    try:
        y = ops.linear_fwd(x, w, b)
        d = ops.linear_dgrad(dy, w, out_dtype=torch.bfloat16)
        torch.cuda.synchronize()
    finally:
        lib.vit_gemm_variant(-1)
    return y, d


@pytest.mark.parametrize("M", [50432, 27580, 22852, 1000])
@pytest.mark.parametrize("N,K", [(2304, 768), (768, 768), (768, 3072), (3072, 768)])
def test_g4_plain_gemms_bitwise_match_8wave_kernels(M, N, K):
    """The plain bf16 forward + f32 bias and input gradient on the 4-wave g4 kernel (csrc/gemm_g4.hip, the
    default since round 6) at the step's shapes -- the full batch and the two forward chains' row counts
    (140 / 116 images) -- against the 8-wave kernels forced (V5 forward, V1 input gradient): the same k order
    (32-deep MFMA chunks in sequence) and the same epilogue arithmetic, so they agree BIT FOR BIT; both
    against an fp64 reference within bf16 output rounding.  The launch counter confirms g4 ran."""
    lib = L.lib()
    bf = torch.bfloat16
    dy = _rnd(M, N, seed=M + N).to(bf).to(DEV)
    x = _rnd(M, K, seed=M + K + 1).to(bf).to(DEV)
    w = (_rnd(N, K, seed=N * K) * 0.05).to(bf).to(DEV)
    b = _rnd(N, seed=7).to(DEV)
    lib.vit_gemm_g4_count(1)
    y4, d4 = _g4_pair(x, w, b, dy)
    assert lib.vit_gemm_g4_count(1) == 2, "the plain GEMMs did not run on g4"
    y5, _ = _g4_pair(x, w, b, dy, variant=5)
    _, d1 = _g4_pair(x, w, b, dy, variant=1)
    assert lib.vit_gemm_g4_count(1) == 0
    assert torch.equal(y4, y5), "g4 forward differs from V5"
    assert torch.equal(d4, d1), "g4 input gradient differs from V1"
    _close(d4, (dy.double() @ w.double()).float(), 8e-3, "g4 dgrad vs fp64")
    _close(y4, (x.double() @ w.double().t() + b.double()).float(), 8e-3, "g4 fwd vs fp64")


@pytest.mark.parametrize("fwd_mode,dgrad_mode,wgs,tpw", [(0, 2, 0, 1), (0, 1, 0, 0), (1, 0, 0, 0), (0, 0, 7, 0),
                                                    (0, 0, 1, 0), (1, 1, 0, 0), (0, 0, 0, 2), (2, 2, 0, 0)])
@pytest.mark.parametrize("M,N,K", [(1, 64, 64), (257, 136, 192), (197 * 3, 640, 448), (2000, 1088, 64),
                                   (513, 256, 3072), (300, 8, 128)])
def test_g4_tile_walks_and_ragged_shapes(fwd_mode, dgrad_mode, wgs, tpw, M, N, K):
    """Every tile walk (stride over G persistent workgroups, G = CUs / 7 / 1 -- one workgroup running every
    tile in sequence -- or ceil(tiles / tpw) workgroups of at most 1 / 2 tiles, or tiles_i workgroups (walk 2, the
    input gradients' default), and the row-band walk) on ragged shapes: M = 1 and 257 (a 1-row last tile), output
    widths 8 / 136 / 448 / 1088 (partial 8-column chunks of the last column tile), a single k-step (K = 64)
    and long reductions; the stage stream crosses tile boundaries with 1..48 k-steps per tile.  The forward
    runs on g4 whenever K % 64 == 0 and N % 8 == 0, the input gradient (reduction N) when N % 64 == 0;
    where g4 ran it is bitwise equal to the 8-wave kernels, and everything is within bf16 rounding of fp64."""
    lib = L.lib()
    bf = torch.bfloat16
    dy = _rnd(M, N, seed=3 * M + N).to(bf).to(DEV)
    x = _rnd(M, K, seed=M + 5 * K).to(bf).to(DEV)
    w = (_rnd(N, K, seed=N + K) * 0.05).to(bf).to(DEV)
    b = _rnd(N, seed=8).to(DEV)
    fwd_g4, dgrad_g4 = K % 64 == 0 and N % 8 == 0, N % 64 == 0 and K % 8 == 0
    lib.vit_gemm_g4_config(fwd_mode, dgrad_mode, wgs, tpw)
    try:
        lib.vit_gemm_g4_count(1)
        y4, d4 = _g4_pair(x, w, b, dy)
        assert lib.vit_gemm_g4_count(1) == int(fwd_g4) + int(dgrad_g4)
    finally:
        lib.vit_gemm_g4_config(0, 2, 0, 1)
    y5, _ = _g4_pair(x, w, b, dy, variant=5)
    _, d1 = _g4_pair(x, w, b, dy, variant=1)
    if fwd_g4:
        assert torch.equal(y4, y5), "g4 forward differs from V5"
    if dgrad_g4:
        assert torch.equal(d4, d1), "g4 input gradient differs from V1"
    _close(y4, (x.double() @ w.double().t() + b.double()).float(), 8e-3, "g4 fwd vs fp64")
    _close(d4, (dy.double() @ w.double()).float(), 8e-3, "g4 dgrad vs fp64")


def _gelu_dgrad(dy, w, pre, variant=-1, g4=1):
    """The GELU' input gradient dy @ w * pre with its fused column sums (the fc1 bias gradient), GEMM
    variant `variant` forced (-1 = default) and the g4 form on / off."""
    lib = L.lib()
    prev = lib.vit_gemm_g4_gelu(g4)
    lib.vit_gemm_variant(variant)
    try:
        db = torch.empty(w.shape[1], device=DEV)
        out = ops.linear_dgrad(dy, w, out_dtype=torch.bfloat16, epi=L.EPI_GELU_BWD, pre=pre, dbias=db)
        torch.cuda.synchronize()
    finally:
        lib.vit_gemm_variant(-1)
        lib.vit_gemm_g4_gelu(prev)
    return out, db


@pytest.mark.parametrize("M,K,N", [(50432, 3072, 768), (1000, 3072, 768), (257, 136, 128), (333, 1088, 192),
                                   (1, 64, 128), (2000, 512, 64)])
def test_g4_gelu_dgrad_matches_v1(M, K, N):
    """The fc2 GELU' input gradient (C = dY W * act', VIT r04 item 3's fused epilogue) on g4 (vit_gemm_g4_gelu:
    the act' tile arrives by LDS-DMA in the two stage slots past the stream's end, the products replace it in
    the LDS image) against the 8-wave V1 kernel forced: the step shape (M = 50432, 3072 columns, reduction
    768), ragged rows / columns and the 2- and 3-k-step reductions.  C agrees BIT FOR BIT (same k order, same
    f32 product, same rounding); the fused column sums (fc1's bias gradient) add the same f32 products in
    another order (V1: its staged rows; g4: a lane's 4 rows, then the 16-lane butterfly), so they are held to
    1e-5 relative of V1 and to fp64.  A one-k-step reduction (N = 64) is not taken by g4 (launch count 0)."""
    lib = L.lib()
    bf = torch.bfloat16
    dy = _rnd(M, N, seed=M + N + 11).to(bf).to(DEV)
    w = (_rnd(N, K, seed=N * K + 3) * 0.05).to(bf).to(DEV)
    pre = (_rnd(M, K, seed=M + K + 5).abs() * 0.6).to(bf).to(DEV)
    lib.vit_gemm_g4_count(1)
    c4, db4 = _gelu_dgrad(dy, w, pre)
    assert lib.vit_gemm_g4_count(1) == (1 if N >= 128 else 0)
    c1, db1 = _gelu_dgrad(dy, w, pre, variant=1, g4=0)
    assert torch.equal(c4, c1), "g4 GELU' input gradient differs from V1"
    ref = (dy.double() @ w.double()) * pre.double()
    _close(c4, ref.float(), 8e-3, "g4 GELU' dgrad vs fp64")
    assert torch.allclose(db4, db1, rtol=1e-5, atol=1e-5 * float(db1.abs().max()) + 1e-30), "column sums vs V1"
    _close(db4, ref.sum(0).float(), 1e-4, "fused column sums vs fp64")


@pytest.mark.parametrize("M,N,K", [(27580, 3072, 768), (22852, 3072, 768), (1000, 3072, 768), (257, 136, 192),
                                   (1, 64, 64), (300, 1088, 128)])
def test_g4_gelu_pair_forward_matches_v5(M, N, K):
    """The fc1 forward with its GELU pair epilogue (C = GELU'(pre), act = GELU(pre), pre = bf16(x W^T + b)) on
    g4 (vit_gemm_g4_gelu bit 1: pre through the LDS image, the pair computed in the row sweep) against the
    8-wave V5 kernel forced, at the two forward chains' row counts and ragged shapes: both outputs BIT FOR BIT
    (same k order, same pre rounding, the same gelu_fast_both), and within bf16 rounding of the exact-erf
    GELU / GELU' of an fp64 pre."""
    lib = L.lib()
    bf = torch.bfloat16
    x = _rnd(M, K, seed=M + K + 21).to(bf).to(DEV)
    w = (_rnd(N, K, seed=N * K + 4) * 0.05).to(bf).to(DEV)
    b = _rnd(N, seed=9).to(DEV)
    prev = lib.vit_gemm_g4_gelu(3)
    try:
        lib.vit_gemm_g4_count(1)
        d4, a4 = ops.linear_fwd(x, w, b, epi=L.EPI_BIAS_GELU)
        torch.cuda.synchronize()
        assert lib.vit_gemm_g4_count(1) == 1, "the GELU pair did not run on g4"
        lib.vit_gemm_variant(5)
        d5, a5 = ops.linear_fwd(x, w, b, epi=L.EPI_BIAS_GELU)
        torch.cuda.synchronize()
    finally:
        lib.vit_gemm_variant(-1)
        lib.vit_gemm_g4_gelu(prev)
    assert torch.equal(d4, d5), "g4 GELU' (C) differs from V5"
    assert torch.equal(a4, a5), "g4 GELU (act) differs from V5"
    pre = (x.double() @ w.double().t() + b.double()).to(bf).double()
    _close(a4, torch.nn.functional.gelu(pre).float(), 8e-3, "act vs fp64 erf GELU")
    _close(d4, _gelu_grad(pre).float(), 8e-3, "GELU' vs fp64")


# ---------------------------------------------------------------------------- LayerNorm

@pytest.mark.parametrize("D", [768, 1024, 64, 200])
@pytest.mark.parametrize("xdt", [torch.float32, torch.bfloat16])
def test_layer_norm_fwd_bwd(D, xdt):
    M = 333
    x = _rnd(M, D, seed=25, scale=2.0).to(xdt)
    w = 1 + _rnd(D, seed=26, scale=0.2)
    b = _rnd(D, seed=27, scale=0.1)
    dy = _rnd(M, D, seed=28)
    dres = _rnd(M, D, seed=29)
    xr = x.float().requires_grad_(True)
    wr, br = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    yr = torch.nn.functional.layer_norm(xr, (D,), wr, br, 1e-6)
    yr.backward(dy)
    for ydt in (torch.float32, torch.bfloat16):
        y, mean, rstd = ops.layer_norm_fwd(x.to(DEV), w.to(DEV), b.to(DEV), 1e-6, ydt)
        _close(y, yr, 1e-5 if ydt == torch.float32 else 8e-3, "ln fwd")
    y, mean, rstd = ops.layer_norm_fwd(x.to(DEV), w.to(DEV), b.to(DEV), 1e-6, torch.float32)
    dx = torch.empty(M, D, device=DEV)
    copy = torch.empty(M, D, dtype=torch.bfloat16, device=DEV)
    dg = torch.empty(D, device=DEV)
    db = torch.empty(D, device=DEV)
    ds = torch.empty(D, device=DEV)
    ops.layer_norm_bwd(x.to(DEV), D, dy.to(DEV), w.to(DEV), mean, rstd, dx, D, M, dres=dres.to(DEV), ldres=D,
                       dx_copy=copy, ld_copy=D, dgamma=dg, dbeta=db, dsum=ds)
    _close(dx, xr.grad + dres, 1e-5, "ln dx")
    _close(ds, (xr.grad + dres).sum(0), 1e-5, "ln dsum")
    _close(copy, xr.grad + dres, 8e-3, "ln dx copy")
    _close(dg, wr.grad, 1e-5, "dgamma")
    _close(db, br.grad, 1e-5, "dbeta")


@pytest.mark.parametrize("D", [768, 1024, 1280, 1792])
def test_add_layer_norm_fwd(D):
    """xs = x + r (f32 + bf16), y = LayerNorm(xs) in bf16, mean/rstd; in place (xs is x) and add-only."""
    M = 333
    x = _rnd(M, D, seed=30, scale=2.0)
    r = _rnd(M, D, seed=31).to(torch.bfloat16)
    w = 1 + _rnd(D, seed=32, scale=0.2)
    b = _rnd(D, seed=33, scale=0.1)
    s = x + r.float()
    yr = torch.nn.functional.layer_norm(s, (D,), w, b, 1e-6)
    xs = torch.empty(M, D, device=DEV)
    y = torch.empty(M, D, dtype=torch.bfloat16, device=DEV)
    mean, rstd = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    ops.add_layer_norm_fwd(x.to(DEV), r.to(DEV), xs, w.to(DEV), b.to(DEV), 1e-6, out=y, mean=mean, rstd=rstd)
    _close(xs, s, 0, "sum")  # one f32 add: exact
    _close(y, yr, 8e-3, "ln")
    _close(mean, s.mean(1), 1e-5, "mean")
    _close(rstd, 1 / (s.var(1, unbiased=False) + 1e-6).sqrt(), 1e-5, "rstd")
    xi = x.to(DEV)
    ops.add_layer_norm_fwd(xi, r.to(DEV), xi)  # add only, in place
    _close(xi, s, 0, "in-place add")
    # f32 branch output and f32 LayerNorm output (the fp32 compute path)
    rf = r.float() + _rnd(M, D, seed=34, scale=1e-3)
    sf = x + rf
    yf = torch.empty(M, D, device=DEV)
    ops.add_layer_norm_fwd(x.to(DEV), rf.to(DEV), xs, w.to(DEV), b.to(DEV), 1e-6, out=yf, mean=mean, rstd=rstd)
    _close(xs, sf, 0, "f32 sum")
    _close(yf, torch.nn.functional.layer_norm(sf, (D,), w, b, 1e-6), 1e-5, "f32 ln")


@pytest.mark.parametrize("dyt", [torch.bfloat16, torch.float32])
def test_layer_norm_bwd_pipelined_matches_plain(dyt):
    """The software-pipelined backward (two row buffers per wave) against the plain row loop:
    dx, bf16 copy and dgamma / dbeta / dsum to rounding at the step's row count per workgroup,
    with ragged workgroups (rows not a multiple of 4 or of the rows per workgroup)."""
    M, D = 4097, 768
    x = _rnd(M, D, seed=40, scale=2.0).to(DEV)
    w = (1 + _rnd(D, seed=41, scale=0.2)).to(DEV)
    b = _rnd(D, seed=42, scale=0.1).to(DEV)
    dy = _rnd(M, D, seed=43).to(DEV).to(dyt)
    dres = _rnd(M, D, seed=44).to(DEV)
    _, mean, rstd = ops.layer_norm_fwd(x, w, b, 1e-6, torch.float32)
    outs = []
    try:
        for v in (0, 1):
            L.lib().vit_layer_norm_bwd_variant(v)
            dx = torch.empty(M, D, device=DEV)
            cp = torch.empty(M, D, dtype=torch.bfloat16, device=DEV)
            dg, db, ds = (torch.empty(D, device=DEV) for _ in range(3))
            ops.layer_norm_bwd(x, D, dy, w, mean, rstd, dx, D, M, dres=dres, ldres=D, dx_copy=cp, ld_copy=D,
                               dgamma=dg, dbeta=db, dsum=ds)
            torch.cuda.synchronize()
            outs.append((dx, cp, dg, db, ds))
    finally:
        L.lib().vit_layer_norm_bwd_variant(1)
    for a, c, nm in zip(*outs, ("dx", "copy", "dgamma", "dbeta", "dsum")):
        _close(c, a, 1e-6 if nm != "copy" else 8e-3, nm)  # same arithmetic; FMA contraction may differ
    xr = x.float().requires_grad_(True)
    torch.nn.functional.layer_norm(xr, (D,), w, b, 1e-6).backward(dy.float())
    _close(outs[1][0], xr.grad + dres, 1e-5, "ln dx")


def test_layer_norm_bwd_compact_rows():
    B, S, D = 3, 5, 768
    x = _rnd(B * S, D, seed=30)
    w, b = 1 + _rnd(D, seed=31, scale=0.1), _rnd(D, seed=32, scale=0.1)
    dy = _rnd(B * S, D, seed=33)
    y, mean, rstd = ops.layer_norm_fwd(x.to(DEV), w.to(DEV), b.to(DEV), 1e-6, torch.float32)
    dx = torch.empty(B * S, D, device=DEV)
    copy = torch.full((B * (S - 1), D), 7.0, dtype=torch.bfloat16, device=DEV)
    ops.layer_norm_bwd(x.to(DEV), D, dy.to(DEV), w.to(DEV), mean, rstd, dx, D, B * S, dx_copy=copy, ld_copy=D,
                       compact_np=S - 1)
    want = dx.cpu().reshape(B, S, D)[:, 1:].reshape(-1, D)
    _close(copy, want, 8e-3, "compact")


# ---------------------------------------------------------------------------- attention

def _sdpa_ref(qkv, B, H, N):
    D = H * 64
    q, k, v = qkv.float().reshape(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    q, k, v = [t.clone().requires_grad_(True) for t in (q, k, v)]
    s = (q @ k.transpose(-2, -1)) * 0.125
    lse = torch.logsumexp(s, -1)
    o = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B * N, D)
    return o, lse.reshape(-1), (q, k, v)


# bf16 backward: one fused kernel for N <= 224 (16 .. 224 cover 1 .. 14 waves, odd and even tile
# counts), the two-kernel form above (225, 257)
@pytest.mark.parametrize("N", [197, 50, 257, 16, 224, 208, 33, 225])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_sdpa_fwd_bwd(N, dtype):
    B, H = 2, 3
    D = H * 64
    qkv = _rnd(B * N, 3 * D, seed=34, scale=1.5).to(dtype)
    do = _rnd(B * N, D, seed=35).to(dtype)
    o_ref, lse_ref, (q, k, v) = _sdpa_ref(qkv, B, H, N)
    o_ref.backward(do.float())
    dq = q.grad.transpose(1, 2).reshape(B * N, D)
    dk = k.grad.transpose(1, 2).reshape(B * N, D)
    dv = v.grad.transpose(1, 2).reshape(B * N, D)
    o, lse = ops.sdpa_fwd(qkv.to(DEV), B, H, N)
    rel = 1e-5 if dtype == torch.float32 else 1.5e-2
    _close(o, o_ref, rel, "o")
    _close(lse, lse_ref, 1e-5 if dtype == torch.float32 else 2e-3, "lse")
    # backward from the reference forward's o so only the bwd kernel is tested
    dbias = torch.empty(3 * D, device=DEV)
    dqkv = ops.sdpa_bwd(qkv.to(DEV), o_ref.detach().to(dtype).to(DEV), do.to(DEV), lse_ref.to(DEV), B, H, N,
                        dbias=dbias)
    g = dqkv.float().cpu()
    _close(dbias, torch.cat([dq, dk, dv], 1).sum(0), 1e-4 if dtype == torch.float32 else 3e-2, "qkv bias grad")
    rel = 1e-4 if dtype == torch.float32 else 3e-2
    _close(g[:, :D], dq, rel, "dq")
    _close(g[:, D:2 * D], dk, rel, "dk")
    _close(g[:, 2 * D:], dv, rel, "dv")


# the fused bf16 backward at step-sized grids (B*H = 1024 .. 1555 workgroups, causal and padded
# key tiles), every (b, h) item checked on its own against torch fp32 autograd
@pytest.mark.parametrize("B,H,N,causal", [(91, 12, 197, False), (311, 5, 197, False), (311, 5, 224, True),
                                          (256, 4, 130, False)])
def test_sdpa_bwd_large_grid(B, H, N, causal):
    D = H * 64
    g = torch.Generator(device=DEV).manual_seed(36)
    qkv = (torch.randn(B * N, 3 * D, device=DEV, generator=g) * 1.5).to(torch.bfloat16)
    do = torch.randn(B * N, D, device=DEV, generator=g).to(torch.bfloat16)
    q, k, v = qkv.float().reshape(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    q, k, v = [t.clone().requires_grad_(True) for t in (q, k, v)]
    s = (q @ k.transpose(-2, -1)) * 0.125
    if causal:
        s = s + torch.full((N, N), float("-inf"), device=DEV).triu_(1)
    lse = torch.logsumexp(s, -1).reshape(-1)
    o_ref = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B * N, D)
    o_ref.backward(do.float())
    dbias = torch.empty(3 * D, device=DEV)
    dqkv = ops.sdpa_bwd(qkv, o_ref.detach().to(torch.bfloat16), do, lse.detach(), B, H, N, dbias=dbias,
                        causal=causal)
    ref = torch.cat([t.grad.transpose(1, 2).reshape(B * N, D) for t in (q, k, v)], 1)
    _close(dqkv.float(), ref, 3e-2, "dqkv")
    _close(dbias, ref.sum(0), 3e-2, "qkv bias grad")
    # every head's rows, not just the global norm: the worst head's relative error
    err = (dqkv.float() - ref).reshape(B, N, 3, H, 64).permute(0, 3, 2, 1, 4).reshape(B * H, -1)
    scl = ref.reshape(B, N, 3, H, 64).permute(0, 3, 2, 1, 4).reshape(B * H, -1)
    worst = (err.norm(dim=1) / scl.norm(dim=1).clamp_min(1e-6)).max().item()
    assert worst < 3e-2, f"worst (b, h) item rel err {worst}"


@pytest.mark.parametrize("N,causal", [(113, False), (150, False), (197, False), (224, False), (197, True),
                                      (224, True)])
def test_sdpa_bwd_fused_matches_two_kernel(N, causal):
    """The whole-head fused backward (the default for N <= 224) against the two-kernel form (dq kernel +
    dk/dv kernel, the N > 224 path): dq / dk / dv agree to bf16 rounding (the forms order some f32
    sums differently: up to one bf16 ulp apart), delta to fp32 rounding, the qkv-bias column sums within
    2e-4 of scale (summed from differently rounded partials); B*H = 300 workgroups."""
    B, H = 25, 12
    D = H * 64
    g = torch.Generator(device=DEV).manual_seed(37)
    qkv = (torch.randn(B * N, 3 * D, device=DEV, generator=g) * 1.5).to(torch.bfloat16)
    do = torch.randn(B * N, D, device=DEV, generator=g).to(torch.bfloat16)
    o, lse = ops.sdpa_fwd(qkv, B, H, N, causal=causal)
    lib = L.lib()
    outs = []
    try:
        assert lib.vit_sdpa_bwd_variant(0) != 0  # the banded form is gone (ABI 8)
        for v in (1, 2):
            assert lib.vit_sdpa_bwd_variant(v) == 0
            dbias = torch.empty(3 * D, device=DEV)
            dqkv = ops.sdpa_bwd(qkv, o, do, lse, B, H, N, dbias=dbias, causal=causal)
            delta = ops.workspace("sdpa_delta", B * H * N * 4, qkv.device).view(torch.float32)[:B * H * N].clone()
            torch.cuda.synchronize()
            outs.append((dqkv.clone(), dbias.clone(), delta))
    finally:
        lib.vit_sdpa_bwd_variant(-1)
    (d0, b0, l0), (d1, b1, l1) = outs
    _close(d1, d0, 8e-3, "dqkv (two-kernel vs fused)")
    _close(l1, l0, 1e-6, "delta")
    _close(b1, b0, 2e-4, "qkv bias grad (two-kernel vs fused)")


@pytest.mark.parametrize("N", [77, 16, 197, 224])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_sdpa_causal_fwd_bwd(N, dtype):
    """Causal mask (CLIP text tower attn_mask: -inf above the diagonal) vs a torch fp32 reference."""
    B, H = 3, 2
    D = H * 64
    qkv = _rnd(B * N, 3 * D, seed=44, scale=1.5).to(dtype)
    do = _rnd(B * N, D, seed=45).to(dtype)
    q, k, v = qkv.float().reshape(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    q, k, v = [t.clone().requires_grad_(True) for t in (q, k, v)]
    s = (q @ k.transpose(-2, -1)) * 0.125 + torch.full((N, N), float("-inf")).triu_(1)
    lse_ref = torch.logsumexp(s, -1).reshape(-1)
    o_ref = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B * N, D)
    o_ref.backward(do.float())
    o, lse = ops.sdpa_fwd(qkv.to(DEV), B, H, N, causal=True)
    _close(o, o_ref, 1e-5 if dtype == torch.float32 else 1.5e-2, "o")
    _close(lse, lse_ref, 1e-5 if dtype == torch.float32 else 2e-3, "lse")
    dqkv = ops.sdpa_bwd(qkv.to(DEV), o_ref.detach().to(dtype).to(DEV), do.to(DEV), lse_ref.detach().to(DEV), B, H, N,
                        causal=True)
    g = dqkv.float().cpu()
    rel = 1e-4 if dtype == torch.float32 else 3e-2
    for i, (name, ref) in enumerate((("dq", q.grad), ("dk", k.grad), ("dv", v.grad))):
        _close(g[:, i * D:(i + 1) * D], ref.transpose(1, 2).reshape(B * N, D), rel, name)


def test_clip_small_kernels():
    """token embedding, row gather/scatter, feature rownorm fwd/bwd, MSE fwd/bwd vs torch fp32."""
    g = torch.Generator().manual_seed(50)
    S, Lq, D, V = 5, 16, 128, 64
    tok = torch.randint(0, V, (S, Lq), generator=g)
    table, pos = torch.randn(V, D, generator=g), torch.randn(Lq, D, generator=g)
    x = ops.token_embed(tok.to(DEV), table.to(DEV), pos.to(DEV))
    _close(x, (table[tok] + pos).reshape(S * Lq, D), 1e-6, "token_embed")
    idx = torch.tensor([3, 17, 40, 79], dtype=torch.int64)
    xg = ops.gather_rows(x, idx.to(DEV))
    _close(xg, x.cpu()[idx], 0, "gather")
    dst = ops.zero_(torch.empty(S * Lq, D, device=DEV))
    ops.scatter_rows(xg, idx.to(DEV), dst)
    ref = torch.zeros(S * Lq, D)
    ref[idx] = x.cpu()[idx]
    _close(dst, ref, 0, "scatter")
    f = torch.randn(7, 96, generator=g).requires_grad_(True)
    ls = torch.tensor([2.3])
    y_ref = ls.exp() * f / f.norm(dim=1, keepdim=True)
    dy = torch.randn(7, 96, generator=g)
    y_ref.backward(dy)
    y, rn = ops.rownorm_fwd(f.detach().to(DEV), ls.to(DEV))
    _close(y, y_ref, 1e-5, "rownorm")
    _close(ops.rownorm_bwd(f.detach().to(DEV), dy.to(DEV), rn, ls.to(DEV)), f.grad, 1e-5, "rownorm bwd")
    p = torch.randn(64, 66, generator=g).requires_grad_(True)
    t = torch.randn(64, 66, generator=g)
    l_ref = torch.nn.functional.mse_loss(p, t)
    l_ref.backward(torch.tensor(0.7))
    _close(ops.mse_fwd(p.detach().to(DEV), t.to(DEV)).reshape(1), l_ref.detach().reshape(1), 1e-6, "mse")
    _close(ops.mse_bwd(p.detach().to(DEV), t.to(DEV), torch.tensor(0.7, device=DEV)), p.grad, 1e-6, "mse bwd")


# ---------------------------------------------------------------------------- CE / SGD / misc

def test_cross_entropy():
    B, C = 37, 1000
    logits = _rnd(B, C, seed=36, scale=3.0)
    tgt = torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(37))
    lr_ = logits.clone().requires_grad_(True)
    loss_ref = torch.nn.functional.cross_entropy(lr_, tgt)
    loss_ref.backward(torch.tensor(0.5))
    loss, row_lse = ops.cross_entropy_fwd(logits.to(DEV), tgt.to(DEV))
    assert abs(loss.item() - loss_ref.item()) < 1e-5 * abs(loss_ref.item())
    d = ops.cross_entropy_bwd(logits.to(DEV), tgt.to(DEV), row_lse, torch.tensor(0.5, device=DEV))
    _close(d, lr_.grad, 1e-5, "dlogits")


def test_fused_sgd_matches_torch_sgd_and_writes_shadow():
    from vit_amd.optim import FusedSGD
    torch.manual_seed(0)
    shapes = [(768, 768), (1000,), (3, 5), (4097,)]
    ps = [torch.nn.Parameter(torch.randn(s)) for s in shapes]
    qs = [torch.nn.Parameter(p.detach().clone().to(DEV)) for p in ps]
    for q in qs[:2]:
        q._vit_shadow = torch.empty(q.shape, dtype=torch.bfloat16, device=DEV)
    ref = torch.optim.SGD(ps, lr=0.1, momentum=0.9, weight_decay=1e-4)
    opt = FusedSGD(qs, lr=0.1, momentum=0.9, weight_decay=1e-4)
    for step in range(3):
        for p, q in zip(ps, qs):
            g = torch.randn(p.shape)
            p.grad = g.clone()
            q.grad = g.to(DEV)
        ref.step()
        opt.step()
        for p, q in zip(ps, qs):
            _close(q, p, 1e-6, "sgd")
    for q in qs[:2]:
        assert torch.equal(q._vit_shadow.cpu(), q.detach().cpu().to(torch.bfloat16))


def test_fused_adamw_matches_torch():
    from vit_amd.optim import FusedAdamW
    torch.manual_seed(1)
    ps = [torch.nn.Parameter(torch.randn(s)) for s in [(32, 1024), (1024,), (7,)]]
    qs = [torch.nn.Parameter(p.detach().clone().to(DEV)) for p in ps]
    ref = torch.optim.AdamW(ps, lr=3e-4, weight_decay=0.01)
    opt = FusedAdamW(qs, lr=3e-4, weight_decay=0.01)
    for step in range(4):
        for p, q in zip(ps, qs):
            g = torch.randn(p.shape)
            p.grad = g.clone()
            q.grad = g.to(DEV)
        ref.step()
        opt.step()
    for p, q in zip(ps, qs):
        _close(q, p, 1e-6, "adamw")


def test_fused_adamw_table_is_static_and_graph_replay_matches_torch():
    """The AdamW tensor table holds pointers and sizes only (its key does not change from step to
    step: ADVICE r02); a captured step() replayed after prepare_replay() follows torch.AdamW, also
    when the lr changes between replays (an lr schedule: the decoupled decay 1 - lr * wd must follow
    it as the step size does -- ADVICE r03; wd = 0.5 makes a stale decay visible at 1e-6)."""
    from vit_amd.optim import FusedAdamW
    torch.manual_seed(3)
    shapes = [(48, 512), (512,), (3,)]
    ps = [torch.nn.Parameter(torch.randn(s)) for s in shapes]
    qs = [torch.nn.Parameter(p.detach().clone().to(DEV)) for p in ps]
    gdev = [torch.zeros(s, device=DEV) for s in shapes]
    for q, g in zip(qs, gdev):
        q.grad = g
    ref = torch.optim.AdamW(ps, lr=3e-4, weight_decay=0.5)
    opt = FusedAdamW(qs, lr=3e-4, weight_decay=0.5)
    grads = [[torch.randn(s) for s in shapes] for _ in range(6)]

    def feed(gs):
        for p, g, gd in zip(ps, gs, gdev):
            p.grad = g.clone()
            gd.copy_(g)

    feed(grads[0])
    ref.step()
    opt.step()  # eager: builds the table
    key = opt._mt[0]._key
    feed(grads[1])
    ref.step()
    opt.step()
    assert opt._mt[0]._key == key  # same table on the next step
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            opt.step()
    torch.cuda.current_stream().wait_stream(s)
    for i, gs in enumerate(grads[2:]):
        for o in (ref, opt):
            o.param_groups[0]["lr"] = 3e-4 * (1 + 10 * i)  # 3e-4, 3.3e-3, 6.3e-3, 9.3e-3
        feed(gs)
        ref.step()
        opt.prepare_replay()
        graph.replay()
    torch.cuda.synchronize()
    for p, q in zip(ps, qs):
        _close(q, p, 1e-6, "adamw graph replay")
    assert all(float(opt.state[q]["step"]) == 6.0 for q in qs)


def test_fused_adamw_resume_continues_bias_correction():
    """The sweep resume (NEWP:1189-1195: optimizer.load_state_dict of the saved state) must
    continue each tensor's bias correction from its saved step, as torch.optim.AdamW does:
    k steps, state_dict, a fresh optimizer loads it, more steps -- against torch doing the same."""
    from vit_amd.optim import FusedAdamW
    torch.manual_seed(2)
    shapes = [(64, 96), (96,), (5,)]
    ps = [torch.nn.Parameter(torch.randn(s)) for s in shapes]
    qs = [torch.nn.Parameter(p.detach().clone().to(DEV)) for p in ps]
    q_shadow = qs[0]
    q_shadow._vit_shadow = torch.empty(q_shadow.shape, dtype=torch.bfloat16, device=DEV)
    ref = torch.optim.AdamW(ps, lr=3e-4, weight_decay=0.01)
    opt = FusedAdamW(qs, lr=3e-4, weight_decay=0.01)
    grads = [[torch.randn(s) for s in shapes] for _ in range(9)]

    def run(ref, opt, steps):
        for gs in steps:
            for p, q, g in zip(ps, qs, gs):
                p.grad = g.clone()
                q.grad = g.to(DEV)
            ref.step()
            opt.step()

    run(ref, opt, grads[:5])
    sd_ref, sd = ref.state_dict(), opt.state_dict()
    assert [float(s["step"]) for s in sd["state"].values()] == [5.0] * 3
    ref2 = torch.optim.AdamW(ps, lr=3e-4, weight_decay=0.01)
    ref2.load_state_dict(sd_ref)
    opt2 = FusedAdamW(qs, lr=3e-4, weight_decay=0.01)
    # the state as a checkpoint holds it: CPU tensors (torch.save -> torch.load map_location cpu)
    sd_cpu = {"state": {k: {n: t.cpu() for n, t in v.items()} for k, v in sd["state"].items()},
              "param_groups": sd["param_groups"]}
    opt2.load_state_dict(sd_cpu)
    run(ref2, opt2, grads[5:])
    for p, q in zip(ps, qs):
        _close(q, p, 1e-6, "adamw resumed")
    assert all(float(opt2.state[q]["step"]) == 9.0 for q in qs)
    # the bf16 GEMM shadow was rewritten in the same pass and is marked fresh
    assert torch.equal(q_shadow._vit_shadow.cpu(), q_shadow.detach().cpu().to(torch.bfloat16))
    assert q_shadow._vit_shadow_version == q_shadow._version


def test_fused_adamw_update_reaches_bf16_forward():
    """A ViT in bf16 trained by FusedAdamW: the next forward must use the updated weights
    (the shadow the GEMMs read is refreshed), i.e. equal a fresh model loaded with them."""
    import vit_amd
    from oracle import vit_ref as R
    cfg = R.ViTConfig(img_size=32, patch_size=16, embed_dim=128, depth=2, num_heads=2, num_classes=10)
    p = R.init_params(cfg, seed=4, random_affine=True)
    kw = dict(img_size=32, patch_size=16, embed_dim=128, depth=2, num_heads=2, num_classes=10,
              compute_dtype=torch.bfloat16)
    m = vit_amd.VisionTransformer(**kw)
    m.load_state_dict(p)
    m = m.to(DEV)
    x = torch.randn(4, 3, 32, 32, generator=torch.Generator().manual_seed(5)).to(DEV)
    y = torch.tensor([1, 2, 3, 4], device=DEV)
    opt = vit_amd.FusedAdamW(m.parameters(), lr=1e-2)
    vit_amd.cross_entropy(m(x), y).backward()
    opt.step()
    with torch.no_grad():
        after = m(x)
    m2 = vit_amd.VisionTransformer(**kw)
    m2.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()})
    m2 = m2.to(DEV)
    with torch.no_grad():
        fresh = m2(x)
    assert torch.equal(after, fresh)


def test_dora_forward_train_dropout_matches_reference_fixture(golden_dir):
    """DoRALayer.forward in train mode (NEWP:465-481: dropout on delta_D, then F.linear) on the HIP
    kernels with the reference's recorded dropout noise: output and every gradient (x, m, A, B,
    bias) against the reference class run on CPU (dora_forward_golden.pt, make_golden.py)."""
    import vit_amd
    from vit_amd.dora import _LinearF32Fn
    fx = torch.load(os.path.join(golden_dir, "dora_forward_golden.pt"), weights_only=True)
    m = fx["m"].clone().to(DEV).requires_grad_(True)
    A = fx["A"].clone().to(DEV).requires_grad_(True)
    Bm = fx["B"].clone().to(DEV).requires_grad_(True)
    b = fx["bias"].clone().to(DEV).requires_grad_(True)
    x = fx["x"].clone().to(DEV).requires_grad_(True)
    W = vit_amd.dora_weight(m, A, Bm, fx["D"].to(DEV), fx["scaling"], fx["noise"].to(DEV))
    y = _LinearF32Fn.apply(x, W, b)
    _close(y, fx["y"], 1e-5, "y")
    y.backward(fx["gy"].to(DEV))
    for t, k in ((x, "dx"), (m, "dm"), (A, "dA"), (Bm, "dB"), (b, "dbias")):
        _close(t.grad, fx[k], 1e-4, k)


def test_dora_layer_forward_train_mode_draws_the_reference_mask():
    """The module path: DoRALayer.forward in train mode on the GPU draws its dropout with the
    same RNG consumption as the reference's ``self.dora_dropout(delta_D)`` (same shape, device and
    generator state), so re-seeding and running the reference's forward in torch on the GPU gives
    the same output; eval mode (and p = 0) is ``F.linear(x, weight, bias)``."""
    import vit_amd
    torch.manual_seed(5)
    base = torch.nn.Linear(64, 48)
    layer = vit_amd.DoRALayer(base, r=4, dora_alpha=16, dora_dropout=0.1).to(DEV).train()
    x = torch.randn(7, 64, device=DEV)
    torch.cuda.manual_seed(9)
    y = layer(x)
    torch.cuda.manual_seed(9)
    with torch.no_grad():
        dD = layer.dora_dropout((layer.delta_D_B @ layer.delta_D_A) * layer.scaling)
        Dn = layer.D + dD
        Wr = (Dn / (torch.norm(Dn, dim=0, keepdim=True) + 1e-8) * layer.m).T
        yr = torch.nn.functional.linear(x, Wr, layer.bias)
    _close(y, yr, 1e-5, "train forward")
    layer.eval()
    with torch.no_grad():
        _close(layer(x), torch.nn.functional.linear(x, layer.weight, layer.bias), 1e-5, "eval forward")


def test_dora_weight_matches_reference_fixture(golden_dir):
    import vit_amd
    fx = torch.load(os.path.join(golden_dir, "dora_golden.pt"), weights_only=True)
    rec = fx["96x80r8"]
    m = rec["m"].clone().to(DEV).requires_grad_(True)
    A = rec["A"].clone().to(DEV).requires_grad_(True)
    Bm = rec["B"].clone().to(DEV).requires_grad_(True)
    W = vit_amd.dora_weight(m, A, Bm, rec["D"].to(DEV), rec["scaling"])
    _close(W, rec["W"], 1e-5, "dora W")
    W.backward(rec["gW"].to(DEV))
    _close(m.grad, rec["dm"], 1e-4, "dm")
    _close(A.grad, rec["dA"], 1e-4, "dA")
    _close(Bm.grad, rec["dB"], 1e-4, "dB")
    # full-size layers: regenerate inputs from the recorded seed, compare summaries
    from oracle import vit_ref as R
    for key in ("1024x1024r32", "768x768r32"):
        r = fx[key]
        torch.manual_seed(r["seed"])
        base = torch.nn.Linear(r["in"], r["out"])
        layer = vit_amd.DoRALayer(base, r=r["r"], dora_alpha=16)
        layer = layer.to(DEV)
        W = layer.weight
        assert abs(W.double().sum().item() - r["W_sum"]) < 1e-4 * abs(r["W_abs"])
        _close(W[0, :64], r["W_row0"], 1e-5, "row0")
        gW = torch.randn(W.shape, generator=torch.Generator().manual_seed(0))  # grads checked on the oracle
        W.backward(gW.to(DEV))
        mo = layer.m.detach().cpu().clone().requires_grad_(True)
        Ao = layer.delta_D_A.detach().cpu().clone().requires_grad_(True)
        Bo = layer.delta_D_B.detach().cpu().clone().requires_grad_(True)
        Wo = R.dora_weight(mo, Ao, Bo, layer.D.cpu(), layer.scaling)
        Wo.backward(gW)
        _close(layer.m.grad, mo.grad, 1e-4, "dm full")
        _close(layer.delta_D_A.grad, Ao.grad, 1e-4, "dA full")
        _close(layer.delta_D_B.grad, Bo.grad, 1e-4, "dB full")
