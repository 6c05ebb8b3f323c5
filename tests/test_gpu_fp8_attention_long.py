"""GPU: the streamed fp8 attention forward (vit_sdpa_fwd_fp8_stream, attn_fwd_fp8_stream<T>).

  1. up to 320 tokens its o and lse are bit for bit the resident fp8 kernel's -- every tile count, one and two
     query blocks, one key in the last tile, causal, and oracle/attn_cases.py's hard softmax inputs: the
     arithmetic check, with no tolerance;
  2. past 320 tokens it is held to its CPU restatement (oracle/attn_fp8_ref.py) under the bounds of
     tests/test_gpu_fp8_attention.py (max 3e-2 and mean 1e-4 of max|o_ref|, lse 1e-4), and up to 641 tokens to
     exact attention (max error 0.12 of max|o|, cosine 0.997).  At (1, 2, 785) and (1, 1, 1025) the restatement
     alone is 0.097 .. 0.104 and 0.9979 .. 0.9981 from exact attention (both dtypes, found on the CPU): the
     format's own error at that length leaves no room for a kernel's share, so those two are held to the
     restatement only;
  3. zero rows, a causal prefix (bit for bit the resident causal run on the first 320 tokens), strided views,
     repeatability, refusals;
  4. vit_base_patch16_384 (bf16) and CLIP-HBA ViT-L/14@336px (fp32) at full depth: RSA with the streamed fp8
     attention within the project's bar of +-0.005 of the bf16 / fp32 path.

Inputs follow tests/test_gpu_fp8_attention.py's ``_qkv(B, H, N, seed=N + B, dtype)``.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import attn_cases as AC  # noqa: E402
from oracle import attn_fp8_ref as F8  # noqa: E402

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float32]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@functools.lru_cache(maxsize=None)
def _qkv(B, H, N, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(B, H, N, 64, generator=g) * s for s in (1.0, 1.3, 0.7))
    q, k, v = (t.to(dtype).float() for t in (q, k, v))
    D = H * 64
    pack = lambda t: t.permute(0, 2, 1, 3).reshape(B * N, D)
    qkv = torch.cat([pack(q), pack(k), pack(v)], 1).to(dtype)
    return q, k, v, qkv


@functools.lru_cache(maxsize=None)
def _restated(B, H, N, dtype, causal=False):
    """The CPU restatement and exact attention of _qkv(B, H, N, N + B, dtype): computed once, never written to."""
    q, k, v, _ = _qkv(B, H, N, N + B, dtype)
    ref, ref_lse = F8.sdpa_fp8(q, k, v, causal=causal)
    return ref, ref_lse, F8.exact_sdpa(q, k, v, causal=causal)


def _count():
    from vit_amd import _lib as L
    return L.lib().vit_sdpa_fp8_stream_count(0)


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _unpack(o, B, H, N):
    return o.float().cpu().reshape(B, N, H, 64).permute(0, 2, 1, 3)


def _hold_to_restatement(got, lse, ref, ref_lse, dtype):
    scale = ref.abs().max().item()
    d = (got - ref.to(dtype).float()).abs()  # o is stored in the qkv dtype
    dl = (lse - ref_lse).abs().max().item()
    print(f"restatement: max {d.max().item() / scale:.3e} mean {d.mean().item() / scale:.3e} of max|o_ref|, lse {dl:.3e}")
    assert d.max().item() <= 3e-2 * scale and d.mean().item() <= 1e-4 * scale, (d.max().item(), d.mean().item())
    assert dl <= 1e-4 * ref_lse.abs().max().item() + 1e-5


def _hold_to_exact(got, ex):
    err = (got - ex).abs().max().item() / ex.abs().max().item()
    cos = torch.nn.functional.cosine_similarity(got.flatten(), ex.flatten(), dim=0).item()
    print(f"exact attention: max err {err:.3e} cosine {cos:.5f}")
    assert err <= 0.12 and cos >= 0.997, (err, cos)


# ---------------------------------------------------------------------------- 1. the resident kernel's bits

# 257 .. 320: two query blocks; 129 and 257: one key in the last tile
@pytest.mark.parametrize("B,H,N,causal", [(3, 2, 16, False), (1, 2, 64, True), (2, 3, 77, True), (2, 2, 129, False),
                                          (2, 2, 129, True), (1, 2, 192, False), (2, 2, 197, False),
                                          (1, 2, 256, False), (1, 2, 257, False), (1, 1, 300, False),
                                          (2, 2, 320, False), (1, 2, 320, True)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_stream_is_bit_for_bit_the_resident_kernel(B, H, N, causal, dtype):
    from vit_amd import ops
    qkv = _qkv(B, H, N, N + B, dtype)[3].to(DEV)
    c0 = _count()
    o_r, lse_r = ops.sdpa_fwd(qkv, B, H, N, causal=causal, fp8=True)
    o_rl, lse_rl = ops.sdpa_fwd(qkv, B, H, N, causal=causal, fp8=True, fp8_long=True)  # <= 320: still resident
    assert _count() == c0
    o_s, lse_s = ops.sdpa_fwd_fp8_stream(qkv, B, H, N, causal=causal)
    assert _count() == c0 + 1
    torch.cuda.synchronize()
    assert torch.isfinite(o_r.float()).all() and torch.isfinite(lse_r).all()
    assert _same_bits(o_s, o_r) and torch.equal(lse_s, lse_r)
    assert _same_bits(o_rl, o_r) and torch.equal(lse_rl, lse_r)


@pytest.mark.parametrize("kind", AC.KINDS)
@pytest.mark.parametrize("N", [257, 320])
@pytest.mark.parametrize("dtype", DTYPES)
def test_stream_is_bit_for_bit_the_resident_kernel_on_hard_inputs(kind, N, dtype):
    from vit_amd import ops
    B, H = 2, 2
    c = AC.make_case(kind, B, H, N, dtype)
    qkv = c.qkv.to(DEV)
    o_r, lse_r = ops.sdpa_fwd(qkv, B, H, N, scale=c.scale, fp8=True)
    o_s, lse_s = ops.sdpa_fwd_fp8_stream(qkv, B, H, N, scale=c.scale)
    torch.cuda.synchronize()
    assert torch.isfinite(o_r.float()).all() and torch.isfinite(lse_r).all()
    assert _same_bits(o_s, o_r) and torch.equal(lse_s, lse_r)


# ---------------------------------------------------------------------------- 2. past 320 tokens

@pytest.mark.parametrize("B,H,N,exact", [(1, 2, 321, True), (2, 2, 384, True), (1, 2, 385, True), (1, 3, 577, True),
                                         (1, 2, 641, True), (1, 2, 785, False), (1, 1, 1025, False)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_stream_past_320_matches_restatement_and_bound(B, H, N, exact, dtype):
    from vit_amd import ops
    qkv = _qkv(B, H, N, N + B, dtype)[3].to(DEV)
    c0 = _count()
    o, lse = ops.sdpa_fwd(qkv, B, H, N, fp8=True, fp8_long=True)
    torch.cuda.synchronize()
    assert _count() == c0 + 1
    ref, ref_lse, ex = _restated(B, H, N, dtype)
    got = _unpack(o, B, H, N)
    _hold_to_restatement(got, lse.cpu().reshape(B, H, N), ref, ref_lse, dtype)
    if exact:
        _hold_to_exact(got, ex)


# ---------------------------------------------------------------------------- 3. zero rows

@pytest.mark.parametrize("dtype", DTYPES)
def test_stream_zero_rows_match_restatement(dtype):
    from vit_amd import ops
    B, H, N = 1, 2, 577
    c = AC.make_case("zerorows", B, H, N, dtype)
    q, k, v = (t.float() for t in AC.split_qkv(c.qkv, B, H, N))
    assert (q[:, :, ::3] == 0).all() and (k[:, :, 1::5] == 0).all() and (v[:, :, 2::7] == 0).all()
    o, lse = ops.sdpa_fwd(c.qkv.to(DEV), B, H, N, fp8=True, fp8_long=True)
    torch.cuda.synchronize()
    got = _unpack(o, B, H, N)
    assert torch.isfinite(got).all() and torch.isfinite(lse).all()
    ref, ref_lse = F8.sdpa_fp8(q, k, v)
    _hold_to_restatement(got, lse.cpu().reshape(B, H, N), ref, ref_lse, dtype)


# ---------------------------------------------------------------------------- 4. causal prefix

@pytest.mark.parametrize("dtype", DTYPES)
def test_stream_causal_prefix_is_the_resident_run(dtype):
    """Under the causal mask a query sees no later key: rows 0..319 of a 577-token image meet tiles 5..9 fully
    masked (alpha = 1 and p = 0, both exact), so they are the resident causal run on the first 320 tokens."""
    from vit_amd import ops
    B, H, N, P = 2, 2, 577, 320
    qkv = _qkv(B, H, N, N + B, dtype)[3].to(DEV)
    o, lse = ops.sdpa_fwd(qkv, B, H, N, causal=True, fp8=True, fp8_long=True)
    for b in range(B):
        head = qkv[b * N:b * N + P].contiguous()
        o_r, lse_r = ops.sdpa_fwd(head, 1, H, P, causal=True, fp8=True)
        torch.cuda.synchronize()
        assert _same_bits(o[b * N:b * N + P], o_r)
        assert torch.equal(lse.view(B, H, N)[b, :, :P], lse_r.view(H, P))
    ref, ref_lse, ex = _restated(B, H, N, dtype, True)
    got = _unpack(o, B, H, N)
    _hold_to_restatement(got, lse.cpu().reshape(B, H, N), ref, ref_lse, dtype)
    _hold_to_exact(got, ex)


# ---------------------------------------------------------------------------- 5. views, 6. repeatable

@pytest.mark.parametrize("dtype", DTYPES)
def test_stream_views_are_bit_equal_to_the_contiguous_run(dtype):
    from vit_amd import ops
    B, H, N = 2, 2, 385
    D = H * 64
    qkv = _qkv(B, H, N, N + B, dtype)[3].to(DEV)
    o0, lse0 = ops.sdpa_fwd_fp8_stream(qkv, B, H, N)
    # qkv as a column slice of a wider buffer
    wide = torch.full((B * N, 3 * D + 8), 7.0, dtype=dtype, device=DEV)
    wide[:, :3 * D] = qkv
    view = wide[:, :3 * D]
    assert view.stride(0) == 3 * D + 8
    o1, lse1 = ops.sdpa_fwd_fp8_stream(view, B, H, N)
    assert _same_bits(o1, o0) and torch.equal(lse1, lse0)
    # o as a column slice of a wider buffer: the other columns stay untouched
    obuf = torch.full((B * N, D + 4), 7.0, dtype=dtype, device=DEV)
    o2, lse2 = ops.sdpa_fwd_fp8_stream(qkv, B, H, N, o=obuf[:, :D])
    assert o2.stride(0) == D + 4
    assert _same_bits(o2.contiguous(), o0) and torch.equal(lse2, lse0) and (obuf[:, D:] == 7.0).all()
    # rows [N, 2N) of the B = 2 input, as the half-batch chain slices them
    o3, lse3 = ops.sdpa_fwd_fp8_stream(qkv[N:2 * N], 1, H, N)
    torch.cuda.synchronize()
    assert _same_bits(o3, o0[N:2 * N]) and torch.equal(lse3, lse0[H * N:])


@pytest.mark.parametrize("dtype", DTYPES)
def test_stream_is_repeatable(dtype):
    from vit_amd import ops
    B, H, N = 1, 3, 577
    qkv = _qkv(B, H, N, N + B, dtype)[3].to(DEV)
    o0, lse0 = ops.sdpa_fwd(qkv, B, H, N, fp8=True, fp8_long=True)
    o1, lse1 = ops.sdpa_fwd(qkv, B, H, N, fp8=True, fp8_long=True)
    torch.cuda.synchronize()
    assert _same_bits(o0, o1) and torch.equal(lse0, lse1)


# ---------------------------------------------------------------------------- 7. refusals

def test_refusals():
    from vit_amd import _lib as L
    from vit_amd import ops
    B, H, N = 1, 2, 321
    D = H * 64
    qkv = _qkv(B, H, N, N + B, torch.bfloat16)[3].to(DEV)
    c0 = _count()
    with pytest.raises(ValueError, match="320"):
        ops.sdpa_fwd(qkv, B, H, N, fp8=True)
    o = torch.empty(B * N, D, dtype=qkv.dtype, device=DEV)
    lse = torch.empty(B * H * N, dtype=torch.float32, device=DEV)
    fn = L.lib().vit_sdpa_fwd_fp8_stream
    args = lambda hd, ld_qkv, ld_o: (L.dt(qkv), B, H, N, hd, L.ptr(qkv), ld_qkv, L.ptr(o), ld_o, L.ptr(lse), 0.125, 0,
                                     L.stream_ptr(qkv.device))
    assert fn(*args(32, 3 * D, D)) != 0        # head_dim != 64
    assert fn(*args(64, 3 * D + 4, D)) != 0    # ld_qkv % 8
    assert fn(*args(64, 3 * D, D + 2)) != 0    # ld_o % 4
    assert _count() == c0                      # nothing was launched
    assert fn(*args(64, 3 * D, D)) == 0
    torch.cuda.synchronize()
    assert _count() == c0 + 1


# ---------------------------------------------------------------------------- 8. models

def _ref_rdm(seed):
    a = np.random.default_rng(seed).random((48, 48))
    ref = (a + a.T) / 2
    np.fill_diagonal(ref, 0)
    return ref


def test_vit_base_384_rsa_streamed_fp8_within_north_star():
    """vit_base_patch16_384 (577 tokens, bf16, full depth): compute_rsa_score with the streamed fp8 attention
    within +-0.005 of the bf16 path; a training forward and backward keep the bf16 attention."""
    import vit_amd
    torch.manual_seed(0)  # the patch embedding's default init; init_weights seeds the rest
    m = vit_amd.create_model("vit_base_patch16_384", compute_dtype=torch.bfloat16)
    m.init_weights(seed=5)
    m = m.to(DEV).eval()
    g = torch.Generator().manual_seed(9)
    imgs = torch.randn(48, 3, 384, 384, generator=g).to(DEV)
    ref = _ref_rdm(11)
    rho_bf16, _ = vit_amd.rsa.compute_rsa_score(m, imgs, ref)
    c0 = _count()
    m.set_attention_fp8(True, long_sequences=True)
    rho_fp8, _ = vit_amd.rsa.compute_rsa_score(m, imgs, ref)
    print(f"rho bf16 {rho_bf16:.6f} streamed fp8 {rho_fp8:.6f}")
    assert _count() > c0
    assert abs(rho_fp8 - rho_bf16) <= 0.005, (rho_fp8, rho_bf16)
    c1 = _count()
    m.train()
    vit_amd.cross_entropy(m(imgs[:2]), torch.tensor([1, 2], device=DEV)).backward()
    torch.cuda.synchronize()
    assert _count() == c1  # training forwards keep the bf16 attention (the backward needs it)
    assert all(torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None)


def test_clip_l14_336_behavioral_rsa_streamed_fp8_within_north_star():
    """CLIP-HBA ViT-L/14@336px (fp32, full depth, DoRA 2 + 1): the behavioural RSA with streamed fp8 attention in
    the frozen blocks within +-0.005 of the fp32 model; a training step runs with finite gradients, its frozen
    blocks in streamed fp8 and its DoRA blocks in fp32."""
    import vit_amd
    from vit_amd import _lib as L
    from vit_amd import sweep as S
    torch.manual_seed(0)
    m = vit_amd.CLIPHBA(["c%d" % i for i in range(66)], "ViT-L/14@336px", pos_embedding=True)
    vit_amd.apply_dora_to_ViT(m, n_vision_layers=2, n_transformer_layers=1, r=32)
    vit_amd.switch_dora_layers(m, freeze_all=True, dora_state=True)
    m = m.to(DEV)
    g = torch.Generator().manual_seed(3)
    imgs = torch.randn(48, 3, 336, 336, generator=g).to(DEV)
    ref = _ref_rdm(1)
    rho32, _ = S.behavioral_rsa(m, imgs, ref)
    c0 = _count()
    m.clip_model.set_attention_fp8(True, long_sequences=True)
    rho8, _ = S.behavioral_rsa(m, imgs, ref)
    print(f"rho fp32 {rho32:.6f} streamed fp8 {rho8:.6f}")
    assert _count() > c0
    assert abs(rho8 - rho32) <= 0.005, (rho8, rho32)
    opt = vit_amd.FusedAdamW([q for q in m.parameters() if q.requires_grad], lr=3e-4)
    c1, f0 = _count(), L.lib().vit_sdpa_long_f32_count(0)
    loss = vit_amd.mse_loss(m(imgs[:4]), torch.randn(4, 66, device=DEV))
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    assert torch.isfinite(loss)
    assert _count() > c1 and L.lib().vit_sdpa_long_f32_count(0) > f0
    grads = [q.grad for q in m.parameters() if q.requires_grad]
    assert grads and all(gr is not None and torch.isfinite(gr).all() for gr in grads)
