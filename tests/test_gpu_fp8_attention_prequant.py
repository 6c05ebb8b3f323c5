"""GPU: the quantise-once fp8 attention forward (vit_sdpa_fp8_quant_kv / attn_fp8_quant_kv<T>,
vit_sdpa_fwd_fp8_pre / attn_fwd_fp8_pre<T>).

The pre-pass builds the very chunk images the streamed kernel (attn_fwd_fp8_stream, §4.17) builds in its LDS ring
and the consumer runs the streamed kernel's tile steps on them, so every comparison here is exact: o and lse are
``ops.sdpa_fwd_fp8_stream``'s bits on the same inputs, at every N, and up to 320 tokens the resident kernel's.  No
tolerance appears in this file.

  1. bit for bit the streamed kernel: one and several query blocks, odd and even chunk counts, N on and off a
     multiple of 64 (the zeroed tail), a last wave with no live query; causal and not;
  2. the same on oracle/attn_cases.py's hard softmax inputs at 321 tokens;
  3. the consumer reads K and V from the workspace alone (qkv's K and V columns overwritten with NaN);
  4. the workspace is fully written and a pure function of K and V (two poisons), and the consumer leaves it alone;
  5. guard bytes around an exactly sized workspace, poisoned strided views of qkv and o;
  6. one workspace serves two qkv that differ in Q alone;
  7. repeatability and the launch counters;  8. refusals;  9. a ViT and 10. a CLIP past 320 tokens, with the
     visual prefix cache's key unchanged by the switch.

Inputs follow tests/test_gpu_fp8_attention_long.py's ``_qkv(B, H, N, seed=N + B, dtype)``.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import attn_cases as AC  # noqa: E402

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float32]
IDS = ["bf16", "f32"]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@functools.lru_cache(maxsize=None)
def _qkv(B, H, N, dtype):
    """The fused qkv [B*N, 3D] on the GPU: made once, never written to."""
    g = torch.Generator().manual_seed(N + B)
    q, k, v = (torch.randn(B, H, N, 64, generator=g) * s for s in (1.0, 1.3, 0.7))
    D = H * 64
    pack = lambda t: t.permute(0, 2, 1, 3).reshape(B * N, D)
    return torch.cat([pack(q), pack(k), pack(v)], 1).to(dtype).to(DEV)


@functools.lru_cache(maxsize=None)
def _streamed(B, H, N, causal, dtype):
    """The reference: the streamed fp8 kernel on _qkv(B, H, N, dtype).  Computed once, never written to."""
    from vit_amd import ops
    o, lse = ops.sdpa_fwd_fp8_stream(_qkv(B, H, N, dtype), B, H, N, causal=causal)
    torch.cuda.synchronize()
    assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all()
    return o, lse


def _counts():
    from vit_amd import _lib as L
    return L.lib().vit_sdpa_fp8_pre_count(0), L.lib().vit_sdpa_fp8_stream_count(0)


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _pair(qkv, B, H, N, **kw):
    from vit_amd import ops
    ws = ops.sdpa_fp8_quant_kv(qkv, B, H, N)
    return ops.sdpa_fwd_fp8_pre(qkv, ws, B, H, N, **kw)


# ---------------------------------------------------------------------------- 1. the streamed kernel's bits

SHAPES = [(3, 2, 16, False), (1, 2, 64, True), (2, 3, 77, True), (2, 2, 129, False), (1, 2, 256, False),
          (1, 2, 257, False), (2, 2, 320, True), (1, 2, 321, False), (2, 2, 384, False), (1, 3, 577, False),
          (1, 2, 785, True)]


@pytest.mark.parametrize("B,H,N,causal", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_pre_is_bit_for_bit_the_streamed_kernel(B, H, N, causal, dtype):
    from vit_amd import ops
    qkv = _qkv(B, H, N, dtype)
    o_s, lse_s = _streamed(B, H, N, causal, dtype)
    ws = ops.sdpa_fp8_quant_kv(qkv, B, H, N)
    assert ws.dtype == torch.uint8 and ws.numel() == ops.sdpa_fp8_kv_bytes(B, H, N)
    o, lse = ops.sdpa_fwd_fp8_pre(qkv, ws, B, H, N, causal=causal)
    torch.cuda.synchronize()
    assert _same_bits(o, o_s) and _same_bits(lse, lse_s)
    if N <= 320:  # and so the resident kernel's
        o_r, lse_r = ops.sdpa_fwd(qkv, B, H, N, causal=causal, fp8=True)
        # up to 320 tokens the switch changes nothing: the resident kernel already quantises once per head
        c0 = _counts()
        o_p, lse_p = ops.sdpa_fwd(qkv, B, H, N, causal=causal, fp8=True, fp8_long=True, fp8_pre=True)
        torch.cuda.synchronize()
        assert _counts() == c0
        assert _same_bits(o, o_r) and _same_bits(lse, lse_r)
        assert _same_bits(o_p, o_r) and _same_bits(lse_p, lse_r)
    else:  # ops.sdpa_fwd's own route: one consumer launch, no streamed one
        c0 = _counts()
        o_p, lse_p = ops.sdpa_fwd(qkv, B, H, N, causal=causal, fp8=True, fp8_long=True, fp8_pre=True)
        torch.cuda.synchronize()
        assert _counts() == (c0[0] + 1, c0[1])
        assert _same_bits(o_p, o_s) and _same_bits(lse_p, lse_s)
        # without fp8_long the switch lifts no refusal
        with pytest.raises(ValueError, match="320"):
            ops.sdpa_fwd(qkv, B, H, N, causal=causal, fp8=True, fp8_pre=True)


# ---------------------------------------------------------------------------- 2. hard softmax inputs

@pytest.mark.parametrize("kind", AC.KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_pre_is_bit_for_bit_the_streamed_kernel_on_hard_inputs(kind, dtype):
    from vit_amd import ops
    B, H, N = 2, 2, 321
    c = AC.make_case(kind, B, H, N, dtype)
    qkv = c.qkv.to(DEV)
    o_s, lse_s = ops.sdpa_fwd_fp8_stream(qkv, B, H, N, scale=c.scale)
    o, lse = _pair(qkv, B, H, N, scale=c.scale)
    torch.cuda.synchronize()
    assert torch.isfinite(o_s.float()).all() and torch.isfinite(lse_s).all()
    assert _same_bits(o, o_s) and _same_bits(lse, lse_s)


# ---------------------------------------------------------------------------- 3. K and V come from the workspace

@pytest.mark.parametrize("B,H,N,causal", [(2, 2, 321, False), (1, 2, 129, True)])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_consumer_reads_k_and_v_from_the_workspace_alone(B, H, N, causal, dtype):
    from vit_amd import ops
    D = H * 64
    o_s, lse_s = _streamed(B, H, N, causal, dtype)
    qkv = _qkv(B, H, N, dtype).clone()
    ws = ops.sdpa_fp8_quant_kv(qkv, B, H, N)
    qkv[:, D:] = float("nan")  # K and V; Q stays
    o, lse = ops.sdpa_fwd_fp8_pre(qkv, ws, B, H, N, causal=causal)
    torch.cuda.synchronize()
    assert torch.isnan(qkv[:, D:].float()).all() and _same_bits(qkv[:, :D], _qkv(B, H, N, dtype)[:, :D])
    assert _same_bits(o, o_s) and _same_bits(lse, lse_s)


# ---------------------------------------------------------------------------- 4. pure function, fully written

@pytest.mark.parametrize("B,H,N", [(2, 2, 321), (1, 3, 64), (2, 1, 16)])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_workspace_is_fully_written_and_a_pure_function_of_k_and_v(B, H, N, dtype):
    from vit_amd import ops
    qkv = _qkv(B, H, N, dtype)
    n = ops.sdpa_fp8_kv_bytes(B, H, N)
    wa = torch.full((n,), 0x7F, dtype=torch.uint8, device=DEV)
    wb = torch.full((n,), 0xA5, dtype=torch.uint8, device=DEV)
    assert ops.sdpa_fp8_quant_kv(qkv, B, H, N, ws=wa) is wa
    ops.sdpa_fp8_quant_kv(qkv, B, H, N, ws=wb)
    torch.cuda.synchronize()
    assert torch.equal(wa, wb)
    # Q plays no part: another Q, the same K and V, the same bytes
    other = qkv.clone()
    other[:, :H * 64] = 3.0
    assert torch.equal(ops.sdpa_fp8_quant_kv(other, B, H, N), wa)
    keep = wa.clone()
    o_a, lse_a = ops.sdpa_fwd_fp8_pre(qkv, wa, B, H, N)
    o_b, lse_b = ops.sdpa_fwd_fp8_pre(qkv, wb, B, H, N)
    torch.cuda.synchronize()
    assert torch.equal(wa, keep) and torch.equal(wb, keep)  # the consumer writes nothing there
    o_s, lse_s = _streamed(B, H, N, False, dtype)
    assert _same_bits(o_a, o_s) and _same_bits(o_b, o_s) and _same_bits(lse_a, lse_s) and _same_bits(lse_b, lse_s)


# ---------------------------------------------------------------------------- 5. guards and views

@pytest.mark.parametrize("B,H,N", [(2, 2, 385), (1, 2, 77)])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_guards_stay_intact_and_views_give_the_contiguous_bits(B, H, N, dtype):
    from vit_amd import ops
    D = H * 64
    qkv = _qkv(B, H, N, dtype)
    o_s, lse_s = _streamed(B, H, N, False, dtype)
    n, G = ops.sdpa_fp8_kv_bytes(B, H, N), 4096
    buf = torch.full((G + n + G,), 0x5C, dtype=torch.uint8, device=DEV)
    ws = buf[G:G + n]
    assert ws.data_ptr() % 16 == 0
    # qkv as a column window of a wider, poisoned buffer
    wide = torch.full((B * N, 3 * D + 16), float("nan"), dtype=dtype, device=DEV)
    wide[:, 8:8 + 3 * D] = qkv
    view = wide[:, 8:8 + 3 * D]
    assert view.stride(0) == 3 * D + 16 and not view.is_contiguous()
    # o as a column window of a wider, poisoned buffer
    obuf = torch.full((B * N, D + 8), 7.0, dtype=dtype, device=DEV)
    oview = obuf[:, 4:4 + D]
    lbuf = torch.full((B * H * N + 16,), 7.0, dtype=torch.float32, device=DEV)
    ops.sdpa_fp8_quant_kv(view, B, H, N, ws=ws)
    o, lse = ops.sdpa_fwd_fp8_pre(view, ws, B, H, N, o=oview, lse=lbuf[8:8 + B * H * N])
    torch.cuda.synchronize()
    assert (buf[:G] == 0x5C).all() and (buf[G + n:] == 0x5C).all()
    assert torch.equal(ws, ops.sdpa_fp8_quant_kv(qkv, B, H, N))  # the contiguous run's workspace
    assert o.stride(0) == D + 8
    assert _same_bits(o.contiguous(), o_s) and _same_bits(lse, lse_s)
    assert (obuf[:, :4] == 7.0).all() and (obuf[:, 4 + D:] == 7.0).all()
    assert (lbuf[:8] == 7.0).all() and (lbuf[8 + B * H * N:] == 7.0).all()
    # rows [N, 2N) of a B = 2 input, as the half-batch chain slices them
    if B == 2:
        o1, lse1 = _pair(qkv[N:2 * N], 1, H, N)
        torch.cuda.synchronize()
        assert _same_bits(o1, o_s[N:2 * N]) and _same_bits(lse1, lse_s[H * N:])


# ---------------------------------------------------------------------------- 6. one workspace, two Q

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_one_workspace_serves_two_q(dtype):
    from vit_amd import ops
    B, H, N = 1, 2, 577
    D = H * 64
    qkv_a = _qkv(B, H, N, dtype)
    qkv_b = qkv_a.clone()
    g = torch.Generator().manual_seed(5)
    qkv_b[:, :D] = (torch.randn(B * N, D, generator=g) * 1.7).to(dtype).to(DEV)
    ws = ops.sdpa_fp8_quant_kv(qkv_a, B, H, N)
    o_a, lse_a = ops.sdpa_fwd_fp8_pre(qkv_a, ws, B, H, N)
    o_b, lse_b = ops.sdpa_fwd_fp8_pre(qkv_b, ws, B, H, N)
    s_a = _streamed(B, H, N, False, dtype)
    s_b = ops.sdpa_fwd_fp8_stream(qkv_b, B, H, N)
    torch.cuda.synchronize()
    assert _same_bits(o_a, s_a[0]) and _same_bits(lse_a, s_a[1])
    assert _same_bits(o_b, s_b[0]) and _same_bits(lse_b, s_b[1])
    assert not _same_bits(o_a, o_b)


# ---------------------------------------------------------------------------- 7. repeatable, counted

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_pre_is_repeatable_and_counted(dtype):
    from vit_amd import ops
    B, H, N = 1, 3, 577
    qkv = _qkv(B, H, N, dtype)
    o_s, lse_s = _streamed(B, H, N, False, dtype)
    c0 = _counts()
    ws = ops.sdpa_fp8_quant_kv(qkv, B, H, N)
    assert _counts() == c0  # the pre-pass is not a consumer launch
    runs = []
    for i in range(3):
        runs.append(ops.sdpa_fwd_fp8_pre(qkv, ws, B, H, N))
        assert _counts() == (c0[0] + i + 1, c0[1])
    torch.cuda.synchronize()
    for o, lse in runs:
        assert _same_bits(o, o_s) and _same_bits(lse, lse_s)
    o, _ = ops.sdpa_fwd_fp8_pre(qkv, ws, B, H, N, lse=None)  # and with no lse asked for at the C level
    from vit_amd import _lib as L
    o2 = torch.empty_like(o)
    L.call("vit_sdpa_fwd_fp8_pre", L.dt(qkv), B, H, N, 64, L.ptr(qkv), qkv.stride(0), L.ptr(ws), ws.numel(), L.ptr(o2),
           o2.stride(0), None, 0.125, 0, L.stream_ptr(qkv.device))
    torch.cuda.synchronize()
    assert _same_bits(o2, o_s)


# ---------------------------------------------------------------------------- 8. refusals

def test_refusals_launch_nothing():
    from vit_amd import _lib as L
    from vit_amd import ops
    B, H, N = 1, 2, 321
    D = H * 64
    qkv = _qkv(B, H, N, torch.bfloat16)
    n = ops.sdpa_fp8_kv_bytes(B, H, N)
    buf = torch.full((n + 16,), 0x33, dtype=torch.uint8, device=DEV)
    ws = buf[:n]
    o = torch.full((B * N, D), 7.0, dtype=qkv.dtype, device=DEV)
    lse = torch.full((B * H * N,), 7.0, dtype=torch.float32, device=DEV)
    s = L.stream_ptr(qkv.device)
    good = dict(N=N, hd=64, ld_qkv=3 * D, ws=L.ptr(ws), ws_bytes=n, ld_o=D)
    quant = lambda a: ("vit_sdpa_fp8_quant_kv", L.dt(qkv), B, H, a["N"], a["hd"], L.ptr(qkv), a["ld_qkv"], a["ws"],
                       a["ws_bytes"], s)
    fwd = lambda a: ("vit_sdpa_fwd_fp8_pre", L.dt(qkv), B, H, a["N"], a["hd"], L.ptr(qkv), a["ld_qkv"], a["ws"],
                     a["ws_bytes"], L.ptr(o), a["ld_o"], L.ptr(lse), 0.125, 0, s)
    bad = [dict(hd=32), dict(N=0), dict(N=-3), dict(ld_qkv=3 * D + 4), dict(ws=None), dict(ws=L.ptr(buf[8:])),
           dict(ws_bytes=n - 1), dict(ws_bytes=0)]
    c0 = _counts()
    for change in bad:
        for mk in (quant, fwd):
            with pytest.raises(RuntimeError):
                L.call(*mk(dict(good, **change)))
    with pytest.raises(RuntimeError):
        L.call(*fwd(dict(good, ld_o=D + 2)))  # ld_o % 4
    with pytest.raises(RuntimeError):  # a workspace sized for fewer chunks
        ops.sdpa_fp8_quant_kv(qkv, B, H, N, ws=torch.empty(ops.sdpa_fp8_kv_bytes(B, H, 320), dtype=torch.uint8, device=DEV))
    torch.cuda.synchronize()
    assert _counts() == c0
    assert (buf == 0x33).all() and (o == 7.0).all() and (lse == 7.0).all()  # nothing ran
    L.call(*quant(good))
    L.call(*fwd(good))
    torch.cuda.synchronize()
    assert _counts() == (c0[0] + 1, c0[1])
    assert _same_bits(o, _streamed(B, H, N, False, torch.bfloat16)[0]) and (buf[n:] == 0x33).all()


def test_kv_bytes_is_positive_and_grows():
    from vit_amd import ops
    base = ops.sdpa_fp8_kv_bytes(1, 1, 1)
    assert base > 0 and base % 16 == 0
    assert ops.sdpa_fp8_kv_bytes(1, 1, 64) == base  # one chunk
    assert ops.sdpa_fp8_kv_bytes(1, 1, 65) > base
    assert ops.sdpa_fp8_kv_bytes(2, 1, 64) > base and ops.sdpa_fp8_kv_bytes(1, 2, 64) > base
    assert ops.sdpa_fp8_kv_bytes(2, 3, 577) == 2 * 3 * 10 * base
    for args in [(0, 1, 1), (1, 0, 1), (1, 1, 0)]:
        with pytest.raises(RuntimeError):
            ops.sdpa_fp8_kv_bytes(*args)


# ---------------------------------------------------------------------------- 9. ViT

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_vit_logits_are_bit_equal_with_the_switch(dtype):
    import vit_amd
    torch.manual_seed(0)
    m = vit_amd.VisionTransformer(img_size=304, patch_size=16, embed_dim=128, depth=2, num_heads=2, num_classes=7,
                                  compute_dtype=dtype)  # 19 * 19 + 1 = 362 tokens
    m.init_weights(seed=3)
    m = m.to(DEV).eval()
    x = torch.randn(3, 3, 304, 304, generator=torch.Generator().manual_seed(4)).to(DEV)
    with torch.no_grad():
        m.set_attention_fp8(True, long_sequences=True)
        c0 = _counts()
        y_stream = m(x)
        torch.cuda.synchronize()
        c1 = _counts()
        assert c1[0] == c0[0] and c1[1] > c0[1]
        m.set_attention_fp8(True, long_sequences=True, prequantize=True)
        y_pre = m(x)
        torch.cuda.synchronize()
        c2 = _counts()
        assert c2[0] - c1[0] == c1[1] - c0[1] and c2[1] == c1[1]
        m.set_attention_fp8(False)
        y_off = m(x)
        torch.cuda.synchronize()
        assert _counts() == c2
    assert torch.isfinite(y_stream.float()).all()
    assert _same_bits(y_pre, y_stream)
    assert not _same_bits(y_off, y_stream)  # fp8 attention did run
    # a training forward and backward keep the bf16 / f32 attention
    m.set_attention_fp8(True, long_sequences=True, prequantize=True)
    m.train()
    vit_amd.cross_entropy(m(x[:2]), torch.tensor([1, 2], device=DEV)).backward()
    torch.cuda.synchronize()
    assert _counts() == c2


# ---------------------------------------------------------------------------- 10. CLIP

VL, TL = 3, 2  # visual / text blocks of the tiny CLIP below


def _tiny_clip():
    from vit_amd import clip
    torch.manual_seed(0)
    cm = clip.CLIP(embed_dim=64, image_resolution=160, vision_layers=VL, vision_width=128, vision_patch_size=8,
                   context_length=77, vocab_size=97, transformer_width=128, transformer_heads=2,
                   transformer_layers=TL)  # 20 * 20 + 1 = 401 visual tokens, 77 text tokens; fp32
    cm.initialize_parameters(seed=6)
    return cm


def test_clip_is_bit_equal_with_the_switch_and_text_launches_no_pre_pass():
    cm = _tiny_clip().to(DEV).eval()
    g = torch.Generator().manual_seed(8)
    img = torch.randn(2, 3, 160, 160, generator=g).to(DEV)
    text = torch.randint(1, 97, (5, 77), generator=g).to(DEV)
    with torch.no_grad():
        cm.set_attention_fp8(True, long_sequences=True)
        c0 = _counts()
        f_s = cm.encode_image(img)
        torch.cuda.synchronize()
        c1 = _counts()
        assert (c1[0] - c0[0], c1[1] - c0[1]) == (0, VL)  # fp32: one launch per visual block
        y_s = cm(img, text)
        cm.set_attention_fp8(True, long_sequences=True, prequantize=True)
        cm._text_cache = None  # the text tower runs again (its key does not see the switch)
        c2 = _counts()
        f_p = cm.encode_image(img)
        torch.cuda.synchronize()
        c3 = _counts()
        assert (c3[0] - c2[0], c3[1] - c2[1]) == (VL, 0)
        t_p = cm.encode_text(text)  # 77 tokens: the resident kernel, neither streamed form
        torch.cuda.synchronize()
        assert _counts() == c3
        y_p = cm(img, text)
        torch.cuda.synchronize()
        assert _counts() == (c3[0] + VL, c3[1])
    assert torch.isfinite(f_s).all() and torch.isfinite(y_s).all() and torch.isfinite(t_p).all()
    assert _same_bits(f_p, f_s) and _same_bits(y_p, y_s)


def test_prefix_cache_built_without_the_switch_serves_with_it():
    import vit_amd
    from vit_amd.prefix_cache import prefix_key
    m = vit_amd.CLIPHBA([f"c{i}" for i in range(5)], "ViT-L/14", pos_embedding=True, clip_model=_tiny_clip(),
                        attention_fp8=True, attention_fp8_long=True)
    vit_amd.apply_dora_to_ViT(m, n_vision_layers=1, n_transformer_layers=1, r=4)  # two frozen visual blocks
    vit_amd.switch_dora_layers(m, freeze_all=True, dora_state=True)
    m = m.to(DEV).eval()
    imgs = torch.randn(4, 3, 160, 160, generator=torch.Generator().manual_seed(2)).to(DEV)
    idx = torch.arange(4)
    c0 = _counts()
    cache = vit_amd.VisualPrefixCache.build(m, imgs, batch_size=4)
    torch.cuda.synchronize()
    c1 = _counts()
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (0, VL - 1)  # the frozen blocks, streamed
    key = prefix_key(m, imgs)
    with torch.no_grad():
        p_off_cached = m(visual_prefix=cache.take(idx))
        p_off = m(imgs)
        m.clip_model.set_attention_fp8(True, long_sequences=True, prequantize=True)
        assert prefix_key(m, imgs) == key and cache.valid_for(m, imgs)
        assert cache.ensure(m, imgs, batch_size=4) is False and cache.builds == 1
        c2 = _counts()
        p_on_cached = m(visual_prefix=cache.take(idx))
        torch.cuda.synchronize()
        c3 = _counts()
        assert (c3[0] - c2[0], c3[1] - c2[1]) == (1, 0)  # the one block behind the cut, pre-quantised (no-grad pass)
        p_on = m(imgs)
        torch.cuda.synchronize()
        assert _counts() == (c3[0] + VL, c3[1])
    assert torch.isfinite(p_off).all()
    assert _same_bits(p_on_cached, p_off_cached) and _same_bits(p_on, p_off)
    assert _same_bits(p_off_cached, p_off)  # the same batch: the same kernels on the same shapes
    # a rebuilt cache holds the same tokens
    again = vit_amd.VisualPrefixCache.build(m, imgs, batch_size=4)
    torch.cuda.synchronize()
    assert _same_bits(again.x, cache.x) and again.key == cache.key
