"""GPU: f32 attention past the resident kernels' 288-token limit.

f32, non-causal operands whose row strides are multiples of 4 elements take the streamed f32 MFMA kernels
(attn_fwd_stream_f32 / attn_bwd_dq_stream_f32 / attn_bwd_dkv_stream_f32: K / V, or Q / dO, pass through a
two-buffer LDS ring of 64-row f32 chunks); causal or misaligned operands keep the generic scalar kernels.
``vit_sdpa_long_f32_count`` counts the vit_sdpa_fwd / vit_sdpa_bwd calls that took them (one per call);
``vit_sdpa_long_count`` keeps counting the bf16 streamed calls only.

Kernel references are torch fp32 autograd built as tests/test_gpu_attention_long.py's ``_case`` builds
them (randn * 1.5, scale 0.125); bounds are the project's f32 ones: o and lse 1e-5, gradients and the
qkv-bias gradient 1e-4, each of the reference's max-abs.  A torch fp32 restatement of the algorithm on the
CPU (64-key chunks, online softmax, exp2 form, backward recomputed from lse) stays at or below 1.7e-6 on
every quantity at N = 289 / 577 / 1025, so the algorithm leaves ~6x room under 1e-5 and ~60x under 1e-4.
Model-level bounds: 1e-3 relative against the CPU oracles (test_gpu_parity / test_clip's f32 bound).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from vit_amd import _lib as L  # noqa: E402
from vit_amd import ops  # noqa: E402

DEV = "cuda"
F32 = torch.float32
TO, TL, TG = 1e-5, 1e-5, 1e-4  # o, lse, gradients (and bias gradient)


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    L.load()
    L.lib().vit_sdpa_long_config(-1)


def _close(got, ref, rel, what=""):
    got = got.detach().float().cpu()
    ref = ref.detach().float().cpu()
    scale = ref.abs().max().item() + 1e-12
    err = (got - ref).abs().max().item()
    print(f"{what}: max err {err:.3e} / scale {scale:.3e} = {err / scale:.3e} (bound {rel:.1e})")
    assert err <= rel * scale, f"{what}: max err {err:.3e} > {rel:.1e} * scale {scale:.3e}"


def _rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return (a - b).abs().max().item() / (b.abs().max().item() + 1e-30)


def _count():
    return L.lib().vit_sdpa_long_f32_count(0)


def _count_bf16():
    return L.lib().vit_sdpa_long_count(0)


_REF = {}


def _case(B, H, N, causal=False, seed=34, dev="cpu"):
    """f32 inputs and the torch fp32 reference (o, lse, [dq | dk | dv]) of one shape; computed once and shared."""
    key = (B, H, N, causal, seed, dev)
    if key not in _REF:
        D = H * 64
        g = torch.Generator().manual_seed(seed)
        qkv = (torch.randn(B * N, 3 * D, generator=g) * 1.5).to(dev)
        do = torch.randn(B * N, D, generator=g).to(dev)
        q, k, v = qkv.reshape(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
        q, k, v = [t.clone().requires_grad_(True) for t in (q, k, v)]
        s = (q @ k.transpose(-2, -1)) * 0.125
        if causal:
            s = s + torch.full((N, N), float("-inf"), device=dev).triu_(1)
        lse = torch.logsumexp(s, -1).reshape(-1)
        o = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B * N, D)
        o.backward(do)
        grads = torch.cat([t.grad.transpose(1, 2).reshape(B * N, D) for t in (q, k, v)], 1)
        _REF[key] = (qkv.to(DEV), do.to(DEV), o.detach(), lse.detach(), grads.detach())
    return _REF[key]


def _check_fwd_bwd(B, H, N, causal=False, seed=34, qkv=None, o_buf=None, dqkv_buf=None):
    """Forward, then the backward from the reference's o and lse, with dbias, all held to the f32 bounds;
    ``qkv`` / ``o_buf`` / ``dqkv_buf`` replace the contiguous operands by views.  Returns (o, lse, dqkv, dbias)."""
    D = H * 64
    qkv_c, do, o_ref, lse_ref, g_ref = _case(B, H, N, causal, seed)
    qkv = qkv_c if qkv is None else qkv
    o, lse = ops.sdpa_fwd(qkv, B, H, N, o=o_buf, causal=causal)
    _close(o, o_ref, TO, "o")
    _close(lse, lse_ref, TL, "lse")
    dbias = torch.empty(3 * D, device=DEV)
    o_in = o_ref.to(DEV)
    if o_buf is not None:  # the backward reads o at the same stride
        o_in = torch.empty(B * N, o_buf.stride(0), device=DEV)[:, :D]
        o_in.copy_(o_ref)
    dqkv = ops.sdpa_bwd(qkv, o_in, do, lse_ref.to(DEV), B, H, N, dqkv=dqkv_buf, dbias=dbias, causal=causal)
    g = dqkv.float().cpu()
    for i, name in enumerate(("dq", "dk", "dv")):
        _close(g[:, i * D:(i + 1) * D], g_ref[:, i * D:(i + 1) * D].cpu(), TG, name)
    _close(dbias, g_ref.sum(0), TG, "qkv bias grad")
    return o, lse, dqkv, dbias


# 289: first past the limit, 33 keys in the last chunk, ragged third query block; 320: chunk multiple;
# 384: three full 128-blocks; 577 = 9 * 64 + 1: one valid key in the last chunk
@pytest.mark.parametrize("N", [289, 320, 384, 577])
def test_sdpa_long_f32_counter(N):
    c0, b0 = _count(), _count_bf16()
    _check_fwd_bwd(2, 3, N)
    assert _count() - c0 == 2  # one forward call + one backward call
    assert _count_bf16() == b0


def test_sdpa_long_f32_streamed_vs_generic_and_repeatable():
    B, H, N = 2, 3, 577
    lib = L.lib()
    runs = []
    try:
        for mode in (1, 1, 0):
            lib.vit_sdpa_long_config(mode)
            c0 = _count()
            out = _check_fwd_bwd(B, H, N)  # both modes hold the fp32 reference bounds
            torch.cuda.synchronize()
            assert _count() - c0 == (2 if mode else 0)
            runs.append([t.clone() for t in out])
    finally:
        lib.vit_sdpa_long_config(-1)
    for a, b, name in zip(runs[0], runs[1], ("o", "lse", "dqkv", "dbias")):
        assert torch.equal(a, b), f"{name}: two streamed runs differ"


def test_sdpa_long_f32_fallbacks():
    lib = L.lib()
    # causal past 288 tokens: the generic kernels
    c0 = _count()
    _check_fwd_bwd(3, 2, 300, causal=True, seed=44)
    assert _count() == c0
    # row strides that are no multiple of 4 elements: the generic kernels
    B, H, N = 2, 3, 289
    D = H * 64
    qkv_c = _case(B, H, N)[0]
    qkv = torch.empty(B * N, 3 * D + 2, device=DEV)[:, :3 * D]
    qkv.copy_(qkv_c)
    o_buf = torch.empty(B * N, D + 2, device=DEV)[:, :D]
    assert qkv.stride(0) % 4 and o_buf.stride(0) % 4
    _check_fwd_bwd(B, H, N, qkv=qkv, o_buf=o_buf)
    assert _count() == c0
    # N = 288 is the resident kernels' whatever the long-sequence mode says
    B, H, N = 2, 3, 288
    qkv, do, o_ref, lse_ref, _ = _case(B, H, N)
    outs = []
    try:
        for mode in (1, 0):
            lib.vit_sdpa_long_config(mode)
            o, lse = ops.sdpa_fwd(qkv, B, H, N)
            dqkv = ops.sdpa_bwd(qkv, o, do, lse, B, H, N)
            torch.cuda.synchronize()
            outs.append((o.clone(), lse.clone(), dqkv.clone()))
    finally:
        lib.vit_sdpa_long_config(-1)
    assert _count() == c0
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    _close(outs[0][0], o_ref, TO, "o")


def test_sdpa_long_f32_strided_output():
    """o and dqkv as views into wider buffers (row strides D + 8 and 3D + 8): the contiguous call's bits, and
    nothing written outside the views."""
    B, H, N = 2, 3, 577
    D = H * 64
    SENT = -12345.0
    c0 = _count()
    ref = _check_fwd_bwd(B, H, N)
    o_w = torch.full((B * N, D + 8), SENT, device=DEV)
    dq_w = torch.full((B * N, 3 * D + 8), SENT, device=DEV)
    got = _check_fwd_bwd(B, H, N, o_buf=o_w[:, :D], dqkv_buf=dq_w[:, :3 * D])
    torch.cuda.synchronize()
    assert _count() - c0 == 4
    for a, b, name in zip(ref, got, ("o", "lse", "dqkv", "dbias")):
        assert torch.equal(a, b), f"{name}: strided and contiguous calls differ"
    assert got[0].data_ptr() == o_w.data_ptr() and got[2].data_ptr() == dq_w.data_ptr()
    assert (o_w[:, D:] == SENT).all() and (dq_w[:, 3 * D:] == SENT).all()


def test_sdpa_long_f32_large_grid_per_head():
    """480 (b, h) items x 3 query blocks (more than one round of workgroups), each item checked on its own."""
    B, H, N = 40, 12, 289
    D = H * 64
    qkv, do, o_ref, lse_ref, ref = _case(B, H, N, seed=36, dev=DEV)
    dbias = torch.empty(3 * D, device=DEV)
    c0 = _count()
    dqkv = ops.sdpa_bwd(qkv, o_ref, do, lse_ref, B, H, N, dbias=dbias)
    assert _count() - c0 == 1
    _close(dqkv, ref, TG, "dqkv")
    _close(dbias, ref.sum(0), TG, "qkv bias grad")
    err = (dqkv - ref).reshape(B, N, 3, H, 64).permute(0, 3, 2, 1, 4).reshape(B * H, -1)
    scl = ref.reshape(B, N, 3, H, 64).permute(0, 3, 2, 1, 4).reshape(B * H, -1)
    worst = (err.norm(dim=1) / scl.norm(dim=1).clamp_min(1e-6)).max().item()
    print(f"worst (b, h) item rel err {worst:.3e}")
    assert worst < 1e-4, f"worst (b, h) item rel err {worst}"


def test_vit_f32_290_tokens_takes_streamed_kernels():
    """The oracle comparison at these shapes is test_gpu_attention_long.test_model_290_tokens_matches_oracle[F32];
    here: the f32 model's forward + CE + backward reach the streamed f32 kernels."""
    import vit_amd
    torch.manual_seed(3)
    m = vit_amd.VisionTransformer(img_size=272, patch_size=16, embed_dim=128, depth=2, num_heads=2, num_classes=10,
                                  compute_dtype=F32).to(DEV)
    g = torch.Generator().manual_seed(22)
    x = torch.randn(3, 3, 272, 272, generator=g).to(DEV)
    y = torch.randint(0, 10, (3,), generator=g).to(DEV)
    c0, b0 = _count(), _count_bf16()
    loss = vit_amd.cross_entropy(m(x), y)
    loss.backward()
    torch.cuda.synchronize()
    assert _count() > c0 and _count_bf16() == b0
    assert torch.isfinite(loss)
    for k, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k


def test_clip_hba_290_tokens_matches_oracle():
    """CLIP-HBA + DoRA (two visual layers, one text layer) on a tiny CLIP with 17 x 17 + 1 = 290 visual tokens,
    fp32, B = 3: predictions, MSE loss and every DoRA gradient within 1e-3 relative of oracle.clip_ref's CPU
    step (test_clip_hba_step_matches_golden's f32 bound)."""
    import vit_amd
    from oracle import clip_ref as CR
    from vit_amd import clip
    t = CR.CLIP_TINY
    cfg = CR.CLIPConfig(image_resolution=136, vision_patch=8, vision_width=128, vision_layers=3, vision_heads=2,
                        embed_dim=t.embed_dim, context_length=t.context_length, vocab_size=t.vocab_size,
                        text_width=t.text_width, text_layers=t.text_layers, text_heads=t.text_heads)
    assert cfg.vision_tokens == 290
    B, T, r = 3, 5, 8
    p = CR.init_params(cfg, seed=15)
    prompts = CR.synthetic_prompts(T, cfg, seed=16)
    cm = clip.build_model(p, compute_dtype=F32)
    assert tuple(cm.visual.positional_embedding.shape) == (290, 128)
    m = vit_amd.CLIPHBA([f"c{i}" for i in range(T)], "ViT-L/14", pos_embedding=True, clip_model=cm,
                        tokenized_prompts=prompts)
    vit_amd.apply_dora_to_ViT(m, n_vision_layers=2, n_transformer_layers=1, r=r)
    vit_amd.switch_dora_layers(m, freeze_all=True, dora_state=True)
    sd = m.state_dict()
    d = CR.init_dora(p, cfg, r=r, seed=0)
    for k in list(d):
        if not k.endswith(".scaling"):  # the oracle's parameters with the product's own A / B draw
            if k.endswith(".m") or k.endswith(".D"):
                assert _rel(sd[k], d[k]) < 1e-6, k
            d[k] = sd[k].detach().clone().float()
    g = torch.Generator().manual_seed(17)
    x = torch.randn(B, 3, 136, 136, generator=g)
    y = torch.randn(B, T, generator=g) * 0.5 + 1.0
    ref_loss, ref_pred, ref_grads = CR.train_step(p, d, {}, x, prompts, y, cfg, lr=3e-4, pos_embedding=True)

    m = m.cuda()
    c0 = _count()
    pred = m(x.cuda())
    loss = vit_amd.mse_loss(pred, y.cuda())
    loss.backward()
    torch.cuda.synchronize()
    assert _count() > c0
    grads = {n: q.grad.detach().cpu() for n, q in m.named_parameters() if q.requires_grad}
    assert len(grads) == 9 and sorted(grads) == sorted(ref_grads)
    print("pred rel", _rel(pred, ref_pred), "loss", float(loss.detach()), ref_loss)
    assert _rel(pred, ref_pred) < 1e-3
    assert abs(float(loss.detach()) - ref_loss) <= 1e-3 * abs(ref_loss)
    for k, rg in ref_grads.items():
        print(k, _rel(grads[k], rg))
        assert _rel(grads[k], rg) < 1e-3, (k, _rel(grads[k], rg))


def test_clip_l14_336_step_runs_and_refuses_fp8():
    import vit_amd
    from vit_amd import clip
    cm = clip.CLIP(**{**clip._BACKBONES["ViT-L/14@336px"], "vision_layers": 2, "transformer_layers": 1})
    assert tuple(cm.visual.positional_embedding.shape) == (577, 1024)
    m = vit_amd.CLIPHBA(["x%d" % i for i in range(6)], "ViT-L/14@336px", pos_embedding=True, clip_model=cm)
    vit_amd.apply_dora_to_ViT(m, n_vision_layers=2, n_transformer_layers=1, r=32)
    vit_amd.switch_dora_layers(m, freeze_all=True, dora_state=True)
    m = m.cuda()
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3, 336, 336, generator=g).to(DEV)
    y = torch.randn(2, 6, generator=g).to(DEV)
    c0 = _count()
    pred = m(x)
    loss = vit_amd.mse_loss(pred, y)
    loss.backward()
    torch.cuda.synchronize()
    assert _count() > c0
    assert tuple(pred.shape) == (2, 6) and torch.isfinite(pred).all() and torch.isfinite(loss)
    with_grad = {n: q.grad for n, q in m.named_parameters() if q.grad is not None}
    assert len(with_grad) == 9 and all(torch.isfinite(gr).all() for gr in with_grad.values())
    m.clip_model.set_attention_fp8(True)
    with torch.no_grad(), pytest.raises(ValueError, match="320"):
        m(x)
    m.clip_model.set_attention_fp8(False)
