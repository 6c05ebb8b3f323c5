"""GPU: attention past the resident kernels' 288-token limit.

bf16, non-causal, aligned operands take the streamed MFMA kernels (K / V, or Q / dO, pass through a
double-buffered LDS ring of 64-row chunks); f32 and causal take the generic scalar kernels.  References
are torch fp32 autograd; tolerances are test_gpu_kernels.test_sdpa_fwd_bwd's for the same quantities
(bf16: o 1.5e-2, lse 2e-3, gradients 3e-2; f32: o / lse 1e-5, gradients 1e-4, relative to the
reference's scale).  ``vit_sdpa_long_count`` counts the vit_sdpa_fwd / vit_sdpa_bwd calls that took the
streamed kernels (one per call).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from vit_amd import _lib as L  # noqa: E402
from vit_amd import ops  # noqa: E402

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32


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


def _tols(dtype):
    """(o, lse, gradients)"""
    return (1e-5, 1e-5, 1e-4) if dtype == F32 else (1.5e-2, 2e-3, 3e-2)


def _count():
    return L.lib().vit_sdpa_long_count(0)


_REF = {}


def _case(B, H, N, dtype, causal=False, seed=34, dev="cpu"):
    """Inputs and the torch fp32 reference (o, lse, [dq | dk | dv]) of one shape; computed once and shared."""
    key = (B, H, N, dtype, causal, seed, dev)
    if key not in _REF:
        D = H * 64
        g = torch.Generator().manual_seed(seed)
        qkv = (torch.randn(B * N, 3 * D, generator=g) * 1.5).to(dtype).to(dev)
        do = torch.randn(B * N, D, generator=g).to(dtype).to(dev)
        q, k, v = qkv.float().reshape(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
        q, k, v = [t.clone().requires_grad_(True) for t in (q, k, v)]
        s = (q @ k.transpose(-2, -1)) * 0.125
        if causal:
            s = s + torch.full((N, N), float("-inf"), device=dev).triu_(1)
        lse = torch.logsumexp(s, -1).reshape(-1)
        o = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B * N, D)
        o.backward(do.float())
        grads = torch.cat([t.grad.transpose(1, 2).reshape(B * N, D) for t in (q, k, v)], 1)
        _REF[key] = (qkv.to(DEV), do.to(DEV), o.detach(), lse.detach(), grads.detach())
    return _REF[key]


def _check_fwd_bwd(B, H, N, dtype, causal=False, seed=34):
    """Forward, then the backward from the reference's o and lse, with dbias; returns (o, lse, dqkv, dbias)."""
    D = H * 64
    qkv, do, o_ref, lse_ref, g_ref = _case(B, H, N, dtype, causal, seed)
    to, tl, tg = _tols(dtype)
    o, lse = ops.sdpa_fwd(qkv, B, H, N, causal=causal)
    _close(o, o_ref, to, "o")
    _close(lse, lse_ref, tl, "lse")
    dbias = torch.empty(3 * D, device=DEV)
    dqkv = ops.sdpa_bwd(qkv, o_ref.to(dtype).to(DEV), do, lse_ref.to(DEV), B, H, N, dbias=dbias, causal=causal)
    g = dqkv.float().cpu()
    for i, name in enumerate(("dq", "dk", "dv")):
        _close(g[:, i * D:(i + 1) * D], g_ref[:, i * D:(i + 1) * D].cpu(), tg, name)
    _close(dbias, g_ref.sum(0), tg, "qkv bias grad")
    return o, lse, dqkv, dbias


# 289: first past the limit; 320, 384: chunk multiples; 577 = 9*64 + 1 and 1025 = 16*64 + 1: one valid
# key in the last chunk; 289, 513, 577, 1025: ragged last 128-query block
@pytest.mark.parametrize("N", [289, 320, 384, 513, 577, 1025])
@pytest.mark.parametrize("dtype", [BF16, F32])
def test_sdpa_long_fwd_bwd(N, dtype):
    c0 = _count()
    _check_fwd_bwd(2, 3, N, dtype)
    # one forward call + one backward call
    assert _count() - c0 == (2 if dtype == BF16 else 0)


def test_sdpa_long_large_grid_per_head():
    """480 (b, h) items (more than 256 CUs x one round), each checked on its own."""
    B, H, N = 40, 12, 289
    D = H * 64
    qkv, do, o_ref, lse_ref, ref = _case(B, H, N, BF16, seed=36, dev=DEV)
    dbias = torch.empty(3 * D, device=DEV)
    c0 = _count()
    dqkv = ops.sdpa_bwd(qkv, o_ref.to(BF16), do, lse_ref, B, H, N, dbias=dbias)
    assert _count() - c0 == 1
    _close(dqkv.float(), ref, 3e-2, "dqkv")
    _close(dbias, ref.sum(0), 3e-2, "qkv bias grad")
    err = (dqkv.float() - ref).reshape(B, N, 3, H, 64).permute(0, 3, 2, 1, 4).reshape(B * H, -1)
    scl = ref.reshape(B, N, 3, H, 64).permute(0, 3, 2, 1, 4).reshape(B * H, -1)
    worst = (err.norm(dim=1) / scl.norm(dim=1).clamp_min(1e-6)).max().item()
    print(f"worst (b, h) item rel err {worst:.3e}")
    assert worst < 3e-2, f"worst (b, h) item rel err {worst}"


def test_sdpa_long_partial_only_mode():
    """dbias == NULL with a partial buffer (what every bf16 block backward uses): the per-image [B][3D]
    partials reduced by the ColBatch against the reference and against the dbias path of the same call."""
    B, H, N = 3, 2, 577
    D = H * 64
    qkv, do, o_ref, lse_ref, ref = _case(B, H, N, BF16)
    args = (qkv, o_ref.to(BF16).to(DEV), do, lse_ref.to(DEV), B, H, N)
    direct = torch.empty(3 * D, device=DEV)
    d0 = ops.sdpa_bwd(*args, dbias=direct)
    g = torch.full((3 * D,), float("nan"), device=DEV)
    rb = ops.ColBatch()
    d1 = ops.sdpa_bwd(*args, dbias=g, reduce_on=rb)
    rb.launch()
    torch.cuda.synchronize()
    assert torch.equal(d0, d1)
    _close(g, ref.sum(0), 3e-2, "ColBatch bias grad vs reference")
    _close(g, direct, 2e-4, "ColBatch bias grad vs dbias path")


def test_sdpa_long_streamed_vs_generic_and_repeatable():
    B, H, N = 2, 3, 577
    lib = L.lib()
    runs = []
    try:
        for mode in (1, 1, 0):
            lib.vit_sdpa_long_config(mode)
            c0 = _count()
            out = _check_fwd_bwd(B, H, N, BF16)  # both modes hold the fp32 reference tolerances
            torch.cuda.synchronize()
            assert _count() - c0 == (2 if mode else 0)
            runs.append([t.clone() for t in out])
        assert lib.vit_sdpa_long_config(-1) == 0  # returns the previous mode
    finally:
        lib.vit_sdpa_long_config(-1)
    for a, b, name in zip(runs[0], runs[1], ("o", "lse", "dqkv", "dbias")):
        assert torch.equal(a, b), f"{name}: two streamed runs differ"


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_sdpa_long_causal(dtype):
    """Causal past 288 tokens takes the generic kernels (no streamed causal form)."""
    c0 = _count()
    _check_fwd_bwd(3, 2, 300, dtype, causal=True, seed=44)
    assert _count() == c0


def test_sdpa_resident_boundary_untouched():
    """N = 288 is the resident kernels' whatever the long-sequence mode says."""
    B, H, N = 2, 3, 288
    qkv, do, o_ref, lse_ref, _ = _case(B, H, N, BF16)
    lib = L.lib()
    outs = []
    c0 = _count()
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
    _close(outs[0][0], o_ref, 1.5e-2, "o")


# ---------------------------------------------------------------------------- whole model

def _rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return (a - b).abs().max().item() / (b.abs().max().item() + 1e-30)


@pytest.fixture(scope="module")
def tiny290():
    """290 tokens (17 x 17 patches + cls), B = 3 (ragged half-batch chains): the CPU fp32 oracle's step."""
    from oracle import vit_ref as R
    cfg = R.ViTConfig(img_size=272, patch_size=16, embed_dim=128, depth=2, num_heads=2, num_classes=10)
    p = R.init_params(cfg, seed=21, random_affine=True)
    g = torch.Generator().manual_seed(22)
    x = torch.randn(3, 3, 272, 272, generator=g)
    y = torch.randint(0, 10, (3,), generator=g)
    leaf = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    logits = R.forward(leaf, x, cfg)
    loss = R.cross_entropy(logits, y)
    loss.backward()
    return cfg, p, x, y, logits.detach(), float(loss.detach()), {k: v.grad.detach() for k, v in leaf.items()}


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_model_290_tokens_matches_oracle(tiny290, dtype):
    """Bounds of tests/test_gpu_parity.py: f32 1e-3 relative on logits, loss and every gradient; bf16
    logits 3e-2 of scale with cosine > 0.999, loss 2e-2, every gradient's norm within 10 %."""
    import vit_amd
    cfg, p, x, y, ref_logits, ref_loss, ref_grads = tiny290
    m = vit_amd.VisionTransformer(img_size=272, patch_size=16, embed_dim=128, depth=2, num_heads=2, num_classes=10,
                                  compute_dtype=dtype)
    m.load_state_dict(p)
    m = m.to(DEV)
    c0 = _count()
    logits = m(x.to(DEV))
    loss = vit_amd.cross_entropy(logits, y.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: v.grad for k, v in m.named_parameters()}
    print("logits rel", _rel(logits, ref_logits), "loss", loss.item(), ref_loss)
    if dtype == F32:
        assert _count() == c0
        assert _rel(logits, ref_logits) < 1e-3
        assert abs(loss.item() - ref_loss) < 1e-3 * abs(ref_loss)
        for k, g in grads.items():
            assert _rel(g, ref_grads[k]) < 1e-3, k
    else:
        assert _count() > c0
        assert _rel(logits, ref_logits) < 3e-2
        cos = torch.nn.functional.cosine_similarity(logits.detach().cpu().flatten(), ref_logits.flatten(), dim=0)
        assert cos.item() > 0.999
        assert abs(loss.item() - ref_loss) < 2e-2
        for k, g in grads.items():
            n = ref_grads[k].norm().item()
            assert abs(g.norm().item() - n) <= 0.1 * n + 1e-9, k


def test_vit_base_384_runs_and_refuses_fp8():
    import vit_amd
    m = vit_amd.create_model("vit_base_patch16_384", num_classes=10, depth=1).to(DEV)
    assert m.pos_embed.shape == (1, 577, 768)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3, 384, 384, generator=g).to(DEV)
    y = torch.tensor([1, 7], device=DEV)
    c0 = _count()
    logits = m(x)
    loss = vit_amd.cross_entropy(logits, y)
    loss.backward()
    torch.cuda.synchronize()
    assert _count() > c0
    assert torch.isfinite(logits).all() and torch.isfinite(loss)
    for k, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
    m.set_attention_fp8(True)
    with torch.no_grad(), pytest.raises(ValueError, match="320"):
        m(x)
    m.set_attention_fp8(False)
    with torch.no_grad():
        assert torch.isfinite(m(x)).all()
