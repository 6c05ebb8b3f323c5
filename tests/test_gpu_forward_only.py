"""GPU: the forward-only path -- act-only fc1 epilogues and the block chain that uses them.

Everything here is an equality: the act-only epilogue must store, bit for bit, what the pair epilogue
stores into act_out on the same kernel path, and a forward-only pass must reproduce the training
chain's outputs bit for bit.
"""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import clip_ref as CR  # noqa: E402
from vit_amd import _lib as L  # noqa: E402
from vit_amd import ops  # noqa: E402

DEV = "cuda"
SENTINEL = -7.0  # exact in bf16; no GELU / QuickGELU output is below -0.2
PAIR_CODES = (L.EPI_BIAS_GELU, L.EPI_BIAS_QGELU)
FWD_CODES = (L.EPI_BIAS_GELU_FWD, L.EPI_BIAS_QGELU_FWD)


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    L.load()


def _rnd(*shape, dtype=torch.float32, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(DEV)


def _padded(M, N, dtype):
    """An [M + 3, N + 8] sentinel-filled buffer; the GEMM output is its [:M, :N] corner."""
    return torch.full((M + 3, N + 8), SENTINEL, dtype=dtype, device=DEV)


def _sentinel_intact(buf, M, N):
    return bool((buf[:M, N:] == SENTINEL).all()) and bool((buf[M:] == SENTINEL).all())


def _linear(epi, x, w, b, y, act_out):
    M, K = x.shape
    N = w.shape[0]
    L.call("vit_linear_fwd", L.dt(x), L.dt(y), epi, M, N, K, L.ptr(x), x.stride(0), L.ptr(w), L.ptr(b), L.ptr(y),
           y.stride(0), None, L.ptr(act_out), L.stream_ptr(x.device))


_BF16_SHAPES = [(591, 640, 448), (1000, 3072, 768), (257, 136, 192), (1, 64, 64), (300, 1088, 128)]
_CASES = ([(torch.bfloat16, s, -1) for s in _BF16_SHAPES]
          + [(torch.bfloat16, s, v) for s in ((591, 640, 448), (1000, 3072, 768)) for v in (1, 5)]
          + [(torch.float32, s, -1) for s in ((591, 640, 448), (1024, 768, 96), (300, 132, 64))]
          # beyond the issue's list: enough 128 x 128 tiles for the dispatcher to pick the f32 MFMA kernel
          + [(torch.float32, (1100, 1024, 64), -1)])


@pytest.mark.parametrize("dtype,shape,variant", _CASES,
                         ids=[f"{str(d)[6:]}-{'x'.join(map(str, s))}-v{v}" for d, s, v in _CASES])
@pytest.mark.parametrize("pair,fwd", list(zip(PAIR_CODES, FWD_CODES)), ids=["gelu", "qgelu"])
def test_act_only_epilogue_bitwise_matches_pair(dtype, shape, variant, pair, fwd):
    M, N, K = shape
    x = _rnd(M, K, dtype=dtype, seed=1)
    w = _rnd(N, K, dtype=dtype, seed=2, scale=K ** -0.5)
    b = _rnd(N, seed=3, scale=0.5)
    if dtype == torch.float32:
        ops._streamk(x.device)  # as ops.linear_fwd does for f32 operands: both calls see the same workspace
    dact, act, only = _padded(M, N, dtype), _padded(M, N, dtype), _padded(M, N, dtype)
    lib = L.lib()
    try:
        if variant >= 0:
            lib.vit_gemm_variant(variant)
        _linear(pair, x, w, b, dact, act)
        _linear(fwd, x, w, b, only, None)  # act_out NULL: the act-only codes write Y alone
        torch.cuda.synchronize()
    finally:
        lib.vit_gemm_variant(-1)
    assert _sentinel_intact(act, M, N) and _sentinel_intact(dact, M, N)
    assert _sentinel_intact(only, M, N), "the act-only epilogue wrote outside its [M, N] output"
    assert torch.isfinite(only[:M, :N].float()).all()
    assert not bool((only[:M, :N] == SENTINEL).any()), "output elements left unwritten"
    assert torch.equal(only[:M, :N], act[:M, :N])


# ---------------------------------------------------------------------------- block chain

class _Spy:
    """Records (epilogue code, weight pointer) of every ops.linear_fwd call."""

    def __init__(self, monkeypatch):
        self.calls = []
        real = ops.linear_fwd

        def spy(x2d, w, bias=None, epi=L.EPI_STORE, **kw):
            self.calls.append((epi, w.data_ptr()))
            return real(x2d, w, bias, epi=epi, **kw)

        monkeypatch.setattr(ops, "linear_fwd", spy)

    def take(self):
        c, self.calls = self.calls, []
        return c

    @staticmethod
    def fc1_codes(calls):
        return [e for e, _ in calls if e in PAIR_CODES + FWD_CODES]


@pytest.fixture
def fwd_only_switch():
    import vit_amd
    prev = vit_amd.set_forward_only(True)
    yield vit_amd.set_forward_only
    vit_amd.set_forward_only(prev)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("B", [1, 3])
def test_forward_only_pass_matches_training_chain(B, dtype, monkeypatch, fwd_only_switch):
    import vit_amd
    torch.manual_seed(5)
    m = vit_amd.VisionTransformer(img_size=64, patch_size=16, embed_dim=256, depth=2, num_heads=4, num_classes=10,
                                  compute_dtype=dtype).cuda()
    x = _rnd(B, 3, 64, 64, seed=7)
    spy = _Spy(monkeypatch)
    with torch.no_grad():
        fwd_only_switch(True)
        y_on, f_on = m(x), m.forward_features(x)
        codes_on = spy.fc1_codes(spy.take())
        fwd_only_switch(False)
        y_off, f_off = m(x), m.forward_features(x)
        codes_off = spy.fc1_codes(spy.take())
    fwd_only_switch(True)
    y_grad = m(x)  # grad enabled, trainable parameters: the autograd node's chain
    codes_grad = spy.fc1_codes(spy.take())
    torch.cuda.synchronize()
    assert codes_on and set(codes_on) == {L.EPI_BIAS_GELU_FWD}, codes_on
    assert codes_off and set(codes_off) == {L.EPI_BIAS_GELU}, codes_off
    assert codes_grad and set(codes_grad) == {L.EPI_BIAS_GELU}, codes_grad
    assert len(codes_on) == len(codes_off) == 2 * len(codes_grad)  # the same launches, two passes vs one
    assert y_grad.requires_grad and not y_on.requires_grad
    assert torch.equal(y_on, y_off) and torch.equal(f_on, f_off)
    assert torch.equal(y_on, y_grad.detach())


def _tiny_hba(gold, dtype):
    """tests/test_clip.py's tiny CLIP-HBA, rebuilt from the same golden fixture."""
    import vit_amd
    from vit_amd import clip
    cfg = CR.CLIP_TINY
    cm = clip.CLIP(embed_dim=cfg.embed_dim, image_resolution=cfg.image_resolution, vision_layers=cfg.vision_layers,
                   vision_width=cfg.vision_width, vision_patch_size=cfg.vision_patch,
                   context_length=cfg.context_length, vocab_size=cfg.vocab_size, transformer_width=cfg.text_width,
                   transformer_heads=cfg.text_heads, transformer_layers=cfg.text_layers, compute_dtype=dtype)
    cm.load_state_dict(CR.init_params(cfg, seed=gold["seed"]), strict=True)
    m = vit_amd.CLIPHBA([f"c{i}" for i in range(gold["T"])], "ViT-L/14", pos_embedding=True, clip_model=cm,
                        tokenized_prompts=gold["prompts"])
    vit_amd.apply_dora_to_ViT(m, n_vision_layers=2, n_transformer_layers=1, r=gold["r"], dora_dropout=0.1)
    vit_amd.switch_dora_layers(m, freeze_all=True, dora_state=True)
    with torch.no_grad():
        for n, q in m.named_parameters():
            if n.endswith(".delta_D_A"):
                q.copy_(gold["dora_A_init"][n])
            elif n.endswith(".delta_D_B"):
                q.copy_(gold["dora_B_init"][n])
    return m


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_cliphba_frozen_prefix_is_forward_only_and_exact(dtype, golden_dir, monkeypatch, fwd_only_switch):
    import vit_amd
    from vit_amd.clip import _first_trainable
    gold = torch.load(os.path.join(golden_dir, "clip_golden.pt"), weights_only=True)
    m = _tiny_hba(gold, dtype).cuda()
    m.clip_model.cache_frozen_text = False  # both steps run the text prefix
    img, tgt = gold["image"].cuda(), gold["target"].cuda()
    spy = _Spy(monkeypatch)

    def step(on):
        fwd_only_switch(on)
        torch.manual_seed(3)
        m.zero_grad(set_to_none=True)
        loss = vit_amd.MSELoss()(m(img), tgt)
        loss.backward()
        torch.cuda.synchronize()
        return (loss.detach().clone(), {n: q.grad.detach().clone() for n, q in m.named_parameters() if q.requires_grad},
                spy.take())

    loss_on, grads_on, calls_on = step(True)
    loss_off, grads_off, calls_off = step(False)
    assert grads_on and grads_on.keys() == grads_off.keys()
    assert torch.equal(loss_on, loss_off)
    for n in grads_on:
        assert torch.equal(grads_on[n], grads_off[n]), n

    def fc1_ptrs(blk):  # the GEMM operand of fc1: the weight itself (f32) or its bf16 shadow
        w = blk.mlp.c_fc.weight
        sh = getattr(w, "_vit_shadow", None)
        return {w.data_ptr()} if sh is None else {w.data_ptr(), sh.data_ptr()}

    fwd_ptrs = {p for e, p in calls_on if e in FWD_CODES}
    pair_ptrs = {p for e, p in calls_on if e in PAIR_CODES}
    frozen, rest = set(), set()
    for tower in (m.clip_model.visual.transformer, m.clip_model.transformer):
        blocks = list(tower.resblocks)
        first = _first_trainable(blocks)
        assert 0 < first < len(blocks)
        for i, blk in enumerate(blocks):
            (frozen if i < first else rest).update(fc1_ptrs(blk))
            # every block in front of the first trainable one took the act-only code, every other the pair
            assert fc1_ptrs(blk) & (fwd_ptrs if i < first else pair_ptrs), (i, first)
    assert fwd_ptrs <= frozen and pair_ptrs <= rest
    assert {e for e, _ in calls_on} >= {L.EPI_BIAS_QGELU_FWD, L.EPI_BIAS_QGELU}
    assert not [e for e, _ in calls_off if e in FWD_CODES]
