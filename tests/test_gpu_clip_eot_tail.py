"""GPU: the EOT tail of the CLIP text tower (``CLIP.set_eot_tail`` / ``CLIPHBA(eot_tail=True)``): the
tower's last block computed for the EOT rows alone, its attention by the one-query kernel at a row per prompt.

Configurations: oracle/clip_ref.py's CLIP_TINY (context length 16: below TAIL_PAD, the backward's rows are padded to
the context length) and the same at context length 77 (the 64-row padded backward); five prompts of unequal lengths,
so the EOT positions differ; DoRA or LoRA on the last two visual blocks and one text block; f32 and bf16 (five
prompts: the bf16 half-batch split is 2 + 3).

Bounds, all the project's (tests/test_gpu_clip_cls_tail.py), none fitted to the new code.  The tail's GEMM and
LayerNorm rows are the dense block's; the one-query attention sums in another order than the MFMA kernels, so switch
on against switch off agrees to rounding: f32 1e-3 relative (predictions and every gradient), bf16 predictions 3e-2
relative, gradients cosine >= 0.99 and norm within 5 %.  f32 also against the float64 oracle (1e-3), and every
adapter gradient's error against the oracle with the tail on is at most 2x the error with it off on the same
inputs, plus 2^-22.  The measured figures are printed before they are asserted.

The visual tower: the switch reaches no visual launch, so image features and their gradients (a loss on
``encode_image`` alone) are bitwise those of switch-off.  Through the logits they cannot be: the text features the
image gradient is multiplied by differ by rounding."""
import csv
import dataclasses
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

from oracle import clip_ref as CR

pytestmark = pytest.mark.gpu

CFGS = {16: CR.CLIP_TINY, 77: dataclasses.replace(CR.CLIP_TINY, context_length=77)}
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["f32", "bf16"]
B, T, RANK = 3, 5, 8
FLOOR = 2.0 ** -22
_REF = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@dataclasses.dataclass
class SimpleCase:
    cfg: object
    p: object
    d: object
    prompts: object
    img: object
    tgt: object
    pred: object
    grads: object


def _case(n):
    """Parameters, DoRA state, prompts, inputs and the float64 oracle's predictions / DoRA gradients for the model
    of context length n; computed once and left unchanged."""
    if n not in _REF:
        cfg = CFGS[n]
        assert cfg.context_length == n
        p = CR.init_params(cfg, seed=60 + n)
        d = CR.init_dora(p, cfg, r=RANK, seed=0)
        prompts = CR.synthetic_prompts(T, cfg, seed=4)
        assert len(set(prompts.reshape(T, n).argmax(-1).tolist())) >= 3, "the EOT positions must differ"
        g = torch.Generator().manual_seed(70 + n)
        img = torch.randn(B, 3, cfg.image_resolution, cfg.image_resolution, generator=g)
        tgt = torch.randn(B, T, generator=g) * 0.5 + 2.0
        keys = CR.trainable_keys(d)
        leaf = OrderedDict((k, v.double().requires_grad_(True) if k in keys else (v.double() if torch.is_tensor(v) else v))
                           for k, v in d.items())
        pred = CR.forward({k: v.double() for k, v in p.items()}, img.double(), prompts, cfg, leaf, True)
        torch.nn.functional.mse_loss(pred, tgt.double()).backward()
        _REF[n] = SimpleCase(cfg, p, d, prompts, img, tgt, pred.detach(),
                             OrderedDict((k, leaf[k].grad.detach()) for k in keys))
    return _REF[n]


def _clip(cfg, p, dtype):
    from vit_amd import clip
    cm = clip.CLIP(embed_dim=cfg.embed_dim, image_resolution=cfg.image_resolution, vision_layers=cfg.vision_layers,
                   vision_width=cfg.vision_width, vision_patch_size=cfg.vision_patch,
                   context_length=cfg.context_length, vocab_size=cfg.vocab_size, transformer_width=cfg.text_width,
                   transformer_heads=cfg.text_heads, transformer_layers=cfg.text_layers, compute_dtype=dtype)
    cm.load_state_dict(p, strict=True)
    return cm


def _hba(n, dtype, tail, adapter="dora", cls_tail=False, text_blocks=1):
    """CLIPHBA on the model of context length n with the oracle's DoRA factors (dora_dropout 0: the oracle has no
    dropout), or with LoRA adapters."""
    import vit_amd
    c = _case(n)
    m = vit_amd.CLIPHBA([f"c{i}" for i in range(T)], "ViT-L/14", pos_embedding=True, clip_model=_clip(c.cfg, c.p, dtype),
                        tokenized_prompts=c.prompts, eot_tail=tail, cls_tail=cls_tail)
    assert m.clip_model.eot_tail is bool(tail) and m.clip_model.cls_tail is bool(cls_tail)
    if adapter == "lora":
        torch.manual_seed(9)
        vit_amd.apply_lora_to_ViT(m, n_vision_layers=2, n_transformer_layers=text_blocks, r=RANK, lora_dropout=0.0)
        vit_amd.unfreeze_lora_layers(m, freeze_all=True)
        with torch.no_grad():  # lora_B starts at zero: give both factors a gradient that depends on the other
            for name, q in m.named_parameters():
                if name.endswith(".lora_B"):
                    q.copy_(torch.randn(q.shape, generator=torch.Generator().manual_seed(len(name))) * 0.05)
        return m.cuda()
    vit_amd.apply_dora_to_ViT(m, n_vision_layers=2, n_transformer_layers=text_blocks, r=RANK, dora_dropout=0.0)
    vit_amd.switch_dora_layers(m, freeze_all=True, dora_state=True)
    with torch.no_grad():
        for name, q in m.named_parameters():
            if name.endswith((".delta_D_A", ".delta_D_B")) and name in c.d:
                q.copy_(c.d[name])
    return m.cuda()


def _count(reset=0):
    from vit_amd import _lib as L
    return L.lib().vit_sdpa_row1_count(reset)


def _step(m, x, target):
    """One forward + MSE backward in train mode; (prediction, gradients of the trainable parameters)."""
    import vit_amd
    m.train()
    for p in m.parameters():
        p.grad = None
    torch.manual_seed(0)
    pred = m(x)
    vit_amd.MSELoss()(pred, target).backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.requires_grad}
    assert grads and all(g is not None for g in grads.values())
    return pred.detach(), grads


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _check_pred(a, b, f32, what):
    r = _rel(a, b)
    print(f"{what}: relative difference {r:.3e}")
    assert r < (1e-3 if f32 else 3e-2), (what, r)


def _check_grad(a, b, f32, what):
    r = _rel(a, b)
    a, b = a.flatten().double().cpu(), b.flatten().double().cpu()
    cos = torch.nn.functional.cosine_similarity(a, b, dim=0).item()
    print(f"{what}: relative difference {r:.3e}, cosine {cos:.8f}")
    if f32:
        assert r < 1e-3, (what, r)
    else:
        assert cos >= 0.99 and abs(a.norm().item() / b.norm().item() - 1) <= 0.05, (what, cos)


def _launches(dtype):
    """One-query launches of one forward at five prompts: a bf16 forward runs two half-batch chains (2 + 3)."""
    return 2 if dtype == torch.bfloat16 else 1


def _short(name):
    return name.split("clip_model.")[-1]


# ---------------------------------------------------------------------------- 1. one training step

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", [16, 77])
def test_step_on_against_off_and_oracle(n, dtype, monkeypatch):
    from vit_amd import clip, ops
    c = _case(n)
    f32 = dtype == torch.float32
    img, tgt = c.img.cuda(), c.tgt.cuda()
    seen, embeds = [], []
    orig = clip._PoolHeadFn.forward
    orig_embed = ops.token_embed

    def spy(ctx, x, *a):
        seen.append(tuple(x.shape))
        return orig(ctx, x, *a)

    def spy_embed(*a):
        embeds.append(1)
        return orig_embed(*a)

    monkeypatch.setattr(clip._PoolHeadFn, "forward", staticmethod(spy))
    monkeypatch.setattr(ops, "token_embed", spy_embed)
    _count(1)
    m_off = _hba(n, dtype, False)
    pred_off, g_off = _step(m_off, img, tgt)
    _step(m_off, img, tgt)
    assert _count(1) == 0, "the switch is off: no one-query launch"
    hits_off = len(embeds)
    del embeds[:]
    m_on = _hba(n, dtype, True)
    pred_on, g_on = _step(m_on, img, tgt)
    assert _count(1) == _launches(dtype), "the tail did not run"
    pred_2, g_2 = _step(m_on, img, tgt)
    # the frozen text blocks' output is cached exactly as with the switch off: one miss, then hits
    assert hits_off == 1 and len(embeds) == 1
    assert torch.equal(pred_2, pred_on) and all(torch.equal(g_2[k], g_on[k]) for k in g_on)
    W = c.cfg.text_width
    assert seen[1] == (T, n, W) and seen[5] == (T, 1, W), seen  # the text pool head of each step (after the visual one)
    tag = f"L={n} {IDS[not f32]}"
    _check_pred(pred_on, pred_off, f32, f"{tag} prediction on/off")
    assert g_on.keys() == g_off.keys() == set(c.grads.keys())
    for k in g_off:
        _check_grad(g_on[k], g_off[k], f32, f"{tag} grad on/off {_short(k)}")
    if f32:
        _check_pred(pred_on, c.pred, True, f"{tag} prediction on/oracle")
        bad = []
        for k, ref in c.grads.items():
            e_off, e_on = _rel(g_off[k], ref), _rel(g_on[k], ref)
            print(f"{tag} grad/oracle {_short(k)}: dense {e_off:.3e} tail {e_on:.3e}")
            if not (e_on < 1e-3 and e_on <= 2.0 * e_off + FLOOR):
                bad.append((k, e_off, e_on))
        assert not bad, bad


# ---------------------------------------------------------------------------- 2. no-grad passes, the visual side

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", [16, 77])
def test_eval_pass_equals_the_training_forward(n, dtype):
    c = _case(n)
    f32 = dtype == torch.float32
    img, tgt = c.img.cuda(), c.tgt.cuda()
    m_off, m_on = _hba(n, dtype, False), _hba(n, dtype, True)
    pred_train, _ = _step(m_on, img, tgt)
    m_on.eval(), m_off.eval()
    _count(1)
    with torch.no_grad():
        p_off = m_off(img)
        assert _count(1) == 0
        p_on = m_on(img)
        assert _count(1) == _launches(dtype)  # the forward-only chain takes the tail too
    assert torch.equal(p_on, pred_train), "no_grad and the training forward differ"
    _check_pred(p_on, p_off, f32, f"L={n} {IDS[not f32]} eval prediction on/off")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_visual_side_is_bitwise_unchanged(dtype):
    n = 77
    c = _case(n)
    img = c.img.cuda()
    w = torch.randn(B, c.cfg.embed_dim, generator=torch.Generator().manual_seed(1)).cuda()
    res = []
    _count(1)
    for tail in (False, True):
        m = _hba(n, dtype, tail)
        f = m.clip_model.encode_image(img, True)
        (f * w).sum().backward()
        torch.cuda.synchronize()
        res.append((f.detach(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}))
    assert _count(1) == 0  # the image tower never takes the row tail
    (f0, g0), (f1, g1) = res
    assert torch.equal(f0, f1) and g0.keys() == g1.keys() and any(".visual." in k for k in g0)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k


# ---------------------------------------------------------------------------- 3. LoRA; two trainable text blocks

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", [16, 77])
def test_lora_step(n, dtype):
    c = _case(n)
    f32 = dtype == torch.float32
    img, tgt = c.img.cuda(), c.tgt.cuda()
    _count(1)
    pred_off, g_off = _step(_hba(n, dtype, False, "lora"), img, tgt)
    assert _count(1) == 0
    pred_on, g_on = _step(_hba(n, dtype, True, "lora"), img, tgt)
    assert _count(1) == _launches(dtype)
    assert g_on.keys() == g_off.keys() and all(k.endswith((".lora_A", ".lora_B")) for k in g_on)
    tag = f"lora L={n} {IDS[not f32]}"
    _check_pred(pred_on, pred_off, f32, f"{tag} prediction on/off")
    for k in g_off:
        _check_grad(g_on[k], g_off[k], f32, f"{tag} grad on/off {_short(k)}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_two_trainable_text_blocks_keep_the_dense_block(dtype):
    """The last block's input then needs a gradient: bit for bit the switch-off step."""
    n = 77
    c = _case(n)
    img, tgt = c.img.cuda(), c.tgt.cuda()
    _count(1)
    pred_off, g_off = _step(_hba(n, dtype, False, "lora", text_blocks=2), img, tgt)
    pred_on, g_on = _step(_hba(n, dtype, True, "lora", text_blocks=2), img, tgt)
    assert _count(1) == 0
    assert torch.equal(pred_on, pred_off) and g_on.keys() == g_off.keys()
    for k in g_off:
        assert torch.equal(g_on[k], g_off[k]), k


# ---------------------------------------------------------------------------- 4. the sweep: AdamW, both tails, the cache

@pytest.fixture(scope="module")
def gold(golden_dir):
    return torch.load(os.path.join(golden_dir, "clip_golden.pt"), weights_only=True)


@pytest.fixture(scope="module")
def data(gold):
    """tests/test_gpu_visual_prefix.py's tiny data: 11 train / 5 test / 6 inference images with targets."""
    g = torch.Generator().manual_seed(5)
    Tn, R = gold["T"], CR.CLIP_TINY.image_resolution
    mk = lambda k: (torch.randn(k, 3, R, R, generator=g).cuda(), (torch.randn(k, Tn, generator=g) * 0.5 + 2.0).cuda())
    train, test = mk(11), mk(5)
    inf = torch.randn(6, 3, R, R, generator=g).cuda()
    a = np.random.default_rng(5).random((6, 6))
    ref = (a + a.T) / 2
    np.fill_diagonal(ref, 0)
    return dict(train=train, test=test, inference=inf, reference_rdm=ref)


def _gold_hba(gold, tails):
    import vit_amd
    cm = _clip(CR.CLIP_TINY, CR.init_params(CR.CLIP_TINY, seed=gold["seed"]), torch.float32)
    m = vit_amd.CLIPHBA([f"c{i}" for i in range(gold["T"])], "ViT-L/14", pos_embedding=True, clip_model=cm,
                        tokenized_prompts=gold["prompts"], cls_tail=tails, eot_tail=tails)
    vit_amd.apply_dora_to_ViT(m, n_vision_layers=2, n_transformer_layers=1, r=gold["r"], dora_dropout=0.1)
    vit_amd.switch_dora_layers(m, freeze_all=True, dora_state=True)
    with torch.no_grad():
        for name, q in m.named_parameters():
            if name.endswith(".delta_D_A"):
                q.copy_(gold["dora_A_init"][name])
            elif name.endswith(".delta_D_B"):
                q.copy_(gold["dora_B_init"][name])
    return m.cuda()


def _sweep(m, data, tmp, tag):
    import vit_amd
    from vit_amd import sweep as S
    from vit_amd.dora import DoRALayer
    opt = vit_amd.FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=3e-4)
    d = tmp / tag
    d.mkdir()
    torch.manual_seed(3)
    rows = S.train_condition(m, opt, vit_amd.MSELoss(), data, epochs=1, training_run=1, perturb_length=0,
                             perturb_type=None, perturb_seed=0, batch_size=4, training_res_path=str(d / "res.csv"),
                             dora_parameters_path=str(d / "dora"), random_state_path=str(d / "rs"),
                             dataloader_generator=torch.Generator().manual_seed(7), resume_from_epoch=0,
                             modules=tuple(k for k, mod in m.named_modules() if isinstance(mod, DoRALayer)),
                             cache_visual_prefix=True, prefix_caches={})
    with open(d / "res.csv", newline="") as fh:
        assert len(list(csv.reader(fh))) == 1 + len(rows)
    return rows


def test_train_condition_with_both_tails_and_the_prefix_cache(gold, data, tmp_path):
    """One epoch of AdamW steps, evaluation and behavioural RSA with eot_tail, cls_tail and cache_visual_prefix."""
    from vit_amd import _lib as L
    _count(1)
    m_off = _gold_hba(gold, False)
    rows_off = _sweep(m_off, data, tmp_path, "off")
    assert _count(1) == 0
    L.lib().vit_sdpa_cls1_count(1)
    m_on = _gold_hba(gold, True)
    before = {k: p.detach().clone() for k, p in m_on.named_parameters() if p.requires_grad}
    rows_on = _sweep(m_on, data, tmp_path, "on")
    assert _count(1) > 0 and L.lib().vit_sdpa_cls1_count(1) > 0
    moved = [k for k, p in m_on.named_parameters() if p.requires_grad and not torch.equal(p.detach(), before[k])]
    assert any(".transformer.resblocks" in k and ".visual." not in k for k in moved), "the text adapter did not move"
    assert len(rows_on) == len(rows_off) == 1
    for a, b in zip(rows_on, rows_off):
        assert a[0] == b[0] and a[5:] == b[5:]
        for name, x, y in zip(("train_loss", "test_loss", "rsa_rho", "rsa_p"), a[1:5], b[1:5]):
            r = abs(x - y) / max(abs(y), 1e-30)
            print(f"sweep epoch {a[0]} {name}: {x!r} vs {y!r}, relative {r:.3e}")
            assert r < 1e-3, (name, x, y)
