"""The cached frozen visual prefix on the GPU: ``ops.gather_blocks``,
``CLIP.visual_prefix`` / ``forward(visual_prefix=...)``, ``VisualPrefixCache`` and the sweep's
``cache_visual_prefix`` switch, on oracle/clip_ref.py's CLIP_TINY (3 visual blocks, width 128, 17 tokens)
with DoRA on the last two visual blocks (one frozen block) or the last one (two frozen blocks).

Bounds.  Same batch (prefix computed from the very batch): the cached step runs the same kernels on the
same shapes in the same order, so predictions and DoRA gradients are compared with ``torch.equal``.
Different batch composition (prefix built in other chunks than the step's batch): the f32 GEMM's stream-K
split depends on M, so f32 is equal to rounding only; the bounds are tests/test_clip.py::
test_clip_hba_step_matches_golden's -- f32 1e-3 relative; bf16 predictions 3e-2 relative, gradients cosine
>= 0.99 and norm within 5 %, parameters 1e-2 relative.  The measured differences are printed.
"""
import csv
import os

import numpy as np
import pytest
import torch

from oracle import clip_ref as CR

pytestmark = pytest.mark.gpu

CFG = CR.CLIP_TINY
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["f32", "bf16"]


@pytest.fixture(scope="module")
def gold(golden_dir):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.load(os.path.join(golden_dir, "clip_golden.pt"), weights_only=True)


def _tiny_hba(gold, dtype, n_vision_layers=2):
    """tests/test_gpu_forward_only.py::_tiny_hba with the DoRA placement as a parameter."""
    import vit_amd
    from vit_amd import clip
    cm = clip.CLIP(embed_dim=CFG.embed_dim, image_resolution=CFG.image_resolution, vision_layers=CFG.vision_layers,
                   vision_width=CFG.vision_width, vision_patch_size=CFG.vision_patch,
                   context_length=CFG.context_length, vocab_size=CFG.vocab_size, transformer_width=CFG.text_width,
                   transformer_heads=CFG.text_heads, transformer_layers=CFG.text_layers, compute_dtype=dtype)
    cm.load_state_dict(CR.init_params(CFG, seed=gold["seed"]), strict=True)
    m = vit_amd.CLIPHBA([f"c{i}" for i in range(gold["T"])], "ViT-L/14", pos_embedding=True, clip_model=cm,
                        tokenized_prompts=gold["prompts"])
    vit_amd.apply_dora_to_ViT(m, n_vision_layers=n_vision_layers, n_transformer_layers=1, r=gold["r"],
                              dora_dropout=0.1)
    vit_amd.switch_dora_layers(m, freeze_all=True, dora_state=True)
    with torch.no_grad():
        for n, q in m.named_parameters():
            if n.endswith(".delta_D_A"):
                q.copy_(gold["dora_A_init"][n])
            elif n.endswith(".delta_D_B"):
                q.copy_(gold["dora_B_init"][n])
    return m


def _dora_modules(m):
    from vit_amd.dora import DoRALayer
    return tuple(n for n, mod in m.named_modules() if isinstance(mod, DoRALayer))


@pytest.fixture(scope="module")
def data(gold):
    """11 train / 5 test / 6 inference images with targets, on the GPU; never written to."""
    g = torch.Generator().manual_seed(5)
    T, R = gold["T"], CFG.image_resolution
    mk = lambda n: (torch.randn(n, 3, R, R, generator=g).cuda(), (torch.randn(n, T, generator=g) * 0.5 + 2.0).cuda())
    train, test = mk(11), mk(5)
    inf = torch.randn(6, 3, R, R, generator=g).cuda()
    a = np.random.default_rng(5).random((6, 6))
    ref = (a + a.T) / 2
    np.fill_diagonal(ref, 0)
    return dict(train=train, test=test, inference=inf, reference_rdm=ref)


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


def _step(m, x=None, prefix=None, target=None):
    """One forward + MSE backward in train mode; (prediction, DoRA gradients)."""
    import vit_amd
    m.train()
    for p in m.parameters():
        p.grad = None
    torch.manual_seed(0)
    pred = m(x) if prefix is None else m(visual_prefix=prefix)
    vit_amd.MSELoss()(pred, target).backward()
    grads = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.requires_grad}
    assert grads and all(g is not None for g in grads.values())
    return pred.detach(), grads


# ---------------------------------------------------------------------------- 1. the gather kernel

@pytest.mark.parametrize("rows, N, W, idx", [
    (7, 17, 128, [3, 0, 6, 3, 5]),        # 5 of 7 rows with a repeat; row_elems = 17 * 128
    (3, 1, 8192 + 4, [2, 1]),             # whole workgroup chunks (256 float4 each) and one more float4
    (4, 5, 2 * 8192 + 1020, [1, 3, 0]),   # 21755 float4 a row: 84 chunks and a ragged 85th
    (1, 17, 128, [0]),                    # a single row
    (3, 1, 4, [2, 2, 0, 1]),              # one float4 per row
], ids=["5of7-repeat", "chunk+1", "ragged-chunks", "single", "one-vector"])
def test_gather_blocks_equals_index_select(gold, rows, N, W, idx):
    from vit_amd import ops
    g = torch.Generator().manual_seed(rows * 1000 + W)
    src = torch.randn(rows, N, W, generator=g).cuda()
    idx = torch.tensor(idx, dtype=torch.int64)
    want = torch.index_select(src, 0, idx.cuda())
    got = ops.gather_blocks(src, idx)
    assert got.shape == want.shape and torch.equal(got, want)
    out = torch.full_like(want, float("nan"))
    assert ops.gather_blocks(src, idx.cuda(), out=out) is out and torch.equal(out, want)  # a device idx, and out=


@pytest.mark.parametrize("bad", [[0, 7], [-1, 2]], ids=["past-the-end", "negative"])
def test_gather_blocks_out_of_range_launches_nothing(gold, monkeypatch, bad):
    from vit_amd import ops
    src = torch.randn(7, 17, 128).cuda()
    out = torch.zeros(2, 17, 128).cuda()
    launched = []
    real = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (launched.append(name), real(name, *a))[1])
    with pytest.raises(IndexError):
        ops.gather_blocks(src, torch.tensor(bad, dtype=torch.int64), out=out)
    assert launched == []
    assert not out.any()
    ops.gather_blocks(src, torch.tensor([0, 6], dtype=torch.int64), out=out)  # the spy does see a launch
    assert launched == ["vit_gather_blocks"]


# ---------------------------------------------------------------------------- 2. same batch: bitwise

@pytest.mark.parametrize("n_vision_layers", [2, 1], ids=["dora2-frozen1", "dora1-frozen2"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_prefix_of_the_same_batch_is_bitwise(gold, dtype, n_vision_layers):
    m = _tiny_hba(gold, dtype, n_vision_layers).cuda()
    img, tgt = gold["image"].cuda(), gold["target"].cuda()
    px, first = m.clip_model.visual_prefix(img, m.pos_embedding)
    assert first == CFG.vision_layers - n_vision_layers
    assert tuple(px.shape) == (img.shape[0], 17, CFG.vision_width) and px.dtype == torch.float32
    assert not px.requires_grad
    m.eval()
    with torch.no_grad():
        assert torch.equal(m(visual_prefix=px), m(img))
    pred_u, g_u = _step(m, x=img, target=tgt)
    pred_c, g_c = _step(m, prefix=px, target=tgt)
    assert torch.equal(pred_c, pred_u)
    assert g_c.keys() == g_u.keys()
    for n in g_u:
        assert torch.equal(g_c[n], g_u[n]), n


def test_prefix_arguments_are_validated(gold):
    m = _tiny_hba(gold, torch.float32).cuda()
    img = gold["image"].cuda()
    px, _ = m.clip_model.visual_prefix(img, True)
    with pytest.raises(ValueError):
        m(img, visual_prefix=px)
    with pytest.raises(ValueError):
        m()
    with pytest.raises(ValueError):
        m(visual_prefix=px[:, :-1])
    with pytest.raises(ValueError):
        m(visual_prefix=px.bfloat16())
    with pytest.raises(ValueError):
        m(visual_prefix=px.cpu())
    import vit_amd
    vit_amd.switch_dora_layers(m, freeze_all=False)  # every block trainable: no prefix
    with pytest.raises(ValueError):
        m.clip_model.visual_prefix(img, True)


# ---------------------------------------------------------------------------- 3. other batch composition

@pytest.mark.parametrize("n_vision_layers", [2, 1], ids=["dora2-frozen1", "dora1-frozen2"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_cached_step_on_a_shuffled_batch(gold, data, dtype, n_vision_layers):
    import vit_amd
    m = _tiny_hba(gold, dtype, n_vision_layers).cuda()
    tr_x, tr_y = data["train"]
    cache = vit_amd.VisualPrefixCache.build(m, tr_x, batch_size=5)  # chunks of 5, 5, 1
    assert cache.builds == 1 and tuple(cache.x.shape) == (11, 17, CFG.vision_width) and cache.valid_for(m, tr_x)
    idx = torch.tensor([9, 2, 10, 4])
    f32 = dtype == torch.float32
    pred_u, g_u = _step(m, x=tr_x[idx], target=tr_y[idx])
    pred_c, g_c = _step(m, prefix=cache.take(idx), target=tr_y[idx])
    assert cache.hits == 1
    _check_pred(pred_c, pred_u, f32, f"{IDS[not f32]} frozen{3 - n_vision_layers} prediction")
    for n in g_u:
        _check_grad(g_c[n], g_u[n], f32, f"{IDS[not f32]} frozen{3 - n_vision_layers} grad {n.split('clip_model.')[1]}")


# ---------------------------------------------------------------------------- 4. the frozen blocks are skipped

def test_cached_step_runs_only_the_trainable_blocks(gold, data, monkeypatch):
    import vit_amd
    from vit_amd import clip
    m = _tiny_hba(gold, torch.float32, 1).cuda()  # two frozen visual blocks
    tr_x, tr_y = data["train"]
    cache = vit_amd.VisualPrefixCache.build(m, tr_x, batch_size=5)
    idx = torch.tensor([1, 7, 3])
    _step(m, x=tr_x[idx], target=tr_y[idx])  # warms the text tower's own cache
    calls = []
    real = clip.run_block
    monkeypatch.setattr(clip, "run_block", lambda *a: (calls.append(1), real(*a))[1])
    _step(m, x=tr_x[idx], target=tr_y[idx])
    uncached, calls[:] = len(calls), []
    hits = cache.hits
    _step(m, prefix=cache.take(idx), target=tr_y[idx])
    live_text = 1  # the last text block carries DoRA; the one in front of it comes from the text cache
    assert uncached == CFG.vision_layers + live_text
    assert len(calls) == 1 + live_text  # one trainable visual block
    assert cache.hits == hits + 1


# ---------------------------------------------------------------------------- 5. / 6. the sweep

def _run(m, data, tmp, tag, cached, caches=None, *, epochs=2, perturb_type=None, training_run=1, perturb_length=0,
         resume_from_epoch=0):
    """train_condition on the tiny model; (rows, saved DoRA parameters of the last epoch)."""
    import vit_amd
    from vit_amd import sweep as S
    opt = vit_amd.FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=3e-4)
    d = tmp / tag
    d.mkdir()
    kw = dict(cache_visual_prefix=True, prefix_caches=caches) if cached else {}
    torch.manual_seed(3)
    rows = S.train_condition(m, opt, vit_amd.MSELoss(), data, epochs=epochs, training_run=training_run,
                             perturb_length=perturb_length, perturb_type=perturb_type, perturb_seed=0, batch_size=4,
                             training_res_path=str(d / "res.csv"), dora_parameters_path=str(d / "dora"),
                             random_state_path=str(d / "rs"), dataloader_generator=torch.Generator().manual_seed(7),
                             resume_from_epoch=resume_from_epoch, modules=_dora_modules(m), **kw)
    with open(d / "res.csv", newline="") as fh:
        on_disk = list(csv.reader(fh))
    assert len(on_disk) == 1 + len(rows)
    sd = torch.load(d / "dora" / f"epoch{epochs}_dora_params.pth", weights_only=True)
    return rows, sd


def _compare_runs(ru, rc, f32, what):
    (rows_u, sd_u), (rows_c, sd_c) = ru, rc
    assert len(rows_c) == len(rows_u)
    for a, b in zip(rows_c, rows_u):
        assert a[0] == b[0] and a[5:] == b[5:]  # epoch and the used_* flags
        for name, x, y in zip(("train_loss", "test_loss", "rsa_rho", "rsa_p"), a[1:5], b[1:5]):
            r = abs(x - y) / max(abs(y), 1e-30)
            print(f"{what} epoch {a[0]} {name}: {x!r} vs {y!r}, relative {r:.3e}")
            assert r < (1e-3 if f32 else 3e-2), (what, name, x, y)
    assert sd_c.keys() == sd_u.keys()
    for n in sd_u:
        r = _rel(sd_c[n], sd_u[n])
        print(f"{what} {n.split('clip_model.')[1]}: relative {r:.3e}")
        assert r < (1e-3 if f32 else 1e-2), (what, n, r)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_train_condition_cached_matches_uncached(gold, data, tmp_path, dtype):
    f32 = dtype == torch.float32
    ru = _run(_tiny_hba(gold, dtype).cuda(), data, tmp_path, "u", False)
    caches = {}
    rc = _run(_tiny_hba(gold, dtype).cuda(), data, tmp_path, "c", True, caches)
    _compare_runs(ru, rc, f32, f"{IDS[not f32]} plain")
    assert sorted(caches) == ["inference", "test", "train"]
    assert [caches[k].builds for k in ("train", "test", "inference")] == [1, 1, 1]
    assert caches["train"].hits == 2 * 3 and caches["train"].bypassed == 0  # 11 images in batches of 4, 2 epochs
    assert caches["test"].hits == 2 * 2 and caches["inference"].hits == 2 * 1


def test_train_condition_target_perturbation_uses_the_cache(gold, data, tmp_path):
    kw = dict(perturb_type="random_target", training_run=1, perturb_length=1)
    ru = _run(_tiny_hba(gold, torch.float32).cuda(), data, tmp_path, "u", False, **kw)
    caches = {}
    rc = _run(_tiny_hba(gold, torch.float32).cuda(), data, tmp_path, "c", True, caches, **kw)
    assert rc[0][0][5] is True and rc[0][1][5] is False  # used_random_targets in epoch 1 only
    _compare_runs(ru, rc, True, "f32 random_target")
    assert caches["train"].hits == 6 and caches["train"].bypassed == 0


def test_train_condition_image_perturbation_bypasses_the_cache(gold, data, tmp_path):
    kw = dict(perturb_type="image_noise", training_run=1, perturb_length=1)  # the window covers epoch 0
    ru = _run(_tiny_hba(gold, torch.float32).cuda(), data, tmp_path, "u", False, **kw)
    caches = {}
    rc = _run(_tiny_hba(gold, torch.float32).cuda(), data, tmp_path, "c", True, caches, **kw)
    assert rc[0][0][8] is True and rc[0][1][8] is False  # used_image_noise in epoch 1 only
    _compare_runs(ru, rc, True, "f32 image_noise")
    assert caches["train"].bypassed == 3 and caches["train"].hits == 3
    assert caches["test"].bypassed == 0 and caches["test"].hits == 4


def test_frozen_weight_change_rebuilds_the_cache(gold, data, tmp_path):
    mu, mc = _tiny_hba(gold, torch.float32).cuda(), _tiny_hba(gold, torch.float32).cuda()
    caches = {}
    _run(mu, data, tmp_path, "u1", False, epochs=1)
    _run(mu, data, tmp_path, "u1b", False, epochs=1)  # the same history as the cached model's two runs
    _run(mc, data, tmp_path, "c1", True, caches, epochs=1)
    assert [caches[k].builds for k in ("train", "test", "inference")] == [1, 1, 1]
    _run(mc, data, tmp_path, "c1b", True, caches, epochs=1)  # nothing changed: kept
    assert [caches[k].builds for k in ("train", "test", "inference")] == [1, 1, 1]
    stale = caches["train"].x.clone()
    g = torch.Generator().manual_seed(1)
    delta = (0.05 * torch.randn(mu.clip_model.visual.transformer.resblocks[0].mlp.c_fc.weight.shape, generator=g)).cuda()
    with torch.no_grad():
        for m in (mu, mc):
            m.clip_model.visual.transformer.resblocks[0].mlp.c_fc.weight.add_(delta)  # a frozen block, in place
    assert not caches["train"].valid_for(mc, data["train"][0])
    ru = _run(mu, data, tmp_path, "u2", False, epochs=1)
    rc = _run(mc, data, tmp_path, "c2", True, caches, epochs=1)
    assert [caches[k].builds for k in ("train", "test", "inference")] == [2, 2, 2]
    assert not torch.equal(caches["train"].x, stale)
    _compare_runs(ru, rc, True, "f32 after the weight change")
