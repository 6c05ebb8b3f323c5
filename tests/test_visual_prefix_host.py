"""Host side of the cached frozen visual prefix, no GPU: the sweep's batch order with
``with_index``, the cache key on CPU tensors, the ``max_bytes`` refusal, and the switch's refusal of a
model with nothing to cache."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import clip_ref as CR

CFG = CR.CLIP_TINY


def _tiny_hba(n_vision_layers=2):
    """oracle/clip_ref.py's CLIP_TINY as a CLIPHBA with DoRA on the last visual blocks, on the CPU."""
    import vit_amd
    from vit_amd import clip
    cm = clip.CLIP(embed_dim=CFG.embed_dim, image_resolution=CFG.image_resolution, vision_layers=CFG.vision_layers,
                   vision_width=CFG.vision_width, vision_patch_size=CFG.vision_patch,
                   context_length=CFG.context_length, vocab_size=CFG.vocab_size, transformer_width=CFG.text_width,
                   transformer_heads=CFG.text_heads, transformer_layers=CFG.text_layers)
    m = vit_amd.CLIPHBA([f"c{i}" for i in range(5)], "ViT-L/14", pos_embedding=True, clip_model=cm)
    if n_vision_layers:
        vit_amd.apply_dora_to_ViT(m, n_vision_layers=n_vision_layers, n_transformer_layers=1, r=4)
    vit_amd.switch_dora_layers(m, freeze_all=True, dora_state=True)
    return m


# ---------------------------------------------------------------------------- batch order

@pytest.mark.parametrize("shuffle", [True, False], ids=["shuffle", "in-order"])
def test_batches_with_index_is_the_same_order_and_draw(shuffle):
    from vit_amd import sweep as S
    g0 = torch.Generator().manual_seed(3)
    x, y = torch.randn(11, 3, 2, 2, generator=g0), torch.randn(11, 5, generator=g0)
    ga, gb = torch.Generator().manual_seed(17), torch.Generator().manual_seed(17)
    plain = list(S._batches(x, y, 4, ga if shuffle else None, shuffle=shuffle))
    indexed = list(S._batches(x, y, 4, gb if shuffle else None, shuffle=shuffle, with_index=True))
    assert [len(b) for b in plain] == [2, 2, 2] and [len(b) for b in indexed] == [3, 3, 3]
    assert [b[0].shape[0] for b in indexed] == [4, 4, 3]  # a ragged last batch
    for (px, py), (ix, iy, idx) in zip(plain, indexed):
        assert torch.equal(px, ix) and torch.equal(py, iy)
        assert idx.dtype == torch.int64 and idx.device.type == "cpu"
        assert torch.equal(x[idx], ix) and torch.equal(y[idx], iy)
    assert sorted(torch.cat([b[2] for b in indexed]).tolist()) == list(range(11))
    assert torch.equal(ga.get_state(), gb.get_state())
    if shuffle:  # and one draw was made, as a DataLoader epoch makes
        assert not torch.equal(ga.get_state(), torch.Generator().manual_seed(17).get_state())
        assert torch.equal(torch.randperm(11, generator=torch.Generator().manual_seed(17)),
                           torch.cat([b[2] for b in indexed]))


# ---------------------------------------------------------------------------- key

def test_key_follows_the_frozen_parameters_and_the_switches():
    from vit_amd.prefix_cache import prefix_key
    m = _tiny_hba(2)
    images = torch.randn(4, 3, 32, 32)
    k0 = prefix_key(m, images)
    assert k0 == prefix_key(m, images) and hash(k0) == hash(prefix_key(m, images))
    assert k0[1] == 1  # one frozen block in front of the two DoRA blocks
    blocks = m.clip_model.visual.transformer.resblocks
    with torch.no_grad():
        for dora in (blocks[1].attn.out_proj, blocks[2].attn.out_proj, m.clip_model.transformer.resblocks[1].attn.out_proj):
            dora.m.add_(1.0)
            dora.delta_D_A.mul_(2.0)
            dora.delta_D_B.add_(0.5)
        blocks[2].mlp.c_fc.weight.add_(1.0)  # frozen, but behind the cut
    assert prefix_key(m, images) == k0  # DoRA (and anything behind the cut) is not in the key
    with torch.no_grad():
        blocks[0].mlp.c_fc.weight.add_(1.0)
    k1 = prefix_key(m, images)
    assert k1 != k0
    with torch.no_grad():
        m.clip_model.visual.ln_pre.bias.add_(1.0)  # the stem
    k2 = prefix_key(m, images)
    assert k2 != k1
    m.clip_model.set_attention_fp8(True)
    k3 = prefix_key(m, images)
    assert k3 != k2
    m.clip_model.set_attention_fp8(False)
    assert prefix_key(m, images) == k2
    m.pos_embedding = False
    assert prefix_key(m, images) != k2
    m.pos_embedding = True
    m.clip_model.compute_dtype = torch.bfloat16
    assert prefix_key(m, images) != k2
    m.clip_model.compute_dtype = torch.float32
    images.add_(1.0)  # the images, in place
    k4 = prefix_key(m, images)
    assert k4 != k2
    assert prefix_key(m, images.clone()) != k4  # other storage
    assert prefix_key(m, images[:3]) != k4  # other shape


def test_key_moves_with_the_cut():
    from vit_amd.prefix_cache import prefix_key
    images = torch.randn(4, 3, 32, 32)
    assert prefix_key(_tiny_hba(2), images)[1] == 1 and prefix_key(_tiny_hba(1), images)[1] == 2


def test_valid_for_and_counters_start_empty():
    import vit_amd
    c = vit_amd.VisualPrefixCache()
    assert (c.hits, c.bypassed, c.builds, c.nbytes) == (0, 0, 0, 0)
    assert not c.valid_for(_tiny_hba(2), torch.randn(2, 3, 32, 32))
    c.bypass()
    assert c.bypassed == 1
    with pytest.raises(RuntimeError):
        c.take(torch.tensor([0]))


# ---------------------------------------------------------------------------- refusals

def test_max_bytes_refusal_comes_before_any_allocation(monkeypatch):
    import vit_amd
    m = _tiny_hba(2)
    images = torch.randn(6, 3, 32, 32)
    need = 6 * 17 * CFG.vision_width * 4
    made = []
    real = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, **k: (made.append(a), real(*a, **k))[1])
    ran = []
    monkeypatch.setattr(m.clip_model, "visual_prefix", lambda *a, **k: ran.append(a))
    with pytest.raises(MemoryError, match=str(need)):
        vit_amd.VisualPrefixCache.build(m, images, batch_size=4, max_bytes=need - 1)
    assert made == [] and ran == []
    # at the limit it goes on to the device work: refused there, the model is on the CPU
    from vit_amd._lib import HipError
    with pytest.raises(HipError):
        vit_amd.VisualPrefixCache.build(m, images, batch_size=4, max_bytes=need)
    assert made == [] and ran == []


def test_check_block_indices_on_the_host():
    from vit_amd import ops
    ops.check_block_indices(torch.tensor([0, 6, 3, 3]), 7)
    ops.check_block_indices(torch.empty(0, dtype=torch.int64), 7)
    for bad in ([7], [-1], [0, 1, 100]):
        with pytest.raises(IndexError):
            ops.check_block_indices(torch.tensor(bad), 7)
    with pytest.raises(TypeError):
        ops.check_block_indices(torch.tensor([0], dtype=torch.int32), 7)
    with pytest.raises(TypeError):
        ops.check_block_indices(torch.zeros(2, 2, dtype=torch.int64), 7)


def _data(n_train=6, n_test=3, n_inf=4):
    g = torch.Generator().manual_seed(0)
    mk = lambda n: (torch.randn(n, 3, 32, 32, generator=g), torch.randn(n, 5, generator=g))
    a = np.random.default_rng(0).random((n_inf, n_inf))
    return dict(train=mk(n_train), test=mk(n_test), inference=torch.randn(n_inf, 3, 32, 32, generator=g),
                reference_rdm=(a + a.T) / 2)


def _train_kw(tmp_path):
    return dict(epochs=1, training_run=1, perturb_length=0, perturb_type=None, batch_size=4,
                training_res_path=str(tmp_path / "res.csv"), dora_parameters_path=str(tmp_path / "dora"),
                random_state_path=str(tmp_path / "rs"), dataloader_generator=torch.Generator().manual_seed(1))


def test_switch_refuses_a_model_with_no_frozen_visual_block(tmp_path):
    import vit_amd
    from vit_amd import sweep as S
    m = _tiny_hba(CFG.vision_layers)  # DoRA on every visual block: the first block is trainable
    opt = torch.optim.AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-3)
    with pytest.raises(ValueError, match="frozen visual block"):
        S.train_condition(m, opt, nn.MSELoss(), _data(), cache_visual_prefix=True, **_train_kw(tmp_path))
    assert not os.path.exists(tmp_path / "res.csv")  # refused at the start, before anything is written
    with pytest.raises(ValueError, match="frozen visual block"):
        vit_amd.VisualPrefixCache.build(m, _data()["train"][0], max_bytes=1 << 30)
    with pytest.raises(ValueError, match="frozen visual block"):
        S.evaluate(m, *_data()["test"], 4, nn.MSELoss(), cache_visual_prefix=True)


def test_switch_refuses_a_model_that_is_no_cliphba(tmp_path):
    from vit_amd import sweep as S

    class Plain(nn.Module):
        def __init__(self):
            super().__init__()
            self.lin = nn.Linear(3 * 32 * 32, 5)

        def forward(self, x):
            return self.lin(x.flatten(1))

    m = Plain()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
    with pytest.raises(ValueError, match="CLIPHBA"):
        S.train_condition(m, opt, nn.MSELoss(), _data(), cache_visual_prefix=True, **_train_kw(tmp_path))
    with pytest.raises(ValueError, match="CLIPHBA"):
        S.run_sweep(lambda: (m, opt), nn.MSELoss(), _data(), [(1, 1)], perturb_type="random_target",
                    out_dir=str(tmp_path / "out"), baseline_dora_path=str(tmp_path / "b"),
                    baseline_random_state_path=str(tmp_path / "b"), epochs=1, cache_visual_prefix=True,
                    batch_size=4)


def test_switch_off_leaves_the_sweep_signature_compatible(tmp_path):
    """Off by default, and ``prefix_caches`` without the switch is an error, not a silent no-op."""
    import inspect
    from vit_amd import sweep as S
    for fn in (S.train_condition, S.evaluate, S.behavioral_rsa, S.run_sweep, S.launch_sweep):
        assert inspect.signature(fn).parameters["cache_visual_prefix"].default is False, fn.__name__
    assert inspect.signature(S._batches).parameters["with_index"].default is False
    with pytest.raises(ValueError):
        S.train_condition(nn.Linear(1, 1), None, nn.MSELoss(), _data(), prefix_caches={}, **_train_kw(tmp_path))
