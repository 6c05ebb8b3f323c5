"""CPU: the host-side surface of the streamed fp8 attention, no GPU needed.

- include/vit_hip.h declares ``vit_sdpa_fwd_fp8_stream`` and ``vit_sdpa_fp8_stream_count``, vit_amd/_lib.py binds
  them and the built library exports them;
- ``ops.check_fp8_tokens`` still refuses past 320 tokens unless the streamed kernel is asked for;
- ``set_attention_fp8(enable, long_sequences)`` on a ViT and on a CLIP: ``True`` alone leaves the streamed form
  off, ``False`` clears both switches; ``CLIPHBA(attention_fp8=, attention_fp8_long=)`` passes them on;
- the visual prefix cache's key follows the new switch, appended last (position 1 is still the cut).
"""
import os
import re

import pytest
import torch

from oracle import clip_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = CR.CLIP_TINY
SDPA_ARGS = "i32, i32, i32, i32, i32, vp, i64, vp, i64, vp, f32, i32, vp".split(", ")


def _tiny_clip():
    from vit_amd import clip
    return clip.CLIP(embed_dim=CFG.embed_dim, image_resolution=CFG.image_resolution, vision_layers=CFG.vision_layers,
                     vision_width=CFG.vision_width, vision_patch_size=CFG.vision_patch,
                     context_length=CFG.context_length, vocab_size=CFG.vocab_size, transformer_width=CFG.text_width,
                     transformer_heads=CFG.text_heads, transformer_layers=CFG.text_layers)


def test_stream_exports_declared_bound_and_built():
    from vit_amd import _lib
    txt = open(os.path.join(ROOT, "include", "vit_hip.h")).read()
    assert re.search(r"\bint\s+vit_sdpa_fwd_fp8_stream\s*\(\s*int\s+dtype\s*,", txt)
    assert re.search(r"\bint\s+vit_sdpa_fp8_stream_count\s*\(\s*int\s+reset\s*\)\s*;", txt)
    assert _lib.SIGNATURES["vit_sdpa_fwd_fp8_stream"] == [getattr(_lib, a) for a in SDPA_ARGS]
    assert _lib.SIGNATURES["vit_sdpa_fwd_fp8_stream"] == _lib.SIGNATURES["vit_sdpa_fwd_fp8"]
    assert _lib.SIGNATURES["vit_sdpa_fp8_stream_count"] == [_lib.i32]
    lib = _lib.load()
    assert hasattr(lib, "vit_sdpa_fwd_fp8_stream") and hasattr(lib, "vit_sdpa_fp8_stream_count")
    assert lib.vit_abi_version() == 10
    assert lib.vit_sdpa_fp8_stream_count(1) >= 0 and lib.vit_sdpa_fp8_stream_count(0) == 0


def test_check_fp8_tokens_refuses_unless_long():
    from vit_amd import ops
    with pytest.raises(ValueError, match="320"):
        ops.check_fp8_tokens(577)
    with pytest.raises(ValueError, match="320"):
        ops.check_fp8_tokens(321, long=False)
    ops.check_fp8_tokens(577, long=True)
    ops.check_fp8_tokens(320)
    ops.check_fp8_tokens(320, long=True)


def test_vit_setter_semantics():
    import vit_amd
    m = vit_amd.VisionTransformer(img_size=32, patch_size=16, embed_dim=128, depth=1, num_heads=2, num_classes=3)
    assert (m._attn_fp8, m._attn_fp8_long) == (False, False)
    m.set_attention_fp8(True)
    assert (m._attn_fp8, m._attn_fp8_long) == (True, False)
    m.set_attention_fp8(True, long_sequences=True)
    assert (m._attn_fp8, m._attn_fp8_long) == (True, True)
    m.set_attention_fp8(True)  # True alone leaves the streamed form off
    assert (m._attn_fp8, m._attn_fp8_long) == (True, False)
    m.set_attention_fp8(True, long_sequences=True)
    m.set_attention_fp8(False)
    assert (m._attn_fp8, m._attn_fp8_long) == (False, False)
    m.set_attention_fp8(False, long_sequences=True)  # nothing to stream with fp8 off
    assert (m._attn_fp8, m._attn_fp8_long) == (False, False)


def test_clip_setter_semantics_and_block_config():
    cm = _tiny_clip()
    assert (cm.attention_fp8, cm.attention_fp8_long) == (False, False)
    cm.set_attention_fp8(True)
    assert (cm.attention_fp8, cm.attention_fp8_long) == (True, False)
    cfg = cm._cfg(2, False, frozen=True)
    assert cfg["attn_fp8"] is True and cfg["attn_fp8_long"] is False
    cm.set_attention_fp8(True, long_sequences=True)
    assert (cm.attention_fp8, cm.attention_fp8_long) == (True, True)
    cfg = cm._cfg(2, False, frozen=True)
    assert cfg["attn_fp8"] is True and cfg["attn_fp8_long"] is True
    with torch.enable_grad():  # a trainable block under grad keeps its own precision
        assert cm._cfg(2, False, frozen=False)["attn_fp8"] is False
    cm.set_attention_fp8(False)
    assert (cm.attention_fp8, cm.attention_fp8_long) == (False, False)


def test_cliphba_passes_both_switches():
    import vit_amd
    names = [f"c{i}" for i in range(5)]
    a = vit_amd.CLIPHBA(names, "ViT-L/14", clip_model=_tiny_clip())
    b = vit_amd.CLIPHBA(names, "ViT-L/14", clip_model=_tiny_clip(), attention_fp8=True)
    c = vit_amd.CLIPHBA(names, "ViT-L/14", clip_model=_tiny_clip(), attention_fp8=True, attention_fp8_long=True)
    d = vit_amd.CLIPHBA(names, "ViT-L/14", clip_model=_tiny_clip(), attention_fp8_long=True)
    got = [(m.clip_model.attention_fp8, m.clip_model.attention_fp8_long) for m in (a, b, c, d)]
    assert got == [(False, False), (True, False), (True, True), (False, False)]


def test_prefix_key_follows_the_long_switch():
    import vit_amd
    from vit_amd.prefix_cache import prefix_key
    m = vit_amd.CLIPHBA([f"c{i}" for i in range(5)], "ViT-L/14", pos_embedding=True, clip_model=_tiny_clip())
    vit_amd.apply_dora_to_ViT(m, n_vision_layers=2, n_transformer_layers=1, r=4)
    vit_amd.switch_dora_layers(m, freeze_all=True, dora_state=True)
    images = torch.randn(4, 3, 32, 32)
    m.clip_model.set_attention_fp8(True)
    k_off = prefix_key(m, images)
    m.clip_model.set_attention_fp8(True, long_sequences=True)
    k_on = prefix_key(m, images)
    assert k_on != k_off and k_on[:-1] == k_off[:-1]
    assert (k_off[-1], k_on[-1]) == (False, True)
    first = len(m.clip_model.visual.transformer.resblocks) - 2
    assert k_on[1] == first and k_off[1] == first
    m.clip_model.set_attention_fp8(True)
    assert prefix_key(m, images) == k_off
