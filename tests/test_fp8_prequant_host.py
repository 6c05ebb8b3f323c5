"""CPU: the host-side surface of the quantise-once fp8 attention, no GPU needed.

- include/vit_hip.h declares ``vit_sdpa_fp8_kv_bytes``, ``vit_sdpa_fp8_quant_kv``, ``vit_sdpa_fwd_fp8_pre`` and
  ``vit_sdpa_fp8_pre_count``, vit_amd/_lib.py binds them, the built library exports them and its ABI is still 10;
- the size query and the refusals that need no device (they return before anything is launched);
- ``set_attention_fp8(enable, long_sequences, prequantize)`` on a ViT and on a CLIP: the stored switch is the
  conjunction of the three, ``prequantize`` without ``long_sequences`` raises, ``False`` clears all three;
  ``CLIPHBA(attention_fp8_prequant=)`` passes it on; ``cfg["attn_fp8_pre"]`` follows the switch;
- the visual prefix key and the text prefix key do not see the switch (the tokens are bit-equal either way);
- ``ops.check_fp8_tokens`` is unchanged: the switch lifts no refusal.
"""
import ctypes
import inspect
import os
import re

import pytest
import torch

from oracle import clip_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = CR.CLIP_TINY
NEW = ("vit_sdpa_fp8_kv_bytes", "vit_sdpa_fp8_quant_kv", "vit_sdpa_fwd_fp8_pre", "vit_sdpa_fp8_pre_count")


def _tiny_clip():
    from vit_amd import clip
    return clip.CLIP(embed_dim=CFG.embed_dim, image_resolution=CFG.image_resolution, vision_layers=CFG.vision_layers,
                     vision_width=CFG.vision_width, vision_patch_size=CFG.vision_patch,
                     context_length=CFG.context_length, vocab_size=CFG.vocab_size, transformer_width=CFG.text_width,
                     transformer_heads=CFG.text_heads, transformer_layers=CFG.text_layers)


def test_exports_declared_bound_and_built():
    from vit_amd import _lib
    i32, i64, f32, vp = _lib.i32, _lib.i64, _lib.f32, _lib.vp
    txt = open(os.path.join(ROOT, "include", "vit_hip.h")).read()
    assert re.search(r"\bint\s+vit_sdpa_fp8_kv_bytes\s*\(\s*int\s+B\s*,\s*int\s+H\s*,\s*int\s+N\s*,\s*int64_t\s*\*\s*bytes\s*\)\s*;", txt)
    assert re.search(r"\bint\s+vit_sdpa_fp8_quant_kv\s*\(\s*int\s+dtype\s*,[^;]*\bvoid\s*\*\s*ws\s*,\s*int64_t\s+ws_bytes\s*,"
                     r"\s*void\s*\*\s*stream\s*\)\s*;", txt)
    assert re.search(r"\bint\s+vit_sdpa_fwd_fp8_pre\s*\(\s*int\s+dtype\s*,[^;]*\bconst\s+void\s*\*\s*ws\s*,\s*int64_t\s+ws_bytes\s*,"
                     r"[^;]*\bint\s+causal\s*,\s*void\s*\*\s*stream\s*\)\s*;", txt)
    assert re.search(r"\bint\s+vit_sdpa_fp8_pre_count\s*\(\s*int\s+reset\s*\)\s*;", txt)
    assert _lib.SIGNATURES["vit_sdpa_fp8_kv_bytes"] == [i32, i32, i32, vp]
    assert _lib.SIGNATURES["vit_sdpa_fp8_quant_kv"] == [i32, i32, i32, i32, i32, vp, i64, vp, i64, vp]
    assert _lib.SIGNATURES["vit_sdpa_fwd_fp8_pre"] == [i32, i32, i32, i32, i32, vp, i64, vp, i64, vp, i64, vp, f32, i32,
                                                       vp]
    assert _lib.SIGNATURES["vit_sdpa_fp8_pre_count"] == [i32]
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NEW)
    assert lib.vit_abi_version() == 10
    assert lib.vit_sdpa_fp8_pre_count(1) >= 0 and lib.vit_sdpa_fp8_pre_count(0) == 0


def test_size_query_and_device_free_refusals():
    from vit_amd import _lib, ops
    lib = _lib.load()
    one = ops.sdpa_fp8_kv_bytes(1, 1, 64)
    assert one > 0 and one % 16 == 0
    # at least the payload of a 64-key chunk: e4m3 K and V images and an E8M0 byte per 32 values of K, per head dim of V
    assert one >= 2 * 64 * 64 + 64 * 2 + 64
    assert ops.sdpa_fp8_kv_bytes(1, 1, 1) == one and ops.sdpa_fp8_kv_bytes(1, 1, 65) == 2 * one
    assert ops.sdpa_fp8_kv_bytes(3, 1, 64) == 3 * one and ops.sdpa_fp8_kv_bytes(1, 5, 64) == 5 * one
    assert ops.sdpa_fp8_kv_bytes(64, 16, 785) == 64 * 16 * 13 * one
    assert ops.sdpa_fp8_kv_bytes(1024, 16, 1025) == 1024 * 16 * 17 * one > 2 ** 31  # the size is an int64
    n = ctypes.c_int64(-1)
    for args in [(0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1, -5)]:
        assert lib.vit_sdpa_fp8_kv_bytes(*args, ctypes.addressof(n)) != 0 and n.value == -1
        with pytest.raises(RuntimeError):
            ops.sdpa_fp8_kv_bytes(*args)
    assert lib.vit_sdpa_fp8_kv_bytes(1, 1, 1, None) != 0
    # the launches' refusals come before any device call: host memory stands in for the pointers, nothing runs
    B, H, N = 1, 2, 321
    D = H * 64
    need = ops.sdpa_fp8_kv_bytes(B, H, N)
    raw = ctypes.create_string_buffer(64)
    a16 = (ctypes.addressof(raw) + 15) // 16 * 16
    quant = lambda hd=64, N=N, ld=3 * D, ws=a16, nb=need: lib.vit_sdpa_fp8_quant_kv(_lib.BF16, B, H, N, hd, a16, ld, ws,
                                                                                  nb, None)
    fwd = lambda hd=64, N=N, ld=3 * D, ws=a16, nb=need, ld_o=D: lib.vit_sdpa_fwd_fp8_pre(
        _lib.BF16, B, H, N, hd, a16, ld, ws, nb, a16, ld_o, None, 0.125, 0, None)
    c0 = lib.vit_sdpa_fp8_pre_count(0), lib.vit_sdpa_fp8_stream_count(0)
    for f in (quant, fwd):
        assert f(hd=32) != 0
        assert f(N=0) != 0
        assert f(ld=3 * D + 4) != 0
        assert f(ws=None) != 0
        assert f(ws=a16 + 8) != 0
        assert f(nb=need - 1) != 0
    assert fwd(ld_o=D + 2) != 0
    assert (lib.vit_sdpa_fp8_pre_count(0), lib.vit_sdpa_fp8_stream_count(0)) == c0


def test_check_fp8_tokens_is_unchanged():
    from vit_amd import ops
    assert list(inspect.signature(ops.check_fp8_tokens).parameters) == ["N", "long"]
    with pytest.raises(ValueError, match="320"):
        ops.check_fp8_tokens(577)
    with pytest.raises(ValueError, match="320"):
        ops.check_fp8_tokens(321, long=False)
    ops.check_fp8_tokens(577, long=True)
    ops.check_fp8_tokens(320)
    sig = inspect.signature(ops.sdpa_fwd).parameters
    assert sig["fp8_pre"].default is False and sig["fp8_long"].default is False and sig["fp8"].default is False


def test_switch_rule():
    from vit_amd import ops
    assert ops.fp8_switches(False) == (False, False, False)
    assert ops.fp8_switches(True) == (True, False, False)
    assert ops.fp8_switches(True, True) == (True, True, False)
    assert ops.fp8_switches(True, True, True) == (True, True, True)
    assert ops.fp8_switches(False, True, True) == (False, False, False)
    assert ops.fp8_switches(False, False, True) == (False, False, False)  # nothing is asked for: no error
    with pytest.raises(ValueError, match="long_sequences"):
        ops.fp8_switches(True, False, True)


def test_vit_setter_semantics():
    import vit_amd
    m = vit_amd.VisionTransformer(img_size=32, patch_size=16, embed_dim=128, depth=1, num_heads=2, num_classes=3)
    state = lambda: (m._attn_fp8, m._attn_fp8_long, m._attn_fp8_pre)
    assert state() == (False, False, False)
    m.set_attention_fp8(True, long_sequences=True, prequantize=True)
    assert state() == (True, True, True)
    m.set_attention_fp8(True, long_sequences=True)  # each call states all three
    assert state() == (True, True, False)
    m.set_attention_fp8(True, True, True)
    with pytest.raises(ValueError):
        m.set_attention_fp8(True, prequantize=True)  # would be a silent no-op
    assert state() == (True, True, True)  # a refused call changes nothing
    m.set_attention_fp8(True)
    assert state() == (True, False, False)
    m.set_attention_fp8(True, True, True)
    m.set_attention_fp8(False)
    assert state() == (False, False, False)
    m.set_attention_fp8(False, long_sequences=True, prequantize=True)
    assert state() == (False, False, False)
    m.set_attention_fp8(False, prequantize=True)
    assert state() == (False, False, False)


def test_clip_setter_semantics_and_block_config():
    cm = _tiny_clip()
    state = lambda: (cm.attention_fp8, cm.attention_fp8_long, cm.attention_fp8_pre)
    assert state() == (False, False, False)
    assert cm._cfg(2, False, frozen=True)["attn_fp8_pre"] is False
    cm.set_attention_fp8(True, long_sequences=True)
    assert state() == (True, True, False) and cm._cfg(2, False, frozen=True)["attn_fp8_pre"] is False
    cm.set_attention_fp8(True, long_sequences=True, prequantize=True)
    assert state() == (True, True, True)
    cfg = cm._cfg(2, False, frozen=True)
    assert cfg["attn_fp8"] is True and cfg["attn_fp8_long"] is True and cfg["attn_fp8_pre"] is True
    with torch.enable_grad():  # a trainable block under grad keeps its own precision: the routing rule is fp8's
        assert cm._cfg(2, False, frozen=False)["attn_fp8"] is False
    with pytest.raises(ValueError):
        cm.set_attention_fp8(True, prequantize=True)
    assert state() == (True, True, True)
    cm.set_attention_fp8(True)
    assert state() == (True, False, False)
    cm.set_attention_fp8(True, True, True)
    cm.set_attention_fp8(False)
    assert state() == (False, False, False) and cm._cfg(2, False, frozen=True)["attn_fp8_pre"] is False


def test_vit_block_config_follows_the_switch(monkeypatch):
    """cfg["attn_fp8_pre"] as _tokens hands it to every block: the stem and the block function are replaced by
    stand-ins that run on the CPU, the rest of _tokens is the model's own."""
    import vit_amd
    from vit_amd import model as M
    m = vit_amd.VisionTransformer(img_size=32, patch_size=16, embed_dim=128, depth=2, num_heads=2, num_classes=3)
    seen = []
    monkeypatch.setattr(M.L, "require_gpu", lambda t: None)
    monkeypatch.setattr(m, "_ensure_shadows", lambda: None)
    monkeypatch.setattr(M._PatchEmbedFn, "apply", lambda x, *a: torch.zeros(x.shape[0], 5, 128))
    monkeypatch.setattr(M, "run_block", lambda x, params, cfg: (seen.append(cfg), x)[1])
    monkeypatch.setattr(M, "_FWD_JOIN", ["block"])  # no side stream to join on the CPU
    x = torch.zeros(1, 3, 32, 32)
    for args, want in [((True, True, True), (True, True, True)), ((True, True), (True, True, False)),
                       ((True,), (True, False, False)), ((False,), (False, False, False))]:
        m.set_attention_fp8(*args)
        seen.clear()
        with torch.no_grad():
            m._tokens(x)
        assert len(seen) == 2
        for cfg in seen:
            assert (cfg["attn_fp8"], cfg["attn_fp8_long"], cfg["attn_fp8_pre"]) == want
    m.set_attention_fp8(True, True, True)
    seen.clear()
    with torch.enable_grad():  # a forward that builds a graph keeps its own precision: fp8's routing rule
        m._tokens(x)
    assert [cfg["attn_fp8"] for cfg in seen] == [False, False]
    # _block_chain hands the switch to both of its ops.sdpa_fwd calls
    src = inspect.getsource(M._block_chain)
    assert src.count("fp8_pre=attn_fp8_pre") == src.count("fp8_long=attn_fp8_long") == 2


def test_cliphba_passes_the_switch():
    import vit_amd
    names = [f"c{i}" for i in range(5)]
    mk = lambda **kw: vit_amd.CLIPHBA(names, "ViT-L/14", clip_model=_tiny_clip(), **kw).clip_model
    got = [(c.attention_fp8, c.attention_fp8_long, c.attention_fp8_pre) for c in (
        mk(), mk(attention_fp8=True, attention_fp8_long=True),
        mk(attention_fp8=True, attention_fp8_long=True, attention_fp8_prequant=True),
        mk(attention_fp8_long=True, attention_fp8_prequant=True))]
    assert got == [(False, False, False), (True, True, False), (True, True, True), (False, False, False)]
    with pytest.raises(ValueError):
        mk(attention_fp8=True, attention_fp8_prequant=True)


def test_prefix_keys_do_not_see_the_switch():
    import vit_amd
    from vit_amd.prefix_cache import prefix_key
    m = vit_amd.CLIPHBA([f"c{i}" for i in range(5)], "ViT-L/14", pos_embedding=True, clip_model=_tiny_clip())
    vit_amd.apply_dora_to_ViT(m, n_vision_layers=2, n_transformer_layers=1, r=4)
    vit_amd.switch_dora_layers(m, freeze_all=True, dora_state=True)
    images = torch.randn(4, 3, 32, 32)
    m.clip_model.set_attention_fp8(True, long_sequences=True)
    k_off = prefix_key(m, images)
    m.clip_model.set_attention_fp8(True, long_sequences=True, prequantize=True)
    k_on = prefix_key(m, images)
    assert k_on == k_off and len(k_on) == 7 and k_on[-1] is True  # the layout test_fp8_long_host.py pins
    # the text prefix key is built from the two older switches alone
    src = inspect.getsource(type(m.clip_model)._text_prefix)
    assert "attention_fp8_long" in src and "attention_fp8_pre" not in src
