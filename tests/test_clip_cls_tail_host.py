"""CPU: host logic of the CLIP visual tower's class-token tail -- the two routing rules over their
truth tables, the switch on ``CLIP`` / ``CLIPHBA``, the declared entry points (tests/test_host_abi.py then checks that
the built library exports them) and, with the launch layer stubbed, which attention entry points the tower's last
block is issued on."""
import itertools
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tail_routing_truth_table():
    from vit_amd.model import wants_cls_tail as w
    for enabled, cls_only, pool, fp8 in itertools.product((False, True), (False, True), ("token", "avg"), (False, True)):
        assert w(enabled, cls_only, pool, fp8) is (enabled and cls_only and pool == "token" and not fp8)


def test_one_query_routing_truth_table():
    """Only a block that runs the tail and asks for it, unmasked, not fp8, with a qkv bias that needs no gradient."""
    from vit_amd.model import wants_cls_attn1 as w
    for tail, req, causal, fp8, bias in itertools.product((False, True), repeat=5):
        assert w(tail, req, causal, fp8, bias) is (tail and req and not causal and not fp8 and not bias)
    assert w(True, True) is True and w(True, None) is False and w(None, True) is False


def test_cfg_route_reads_the_block_cfg():
    from vit_amd.model import _cfg_attn1 as r
    base = dict(cls_tail=True, cls_attn1=True, causal=False, attn_fp8=False)
    assert r(base, False) is True and r(base, True) is False
    assert r(dict(base, cls_tail=False), False) is False   # the key alone is not honoured
    assert r(dict(cls_tail=True), False) is False          # the ViT path never sets it
    assert r(dict(base, causal=True), False) is False and r(dict(base, attn_fp8=True), False) is False


def _tiny_clip(dtype=torch.float32):
    from vit_amd import clip
    return clip.CLIP(embed_dim=96, image_resolution=72, vision_layers=3, vision_width=128, vision_patch_size=8,
                     context_length=16, vocab_size=64, transformer_width=128, transformer_heads=2,
                     transformer_layers=2, compute_dtype=dtype)


def test_switch_sets_and_clears_the_flag():
    import vit_amd
    cm = _tiny_clip()
    assert cm.cls_tail is False
    cm.set_cls_tail()
    assert cm.cls_tail is True
    cm.set_cls_tail(False)
    assert cm.cls_tail is False
    prompts = torch.zeros(2, 1, 16, dtype=torch.int64)
    for kw, want in (({}, False), (dict(cls_tail=False), False), (dict(cls_tail=True), True)):
        m = vit_amd.CLIPHBA(["a", "b"], "ViT-L/14", clip_model=_tiny_clip(), tokenized_prompts=prompts, **kw)
        assert m.clip_model.cls_tail is want
        m.clip_model.set_cls_tail(not want)
        assert m.clip_model.cls_tail is (not want)


def test_header_declares_and_loader_binds_the_entry_points():
    from vit_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vit_hip.h")).read(), flags=re.S)
    for name in ("vit_sdpa_cls1_fwd", "vit_sdpa_cls1_bwd", "vit_sdpa_cls1_count"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", txt), name
        assert name in _lib.exported_symbols()
    assert re.search(r"\bint\s+vit_sdpa_cls1_count\s*\(\s*int\s+reset\s*\)\s*;", txt)
    i32, i64, f32, vp = _lib.i32, _lib.i64, _lib.f32, _lib.vp
    assert _lib.SIGNATURES["vit_sdpa_cls1_fwd"] == [i32] * 5 + [vp, i64, vp, i64, vp, f32, vp]
    assert _lib.SIGNATURES["vit_sdpa_cls1_bwd"] == [i32] * 5 + [vp, i64, vp, i64, vp, i64, vp, vp, i64, f32, vp]
    assert _lib.SIGNATURES["vit_sdpa_cls1_count"] == [i32]
    assert _lib.load().vit_abi_version() == 10  # additive


def test_counter_reads_and_resets_without_a_gpu():
    from vit_amd import _lib
    lib = _lib.load()
    lib.vit_sdpa_cls1_count(1)
    assert lib.vit_sdpa_cls1_count(0) == 0


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """The refusals come before anything touches the device, so they can be checked without one."""
    from vit_amd import _lib
    lib = _lib.load()
    invalid = 1  # hipErrorInvalidValue
    a = 1 << 20  # an aligned non-null address; never dereferenced by a refused call
    fwd = lambda dt=1, B=2, H=2, N=17, hd=64, ldq=384, ldo=128, q=a, o=a, l=a: \
        lib.vit_sdpa_cls1_fwd(dt, B, H, N, hd, q, ldq, o, ldo, l, 0.125, None)
    bwd = lambda dt=1, B=2, H=2, N=17, hd=64, ldq=384, ldo=128, ldd=128, ldg=384, q=a, g=a: \
        lib.vit_sdpa_cls1_bwd(dt, B, H, N, hd, q, ldq, a, ldo, a, ldd, a, g, ldg, 0.125, None)
    lib.vit_sdpa_cls1_count(1)
    for rc in (fwd(hd=32), fwd(N=0), fwd(N=-3), fwd(N=2049), fwd(ldq=386), fwd(ldo=130), fwd(dt=0, ldq=386),
               fwd(ldq=256), fwd(q=a + 8), fwd(o=None), fwd(l=None), fwd(dt=2),
               bwd(hd=32), bwd(N=0), bwd(N=2049), bwd(ldq=386), bwd(ldo=130), bwd(ldd=130), bwd(ldg=386),
               bwd(ldg=256), bwd(g=a + 2), bwd(q=None)):
        assert rc == invalid
    assert lib.vit_sdpa_cls1_count(0) == 0


class _NoSide:
    """The model's two-stream helper with no second stream (what it is on a device without one)."""
    on = False

    def __init__(self, dev):
        pass

    def run(self, fn):
        return fn()

    def join(self):
        pass

    def guard(self, *ts):
        pass


@pytest.fixture
def launches(monkeypatch):
    """Every kernel launch recorded as (entry point, arguments) instead of run; tensors live on the CPU."""
    from vit_amd import _lib, model, ops
    rec = []
    monkeypatch.setattr(ops, "call", lambda name, *a: rec.append((name, a)))
    monkeypatch.setattr(_lib, "call", lambda name, *a: rec.append((name, a)))
    monkeypatch.setattr(ops, "_streamk", lambda device, stream=None: None)
    monkeypatch.setattr(_lib, "require_gpu", lambda t: None)
    monkeypatch.setattr(_lib, "stream_ptr", lambda device=None: 0)
    monkeypatch.setattr(model, "_Side", _NoSide)
    real = _lib.load()

    class Lib:  # the host-only queries answer; the one launch made through the handle is recorded
        def __getattr__(self, name):
            return getattr(real, name)

        def vit_linear_wgrad_partials2(self, *a):
            rec.append(("vit_linear_wgrad_partials2", a))
            return 0

    monkeypatch.setattr(_lib, "lib", lambda: Lib())
    return rec


B, N, W, H = 3, 82, 128, 2


def _trainable_tail(cm, bias=False):
    """Everything frozen but out_proj.weight of the last two visual blocks (where the adapters sit)."""
    for p in cm.parameters():
        p.requires_grad = False
    for blk in list(cm.visual.transformer.resblocks)[-2:]:
        blk.attn.out_proj.weight.requires_grad = True
    cm.visual.transformer.resblocks[-1].attn.in_proj_bias.requires_grad = bias
    return cm


def _names(rec, prefix="vit_sdpa"):
    return [(nm, a[1:4]) for nm, a in rec if nm.startswith(prefix)]


def _tail_launches(rec):
    """Launches only the class-token tail makes."""
    return [nm for nm, a in rec if nm in ("vit_sdpa_fwd_cls", "vit_sdpa_cls1_fwd", "vit_sdpa_cls1_bwd",
                                          "vit_layer_norm_bwd_cls")]


def test_last_visual_block_runs_the_one_query_kernels(launches):
    cm = _trainable_tail(_tiny_clip())
    cm.set_cls_tail(True)
    img = torch.zeros(B, 3, 72, 72)
    y = cm.encode_image(img)
    assert y.shape == (B, 96)
    assert _names(launches) == [("vit_sdpa_fwd", (B, H, N))] * 2 + [("vit_sdpa_cls1_fwd", (B, H, N))]
    fwd = [a for nm, a in launches if nm == "vit_sdpa_cls1_fwd"][0]
    assert fwd[6] == 3 * W and fwd[8] == W  # the compact o: row stride D
    gathered = [a for nm, a in launches if nm == "vit_gather_rows"]
    assert gathered[-1][0] == B  # the pool head gathers B rows of the [B, 1, W] output
    del launches[:]
    y.sum().backward()
    # the last block's backward: the one-query kernel from the class rows of dO, 64 padded rows apart (the block
    # in front of it needs its out_proj gradient alone: no attention backward)
    assert _names(launches) == [("vit_sdpa_cls1_bwd", (B, H, N))]
    bwd = [a for nm, a in launches if nm == "vit_sdpa_cls1_bwd"][0]
    assert bwd[8] == W and bwd[10] == 64 * W and bwd[13] == 3 * W
    assert not [1 for nm, a in launches if nm == "vit_copy_rows_padded" and a[1:3] == (B, W) and a[6] == N * W], \
        "no zero-filled dense dO"


def test_switch_off_cut_and_bias_gradient_keep_todays_route(launches):
    cm = _trainable_tail(_tiny_clip())
    img = torch.zeros(B, 3, 72, 72)
    cm.encode_image(img).sum().backward()  # the switch is off
    assert not _tail_launches(launches)
    del launches[:]
    cm.set_cls_tail(True)
    px, first = cm.visual_prefix(img)
    assert first == 1 and px.shape == (B, N, W) and not _tail_launches(launches)
    del launches[:]
    with torch.no_grad():
        cm.encode_image(prefix=px)  # the forward-only chain takes the tail too
    assert _names(launches) == [("vit_sdpa_fwd", (B, H, N)), ("vit_sdpa_cls1_fwd", (B, H, N))]
    del launches[:]
    cm.set_attention_fp8(True)
    with torch.no_grad():
        cm.encode_image(img)  # fp8 passes keep the dense block
    assert _names(launches) == [("vit_sdpa_fwd_fp8", (B, H, N))] * 3
    cm.set_attention_fp8(False)
    del launches[:]
    _trainable_tail(cm, bias=True)
    cm.encode_image(prefix=px).sum().backward()  # a trainable qkv bias: the tail with its dense attention
    assert _names(launches) == [("vit_sdpa_fwd", (B, H, N)), ("vit_sdpa_fwd_cls", (B, H, N)),
                                ("vit_sdpa_bwd", (B, H, N))]


def test_vit_path_never_asks_for_the_one_query_kernels(launches):
    import vit_amd
    m = vit_amd.VisionTransformer(img_size=128, patch_size=16, embed_dim=128, depth=2, num_heads=2, num_classes=10)
    prev = vit_amd.set_cls_tail(True)
    try:
        m(torch.zeros(2, 3, 128, 128)).sum().backward()
    finally:
        vit_amd.set_cls_tail(prev)
    assert [nm for nm, a in launches if nm.startswith("vit_sdpa")] == ["vit_sdpa_fwd", "vit_sdpa_fwd_cls",
                                                                      "vit_sdpa_bwd", "vit_sdpa_bwd"]
