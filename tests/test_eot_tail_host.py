"""CPU: host logic of the CLIP text tower's EOT tail -- the declared entry points and their
refusals, the routing rule over its truth table, the switch on ``CLIP`` / ``CLIPHBA`` and, with the launch layer
stubbed, the launches ``encode_text`` issues with the switch off (the list as it was before the tail existed,
written out below), on in a training step, on under ``no_grad`` and with two trainable text blocks."""
import itertools
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------- entry points

def test_header_declares_and_loader_binds_the_entry_points():
    from vit_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vit_hip.h")).read(), flags=re.S)
    for name in ("vit_sdpa_row1_fwd", "vit_sdpa_row1_count"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", txt), name
        assert name in _lib.exported_symbols()
    assert re.search(r"\bint\s+vit_sdpa_row1_count\s*\(\s*int\s+reset\s*\)\s*;", txt)
    assert re.search(r"vit_sdpa_row1_fwd\s*\(\s*int dtype, int B, int H, int N, int head_dim, const void\* qkv, "
                     r"int64_t ld_qkv,\s*const int64_t\* qrow, int causal, void\* o_row, int64_t ld_o, "
                     r"float\* lse_row, float scale,\s*void\* stream\s*\)\s*;", txt)
    i32, i64, f32, vp = _lib.i32, _lib.i64, _lib.f32, _lib.vp
    assert _lib.SIGNATURES["vit_sdpa_row1_fwd"] == [i32] * 5 + [vp, i64, vp, i32, vp, i64, vp, f32, vp]
    assert _lib.SIGNATURES["vit_sdpa_row1_count"] == [i32]
    assert _lib.load().vit_abi_version() == 10  # additive
    from vit_amd import ops
    assert callable(ops.sdpa_row1_fwd)


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """The refusals come before anything touches the device, so they can be checked without one."""
    from vit_amd import _lib
    lib = _lib.load()
    invalid = 1  # hipErrorInvalidValue
    a = 1 << 20  # an aligned non-null address; never dereferenced by a refused call
    fwd = lambda dt=1, B=2, H=2, N=17, hd=64, ldq=384, ldo=128, q=a, r=a, o=a, l=a, causal=1: \
        lib.vit_sdpa_row1_fwd(dt, B, H, N, hd, q, ldq, r, causal, o, ldo, l, 0.125, None)
    lib.vit_sdpa_row1_count(1)
    assert lib.vit_sdpa_row1_count(0) == 0
    for rc in (fwd(hd=32), fwd(hd=128), fwd(N=0), fwd(N=-3), fwd(N=2049), fwd(q=None), fwd(r=None), fwd(o=None),
               fwd(l=None), fwd(ldq=386), fwd(ldo=130), fwd(dt=0, ldq=386), fwd(dt=0, ldo=130), fwd(ldq=256),
               fwd(q=a + 8), fwd(o=a + 4), fwd(dt=2), fwd(causal=0, hd=32), fwd(causal=0, N=2049)):
        assert rc == invalid
    assert lib.vit_sdpa_row1_count(0) == 0


# ---------------------------------------------------------------------------- routing

def test_row_tail_routing_truth_table():
    from vit_amd.model import wants_row_tail as w
    for req, fp8, up in itertools.product((False, True), repeat=3):
        assert w(req, fp8, up) is (req and not fp8 and not up)
    assert w(True) is True and w(None) is False and w(False) is False


def test_cfg_route_reads_the_block_cfg():
    from vit_amd.model import _cfg_row_tail as r
    rows = torch.tensor([3, 1], dtype=torch.int64)
    assert r(dict(row_tail=rows), False) is rows
    assert r(dict(row_tail=rows), True) is None            # something upstream of proj needs a gradient
    assert r(dict(row_tail=rows, attn_fp8=True), False) is None
    assert r(dict(), False) is None and r(dict(row_tail=None), False) is None


def _tiny_clip(dtype=torch.float32, context_length=16):
    from vit_amd import clip
    return clip.CLIP(embed_dim=96, image_resolution=32, vision_layers=2, vision_width=128, vision_patch_size=8,
                     context_length=context_length, vocab_size=64, transformer_width=128, transformer_heads=2,
                     transformer_layers=3, compute_dtype=dtype)


def test_switch_sets_and_clears_the_flag():
    import vit_amd
    cm = _tiny_clip()
    assert cm.eot_tail is False
    cm.set_eot_tail()
    assert cm.eot_tail is True
    cm.set_eot_tail(False)
    assert cm.eot_tail is False
    prompts = torch.zeros(2, 1, 16, dtype=torch.int64)
    for kw, want in (({}, False), (dict(eot_tail=False), False), (dict(eot_tail=True), True)):
        m = vit_amd.CLIPHBA(["a", "b"], "ViT-L/14", clip_model=_tiny_clip(), tokenized_prompts=prompts, **kw)
        assert m.clip_model.eot_tail is want and m.clip_model.cls_tail is False


# ---------------------------------------------------------------------------- recorded launches

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


S, W, H = 5, 128, 2
EOT_POS = (3, 9, 1, 14, 6)  # unequal prompt lengths


def _prompts(Lq):
    t = torch.zeros(S, Lq, dtype=torch.int64)
    for s, e in enumerate(EOT_POS):
        e = min(e, Lq - 1)
        t[s, :e] = torch.arange(1, e + 1) % 50 + 1
        t[s, e] = 63
    return t


def _trainable(cm, text_blocks=1):
    """Everything frozen but out_proj.weight of the last ``text_blocks`` text blocks (where the adapters sit)."""
    for p in cm.parameters():
        p.requires_grad = False
    for blk in list(cm.transformer.resblocks)[-text_blocks:]:
        blk.attn.out_proj.weight.requires_grad = True
    return cm


def _names(rec):
    return [nm for nm, a in rec]


def _sdpa(rec):
    return [(nm, a[1:4]) for nm, a in rec if nm.startswith("vit_sdpa")]


# encode_text with one trainable text block of three, f32, as the tree issued it before the EOT tail existed:
# the token embedding, two frozen blocks on the forward-only chain, the trainable block on the training chain
# (fc1 on the epilogue that also stores act'), the pool head.
_FWD_ONLY_BLOCK = ["vit_layer_norm_fwd", "vit_linear_fwd", "vit_sdpa_fwd", "vit_linear_fwd", "vit_layer_norm_fwd",
                   "vit_linear_fwd", "vit_linear_fwd"]
_POOL_HEAD = ["vit_gather_rows", "vit_layer_norm_fwd", "vit_gemm"]
DENSE_FWD = ["vit_token_embed"] + _FWD_ONLY_BLOCK * 3 + _POOL_HEAD
# the tail: ln_1 and qkv, the one-query kernel, the EOT rows of the stream, then the dense block's four launches
TAIL_BLOCK = ["vit_layer_norm_fwd", "vit_linear_fwd", "vit_sdpa_row1_fwd", "vit_gather_rows", "vit_linear_fwd",
              "vit_layer_norm_fwd", "vit_linear_fwd", "vit_linear_fwd"]
TAIL_FWD = ["vit_token_embed"] + _FWD_ONLY_BLOCK * 2 + TAIL_BLOCK + _POOL_HEAD


@pytest.mark.parametrize("Lq", [16, 77])
def test_switch_off_issues_the_dense_list(launches, Lq):
    text = _prompts(Lq)
    cm = _trainable(_tiny_clip(context_length=Lq))
    y = cm.encode_text(text)
    assert y.shape == (S, 96)
    assert _names(launches) == DENSE_FWD
    assert _sdpa(launches) == [("vit_sdpa_fwd", (S, H, Lq))] * 3
    off_fwd = list(launches)
    del launches[:]
    y.sum().backward()
    off_bwd = _names(launches)
    assert "vit_sdpa_bwd" not in off_bwd and "vit_scatter_rows" in off_bwd
    # a second model with the switch set and cleared again: the same launches with the same scalar arguments
    del launches[:]
    cm2 = _trainable(_tiny_clip(context_length=Lq))
    cm2.set_eot_tail(True)
    cm2.set_eot_tail(False)
    y2 = cm2.encode_text(text)
    scalars = lambda rec: [(nm, tuple(v for v in a if isinstance(v, (int, float)) and not isinstance(v, bool)
                                      and abs(v) < 1 << 20)) for nm, a in rec]
    assert scalars(launches) == scalars(off_fwd)
    del launches[:]
    y2.sum().backward()
    assert _names(launches) == off_bwd


@pytest.mark.parametrize("Lq", [16, 77])
def test_switch_on_training_step_runs_the_one_query_kernel(launches, Lq):
    from vit_amd import model
    text = _prompts(Lq)
    cm = _trainable(_tiny_clip(context_length=Lq))
    cm.cache_frozen_text = False  # every call below issues the frozen blocks too
    y_off = cm.encode_text(text)
    del launches[:]
    y_off.sum().backward()
    off_bwd = list(launches)
    del launches[:]
    cm.set_eot_tail(True)
    y = cm.encode_text(text)
    assert y.shape == (S, 96)
    assert _names(launches) == TAIL_FWD
    # one one-query launch in place of the last block's dense attention
    assert _sdpa(launches) == [("vit_sdpa_fwd", (S, H, Lq))] * 2 + [("vit_sdpa_row1_fwd", (S, H, Lq))]
    fwd = [a for nm, a in launches if nm == "vit_sdpa_row1_fwd"][0]
    assert fwd[6] == 3 * W and fwd[8] == 1 and fwd[10] == W  # qkv rows, causal, the compact o: row stride D
    gathered = [a for nm, a in launches if nm == "vit_gather_rows"]
    assert [a[0] for a in gathered] == [S, S] and gathered[0][3] == W and gathered[1][3] == W
    # the GEMMs and LayerNorms behind attention see S rows, those in front of it S * Lq
    tail = launches[-len(TAIL_BLOCK) - len(_POOL_HEAD):-len(_POOL_HEAD)]
    rows = [a[3] for nm, a in tail if nm == "vit_linear_fwd"]
    assert rows == [S * Lq, S, S, S], rows
    del launches[:]
    y.sum().backward()
    names = _names(launches)
    assert "vit_sdpa_bwd" not in names and "vit_sdpa_cls1_bwd" not in names
    assert not [nm for nm in names if nm.startswith("vit_sdpa")]
    # the padded backward: P rows per prompt (64 above TAIL_PAD, else the context length)
    P = model.tail_pad(Lq)
    assert P == (64 if Lq > 64 else Lq)
    wg = [a for nm, a in launches if nm.startswith("vit_linear_wgrad") or nm.startswith("vit_linear_dgrad")]
    assert wg, names
    pads = [a for nm, a in launches if nm == "vit_copy_rows_padded"]
    assert pads and all(a[1] == S for a in pads)
    # the same kinds of launches as the dense backward but for the row padding: nothing new, nothing missing
    assert set(names) - {"vit_copy_rows_padded"} == set(_names(off_bwd)) - {"vit_copy_rows_padded"}


def test_switch_on_no_grad_runs_the_same_forward(launches):
    text = _prompts(16)
    cm = _trainable(_tiny_clip())
    cm.set_eot_tail(True)
    with torch.no_grad():
        y = cm.encode_text(text)
    assert y.shape == (S, 96)
    assert _names(launches) == TAIL_FWD
    assert _sdpa(launches) == [("vit_sdpa_fwd", (S, H, 16))] * 2 + [("vit_sdpa_row1_fwd", (S, H, 16))]


def test_two_trainable_text_blocks_run_dense(launches):
    """The last block's input then needs a gradient: the rule sends it dense, attention backward included."""
    text = _prompts(16)
    cm = _trainable(_tiny_clip(), text_blocks=2)
    cm.set_eot_tail(True)
    y = cm.encode_text(text)
    assert _names(launches) == DENSE_FWD
    del launches[:]
    y.sum().backward()
    assert _sdpa(launches) == [("vit_sdpa_bwd", (S, H, 16))]
    assert "vit_sdpa_row1_fwd" not in _names(launches)
    # under no_grad nothing needs a gradient: the tail again
    del launches[:]
    with torch.no_grad():
        cm.encode_text(text)
    assert _sdpa(launches)[-1] == ("vit_sdpa_row1_fwd", (S, H, 16))


def test_trainable_in_proj_and_fp8_passes_run_dense(launches):
    text = _prompts(16)
    cm = _trainable(_tiny_clip())
    cm.transformer.resblocks[-1].attn.in_proj_bias.requires_grad = True
    cm.set_eot_tail(True)
    cm.encode_text(text)
    assert "vit_sdpa_row1_fwd" not in _names(launches)
    del launches[:]
    cm.transformer.resblocks[-1].attn.in_proj_bias.requires_grad = False
    cm.set_attention_fp8(True)
    with torch.no_grad():
        cm.encode_text(text)
    assert _sdpa(launches) == [("vit_sdpa_fwd_fp8", (S, H, 16))] * 3


def test_positions_are_clamped_for_the_gather():
    from vit_amd.model import _row_tail_flat
    rows = torch.tensor([-5, 0, 7, 21], dtype=torch.int64)
    assert _row_tail_flat(rows, 4, 16).tolist() == [0, 16, 39, 63]
    with pytest.raises(ValueError):
        _row_tail_flat(rows.to(torch.int32), 4, 16)
    with pytest.raises(ValueError):
        _row_tail_flat(rows, 3, 16)
