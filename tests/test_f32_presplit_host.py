"""CPU: the pre-split weight image of the fp32 "high" GEMMs and the host-side surface of its switch.

- ``image_ref`` / ``image_inverse`` restate the image in torch: per 128-byte block of 32 reduction values, four
  16-byte ``hi`` chunks then four ``lo`` chunks, ``hi`` chunk ``g`` holding as element ``j`` the bf16 ``hi`` of
  ``k = 16 (j >> 2) + 4 g + (j & 3)``.  tests/test_gpu_f32_presplit.py imports them as its reference.  The chunk order
  is checked here against a loop that restates what the kernel does with an f32 operand -- lane group ``g`` reads
  chunk ``c = 4 h + g`` in k half ``h`` (``frag``) and packs value ``t`` of that read as element ``j = 4 h + t``
  (``split8``) -- not against the permutation ``image_ref`` is written with;
- the setter's keyword, the getter and the environment variables;
- the new symbols, with the ABI still 10;
- the register metadata of the new kernels in the built object;
- both frozen-prefix cache keys are the same with and without pre-splitting.
"""
import os
import subprocess
import sys

import pytest
import torch

import test_f32_split_host as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def image_ref(w):
    """The image of an f32 matrix [rows, red] (red % 32 == 0): an f32-typed tensor [rows, red] of the same bytes the
    pre-pass writes."""
    rows, red = w.shape
    assert red % 32 == 0
    hi, lo = H.split(w)

    def chunks(v):  # [rows, kb, h, g, t] -> [rows, kb, g, (h, t)]
        return v.reshape(rows, red // 32, 2, 4, 4).permute(0, 1, 3, 2, 4).reshape(rows, red // 32, 4, 8)

    blocks = torch.cat([chunks(hi), chunks(lo)], dim=2)  # [rows, kb, 8 chunks, 8 bf16]
    return blocks.to(torch.bfloat16).contiguous().view(rows, red * 2).view(torch.float32)


def image_inverse(img):
    """(hi, lo) as f32 matrices [rows, red] from an image."""
    rows, red = img.shape
    blocks = img.contiguous().view(torch.bfloat16).float().reshape(rows, red // 32, 2, 4, 2, 4)  # kb, hi/lo, g, h, t
    back = blocks.permute(0, 1, 2, 4, 3, 5).reshape(rows, red // 32, 2, 32)
    return back[:, :, 0].reshape(rows, red), back[:, :, 1].reshape(rows, red)


def scaled_randn(rows, cols, seed):
    """randn with |x| in [2^-20, 2^20] and not bf16-valued for nearly every element: lo != 0."""
    x = torch.randn(rows, cols, generator=torch.Generator().manual_seed(seed))
    return torch.copysign(x.abs().clamp(2.0 ** -20, 2.0 ** 20), x)


@pytest.fixture(autouse=True)
def _restore_highest():
    yield
    from vit_amd import ops
    ops.set_float32_matmul_precision("highest")


@pytest.mark.parametrize("shape", [(128, 32), (136, 96), (64, 1024)], ids=str)
def test_image_round_trip_and_error(shape):
    w = scaled_randn(*shape, seed=11 + shape[1])
    hi, lo = H.split(w)
    assert float((lo != 0).float().mean()) > 0.9
    img = image_ref(w)
    assert img.shape == w.shape and img.dtype == torch.float32 and img.is_contiguous()  # the weight's pitch and size
    bhi, blo = image_inverse(img)
    assert torch.equal(bhi, hi) and torch.equal(blo, lo)
    assert bool(((w - bhi - blo).abs() <= 2.0 ** -16 * w.abs()).all())
    # the transposed form is the plain form of the transpose
    if shape[0] % 32 == 0:
        thi, tlo = image_inverse(image_ref(w.T.contiguous()))
        assert torch.equal(thi, hi.T) and torch.equal(tlo, lo.T)


def test_chunk_order_is_what_the_fragment_reads_pack():
    rows, red = 24, 96
    w = scaled_randn(rows, red, seed=5)
    hi, lo = H.split(w)
    bits = image_ref(w).view(torch.bfloat16).float()  # [rows, red * 2] bf16 elements
    for kb in range(red // 32):
        for g in range(4):          # lane group
            packs = {"hi": [None] * 8, "lo": [None] * 8}
            for h in range(2):      # frag: k half h reads 16-byte chunk c = 4 h + g of the f32 block
                c = 4 * h + g
                for t in range(4):  # split8: value t of that read is element j = 4 h + t
                    k = kb * 32 + 4 * c + t
                    assert 4 * c + t == 16 * h + 4 * g + t
                    packs["hi"][4 * h + t] = hi[:, k]
                    packs["lo"][4 * h + t] = lo[:, k]
            # the image read: chunk g (the h = 0 read) is the hi pack, chunk 4 + g (the h = 1 read) the lo pack
            for j in range(8):
                assert torch.equal(bits[:, kb * 64 + g * 8 + j], packs["hi"][j]), (kb, g, j)
                assert torch.equal(bits[:, kb * 64 + (4 + g) * 8 + j], packs["lo"][j]), (kb, g, j)
                assert torch.equal(packs["hi"][j], hi[:, kb * 32 + 16 * (j >> 2) + 4 * g + (j & 3)])


def test_setter_keyword_and_getter():
    import vit_amd
    from vit_amd import _lib
    lib = _lib.load()
    assert vit_amd.get_float32_matmul_presplit() is False or os.environ.get("VIT_F32_MATMUL_PRESPLIT") == "1"
    vit_amd.set_float32_matmul_precision("high", presplit_weights=True)
    assert vit_amd.get_float32_matmul_presplit() is True and vit_amd.get_float32_matmul_precision() == "high"
    vit_amd.set_float32_matmul_precision("high")          # the keyword resets on every call
    assert vit_amd.get_float32_matmul_presplit() is False and vit_amd.get_float32_matmul_precision() == "high"
    vit_amd.set_float32_matmul_precision("high", True)
    assert vit_amd.get_float32_matmul_presplit() is True
    with pytest.raises(ValueError, match="presplit_weights"):
        vit_amd.set_float32_matmul_precision("highest", presplit_weights=True)
    assert vit_amd.get_float32_matmul_presplit() is True and lib.vit_gemm_f32_precision(-1) == 1  # nothing changed
    lib.vit_gemm_f32_precision(0)                          # the C switch alone: "highest" has no images
    assert vit_amd.get_float32_matmul_presplit() is False
    lib.vit_gemm_f32_precision(1)
    vit_amd.set_float32_matmul_precision("highest")        # existing positional calls keep working
    assert vit_amd.get_float32_matmul_presplit() is False and vit_amd.get_float32_matmul_precision() == "highest"
    vit_amd.set_float32_matmul_precision("high")
    assert vit_amd.get_float32_matmul_presplit() is False


def test_environment_variables_set_the_initial_state():
    code = ("import sys; sys.path.insert(0, %r); from vit_amd import ops; "
            "print(ops.get_float32_matmul_precision(), ops.get_float32_matmul_presplit())"
            % os.path.join(ROOT, "vit-project_amd"))
    env = {k: v for k, v in os.environ.items() if k not in ("VIT_F32_MATMUL", "VIT_F32_MATMUL_PRESPLIT")}
    for extra, want in (({"VIT_F32_MATMUL": "high", "VIT_F32_MATMUL_PRESPLIT": "1"}, ["high", "True"]),
                        ({"VIT_F32_MATMUL": "high"}, ["high", "False"]),
                        ({"VIT_F32_MATMUL_PRESPLIT": "1"}, ["highest", "False"]),
                        ({"VIT_F32_MATMUL": "high", "VIT_F32_MATMUL_PRESPLIT": "0"}, ["high", "False"])):
        out = subprocess.run([sys.executable, "-c", code], env=dict(env, **extra), capture_output=True, text=True,
                             check=True).stdout.split()
        assert out[-2:] == want, (extra, out)


def test_sweep_workers_are_handed_the_switch(monkeypatch):
    import vit_amd
    from vit_amd import sweep as S
    seen = {}

    def fake_run_sweep(*a, **kw):
        seen["state"] = (vit_amd.get_float32_matmul_precision(), vit_amd.get_float32_matmul_presplit())
        seen["kw"] = kw
        return []

    class Q:
        def put(self, item):
            pass

    monkeypatch.setattr(S, "run_sweep", fake_run_sweep)
    S._sweep_worker(0, 1, None, None, {}, [], {"float32_matmul": "high", "float32_matmul_presplit": True}, Q(), [])
    assert seen["state"] == ("high", True) and "float32_matmul_presplit" not in seen["kw"]
    S._sweep_worker(0, 1, None, None, {}, [], {"float32_matmul": "high"}, Q(), [])
    assert seen["state"] == ("high", False)


def test_new_symbols_are_declared_and_bound():
    from vit_amd import _lib
    lib = _lib.load()
    i32, i64, vp = _lib.i32, _lib.i64, _lib.vp
    assert lib.vit_abi_version() == 10  # additive
    hdr = open(os.path.join(ROOT, "include", "vit_hip.h")).read()
    for name in ("vit_gemm_f32_weight_image", "vit_linear_fwd_wimg", "vit_linear_dgrad_wimg",
                 "vit_gemm_f32_presplit_count"):
        assert name in _lib.exported_symbols() and hasattr(lib, name) and f"int {name}(" in hdr
    assert _lib.SIGNATURES["vit_gemm_f32_presplit_count"] == [i32]
    assert _lib.SIGNATURES["vit_gemm_f32_weight_image"] == [i32, i32, vp, i64, i32, vp, vp]
    # the arguments of the existing entries plus one image pointer in front of the stream
    for name in ("vit_linear_fwd", "vit_linear_dgrad"):
        old = _lib.SIGNATURES[name]
        assert _lib.SIGNATURES[name + "_wimg"] == old[:-1] + [vp] + old[-1:]
    assert lib.vit_gemm_f32_presplit_count(1) >= 0 and lib.vit_gemm_f32_presplit_count(0) == 0
    # the shape rule is checked on the host before anything is launched: no GPU needed to be refused
    assert lib.vit_gemm_f32_weight_image(64, 40, 16, 40, 0, 16, None) == 1
    assert lib.vit_gemm_f32_weight_image(40, 64, 16, 64, 1, 16, None) == 1
    assert lib.vit_gemm_f32_weight_image(64, 64, 20, 64, 0, 16, None) == 1   # misaligned W
    assert lib.vit_gemm_f32_weight_image(64, 64, 16, 66, 0, 16, None) == 1   # rows not 16-byte aligned
    assert lib.vit_gemm_f32_weight_image(64, 64, 16, 64, 0, 24, None) == 1   # misaligned image


def test_image_kernels_have_no_spills_and_fit_two_workgroups_per_cu():
    obj = os.path.join(ROOT, "vit-project_amd", "csrc", "build", "gemm.o")
    if not os.path.exists(obj) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("gemm.o not built / no ROCm LLVM tools")
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kres.sh"), obj, "4f32w"], capture_output=True, text=True,
                         check=True).stdout.splitlines()
    gemms = [l for l in out if "gemm_kernel" in l or "gemm_sk_kernel" in l]
    # store, residual, two pairs, two act-only forms, two act' input gradients; each as a plain and a stream-K kernel
    assert len(gemms) == 16 and len(out) == 18, out
    assert not [l for l in out if "f32m" in l]
    bad = [l for l in out if " spill 0 " not in l or " priv 0 " not in l]
    assert not bad, bad[:5]
    assert all(int(l.split()[0]) <= 256 for l in out)
    assert all(int(l.split()[-1]) == 0 for l in gemms)  # the 64 KiB ring is dynamic LDS: no static allocation


def test_cache_keys_do_not_depend_on_presplitting(monkeypatch):
    import vit_amd
    from vit_amd import clip, ops
    from vit_amd.prefix_cache import prefix_key
    m = vit_amd.CLIPHBA([f"c{i}" for i in range(5)], "ViT-L/14", pos_embedding=True, clip_model=H._tiny_clip())
    vit_amd.apply_dora_to_ViT(m, n_vision_layers=2, n_transformer_layers=1, r=4)
    vit_amd.switch_dora_layers(m, freeze_all=True, dora_state=True)
    images = torch.randn(4, 3, 32, 32)
    cm = H._tiny_clip()
    cm.cache_frozen_text = True
    for p in cm.parameters():
        p.requires_grad = False
    for p in cm.transformer.resblocks[-1].parameters():
        p.requires_grad = True
    monkeypatch.setattr(ops, "token_embed", lambda text, table, pos: table[text] + pos)
    monkeypatch.setattr(clip, "run_block", lambda x, params, cfg: x)
    text = torch.randint(0, H.CFG.vocab_size, (3, H.CFG.context_length))

    def text_key():
        cm._text_cache = None
        cm._text_prefix(text)
        return cm._text_cache[0]

    vit_amd.set_float32_matmul_precision("high")
    k_img, k_text = prefix_key(m, images), text_key()
    vit_amd.set_float32_matmul_precision("high", presplit_weights=True)
    assert prefix_key(m, images) == k_img and len(k_img) == 7
    hit = cm._text_cache
    cm._text_prefix(text)
    assert cm._text_cache is hit, "a text cache filled in-loop was rebuilt under pre-splitting"
    assert text_key() == k_text
