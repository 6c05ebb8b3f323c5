"""CPU: the host-side surface and the arithmetic rule of the fp32 "high" GEMM mode (bf16x3).

- ``split`` / ``x3_f64`` restate the kernel's rule in torch: ``hi = bf16_rne(x)``, ``lo = bf16_rne(x - hi)``, the
  three products ``hi*lo + lo*hi + hi*hi`` summed in float64.  tests/test_gpu_f32_split.py imports them as its
  reference.  The restatement alone stays inside the contract's bound

      |C - C64| <= (3 * 2^-18 + (R + 3) * 2^-24) * |P| |Q|^T

  (three terms of the typical size 2^-18 -- each operand's hi + lo remainder and the dropped lo*lo product -- and
  R + 3 roundings of an f32 accumulation), and is exact, and distinguishable from the full product and from
  hi*hi, on 9-bit integers;
- the setter and getter, with the library loaded and no GPU;
- both frozen-prefix cache keys follow the mode;
- no f32m kernel instantiation spills or uses scratch (register metadata of the built object).
"""
import os
import re
import subprocess
import sys

import pytest
import torch

from oracle import clip_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = CR.CLIP_TINY


def split(x):
    """(hi, lo) of an f32 tensor, as f32 tensors holding bf16 values."""
    x = x.float()
    hi = x.to(torch.bfloat16).float()
    lo = (x - hi).to(torch.bfloat16).float()
    return hi, lo


def x3_f64(p, q):
    """p [M, R] q [N, R]^T as the kernel forms it, without its f32 accumulation error: float64."""
    (ph, pl), (qh, ql) = split(p), split(q)
    d = lambda a, b: a.double() @ b.double().T
    return d(ph, ql) + d(pl, qh) + d(ph, qh)


def bound(p, q, split_form=True):
    """The per-element bound on |C - C64| of the contract (``split_form``) or of an f32 accumulation alone."""
    R = p.shape[1]
    mag = p.double().abs() @ q.double().abs().T
    return ((3 * 2.0 ** -18 if split_form else 0.0) + (R + 3) * 2.0 ** -24) * mag


def nine_bit_case(M, N, R, p9=True, q9=True, seed=1):
    """Integer operands: 9-bit (|v| <= 511, hi + lo exact, lo != 0 for most) or bf16-exact (|v| <= 2 / |v| <= 1),
    q thinned to one non-zero in four: every partial sum is an integer below 2^24, so any f32 summation order
    gives sum(p q - p_lo q_lo) exactly."""
    g = torch.Generator().manual_seed(seed + 1009 * M + 31 * N + R + 2 * p9 + q9)
    p = torch.randint(-511, 512, (M, R), generator=g) if p9 else torch.randint(-2, 3, (M, R), generator=g)
    q = torch.randint(-511, 512, (N, R), generator=g) if q9 else torch.randint(-1, 2, (N, R), generator=g)
    q = q * (torch.arange(R) % 4 == 0)
    return p.float(), q.float()


@pytest.fixture(autouse=True)
def _restore_highest():
    yield
    from vit_amd import ops
    ops.set_float32_matmul_precision("highest")


@pytest.mark.parametrize("positive", [False, True], ids=["randn", "abs"])
@pytest.mark.parametrize("R", [32, 1024, 4096])
def test_restatement_stays_inside_the_bound(R, positive):
    g = torch.Generator().manual_seed(7 + R)
    p, q = torch.randn(128, R, generator=g), torch.randn(128, R, generator=g)
    if positive:
        p, q = p.abs(), q.abs()
    ref = p.double() @ q.double().T
    frac = ((x3_f64(p, q) - ref).abs() / bound(p, q)).max().item()
    print(f"R={R} positive={positive}: {frac:.3f} of the bound")
    assert frac <= 1.0
    # what one rounding to bf16 (8 significant bits) guarantees per value: half an ulp is at most 2^-8 |x|, so the
    # two-term split is within 2^-16 |x|.  (The bound's 2^-18 is the typical size, a quarter of this worst case: it
    # holds for sums over data whose roundings are not all at their worst together, which is what is tested.)
    hi, lo = split(p)
    assert bool(((p - hi).abs() <= 2.0 ** -8 * p.abs()).all())
    assert bool(((p - hi - lo).abs() <= 2.0 ** -16 * p.abs()).all())


def test_nine_bit_integers_are_exact_and_tell_the_three_forms_apart():
    p, q = nine_bit_case(128, 128, 128)
    (ph, pl), (qh, ql) = split(p), split(q)
    assert torch.equal(ph + pl, p) and torch.equal(qh + ql, q)
    d = lambda a, b: a.double() @ b.double().T
    full, hh, x3 = d(p, q), d(ph, qh), x3_f64(p, q)
    assert torch.equal(x3, full - d(pl, ql))
    assert float((p.abs().double() @ q.abs().double().T).max()) < 2 ** 24  # every partial sum is an f32 integer
    assert torch.equal(x3.float().double(), x3)
    assert float((x3 != full).double().mean()) > 0.5
    assert bool((x3 != hh).any()) and float((x3 != hh).double().mean()) > 0.9
    # a bf16-exact operand has lo = 0: the three products are the whole product
    pb, qb = nine_bit_case(128, 128, 128, p9=False, q9=False)
    assert torch.equal(x3_f64(pb, qb), d(pb, qb))
    p1, q1 = nine_bit_case(128, 128, 128, q9=False)
    assert torch.equal(x3_f64(p1, q1), d(p1, q1))


def test_setter_and_getter_round_trip_without_a_gpu():
    import vit_amd
    from vit_amd import _lib
    lib = _lib.load()
    for name in ("vit_gemm_f32_precision", "vit_gemm_f32_count", "vit_gemm_f32_split_count"):
        assert name in _lib.exported_symbols() and hasattr(lib, name)
        assert _lib.SIGNATURES[name] == [_lib.i32]
    assert lib.vit_abi_version() == 10  # additive
    if os.environ.get("VIT_F32_MATMUL", "") in ("", "highest"):
        assert lib.vit_gemm_f32_precision(-1) == 0
    vit_amd.set_float32_matmul_precision("highest")
    assert vit_amd.get_float32_matmul_precision() == "highest"
    vit_amd.set_float32_matmul_precision("high")
    assert vit_amd.get_float32_matmul_precision() == "high" and lib.vit_gemm_f32_precision(-1) == 1
    with pytest.raises(ValueError, match="compute_dtype=torch.bfloat16"):
        vit_amd.set_float32_matmul_precision("medium")
    for junk in ("HIGH", "", None, 1, "tf32"):
        with pytest.raises(ValueError):
            vit_amd.set_float32_matmul_precision(junk)
    assert vit_amd.get_float32_matmul_precision() == "high"  # a refused call changes nothing
    assert lib.vit_gemm_f32_precision(7) == 1 and lib.vit_gemm_f32_precision(-1) == 1  # the C entry ignores junk
    vit_amd.set_float32_matmul_precision("highest")
    assert vit_amd.get_float32_matmul_precision() == "highest" and lib.vit_gemm_f32_precision(-1) == 0
    assert lib.vit_gemm_f32_count(1) >= 0 and lib.vit_gemm_f32_count(0) == 0
    assert lib.vit_gemm_f32_split_count(1) >= 0 and lib.vit_gemm_f32_split_count(0) == 0


def test_environment_variable_sets_the_initial_mode():
    code = ("import sys; sys.path.insert(0, %r); from vit_amd import ops; print(ops.get_float32_matmul_precision())"
            % os.path.join(ROOT, "vit-project_amd"))
    for val, want in (("high", "high"), ("highest", "highest"), ("medium", "highest")):
        out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, VIT_F32_MATMUL=val),
                             capture_output=True, text=True, check=True).stdout.split()
        assert out[-1] == want, (val, out)


def _tiny_clip():
    from vit_amd import clip
    return clip.CLIP(embed_dim=CFG.embed_dim, image_resolution=CFG.image_resolution, vision_layers=CFG.vision_layers,
                     vision_width=CFG.vision_width, vision_patch_size=CFG.vision_patch,
                     context_length=CFG.context_length, vocab_size=CFG.vocab_size, transformer_width=CFG.text_width,
                     transformer_heads=CFG.text_heads, transformer_layers=CFG.text_layers)


def test_prefix_key_follows_the_mode():
    import vit_amd
    from vit_amd.prefix_cache import prefix_key
    m = vit_amd.CLIPHBA([f"c{i}" for i in range(5)], "ViT-L/14", pos_embedding=True, clip_model=_tiny_clip())
    vit_amd.apply_dora_to_ViT(m, n_vision_layers=2, n_transformer_layers=1, r=4)
    vit_amd.switch_dora_layers(m, freeze_all=True, dora_state=True)
    images = torch.randn(4, 3, 32, 32)
    k_highest = prefix_key(m, images)
    vit_amd.set_float32_matmul_precision("high")
    k_high = prefix_key(m, images)
    assert k_high != k_highest
    # the layout older tests pin: 7 elements, the cut second, the streamed-fp8 switch last
    assert len(k_high) == len(k_highest) == 7 and k_high[1] == k_highest[1] and k_high[-1] is k_highest[-1] is False
    assert [i for i in range(7) if k_high[i] != k_highest[i]] == [2]
    assert k_highest[2] == m.clip_model.compute_dtype and k_high[2] == (m.clip_model.compute_dtype, "high")
    vit_amd.set_float32_matmul_precision("highest")
    assert prefix_key(m, images) == k_highest


def test_text_cache_key_follows_the_mode(monkeypatch):
    import vit_amd
    from vit_amd import clip, ops
    cm = _tiny_clip()
    cm.cache_frozen_text = True
    for p in cm.parameters():
        p.requires_grad = False
    for p in cm.transformer.resblocks[-1].parameters():
        p.requires_grad = True
    # the device work behind the key is not what this test is about: stand-ins that run on the CPU
    monkeypatch.setattr(ops, "token_embed", lambda text, table, pos: table[text] + pos)
    monkeypatch.setattr(clip, "run_block", lambda x, params, cfg: x)
    text = torch.randint(0, CFG.vocab_size, (3, CFG.context_length))

    def key():
        cm._text_cache = None
        cm._text_prefix(text)
        return cm._text_cache[0]

    k_highest = key()
    vit_amd.set_float32_matmul_precision("high")
    hit = cm._text_cache
    cm._text_prefix(text)
    assert cm._text_cache is not hit, "a text cache filled in one mode was read in the other"
    k_high = key()
    assert k_high != k_highest and k_high[:-1] == k_highest[:-1]
    assert (k_highest[-1], k_high[-1]) == ("highest", "high")
    vit_amd.set_float32_matmul_precision("highest")
    assert key() == k_highest


def test_f32m_kernels_have_no_spills_in_either_mode():
    obj = os.path.join(ROOT, "vit-project_amd", "csrc", "build", "gemm.o")
    if not os.path.exists(obj) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("gemm.o not built / no ROCm LLVM tools")
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kres.sh"), obj, "f32m"], capture_output=True, text=True,
                         check=True).stdout.splitlines()
    plain = [l for l in out if re.search(r"ffLi0EEEv", l)]  # <.., float, float, SPLIT> in the mangled name
    high = [l for l in out if re.search(r"ffLi1EEEv", l)]
    assert out and len(plain) + len(high) == len(out)
    assert len(high) == len(plain) > 0, "every f32m kernel has a SPLIT = 0 and a SPLIT = 1 instantiation"
    bad = [l for l in out if " spill 0 " not in l or " priv 0 " not in l]
    assert not bad, bad[:5]
    # two workgroups per CU: 8 waves on 4 SIMDs of 512 registers each
    assert all(int(l.split()[0]) <= 256 for l in out)
