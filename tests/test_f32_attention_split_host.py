"""CPU: the arithmetic rule, the bound and the host-side surface of the fp32 "high" attention mode (bf16x3 in the
resident f32 attention kernels).

- ``x3_attention`` restates the kernels' rule in float64 on an ``oracle.attn_cases`` case: q, k, v, dO, p and dS
  are split as ``hi = bf16_rne(x)``, ``lo = bf16_rne(x - hi)`` (p and dS rounded to f32 first, as the kernels hold
  them), every matrix product is ``hi lo + lo hi + hi hi`` summed in float64, everything else is float64.  The
  backward is fed the reference's o (as f32) and lse, as the conformance tests feed it.  ``hh_only=True`` keeps the
  ``hi hi`` product alone: what a kernel that lost its ``lo`` terms would compute.
- ``bounds`` derives the bound of every figure tests/test_gpu_attention_conformance.py reports:

      bound = max(project f32 bound, 4 x torch-f32 error) + 2 x (the restatement's own error on that case)

  The first term is what the conformance test grants an f32 kernel (accumulation order, hardware exp2 / log2); the
  second is the error the rule cannot avoid, twice because the kernels form p and dS in f32, not float64: a last-bit
  difference there can move a ``hi`` by one bf16 ulp, which ``lo`` gives back only to second order.
- The bound cannot hide a kernel without its ``lo`` terms: on every case with at least 16 tokens the ``hi hi``-only
  restatement is at least 10x past it on every figure.
- The setter, the getter and ``VIT_F32_ATTENTION``; both frozen-prefix cache keys; the register metadata of every
  new instantiation in the built object.

tests/test_gpu_f32_attention_split.py imports the restatement, ``figures`` and ``bounds``.
"""
import math
import os
import re
import subprocess
import sys

import pytest
import torch

from oracle import attn_cases as AC
from oracle import clip_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = CR.CLIP_TINY
B, H = 2, 2
F32 = torch.float32


# ---------------------------------------------------------------------------- 1. the rule, in float64

def split(x):
    """(hi, lo) of a tensor of f32 values, as float64 tensors holding bf16 values."""
    x = x.float()
    hi = x.to(torch.bfloat16).float()
    lo = (x - hi).to(torch.bfloat16).float()
    return hi.double(), lo.double()


def x3_matmul(a, b, hh_only=False):
    """a @ b as the kernels form it, without their f32 accumulation error."""
    (ah, al), (bh, bl) = split(a), split(b)
    if hh_only:
        return ah @ bh
    return ah @ bl + al @ bh + ah @ bh


def _f32(x):
    return x.float().double()


def x3_attention(case, hh_only=False):
    """(o, lse, grads, colsum) of an f32 case under the rule, float64 (see the module docstring)."""
    assert case.dtype == F32
    Bc, Hc, N = case.B, case.H, case.N
    mm = lambda a, b: x3_matmul(a, b, hh_only)
    q, k, v = AC.split_qkv(case.qkv.double(), Bc, Hc, N)
    do = AC.unpack(case.do.double(), Bc, Hc, N)
    kT, vT = k.transpose(-1, -2), v.transpose(-1, -2)
    masked = AC._mask(N) if case.causal else None
    s = mm(q, kT) * case.scale
    if masked is not None:
        s = s.masked_fill(masked, -math.inf)
    m = s.amax(-1, keepdim=True)
    p = _f32(torch.exp(s - m))
    l = p.sum(-1, keepdim=True)
    o = mm(p, v) / l
    lse = (m + torch.log(l)).squeeze(-1)

    o_in = AC.unpack(_f32(case.o), Bc, Hc, N)
    lse_in = _f32(case.lse).reshape(Bc, Hc, N, 1)
    p = _f32(torch.exp(s - lse_in))
    delta = (do * o_in).sum(-1, keepdim=True)
    ds = p * (mm(do, vT) - delta)
    if masked is not None:
        ds = ds.masked_fill(masked, 0.0)
    ds = _f32(ds)
    dq = mm(ds, k) * case.scale
    dk = mm(ds.transpose(-1, -2), q) * case.scale
    dv = mm(p.transpose(-1, -2), do)
    grads = torch.cat([AC.pack(dq), AC.pack(dk), AC.pack(dv)], 1)
    return AC.pack(o), lse.reshape(-1), grads, grads.sum(0)


# ---------------------------------------------------------------------------- 2. the figures and their bound

FWD_FIGS = ("o", "o row", "lse")
BWD_FIGS = ("dq", "dk", "dv", "dv row", "dqkv item", "qkv bias grad")
PROJECT = {"o": AC.F32_O, "o row": AC.F32_O, "lse": AC.F32_LSE, "dq": AC.F32_GRAD, "dk": AC.F32_GRAD,
           "dv": AC.F32_GRAD, "dv row": AC.F32_GRAD, "dqkv item": AC.F32_GRAD, "qkv bias grad": AC.F32_GRAD}


def figures(c, o=None, lse=None, grads=None, colsum=None):
    """The conformance test's figures of a result against the case's float64 reference, by name; the forward's
    when ``o`` and ``lse`` are given, the backward's when ``grads`` and ``colsum`` are."""
    N, D = c.N, c.D
    f = {}
    if o is not None:
        f["o"] = AC.rel_max(o, c.o)
        f["o row"] = AC.row_rel(o, c.o, c.B, c.H, N)
        f["lse"] = AC.rel_max(lse, c.lse)
    if grads is not None:
        g = grads.detach().double().cpu()
        blk = lambda x, i: x[:, i * D:(i + 1) * D]
        for i, name in enumerate(("dq", "dk", "dv")):
            f[name] = AC.rel_max(blk(g, i), blk(c.grads, i), c.grads)
        f["dv row"] = AC.row_rel(blk(g, 2), blk(c.grads, 2), c.B, c.H, N)
        f["dqkv item"] = AC.item_rel(g, c.grads, c.B, c.H, N)
        f["qkv bias grad"] = AC.rel_max(colsum, c.colsum)
    return f


_BOUNDS = {}


def bounds(c):
    """{figure: (bound, torch-f32 error, the restatement's error)} of an f32 case; computed once per case."""
    key = (c.kind, c.B, c.H, c.N, c.causal, c.scale)
    if key not in _BOUNDS:
        te, re_ = figures(c, *AC.torch_f32(c)), figures(c, *x3_attention(c))
        _BOUNDS[key] = {k: (max(PROJECT[k], 4 * te[k]) + 2 * re_[k], te[k], re_[k]) for k in PROJECT}
    return _BOUNDS[key]


KINDS = AC.KINDS + ("offset4",)
SHAPES = [(16, False), (33, False), (77, True), (197, False), (257, False), (273, True), (288, False)]


@pytest.mark.parametrize("N,causal", SHAPES, ids=[f"N{n}{'-causal' if c else ''}" for n, c in SHAPES])
def test_bound_cannot_hide_a_kernel_without_its_lo_terms(N, causal):
    """Every kind: the restatement is inside its own bound (trivially: the bound holds twice its error), and the
    ``hi hi``-only form is at least 10x past the bound on every figure."""
    worst = {}
    for kind in KINDS:
        c = AC.make_case(kind, B, H, N, F32, causal=causal)
        bd = bounds(c)
        hh = figures(c, *x3_attention(c, hh_only=True))
        for k, (bound, te, re_) in bd.items():
            ratio = hh[k] / bound
            print(f"FIG {kind} N={N}{' causal' if causal else ''} | {k}: x3 {re_:.2e} torch-f32 {te:.2e} bound "
                  f"{bound:.2e} hi*hi {hh[k]:.2e} ({ratio:.0f}x)")
            assert re_ <= bound
            if ratio < worst.get(k, (math.inf,))[0]:
                worst[k] = (ratio, kind)
    print({k: f"{r:.0f}x ({kind})" for k, (r, kind) in worst.items()})
    bad = {k: v for k, v in worst.items() if not v[0] >= 10}
    assert not bad, bad


def test_restatement_gives_up_one_to_two_digits_where_bf16_gives_up_four():
    """The figures DESIGN §4.23 quotes (B = H = 2, N = 288): the rule's own error in o stays within a factor 40 of
    torch's float32 evaluation, and ``hi hi`` alone is more than 100x worse than the rule."""
    for kind in ("base", "offset"):
        c = AC.make_case(kind, B, H, 288, F32)
        x3, hh, te = (figures(c, *r) for r in (x3_attention(c), x3_attention(c, hh_only=True), AC.torch_f32(c)))
        print(kind, {k: f"x3 {x3[k]:.1e} f32 {te[k]:.1e} hh {hh[k]:.1e}" for k in ("o", "dq")})
        assert x3["o"] <= 40 * te["o"] and hh["o"] >= 100 * x3["o"] and hh["dq"] >= 100 * x3["dq"]


def test_restatement_is_the_reference_on_bf16_valued_inputs_up_to_p_and_ds():
    """Operands that hold bf16 values have lo = 0: S and dP are the float64 products exactly, so only the split of p
    and dS is left, and that is far below the f32 project bounds."""
    c = AC.make_case("base", B, H, 33, torch.bfloat16)
    c.qkv, c.do, c.dtype = c.qkv.float(), c.do.float(), F32
    q, k, _ = AC.split_qkv(c.qkv.double(), B, H, 33)
    assert torch.equal(x3_matmul(q, k.transpose(-1, -2)), q @ k.transpose(-1, -2))
    f = figures(c, *x3_attention(c))
    assert all(f[k] <= PROJECT[k] for k in f), f


# ---------------------------------------------------------------------------- 4. setter, getter, environment

@pytest.fixture(autouse=True)
def _restore_highest():
    yield
    from vit_amd import ops
    ops.set_float32_matmul_precision("highest")
    ops.set_float32_attention_precision("highest")


def test_setter_and_getter_round_trip_without_a_gpu():
    import vit_amd
    from vit_amd import _lib
    lib = _lib.load()
    for name in ("vit_sdpa_f32_precision", "vit_sdpa_f32_split_count"):
        assert name in _lib.exported_symbols() and hasattr(lib, name)
        assert _lib.SIGNATURES[name] == [_lib.i32]
    assert lib.vit_abi_version() == 10  # additive
    if os.environ.get("VIT_F32_ATTENTION", "") in ("", "highest"):
        assert lib.vit_sdpa_f32_precision(-1) == 0
    vit_amd.set_float32_attention_precision("highest")
    assert vit_amd.get_float32_attention_precision() == "highest"
    vit_amd.set_float32_attention_precision("high")
    assert vit_amd.get_float32_attention_precision() == "high" and lib.vit_sdpa_f32_precision(-1) == 1
    for junk in ("HIGH", "", None, 1, "tf32", "medium"):
        with pytest.raises(ValueError):
            vit_amd.set_float32_attention_precision(junk)
    assert vit_amd.get_float32_attention_precision() == "high"  # a refused call changes nothing
    assert lib.vit_sdpa_f32_precision(7) == 1 and lib.vit_sdpa_f32_precision(-2) == 1
    assert lib.vit_sdpa_f32_precision(-1) == 1  # the C entry ignores junk
    assert lib.vit_sdpa_f32_precision(0) == 1 and lib.vit_sdpa_f32_precision(1) == 0  # returns the previous setting
    vit_amd.set_float32_attention_precision("highest")
    assert vit_amd.get_float32_attention_precision() == "highest" and lib.vit_sdpa_f32_precision(-1) == 0
    assert lib.vit_sdpa_f32_split_count(1) >= 0 and lib.vit_sdpa_f32_split_count(0) == 0


def test_the_two_switches_are_independent():
    import vit_amd
    vit_amd.set_float32_matmul_precision("high")
    assert vit_amd.get_float32_attention_precision() == "highest"
    vit_amd.set_float32_attention_precision("high")
    assert vit_amd.get_float32_matmul_precision() == "high"
    vit_amd.set_float32_matmul_precision("highest")
    assert vit_amd.get_float32_attention_precision() == "high"
    vit_amd.set_float32_attention_precision("highest")
    assert vit_amd.get_float32_matmul_precision() == "highest"


def test_environment_variable_sets_the_initial_mode():
    code = ("import sys; sys.path.insert(0, %r); from vit_amd import ops; "
            "print(ops.get_float32_attention_precision(), ops.get_float32_matmul_precision())"
            % os.path.join(ROOT, "vit-project_amd"))
    env = {k: v for k, v in os.environ.items() if k not in ("VIT_F32_ATTENTION", "VIT_F32_MATMUL")}
    for val, want in (("high", "high"), ("medium", "highest")):
        out = subprocess.run([sys.executable, "-c", code], env=dict(env, VIT_F32_ATTENTION=val), capture_output=True,
                             text=True, check=True).stdout.split()
        assert out[-2:] == [want, "highest"], (val, out)
    # unset: the default, and the GEMM's variable does not move it
    out = subprocess.run([sys.executable, "-c", code], env=dict(env, VIT_F32_MATMUL="high"), capture_output=True,
                         text=True, check=True).stdout.split()
    assert out[-2:] == ["highest", "high"], out


# ---------------------------------------------------------------------------- 5. cache keys

def _tiny_clip():
    from vit_amd import clip
    return clip.CLIP(embed_dim=CFG.embed_dim, image_resolution=CFG.image_resolution, vision_layers=CFG.vision_layers,
                     vision_width=CFG.vision_width, vision_patch_size=CFG.vision_patch,
                     context_length=CFG.context_length, vocab_size=CFG.vocab_size, transformer_width=CFG.text_width,
                     transformer_heads=CFG.text_heads, transformer_layers=CFG.text_layers)


def test_prefix_key_follows_the_attention_mode():
    import vit_amd
    from vit_amd.prefix_cache import prefix_key
    m = vit_amd.CLIPHBA([f"c{i}" for i in range(5)], "ViT-L/14", pos_embedding=True, clip_model=_tiny_clip())
    vit_amd.apply_dora_to_ViT(m, n_vision_layers=2, n_transformer_layers=1, r=4)
    vit_amd.switch_dora_layers(m, freeze_all=True, dora_state=True)
    images = torch.randn(4, 3, 32, 32)
    dt = m.clip_model.compute_dtype
    k_highest = prefix_key(m, images)
    assert len(k_highest) == 7 and k_highest[2] == dt  # exactly the key it has always been
    vit_amd.set_float32_matmul_precision("high")
    k_gemm = prefix_key(m, images)
    assert k_gemm[2] == (dt, "high")  # the GEMM switch alone: the key of DESIGN 4.22
    vit_amd.set_float32_attention_precision("high")
    k_both = prefix_key(m, images)
    vit_amd.set_float32_matmul_precision("highest")
    k_attn = prefix_key(m, images)
    keys = [k_highest, k_gemm, k_both, k_attn]
    assert len({k[2] if isinstance(k[2], tuple) else (k[2],) for k in keys}) == 4, "four modes, four keys"
    for k in keys:  # the layout older tests pin: 7 elements, the cut second, the streamed-fp8 switch last
        assert len(k) == 7 and k[1] == k_highest[1] and k[-1] is False
        assert [i for i in range(7) if k[i] != k_highest[i]] in ([], [2])
    vit_amd.set_float32_attention_precision("highest")
    assert prefix_key(m, images) == k_highest


def test_text_cache_key_follows_the_attention_mode(monkeypatch):
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
    assert k_highest[-1] == "highest" and len(k_highest) == 9  # today's key: the GEMM mode is its last element
    vit_amd.set_float32_attention_precision("high")
    hit = cm._text_cache
    cm._text_prefix(text)
    assert cm._text_cache is not hit, "a text cache filled in one attention mode was read in the other"
    k_high = key()
    assert k_high != k_highest and k_high[:len(k_highest)] == k_highest
    vit_amd.set_float32_matmul_precision("high")
    assert key() not in (k_highest, k_high)
    vit_amd.set_float32_matmul_precision("highest")
    vit_amd.set_float32_attention_precision("highest")
    assert key() == k_highest


def test_launch_sweep_hands_the_attention_mode_to_its_workers(monkeypatch):
    import vit_amd
    from vit_amd import sweep as S
    seen = {}

    def fake_run_sweep(*a, **kw):
        seen["kw"] = kw
        seen["modes"] = (vit_amd.get_float32_matmul_precision(), vit_amd.get_float32_attention_precision())
        return []

    class Q:
        def put(self, x):
            seen["out"] = x

    monkeypatch.setattr(S, "run_sweep", fake_run_sweep)
    S._sweep_worker(0, 1, None, None, {}, [], {"float32_matmul": "highest", "float32_attention": "high"}, Q(), [])
    assert seen["modes"] == ("highest", "high") and "float32_attention" not in seen["kw"]

    # launch_sweep itself, with processes that run inline: what it hands each worker
    import queue
    import torch.multiprocessing as mp
    handed = []

    class Ctx:
        Queue = staticmethod(queue.Queue)

        class Process:
            def __init__(self, target, args):
                self.target, self.args, self.exitcode = target, args, None

            def start(self):
                handed.append(dict(self.args[6]))
                self.target(*self.args)
                self.exitcode = 0

            def join(self):
                pass

            def terminate(self):
                pass

    monkeypatch.setattr(mp, "get_context", lambda kind: Ctx)
    vit_amd.set_float32_matmul_precision("high")
    vit_amd.set_float32_attention_precision("highest")
    assert S.launch_sweep(1, None, None, {}, []) == {0: []}
    vit_amd.set_float32_matmul_precision("highest")
    vit_amd.set_float32_attention_precision("high")
    S.launch_sweep(1, None, None, {}, [])
    assert [(h["float32_matmul"], h["float32_attention"]) for h in handed] == [("high", "highest"), ("highest", "high")]


# ---------------------------------------------------------------------------- 6. register metadata

def _wps(nt, dkv):
    """Waves per SIMD the launch bound of an instantiation asks for (F32X3 in csrc/attention.hip): two workgroups
    of 8 waves per CU while the four images (and dkv's two strips) fit twice in 160 KiB of LDS, else one."""
    rows = (nt + 1) // 2 * 32
    lds = 4 * rows * 128 + (2 * rows * 4 if dkv else 0)
    assert lds <= 163840
    return 4 if 2 * lds <= 163840 else 2


def test_f32x3_kernels_have_no_spills_and_fit_their_launch_bounds():
    obj = os.path.join(ROOT, "vit-project_amd", "csrc", "build", "attention.o")
    if not os.path.exists(obj) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("attention.o not built / no ROCm LLVM tools")
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kres.sh"), obj, "f32x3"], capture_output=True,
                         text=True, check=True).stdout.splitlines()
    seen = set()
    for l in out:
        m = re.search(r"_Z\d+attn_(fwd|bwd_dq|bwd_dkv)_f32x3ILi(\d+)E(?:Lb([01])E)?E", l)
        assert m, l
        kern, nt, causal = m.group(1), int(m.group(2)), m.group(3)
        seen.add((kern, nt, causal))
        assert " spill 0 " in l and " priv 0 " in l, l
        f = l.split()
        vgpr, agpr = int(f[0]), 0 if f[1] == "None" else int(f[1])  # a kernel without AGPRs has no .agpr_count
        assert vgpr + agpr <= 512 // _wps(nt, kern == "bwd_dkv"), l
        assert int(re.search(r" lds (\d+)$", l).group(1)) == 0, l  # all of it dynamic: the formula in _wps
    want = {(k, nt, c) for nt in range(1, 19) for k, c in (("fwd", "0"), ("fwd", "1"), ("bwd_dq", None),
                                                          ("bwd_dkv", None))}
    assert seen == want, (want - seen, seen - want)
