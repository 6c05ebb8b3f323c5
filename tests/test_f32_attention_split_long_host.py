"""CPU: the streamed form of the fp32 "high" attention mode (bf16x3 in the streamed f32 attention kernels past 288
tokens, ``set_float32_attention_precision("high", long_sequences=True)``).

- ``x3_forward_chunked`` restates the streamed forward in float64 on an ``oracle.attn_cases`` case: the keys arrive
  in 64-key chunks, ``p = f32(exp(s - m_running))`` is split per chunk, ``o`` and ``l`` are rescaled by
  ``exp(m_old - m_new)``.  The backward has no running state: chunking only reorders sums that the float64
  restatement ``x3_attention`` of tests/test_f32_attention_split_host.py forms exactly, so that one stands for it.
- The bound of every figure is ``bounds`` of that file, unchanged: it is derived from the float64 reference, torch's
  float32 evaluation and the resident restatement.  Here: the chunked restatement stays inside it past 288 tokens,
  and a forward or backward without its ``lo`` terms is at least 10x past it.
- The setter's ``long_sequences`` keyword, the getter, ``VIT_F32_ATTENTION_LONG``, the two exports, the visual
  prefix key, the sweep hand-off and the register metadata of the three kernels in the built object.

tests/test_gpu_f32_attention_split_long.py holds the kernels to the same bounds.
"""
import math
import os
import re
import subprocess
import sys

import pytest
import torch

from oracle import attn_cases as AC

import test_f32_attention_split_host as HS

ROOT = HS.ROOT
B, H = HS.B, HS.H
F32 = torch.float32
CHUNK = 64
LONG_N = (289, 321, 577)  # 33 keys in the last chunk; one key in it; the 336-pixel workload's count


@pytest.fixture(autouse=True)
def _restore_highest():
    yield
    from vit_amd import ops
    ops.set_float32_matmul_precision("highest")
    ops.set_float32_attention_precision("highest")


# ---------------------------------------------------------------------------- 1. the streamed forward, in float64

def x3_forward_chunked(case, hh_only=False):
    """(o, lse) of an f32, non-causal case as the streamed kernels form them, without their f32 accumulation error."""
    assert case.dtype == F32 and not case.causal
    Bc, Hc, N = case.B, case.H, case.N
    mm = lambda a, b: HS.x3_matmul(a, b, hh_only)
    q, k, v = AC.split_qkv(case.qkv.double(), Bc, Hc, N)
    m = torch.full((Bc, Hc, N, 1), -math.inf, dtype=torch.float64)
    l = torch.zeros(Bc, Hc, N, 1, dtype=torch.float64)
    o = torch.zeros(Bc, Hc, N, 64, dtype=torch.float64)
    for j0 in range(0, N, CHUNK):
        kc, vc = k[:, :, j0:j0 + CHUNK], v[:, :, j0:j0 + CHUNK]
        s = mm(q, kc.transpose(-1, -2)) * case.scale
        mn = torch.maximum(m, s.amax(-1, keepdim=True))
        alpha = torch.exp(m - mn)  # first chunk: exp(-inf) = 0
        p = HS._f32(torch.exp(s - mn))
        l = l * alpha + p.sum(-1, keepdim=True)  # the sum is of the unsplit p
        o = o * alpha + mm(p, vc)
        m = mn
    return AC.pack(o / l), (m + torch.log(l)).reshape(-1)


@pytest.mark.parametrize("N", LONG_N)
def test_chunked_restatement_holds_the_bound_and_hi_hi_alone_does_not(N):
    """Every kind past 288 tokens: the chunked forward is inside ``HS.bounds``; the ``hi hi``-only chunked forward
    and the ``hi hi``-only backward are at least 10x past it on every figure."""
    worst = {}
    for kind in HS.KINDS:
        c = AC.make_case(kind, B, H, N, F32)
        bd = HS.bounds(c)
        fwd = HS.figures(c, *x3_forward_chunked(c))
        hh = HS.figures(c, *x3_forward_chunked(c, hh_only=True))
        _, _, grads, colsum = HS.x3_attention(c, hh_only=True)
        hh.update(HS.figures(c, grads=grads, colsum=colsum))
        for k, (bound, te, re_) in bd.items():
            if k in fwd:
                print(f"FIG {kind} N={N} | {k}: chunked x3 {fwd[k]:.2e} resident x3 {re_:.2e} torch-f32 {te:.2e} "
                      f"bound {bound:.2e}")
                assert fwd[k] <= bound, (kind, k, fwd[k], bound)
            ratio = hh[k] / bound
            print(f"FIG {kind} N={N} | {k}: hi*hi {hh[k]:.2e} bound {bound:.2e} ({ratio:.0f}x)")
            if ratio < worst.get(k, (math.inf,))[0]:
                worst[k] = (ratio, kind)
    print({k: f"{r:.0f}x ({kind})" for k, (r, kind) in worst.items()})
    assert set(worst) == set(HS.FWD_FIGS + HS.BWD_FIGS)
    bad = {k: v for k, v in worst.items() if not v[0] >= 10}
    assert not bad, bad


def test_chunked_restatement_is_the_resident_one_up_to_the_running_maximum():
    """On ``base`` at 289 tokens the chunked and the resident restatements' o errors agree to a factor 1.5: chunking
    moves the split of p (it is taken against the running maximum), nothing else."""
    c = AC.make_case("base", B, H, 289, F32)
    ch = HS.figures(c, *x3_forward_chunked(c))
    re_ = HS.figures(c, *HS.x3_attention(c)[:2])
    print({k: (f"{ch[k]:.2e}", f"{re_[k]:.2e}") for k in ch})
    assert ch["o"] <= 1.5 * re_["o"] and re_["o"] <= 1.5 * ch["o"]


# ---------------------------------------------------------------------------- 3. setter, getter, environment

def test_long_switch_round_trip_without_a_gpu():
    import vit_amd
    from vit_amd import _lib
    lib = _lib.load()
    vit_amd.set_float32_attention_precision("highest")
    assert vit_amd.get_float32_attention_long() is False and lib.vit_sdpa_f32_long_precision(-1) == 0
    with pytest.raises(ValueError):
        vit_amd.set_float32_attention_precision("highest", long_sequences=True)
    assert vit_amd.get_float32_attention_precision() == "highest" and lib.vit_sdpa_f32_long_precision(-1) == 0
    vit_amd.set_float32_attention_precision("high", long_sequences=True)
    assert vit_amd.get_float32_attention_precision() == "high" and vit_amd.get_float32_attention_long() is True
    assert lib.vit_sdpa_f32_precision(-1) == 1 and lib.vit_sdpa_f32_long_precision(-1) == 1
    with pytest.raises(ValueError):  # refused, and nothing changes
        vit_amd.set_float32_attention_precision("highest", long_sequences=True)
    with pytest.raises(ValueError):
        vit_amd.set_float32_attention_precision("medium", long_sequences=True)
    assert vit_amd.get_float32_attention_precision() == "high" and vit_amd.get_float32_attention_long() is True
    assert lib.vit_sdpa_f32_long_precision(7) == 1 and lib.vit_sdpa_f32_long_precision(-2) == 1
    assert lib.vit_sdpa_f32_long_precision(-1) == 1  # the C entry ignores junk
    assert lib.vit_sdpa_f32_long_precision(0) == 1 and lib.vit_sdpa_f32_long_precision(1) == 0  # the previous setting
    # the C switch alone does not make the getter true: the kernels need both
    lib.vit_sdpa_f32_precision(0)
    assert vit_amd.get_float32_attention_long() is False and lib.vit_sdpa_f32_long_precision(-1) == 1
    lib.vit_sdpa_f32_precision(1)
    assert vit_amd.get_float32_attention_long() is True
    vit_amd.set_float32_attention_precision("high")  # a one-argument call clears the long switch
    assert vit_amd.get_float32_attention_precision() == "high" and vit_amd.get_float32_attention_long() is False
    assert lib.vit_sdpa_f32_long_precision(-1) == 0
    vit_amd.set_float32_attention_precision("high", long_sequences=True)
    vit_amd.set_float32_attention_precision("highest")  # as the existing tests' teardowns call it
    assert lib.vit_sdpa_f32_precision(-1) == 0 and lib.vit_sdpa_f32_long_precision(-1) == 0
    assert lib.vit_sdpa_long_f32_split_count(1) >= 0 and lib.vit_sdpa_long_f32_split_count(0) == 0


def test_environment_variable_sets_the_initial_long_switch():
    code = ("import sys; sys.path.insert(0, %r); from vit_amd import ops, _lib; "
            "print(ops.get_float32_attention_precision(), ops.get_float32_attention_long(), "
            "_lib.lib().vit_sdpa_f32_long_precision(-1))" % os.path.join(ROOT, "vit-project_amd"))
    env = {k: v for k, v in os.environ.items() if k not in ("VIT_F32_ATTENTION", "VIT_F32_ATTENTION_LONG")}
    for extra, want in (({"VIT_F32_ATTENTION": "high", "VIT_F32_ATTENTION_LONG": "1"}, ["high", "True", "1"]),
                        ({"VIT_F32_ATTENTION_LONG": "1"}, ["highest", "False", "1"]),  # alone: attention stays exact
                        ({"VIT_F32_ATTENTION": "high"}, ["high", "False", "0"]),
                        ({"VIT_F32_ATTENTION": "high", "VIT_F32_ATTENTION_LONG": "yes"}, ["high", "False", "0"]),
                        ({}, ["highest", "False", "0"])):
        out = subprocess.run([sys.executable, "-c", code], env=dict(env, **extra), capture_output=True, text=True,
                             check=True).stdout.split()
        assert out[-3:] == want, (extra, out)


# ---------------------------------------------------------------------------- 4. exports

def test_exports_are_declared_built_and_bound():
    import vit_amd
    from vit_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "vit_hip.h")).read()
    for name in ("vit_sdpa_f32_long_precision", "vit_sdpa_long_f32_split_count"):
        assert name in _lib.exported_symbols() and hasattr(lib, name)
        assert _lib.SIGNATURES[name] == [_lib.i32]
        assert re.search(r"\bint %s\(int \w+\);" % name, header), name
    assert lib.vit_abi_version() == 10  # additive
    assert "get_float32_attention_long" in vit_amd.__all__ and callable(vit_amd.get_float32_attention_long)


# ---------------------------------------------------------------------------- 5. the visual prefix key

def test_prefix_key_follows_the_long_switch():
    import vit_amd
    from vit_amd.prefix_cache import prefix_key
    m = vit_amd.CLIPHBA([f"c{i}" for i in range(5)], "ViT-L/14", pos_embedding=True, clip_model=HS._tiny_clip())
    vit_amd.apply_dora_to_ViT(m, n_vision_layers=2, n_transformer_layers=1, r=4)
    vit_amd.switch_dora_layers(m, freeze_all=True, dora_state=True)
    images = torch.randn(4, 3, 32, 32)
    dt = m.clip_model.compute_dtype
    k_highest = prefix_key(m, images)
    assert len(k_highest) == 7 and k_highest[2] == dt
    vit_amd.set_float32_matmul_precision("high")
    k_gemm = prefix_key(m, images)
    vit_amd.set_float32_attention_precision("high")
    k_both = prefix_key(m, images)
    assert k_both[2] == (dt, "high", "attention-high")  # the long switch off: the key of DESIGN 4.23
    vit_amd.set_float32_attention_precision("high", long_sequences=True)
    k_both_long = prefix_key(m, images)
    assert k_both_long[2] == (dt, "high", "attention-high-long")
    vit_amd.set_float32_matmul_precision("highest")
    k_long = prefix_key(m, images)
    assert k_long[2] == (dt, "highest", "attention-high-long")
    keys = [k_highest, k_gemm, k_both, k_both_long, k_long]
    assert len({k[2] if isinstance(k[2], tuple) else (k[2],) for k in keys}) == 5, "five modes, five keys"
    for k in keys:
        assert len(k) == 7 and k[1] == k_highest[1] and k[-1] is False
        assert [i for i in range(7) if k[i] != k_highest[i]] in ([], [2])
    vit_amd.set_float32_attention_precision("high")
    assert prefix_key(m, images)[2] == (dt, "highest", "attention-high")
    vit_amd.set_float32_attention_precision("highest")
    assert prefix_key(m, images) == k_highest


# ---------------------------------------------------------------------------- 6. sweep hand-off

def test_launch_sweep_hands_the_long_switch_to_its_workers(monkeypatch):
    import vit_amd
    from vit_amd import sweep as S
    seen = {}

    def fake_run_sweep(*a, **kw):
        seen["kw"] = kw
        seen["modes"] = (vit_amd.get_float32_attention_precision(), vit_amd.get_float32_attention_long())
        return []

    class Q:
        def put(self, x):
            seen["out"] = x

    monkeypatch.setattr(S, "run_sweep", fake_run_sweep)
    worker = lambda kw: S._sweep_worker(0, 1, None, None, {}, [], kw, Q(), [])
    worker({"float32_attention": "high", "float32_attention_long": True})
    assert seen["modes"] == ("high", True)
    assert "float32_attention" not in seen["kw"] and "float32_attention_long" not in seen["kw"]
    worker({"float32_attention": "high"})  # a settings dict from before the switch existed: off
    assert seen["modes"] == ("high", False)
    worker({"float32_attention": "high", "float32_attention_long": False})
    assert seen["modes"] == ("high", False)

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
    vit_amd.set_float32_attention_precision("high", long_sequences=True)
    assert S.launch_sweep(1, None, None, {}, []) == {0: []}
    assert seen["modes"] == ("high", True)
    vit_amd.set_float32_attention_precision("high")
    S.launch_sweep(1, None, None, {}, [])
    assert seen["modes"] == ("high", False)
    assert [(h["float32_attention"], h["float32_attention_long"]) for h in handed] == [("high", True), ("high", False)]


# ---------------------------------------------------------------------------- 7. register metadata

# waves per SIMD of each kernel's launch bound (csrc/attention.hip): forward and dq two workgroups of 8 waves per
# CU, dkv one (kf, vf as hi and lo, dk and dv stay live across the kernel)
WPS = {"attn_fwd_stream_x3": 4, "attn_bwd_dq_stream_x3": 4, "attn_bwd_dkv_stream_x3": 2}


def test_stream_x3_kernels_have_no_spills_and_fit_their_launch_bounds():
    obj = os.path.join(ROOT, "vit-project_amd", "csrc", "build", "attention.o")
    if not os.path.exists(obj) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("attention.o not built / no ROCm LLVM tools")
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kres.sh"), obj, "stream_x3"], capture_output=True,
                         text=True, check=True).stdout.splitlines()
    seen = set()
    for l in out:
        m = re.search(r"_Z\d+(attn_(?:fwd|bwd_dq|bwd_dkv)_stream_x3)PKf", l)
        assert m, l
        seen.add(m.group(1))
        assert " spill 0 " in l and " priv 0 " in l, l
        f = l.split()
        vgpr, agpr = int(f[0]), 0 if f[1] == "None" else int(f[1])  # a kernel without AGPRs has no .agpr_count
        print(m.group(1), vgpr, agpr)
        assert vgpr + agpr <= 512 // WPS[m.group(1)], l
        assert int(re.search(r" lds (\d+)$", l).group(1)) == 0, l  # the ring is dynamic LDS
    assert len(out) == 3 and seen == set(WPS), out
