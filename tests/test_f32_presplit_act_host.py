"""CPU: pre-split activation images for the fp32 "high" GEMMs -- the host-side surface.

- the third switch of ``set_float32_matmul_precision``: its ``ValueError`` cases, the rule that every call sets all
  three switches, the getter, the environment variable and the ``launch_sweep`` hand-off;
- the new symbols, with the ABI still 10, and the host-only MFMA-path query;
- ``epilogue_image_ref``: a numpy statement of what the image-writing GEMM epilogue stores -- the fragment pair
  (2m, 2m + 1) of lane group g becomes hi chunk g and lo chunk g of k-block m -- checked against
  tests/test_f32_presplit_host.py's image rule for every (m, g); and the same for the LayerNorm producers' lane
  exchange (the partner four lanes away);
- registers / scratch / LDS of the new kernels, read from the built object.

tests/test_gpu_f32_presplit_act.py compares the kernels with the in-loop split on raw bits.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import test_f32_presplit_host as PH
import test_f32_split_host as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _restore_highest():
    yield
    from vit_amd import ops
    ops.set_float32_matmul_precision("highest")


# ---------------------------------------------------------------------------- the switch

def _state():
    import vit_amd
    return (vit_amd.get_float32_matmul_precision(), vit_amd.get_float32_matmul_presplit(),
            vit_amd.get_float32_matmul_presplit_activations())


def test_setter_needs_all_three_and_resets_all_three():
    import vit_amd
    from vit_amd import _lib
    lib = _lib.load()
    vit_amd.set_float32_matmul_precision("high", presplit_weights=True, presplit_activations=True)
    assert _state() == ("high", True, True)
    # refused combinations raise and change nothing
    for args, kw in ((("high",), dict(presplit_activations=True)),
                     (("highest",), dict(presplit_activations=True)),
                     (("highest",), dict(presplit_weights=True, presplit_activations=True)),
                     (("high",), dict(presplit_weights=False, presplit_activations=True))):
        with pytest.raises(ValueError, match="presplit"):
            vit_amd.set_float32_matmul_precision(*args, **kw)
        assert _state() == ("high", True, True), (args, kw)
    # every call sets all three switches
    vit_amd.set_float32_matmul_precision("high", presplit_weights=True)
    assert _state() == ("high", True, False)
    vit_amd.set_float32_matmul_precision("high", True, True)
    assert _state() == ("high", True, True)
    vit_amd.set_float32_matmul_precision("high")
    assert _state() == ("high", False, False)
    vit_amd.set_float32_matmul_precision("high", True, True)
    lib.vit_gemm_f32_precision(0)                     # the C switch alone: "highest" has no images of either kind
    assert _state() == ("highest", False, False)
    lib.vit_gemm_f32_precision(1)
    assert _state() == ("high", True, True)
    vit_amd.set_float32_matmul_precision("highest")
    assert _state() == ("highest", False, False)


def test_environment_variable_sets_the_initial_state():
    code = ("import sys; sys.path.insert(0, %r); from vit_amd import ops; "
            "print(ops.get_float32_matmul_precision(), ops.get_float32_matmul_presplit(), "
            "ops.get_float32_matmul_presplit_activations())" % os.path.join(ROOT, "vit-project_amd"))
    names = ("VIT_F32_MATMUL", "VIT_F32_MATMUL_PRESPLIT", "VIT_F32_MATMUL_PRESPLIT_ACT")
    env = {k: v for k, v in os.environ.items() if k not in names}
    for vals, want in ((("high", "1", "1"), ["high", "True", "True"]),
                       (("high", "1", None), ["high", "True", "False"]),
                       (("high", "1", "0"), ["high", "True", "False"]),
                       (("high", None, "1"), ["high", "False", "False"]),
                       ((None, "1", "1"), ["highest", "False", "False"])):
        extra = {k: v for k, v in zip(names, vals) if v is not None}
        out = subprocess.run([sys.executable, "-c", code], env=dict(env, **extra), capture_output=True, text=True,
                             check=True).stdout.split()
        assert out[-3:] == want, (extra, out)


def test_sweep_workers_are_handed_the_switch(monkeypatch):
    import vit_amd
    from vit_amd import sweep as S
    seen = {}

    def fake_run_sweep(*a, **kw):
        seen["state"] = _state()
        seen["kw"] = kw
        return []

    class Q:
        def put(self, item):
            pass

    monkeypatch.setattr(S, "run_sweep", fake_run_sweep)
    kw = {"float32_matmul": "high", "float32_matmul_presplit": True, "float32_matmul_presplit_act": True}
    S._sweep_worker(0, 1, None, None, {}, [], dict(kw), Q(), [])
    assert seen["state"] == ("high", True, True) and "float32_matmul_presplit_act" not in seen["kw"]
    del kw["float32_matmul_presplit_act"]               # a caller from before the switch: the default is off
    S._sweep_worker(0, 1, None, None, {}, [], dict(kw), Q(), [])
    assert seen["state"] == ("high", True, False)

    # launch_sweep reads the caller's state into the workers' keywords
    class Ctx:
        def Queue(self):
            return self

        def Process(self, target, args):
            seen["worker_kw"] = args[6]
            raise RuntimeError("stop before a process starts")

    import torch.multiprocessing as mp
    monkeypatch.setattr(mp, "get_context", lambda kind: Ctx())
    for third in (True, False):
        vit_amd.set_float32_matmul_precision("high", presplit_weights=True, presplit_activations=third)
        with pytest.raises(RuntimeError, match="stop before"):
            S.launch_sweep(1, None, None, {}, [])
        assert seen["worker_kw"]["float32_matmul_presplit_act"] is third
        assert seen["worker_kw"]["float32_matmul_presplit"] is True


# ---------------------------------------------------------------------------- symbols and the query

def test_new_symbols_are_declared_and_bound():
    from vit_amd import _lib
    lib = _lib.load()
    i32, i64, vp = _lib.i32, _lib.i64, _lib.vp
    assert lib.vit_abi_version() == 10  # additive
    assert _lib.F32_SPLIT == 2
    hdr = open(os.path.join(ROOT, "include", "vit_hip.h")).read()
    assert "VIT_DTYPE_F32_SPLIT = 2" in hdr
    assert _lib.SIGNATURES["vit_layer_norm_fwd_image_ok"] == [i32, i32, i64, C.c_uint64]
    for name in ("vit_gemm_f32_presplit_act_count", "vit_linear_fwd_f32_mfma", "vit_layer_norm_fwd_image_ok"):
        assert name in _lib.exported_symbols() and hasattr(lib, name) and f"int {name}(" in hdr
    assert _lib.SIGNATURES["vit_gemm_f32_presplit_act_count"] == [i32]
    assert _lib.SIGNATURES["vit_linear_fwd_f32_mfma"] == [i32, i32, i32, vp, i64, vp]
    assert lib.vit_gemm_f32_presplit_act_count(1) >= 0 and lib.vit_gemm_f32_presplit_act_count(0) == 0


def test_the_mfma_path_query_is_the_dispatch_rule():
    from vit_amd import _lib
    q = _lib.load().vit_linear_fwd_f32_mfma
    assert q(1024, 1024, 32, 16, 32, 16) == 1           # 64 tiles, one k-step
    assert q(1032, 1028, 96, 16, 100, 32) == 1          # ragged tiles, a row pitch past K
    assert q(1024, 1024 - 128, 64, 16, 64, 16) == 0     # 56 tiles
    assert q(896 + 127, 1024, 64, 16, 64, 16) == 1      # 8 x 8 tiles with a ragged last row tile
    assert q(896, 1024, 64, 16, 64, 16) == 0            # 7 x 8 = 56 tiles
    assert q(1024, 1024, 48, 16, 48, 16) == 0           # K % 32
    assert q(1024, 1022, 64, 16, 64, 16) == 0           # N % 4
    assert q(1024, 1024, 64, 16, 66, 16) == 0           # rows not 16-byte aligned
    assert q(1024, 1024, 64, 20, 64, 16) == 0           # misaligned X
    assert q(1024, 1024, 64, 16, 64, 24) == 0           # misaligned W
    assert q(0, 1024, 64, 16, 64, 16) == 0


def test_the_layer_norm_query_is_the_entry_points_rule():
    from vit_amd import _lib
    q = _lib.load().vit_layer_norm_fwd_image_ok
    for D in (256, 512, 768, 1024, 1536, 2048):
        assert q(0, D, D, 16) == 1 and q(1, D, D, 16) == 1, D
    for D in (1280, 1792):   # the plain entry runs its element-wise kernel at these widths, the fused one a vector kernel
        assert q(0, D, D, 16) == 0 and q(1, D, D, 16) == 1, D
    for D in (96, 384, 2304, 0):
        assert q(0, D, D, 16) == 0 and q(1, D, D, 16) == 0, D
    assert q(0, 256, 256 | 258, 16) == 0      # one stride of the call not a multiple of 4
    assert q(1, 256, 256, 16 | 24) == 0       # one address of the call not 16-byte aligned
    # ... and the entry points refuse what the query refuses, on the host
    lib, S, F = _lib.load(), _lib.F32_SPLIT, _lib.F32
    assert lib.vit_layer_norm_fwd(F, S, 4, 1280, 16, 1280, 16, 1280, 16, 16, None, None, 1e-5, None) == 1
    assert lib.vit_layer_norm_fwd(F, S, 4, 384, 16, 384, 16, 384, 16, 16, None, None, 1e-5, None) == 1


def test_image_calls_are_refused_on_the_host_before_any_launch():
    """No GPU is touched by a refused call: the library answers from the arguments alone."""
    from vit_amd import _lib
    lib = _lib.load()
    S, F = _lib.F32_SPLIT, _lib.F32
    prev = lib.vit_gemm_f32_precision(1)
    try:
        fwd = lambda dt, odt, epi, M, N, K, wimg=16: lib.vit_linear_fwd_wimg(  # noqa: E731
            dt, odt, epi, M, N, K, 16, K, 16, None, 16, N, 16, None, wimg, None)
        assert fwd(S, F, _lib.EPI_STORE, 1024, 1024, 64, wimg=None) == 1       # no weight image
        assert fwd(S, F, _lib.EPI_STORE, 896, 1024, 64) == 1                   # under 64 tiles
        assert fwd(S, F, _lib.EPI_STORE, 1024, 1024, 48) == 1                  # K % 32
        assert fwd(S, F, _lib.EPI_BIAS_GELU, 1024, 1024, 64) == 1              # a pair epilogue
        assert lib.vit_linear_fwd_wimg(S, F, _lib.EPI_STORE, 1024, 1024, 64, 16, 64, 16, None, 16, 1024, None, 16, 16,
                                       None) == 1                              # an act_out no accepted epilogue writes
        assert fwd(S, _lib.BF16, _lib.EPI_STORE, 1024, 1024, 64) == 1
        assert fwd(_lib.BF16, S, _lib.EPI_STORE, 1024, 1024, 64) == 1
        assert fwd(F, S, _lib.EPI_STORE, 1024, 1028, 64) == 1                  # an image output needs N % 32 == 0
        assert fwd(F, S, _lib.EPI_RESID, 1024, 1024, 64) == 1                  # no image output behind the residual
        assert lib.vit_linear_fwd(S, F, _lib.EPI_STORE, 1024, 1024, 64, 16, 64, 16, None, 16, 1024, None, None,
                                  None) == 1                                   # the entry without an image argument
        lib.vit_gemm_f32_precision(0)
        assert fwd(S, F, _lib.EPI_STORE, 1024, 1024, 64) == 1                  # "highest"
        assert fwd(F, S, _lib.EPI_STORE, 1024, 1024, 64) == 1
        # LayerNorm: the element-wise kernel has no image form
        ln = lib.vit_layer_norm_fwd
        assert ln(F, S, 4, 96, 16, 96, 16, 96, 16, 16, None, None, 1e-5, None) == 1
        assert ln(F, S, 4, 256, 16, 256, 24, 256, 16, 16, None, None, 1e-5, None) == 1     # misaligned y
        assert ln(_lib.BF16, S, 4, 256, 16, 256, 16, 256, 16, 16, None, None, 1e-5, None) == 1
        aln = lib.vit_add_layer_norm_fwd
        assert aln(F, S, 4, 96, 16, 96, 16, 96, 16, 96, 16, 96, 16, 16, 16, 16, 1e-5, None) == 1
        assert aln(_lib.BF16, S, 4, 256, 16, 256, 16, 256, 16, 256, 16, 256, 16, 16, 16, 16, 1e-5, None) == 1
        assert lib.vit_gemm_f32_presplit_act_count(1) == 0
    finally:
        lib.vit_gemm_f32_precision(prev)


# ---------------------------------------------------------------------------- what the producers store

def _split8(x0, x1):
    """bf16_split.hpp's split8 on [rows, 4] halves: (hi, lo) as [rows, 8] bf16-valued f32, element j = 4 h + t."""
    x = torch.cat([x0, x1], dim=1)
    return H.split(x)


def epilogue_image_ref(y):
    """The bytes the image-writing GEMM epilogue stores for an f32 result y [rows, N] (N % 64 == 0), stated per
    wave column block (64 columns), accumulator fragment pair and lane group: an f32-typed [rows, N] tensor."""
    rows, N = y.shape
    out = torch.zeros(rows, N * 2, dtype=torch.bfloat16)            # 2 bf16 per 4-byte cell
    for jw in range(0, N, 64):                                      # a wave's 64 columns: 4 fragments of 16
        for m in range(2):                                          # fragment pair (2m, 2m + 1) = k-block m of the wave
            for g in range(4):                                      # lane group g = lane >> 4 holds 4 columns of each
                c0 = jw + (2 * m) * 16 + 4 * g                      # acc[a][2m]:     columns 32m + 4g .. + 3
                c1 = jw + (2 * m + 1) * 16 + 4 * g                  # acc[a][2m + 1]: columns 32m + 16 + 4g .. + 3
                hi, lo = _split8(y[:, c0:c0 + 4], y[:, c1:c1 + 4])
                byte = (jw + 32 * m) * 4 + 16 * g                   # hi chunk g of that row's k-block; lo 64 bytes on
                out[:, byte // 2:byte // 2 + 8] = hi.to(torch.bfloat16)
                out[:, (byte + 64) // 2:(byte + 64) // 2 + 8] = lo.to(torch.bfloat16)
    return out.view(torch.float32)


def layer_norm_image_ref(y):
    """The bytes the LayerNorm producers store for an f32 result y [rows, D] (D % 256 == 0): lane l of group k owns
    columns 4 (64 k + l) .. + 3 and stores 16 bytes at that address; its partner is lane l ^ 4."""
    rows, D = y.shape
    out = torch.zeros(rows, D * 2, dtype=torch.bfloat16)
    for k in range(D // 256):
        for lane in range(64):
            c, p = 4 * (64 * k + lane), 4 * (64 * k + (lane ^ 4))
            upper = bool(lane & 4)
            x0, x1 = (y[:, p:p + 4], y[:, c:c + 4]) if upper else (y[:, c:c + 4], y[:, p:p + 4])
            hi, lo = _split8(x0, x1)
            out[:, 2 * c:2 * c + 8] = (lo if upper else hi).to(torch.bfloat16)
    return out.view(torch.float32)


@pytest.mark.parametrize("N", [64, 192])
def test_fragment_pairs_are_the_image_chunks(N):
    y = PH.scaled_randn(24, N, seed=7 + N)
    want = PH.image_ref(y)
    got = epilogue_image_ref(y)
    assert np.array_equal(got.numpy().view(np.uint32), want.numpy().view(np.uint32))
    # ... and per (m, g): the chunk is the hi / lo of k = 16 (j >> 2) + 4 g + (j & 3) of k-block m
    hi, lo = H.split(y)
    bits = got.view(torch.bfloat16).float()
    for kb in range(N // 32):
        for g in range(4):
            for j in range(8):
                k = kb * 32 + 16 * (j >> 2) + 4 * g + (j & 3)
                assert torch.equal(bits[:, kb * 64 + g * 8 + j], hi[:, k]), (kb, g, j)
                assert torch.equal(bits[:, kb * 64 + (4 + g) * 8 + j], lo[:, k]), (kb, g, j)


@pytest.mark.parametrize("D", [256, 768])
def test_layer_norm_lane_exchange_is_the_image(D):
    y = PH.scaled_randn(5, D, seed=3 + D)
    got, want = layer_norm_image_ref(y), PH.image_ref(y)
    assert np.array_equal(got.numpy().view(np.uint32), want.numpy().view(np.uint32))


# ---------------------------------------------------------------------------- the built kernels

def _kres(obj, pattern):
    return subprocess.run(["bash", os.path.join(ROOT, "tools", "kres.sh"), obj, pattern], capture_output=True,
                          text=True, check=True).stdout.splitlines()


def _tools(obj):
    if not os.path.exists(obj) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip(os.path.basename(obj) + " not built / no ROCm LLVM tools")


def test_activation_image_gemms_have_no_spills_and_fit_two_workgroups_per_cu():
    obj = os.path.join(ROOT, "vit-project_amd", "csrc", "build", "gemm.o")
    _tools(obj)
    out = _kres(obj, "4f32a")
    gemms = [l for l in out if "gemm_kernel" in l or "gemm_sk_kernel" in l]
    # image X with f32 Y: store, residual, two act-only forms; image Y (store, two act-only forms) behind an f32 X
    # and behind an image X; each as a plain and a stream-K kernel
    assert len(gemms) == 20 and len(out) == 20, out
    bad = [l for l in out if " spill 0 " not in l or " priv 0 " not in l]
    assert not bad, bad[:5]
    for l in out:
        f = l.split()
        vgpr, agpr = int(f[0]), 0 if f[1] == "None" else int(f[1])
        assert vgpr + agpr <= 256, l                     # __launch_bounds__(256, 2): two workgroups of 4 waves a CU
        assert int(f[-1]) == 0, l                        # the ring is dynamic LDS (64 KiB + 16 <= 81 920): none static
    # the sibling namespaces hold what they held
    assert len(_kres(obj, "4f32w")) == 18


def test_layer_norm_image_kernels_have_no_spills_and_no_lds():
    obj = os.path.join(ROOT, "vit-project_amd", "csrc", "build", "norm.o")
    _tools(obj)
    out = _kres(obj, "6f32img")
    # ln_fwd: NV 1, 2, 3, 4, 6, 8 (no element-wise instantiation exists); add_ln_fwd: NV 1 .. 8
    assert len([l for l in out if "add_ln_fwd_kernel" in l]) == 8, out
    plain = [l for l in out if "add_ln_fwd_kernel" not in l and "ln_fwd_kernel" in l]
    assert len(plain) == 6 and not [l for l in plain if "ILi0E" in l], out
    assert len(out) == 14
    for l in out:
        assert " spill 0 " in l and " priv 0 " in l and int(l.split()[-1]) == 0, l
