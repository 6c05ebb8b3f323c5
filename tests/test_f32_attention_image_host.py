"""CPU: pre-split images through fp32 "high" attention -- the host-side surface.

- the third switch of ``set_float32_attention_precision``: ``ValueError`` with "highest", every call sets all three
  switches, the getter, the environment variable and the ``launch_sweep`` hand-off;
- the new symbols, with the ABI still 10; the host-only query over a grid of (N, causal, long, mode, pitch), and
  ``vit_sdpa_fwd_image`` refused on the host before any launch;
- a torch restatement of what the image kernels do with image bytes, against tests/test_f32_presplit_host.py's image
  rule and tests/test_f32_split_host.py's split: the chunk copy of K / V into the LDS granules, the granule mapping
  of the issue's text, the lane's own row fragments, and the o store;
- registers / scratch of the new kernels, read from the built object, against the occupancy of their f32 twins.

tests/test_gpu_f32_attention_image.py compares the kernels with the f32 "high" forms on raw bits.
"""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest
import torch

import test_f32_presplit_host as PH
import test_f32_split_host as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _restore_highest():
    yield
    from vit_amd import _lib, ops
    ops.set_float32_attention_precision("highest")
    _lib.load().vit_sdpa_long_config(-1)


# ---------------------------------------------------------------------------- the switch

def _state():
    import vit_amd
    return (vit_amd.get_float32_attention_precision(), vit_amd.get_float32_attention_long(),
            vit_amd.get_float32_attention_presplit())


def test_setter_needs_high_and_resets_all_three():
    import vit_amd
    from vit_amd import _lib
    lib = _lib.load()
    vit_amd.set_float32_attention_precision("high", long_sequences=True, presplit=True)
    assert _state() == ("high", True, True)
    with pytest.raises(ValueError, match="presplit"):
        vit_amd.set_float32_attention_precision("highest", presplit=True)
    assert _state() == ("high", True, True), "a refused call changed a switch"
    with pytest.raises(ValueError):
        vit_amd.set_float32_attention_precision("highest", long_sequences=True, presplit=True)
    assert _state() == ("high", True, True)
    # every call sets all three switches
    vit_amd.set_float32_attention_precision("high", presplit=True)
    assert _state() == ("high", False, True)
    vit_amd.set_float32_attention_precision("high", long_sequences=True)
    assert _state() == ("high", True, False)
    vit_amd.set_float32_attention_precision("high", True, True)
    assert _state() == ("high", True, True)
    vit_amd.set_float32_attention_precision("high")
    assert _state() == ("high", False, False)
    vit_amd.set_float32_attention_precision("high", presplit=True)
    lib.vit_sdpa_f32_precision(0)                      # the C switch alone: "highest" carries no image
    assert _state() == ("highest", False, False)
    lib.vit_sdpa_f32_precision(1)
    assert _state() == ("high", False, True)
    vit_amd.set_float32_attention_precision("highest")
    assert _state() == ("highest", False, False)
    # independent of the GEMM switches
    assert vit_amd.get_float32_matmul_precision() == "highest"


def test_environment_variable_sets_the_initial_state():
    code = ("import sys; sys.path.insert(0, %r); from vit_amd import ops; "
            "print(ops.get_float32_attention_precision(), ops.get_float32_attention_long(), "
            "ops.get_float32_attention_presplit())" % os.path.join(ROOT, "vit-project_amd"))
    names = ("VIT_F32_ATTENTION", "VIT_F32_ATTENTION_LONG", "VIT_F32_ATTENTION_PRESPLIT")
    env = {k: v for k, v in os.environ.items() if k not in names}
    for vals, want in ((("high", "1", "1"), ["high", "True", "True"]),
                       (("high", None, "1"), ["high", "False", "True"]),
                       (("high", "1", None), ["high", "True", "False"]),
                       (("high", None, "0"), ["high", "False", "False"]),
                       ((None, None, "1"), ["highest", "False", "False"])):
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
    kw = {"float32_attention": "high", "float32_attention_long": True, "float32_attention_presplit": True}
    S._sweep_worker(0, 1, None, None, {}, [], dict(kw), Q(), [])
    assert seen["state"] == ("high", True, True) and "float32_attention_presplit" not in seen["kw"]
    del kw["float32_attention_presplit"]               # a caller from before the switch: the default is off
    S._sweep_worker(0, 1, None, None, {}, [], dict(kw), Q(), [])
    assert seen["state"] == ("high", True, False)

    class Ctx:
        def Queue(self):
            return self

        def Process(self, target, args):
            seen["worker_kw"] = args[6]
            raise RuntimeError("stop before a process starts")

    import torch.multiprocessing as mp
    monkeypatch.setattr(mp, "get_context", lambda kind: Ctx())
    for third in (True, False):
        vit_amd.set_float32_attention_precision("high", long_sequences=True, presplit=third)
        with pytest.raises(RuntimeError, match="stop before"):
            S.launch_sweep(1, None, None, {}, [])
        assert seen["worker_kw"]["float32_attention_presplit"] is third
        assert seen["worker_kw"]["float32_attention_long"] is True


# ---------------------------------------------------------------------------- symbols, the query, refusals

def test_new_symbols_are_declared_and_bound():
    from vit_amd import _lib
    lib = _lib.load()
    i32, i64, f32, vp = _lib.i32, _lib.i64, _lib.f32, _lib.vp
    assert lib.vit_abi_version() == 10  # additive
    hdr = open(os.path.join(ROOT, "include", "vit_hip.h")).read()
    for name in ("vit_sdpa_fwd_image", "vit_sdpa_fwd_takes_image", "vit_sdpa_f32_image_count"):
        assert name in _lib.exported_symbols() and hasattr(lib, name) and f"int {name}(" in hdr
    assert _lib.SIGNATURES["vit_sdpa_fwd_image"] == [i32, i32, i32, i32, vp, i64, vp, i64, vp, f32, i32, vp]
    assert _lib.SIGNATURES["vit_sdpa_fwd_takes_image"] == [i32, i32, i32, i32, i32, i64, C.c_uint64]
    assert _lib.SIGNATURES["vit_sdpa_f32_image_count"] == [i32]
    assert lib.vit_sdpa_f32_image_count(1) >= 0 and lib.vit_sdpa_f32_image_count(0) == 0
    import vit_amd
    from vit_amd import ops
    assert vit_amd.get_float32_attention_presplit is ops.get_float32_attention_presplit
    assert callable(ops.sdpa_fwd_takes_image)


def test_the_query_is_the_dispatch_rule():
    """True exactly where vit_sdpa_fwd with f32 tensors takes the bf16x3 kernels."""
    from vit_amd import _lib
    lib = _lib.load()
    q = lib.vit_sdpa_fwd_takes_image
    for mode in (0, 1):
        for long in (0, 1):
            for streamed in (1, 0):
                lib.vit_sdpa_f32_precision(mode)
                lib.vit_sdpa_f32_long_precision(long)
                lib.vit_sdpa_long_config(streamed)
                for N in (1, 16, 77, 257, 288, 289, 577, 785):
                    for causal in (0, 1):
                        for pitch in (384, 388, 390, 385):
                            want = (mode == 1 and pitch % 4 == 0
                                    and (N <= 288 or (not causal and long == 1 and streamed == 1)))
                            got = q(2, 2, N, 64, causal, pitch | 132, 16)
                            assert bool(got) == want, (mode, long, streamed, N, causal, pitch)
    lib.vit_sdpa_f32_precision(1)
    lib.vit_sdpa_long_config(-1)
    assert q(2, 2, 77, 64, 0, 384 | 128, 16) == 1
    assert q(2, 2, 77, 32, 0, 384 | 128, 16) == 0          # head_dim
    assert q(2, 2, 77, 64, 0, 384 | 130, 16) == 0          # the o pitch
    assert q(2, 2, 77, 64, 0, 384 | 128, 16 | 8) == 0      # qkv or o not 16-byte aligned
    assert q(2, 2, 0, 64, 0, 384 | 128, 16) == 0
    # the Python query: the dtype and the unit column stride too
    from vit_amd import ops
    qkv, o, lse = torch.empty(2 * 77, 384), torch.empty(2 * 77, 128), torch.empty(2 * 2 * 77)
    aligned = (qkv.data_ptr() | o.data_ptr()) % 16 == 0
    assert ops.sdpa_fwd_takes_image(qkv, 2, 2, 77, o, lse) is aligned
    assert ops.sdpa_fwd_takes_image(qkv, 2, 2, 77, o, torch.empty(2 * 2 * 77 + 1)[1:]) is aligned   # lse: any address
    assert ops.sdpa_fwd_takes_image(qkv.bfloat16(), 2, 2, 77, o, lse) is False
    assert ops.sdpa_fwd_takes_image(qkv, 2, 2, 77, o.bfloat16(), lse) is False
    assert ops.sdpa_fwd_takes_image(torch.empty(384, 2 * 77).T, 2, 2, 77, o, lse) is False


def test_image_calls_are_refused_on_the_host_before_any_launch():
    """No GPU is touched by a refused call: the library answers from the arguments alone."""
    from vit_amd import _lib
    lib = _lib.load()

    def fwd(N=77, causal=0, hd=64, heads=2, ld_qkv=388, ld_o=132, qkv=16, o=32, lse=48):
        return lib.vit_sdpa_fwd_image(2, heads, N, hd, qkv, ld_qkv, o, ld_o, lse, 0.125, causal, None)

    lib.vit_sdpa_f32_image_count(1)
    lib.vit_sdpa_f32_precision(0)
    lib.vit_sdpa_f32_long_precision(1)
    assert fwd() == 1 and fwd(N=289) == 1                          # "highest"
    lib.vit_sdpa_f32_precision(1)
    lib.vit_sdpa_f32_long_precision(0)
    assert fwd(N=289) == 1                                         # past 288 tokens without the long switch
    lib.vit_sdpa_f32_long_precision(1)
    assert fwd(N=289, causal=1) == 1                               # no causal streamed form
    assert fwd(hd=32, heads=4) == 1
    assert fwd(ld_qkv=387) == 1 and fwd(ld_o=130) == 1             # a row pitch that is no multiple of 4 floats
    assert fwd(qkv=20) == 1 and fwd(o=40) == 1                     # (lse is stored a float at a time: any address)
    assert fwd(qkv=None) == 1 and fwd(o=None) == 1 and fwd(lse=None) == 1
    assert fwd(N=0) == 1
    lib.vit_sdpa_long_config(0)
    assert fwd(N=289) == 1                                         # the streamed kernels switched off
    assert lib.vit_sdpa_f32_image_count(1) == 0


# ---------------------------------------------------------------------------- what the kernels do with image bytes

def _head_image(x):
    """The image bytes of a head slice x [rows, 64] as bf16 elements [rows, 128] (256 bytes a row), and x's split."""
    return PH.image_ref(x).view(torch.bfloat16).float(), H.split(x)


def _bytes(bits, byte, n=8):
    """n bytes of every row from byte offset ``byte``: n / 2 bf16 elements."""
    return bits[:, byte // 2:(byte + n) // 2]


def test_granule_mapping_of_an_image_row():
    """The LDS granule (r, c) holds head dims 8c .. 8c + 7: two 8-byte pieces of the hi region, the same + 64 of lo."""
    x = PH.scaled_randn(9, 64, seed=41)
    bits, (hi, lo) = _head_image(x)
    assert float((lo != 0).float().mean()) > 0.9
    for c in range(8):
        m, k0 = c >> 2, 8 * (c & 3)
        hh, ga = k0 >> 4, (k0 & 15) >> 2
        a, b = 128 * m + 16 * ga + 8 * hh, 128 * m + 16 * (ga + 1) + 8 * hh
        assert torch.equal(torch.cat([_bytes(bits, a), _bytes(bits, b)], 1), hi[:, 8 * c:8 * c + 8]), c
        assert torch.equal(torch.cat([_bytes(bits, a + 64), _bytes(bits, b + 64)], 1), lo[:, 8 * c:8 * c + 8]), c


def test_chunk_copy_fills_the_granules_split8_would_have_written():
    """x3_put_chunk: thread c copies the 16-byte hi and lo chunk g = c & 3 of k-block m = c >> 2 as two 8-byte
    pieces each, into half g & 1 of the granules 4m + (g >> 1) and 4m + 2 + (g >> 1); the eight threads of a row
    fill every granule once, with what the f32 form stores there."""
    x = PH.scaled_randn(9, 64, seed=42)
    bits, (hi, lo) = _head_image(x)
    img = {"hi": torch.full((9, 8, 8), float("nan")), "lo": torch.full((9, 8, 8), float("nan"))}  # [row, granule, j]
    writes = 0
    for c in range(8):
        m, g = c >> 2, c & 3
        for name, u in (("hi", 0), ("lo", 1)):
            chunk = _bytes(bits, m * 128 + u * 64 + g * 16, 16)        # x3_chunk
            c0, half = (c & 4) + ((c & 3) >> 1), (c & 1) * 4           # bf16 elements
            assert torch.isnan(img[name][:, c0, half:half + 4]).all() and torch.isnan(img[name][:, c0 + 2, half:half + 4]).all()
            img[name][:, c0, half:half + 4] = chunk[:, :4]
            img[name][:, c0 + 2, half:half + 4] = chunk[:, 4:]
            writes += 2
    assert writes == 32
    assert torch.equal(img["hi"].reshape(9, 64), hi) and torch.equal(img["lo"].reshape(9, 64), lo)


def test_row_fragments_from_an_image_row():
    """x3_row_image: lane group g's fragment kk is head dims 32 kk + 8g .. + 7, split."""
    x = PH.scaled_randn(16, 64, seed=43)
    bits, (hi, lo) = _head_image(x)
    for g in range(4):
        base = (g & 1) * 32 + (g >> 1) * 8
        for kk in range(2):
            w = [_bytes(bits, base + kk * 128 + (u >> 1) * 64 + (u & 1) * 16) for u in range(4)]
            d0 = kk * 32 + g * 8
            assert torch.equal(torch.cat(w[:2], 1), hi[:, d0:d0 + 8]), (g, kk)
            assert torch.equal(torch.cat(w[2:], 1), lo[:, d0:d0 + 8]), (g, kk)


def test_o_store_writes_the_image_of_the_row():
    """x3_store_row_image: the lane of group g holds columns 16 dt + 4g .. + 3 in oacc[dt]; split8(oacc[2m],
    oacc[2m + 1]) is hi / lo chunk g of k-block m."""
    o = PH.scaled_randn(16, 64, seed=44)
    out = torch.zeros(16, 128, dtype=torch.bfloat16)
    for g in range(4):
        oacc = [o[:, 16 * dt + 4 * g:16 * dt + 4 * g + 4] for dt in range(4)]
        for m in range(2):
            hi, lo = H.split(torch.cat([oacc[2 * m], oacc[2 * m + 1]], 1))
            byte = 128 * m + 16 * g
            out[:, byte // 2:byte // 2 + 8] = hi.to(torch.bfloat16)
            out[:, (byte + 64) // 2:(byte + 64) // 2 + 8] = lo.to(torch.bfloat16)
    want = PH.image_ref(o)
    assert torch.equal(out.view(torch.float32).view(torch.int32), want.view(torch.int32))


# ---------------------------------------------------------------------------- the built kernels

def _kres(obj, pattern):
    return subprocess.run(["bash", os.path.join(ROOT, "tools", "kres.sh"), obj, pattern], capture_output=True,
                          text=True, check=True).stdout.splitlines()


def _regs(line):
    f = line.split()
    return int(f[0]) + (0 if f[1] == "None" else int(f[1]))


def test_image_kernels_have_no_spills_and_keep_their_twins_occupancy():
    obj = os.path.join(ROOT, "vit-project_amd", "csrc", "build", "attention.o")
    if not os.path.exists(obj) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("attention.o not built / no ROCm LLVM tools")
    res = _kres(obj, "attn_fwd_image_x3ILi")
    twins = _kres(obj, "attn_fwd_f32x3ILi")
    assert len(res) == len(twins) == 36, (len(res), len(twins))    # 18 tile counts, causal or not
    for line in res + twins:
        assert " spill 0 " in line and " priv 0 " in line and int(line.split()[-1]) == 0, line
        nt = int(re.search(r"ILi(\d+)ELb", line).group(1))
        lds = 4 * ((nt + 1) // 2) * 32 * 128                       # F32X3<NT>::LDS
        wps = 4 if 2 * lds <= 163840 else 2                        # F32X3<NT>::WPS: waves per SIMD
        assert _regs(line) <= 512 // wps, line
    st, st_twin = _kres(obj, "attn_fwd_image_stream"), _kres(obj, "attn_fwd_stream_x3PKf")
    assert len(st) == 1 and len(st_twin) == 1
    for line in st + st_twin:
        assert " spill 0 " in line and " priv 0 " in line and int(line.split()[-1]) == 0, line
        assert _regs(line) <= 128, line                            # __launch_bounds__(512, 4)
