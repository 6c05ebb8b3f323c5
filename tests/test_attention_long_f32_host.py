"""CPU: the host-side surface of the streamed f32 attention (no GPU needed).

- the ``ViT-L/14@336px`` backbone entry is ViT-L/14 at resolution 336;
- include/vit_hip.h declares ``vit_sdpa_long_f32_count`` and vit_amd/_lib.py binds it (test_host_abi's export
  test then checks the built library against both);
- the three streamed f32 kernels are in the built attention object with no VGPR spill and no scratch
  (tools/kres.sh; skipped when the object is not built, as tests/test_kernel_resources.py).
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "vit-project_amd", "csrc", "build")
LLVM = "/opt/rocm/lib/llvm/bin"
KERNELS = ("attn_fwd_stream_f32", "attn_bwd_dq_stream_f32", "attn_bwd_dkv_stream_f32")


def test_vit_l14_336_backbone_entry():
    from vit_amd import clip
    e = clip._BACKBONES["ViT-L/14@336px"]
    assert e["image_resolution"] == 336
    assert {**e, "image_resolution": 224} == clip._BACKBONES["ViT-L/14"]
    assert (e["image_resolution"] // e["vision_patch_size"]) ** 2 + 1 == 577 and e["vision_width"] // 64 == 16


def test_long_f32_count_declared_and_bound():
    from vit_amd import _lib
    txt = open(os.path.join(ROOT, "include", "vit_hip.h")).read()
    assert re.search(r"\bint\s+vit_sdpa_long_f32_count\s*\(\s*int\s+reset\s*\)\s*;", txt)
    assert _lib.SIGNATURES["vit_sdpa_long_f32_count"] == [_lib.i32]
    assert "vit_sdpa_long_f32_count" in _lib.exported_symbols()


def test_streamed_f32_kernels_have_no_spills():
    obj = os.path.join(BUILD, "attention.o")
    if not os.path.exists(obj) or not os.path.exists(f"{LLVM}/llvm-readelf"):
        pytest.skip("attention.o not built / no ROCm LLVM tools")
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kres.sh"), obj, "stream_f32"],
                         capture_output=True, text=True, check=True).stdout.splitlines()
    for name in KERNELS:
        mine = [l for l in out if re.search(r"\d" + name + r"PK", l)]
        assert len(mine) == 1, (name, out)
        assert " spill 0 " in mine[0] and " priv 0 " in mine[0], mine[0]
