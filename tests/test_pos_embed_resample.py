"""CPU: resampling the absolute position embedding when a checkpoint meets a model of another
resolution (vit_amd.resample_abs_pos_embed / adapt_state_dict, timm's semantics)."""
import pytest
import torch
import torch.nn.functional as F

import vit_amd
from vit_amd import adapt_state_dict, resample_abs_pos_embed


def _posemb(side, C=32, seed=0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(1, 1 + side * side, C, generator=g).to(dtype)


def test_same_size_returns_the_same_tensor():
    pe = _posemb(14)
    assert resample_abs_pos_embed(pe, (14, 14)) is pe
    assert resample_abs_pos_embed(pe, 14, old_size=(14, 14)) is pe


def test_14_to_24_shape_and_prefix():
    pe = _posemb(14)
    out = resample_abs_pos_embed(pe, (24, 24))
    assert out.shape == (1, 577, 32) and out.dtype == pe.dtype
    assert torch.equal(out[:, :1], pe[:, :1])


def test_constant_grid_stays_constant():
    pe = torch.full((1, 197, 8), 0.37)
    pe[:, 0] = -2.0
    out = resample_abs_pos_embed(pe, (24, 24))
    assert (out[:, 1:] - 0.37).abs().max().item() <= 1e-6
    assert torch.equal(out[:, 0], pe[:, 0])


@pytest.mark.parametrize("new", [(24, 24), (7, 7), (12, 20)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_equals_interpolate_on_the_grid(new, dtype):
    pe = _posemb(14, dtype=dtype, seed=3)
    C = pe.shape[-1]
    grid = pe[:, 1:].float().reshape(1, 14, 14, C).permute(0, 3, 1, 2)
    want = F.interpolate(grid, size=new, mode="bicubic", antialias=True, align_corners=False)
    want = want.permute(0, 2, 3, 1).reshape(1, new[0] * new[1], C).to(dtype)
    out = resample_abs_pos_embed(pe, new)
    assert out.dtype == dtype
    assert torch.equal(out[:, 1:], want)
    assert torch.equal(out[:, :1], pe[:, :1])


def test_no_prefix_and_bad_old_size():
    pe = _posemb(6)[:, 1:]
    assert resample_abs_pos_embed(pe, 9, num_prefix_tokens=0).shape == (1, 81, 32)
    with pytest.raises(ValueError):
        resample_abs_pos_embed(pe, 9, old_size=(5, 5), num_prefix_tokens=0)
    with pytest.raises(ValueError):
        resample_abs_pos_embed(_posemb(6)[:, :-1], 9)  # 35 grid tokens: not square


def _small(img_size, num_classes=10):
    return vit_amd.VisionTransformer(img_size=img_size, patch_size=16, embed_dim=128, depth=1, num_heads=2,
                                     num_classes=num_classes)


def test_adapt_state_dict_loads_224_into_384():
    src, dst = _small(224), _small(384)
    sd = src.state_dict()
    with pytest.raises(RuntimeError):
        dst.load_state_dict(sd, strict=True)
    new = adapt_state_dict(sd, dst)
    assert sd["pos_embed"].shape == (1, 197, 128)  # the input is left alone
    dst.load_state_dict(new, strict=True)
    assert dst.pos_embed.shape == (1, 577, 128)
    assert torch.equal(dst.pos_embed[:, :1], src.pos_embed[:, :1])
    assert torch.equal(dst.pos_embed.detach(), resample_abs_pos_embed(src.pos_embed.detach(), (24, 24)))
    assert torch.equal(dst.blocks[0].attn.qkv.weight, src.blocks[0].attn.qkv.weight)
    assert new["head.weight"].data_ptr() != sd["head.weight"].data_ptr()  # a copy


def test_adapt_state_dict_refuses_other_mismatches():
    sd = _small(224, num_classes=7).state_dict()
    with pytest.raises(ValueError, match="head.weight"):
        adapt_state_dict(sd, _small(384, num_classes=10))


def test_new_model_configs():
    from vit_amd.model import _MODEL_CFGS
    tokens = {k: (c["img_size"] // c["patch_size"]) ** 2 + 1 for k, c in _MODEL_CFGS.items()}
    assert tokens["vit_base_patch16_384"] == 577 and tokens["vit_large_patch16_384"] == 577
    assert tokens["vit_base_patch8_224"] == 785
