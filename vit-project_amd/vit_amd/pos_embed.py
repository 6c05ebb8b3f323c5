"""Loading a checkpoint into a model of another resolution: the absolute position embedding is the
one tensor whose shape depends on the image size.  One-time host work in plain torch (no kernel)."""
from __future__ import annotations

import math
from collections import OrderedDict

import torch
import torch.nn.functional as F


def _pair(size):
    if isinstance(size, (tuple, list)):
        h, w = size
        return int(h), int(w)
    return int(size), int(size)


def resample_abs_pos_embed(posemb, new_size, old_size=None, num_prefix_tokens=1):
    """timm's ``resample_abs_pos_embed``: ``posemb`` [1, P + h*w, C] -> [1, P + H*W, C].

    The P prefix tokens (class token) pass through untouched; the grid part is reshaped to
    [1, C, h, w] and resampled in fp32 with bicubic interpolation (``antialias=True``,
    ``align_corners=False``), then cast back to the input dtype.  ``old_size`` defaults to the square
    grid the token count implies.  The same grid in returns ``posemb`` itself."""
    new_h, new_w = _pair(new_size)
    n_grid = posemb.shape[1] - num_prefix_tokens
    if old_size is None:
        hw = int(math.isqrt(n_grid))
        if hw * hw != n_grid:
            raise ValueError(f"position embedding of {n_grid} grid tokens is not square: pass old_size")
        old_h, old_w = hw, hw
    else:
        old_h, old_w = _pair(old_size)
        if old_h * old_w != n_grid:
            raise ValueError(f"old_size {old_h}x{old_w} does not match {n_grid} grid tokens")
    if (old_h, old_w) == (new_h, new_w):
        return posemb
    prefix, grid = posemb[:, :num_prefix_tokens], posemb[:, num_prefix_tokens:]
    C = posemb.shape[-1]
    g = grid.to(torch.float32).reshape(1, old_h, old_w, C).permute(0, 3, 1, 2)
    g = F.interpolate(g, size=(new_h, new_w), mode="bicubic", antialias=True, align_corners=False)
    g = g.permute(0, 2, 3, 1).reshape(1, new_h * new_w, C).to(posemb.dtype)
    return torch.cat([prefix, g], dim=1) if num_prefix_tokens else g


def adapt_state_dict(state_dict, model):
    """A copy of ``state_dict`` that ``model.load_state_dict(..., strict=True)`` accepts when the two
    differ only in resolution: ``pos_embed`` is resampled to the model's patch grid.  Any other shape
    mismatch raises ``ValueError`` (a different width, depth-independent head size, patch size...)."""
    own = model.state_dict()
    out = OrderedDict()
    for k, v in state_dict.items():
        if k in own and tuple(v.shape) != tuple(own[k].shape):
            if k != "pos_embed":
                raise ValueError(f"{k}: checkpoint shape {tuple(v.shape)} does not fit the model's "
                                 f"{tuple(own[k].shape)} (only pos_embed is resampled)")
            P = getattr(model, "num_prefix_tokens", 1)
            pe = model.patch_embed
            side = pe.img_size // pe.patch_size
            v = resample_abs_pos_embed(v, (side, side), num_prefix_tokens=P)
            if tuple(v.shape) != tuple(own[k].shape):
                raise ValueError(f"pos_embed: resampled shape {tuple(v.shape)} does not fit the model's "
                                 f"{tuple(own[k].shape)}")
        out[k] = v.clone()
    return out
