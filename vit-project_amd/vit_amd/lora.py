"""LoRA adapter layer: drop-in for ``LoRALayer`` (NEWP:307-336, repeated in BASEP:193-222).

Same constructor, attributes (``original_layer``, ``r``, ``lora_alpha``, ``lora_dropout``, ``scaling``),
parameter names (``lora_A`` [r, out], ``lora_B`` [in, r]), state-dict keys and RNG consumption (``randn`` for
A, then ``kaiming_uniform_`` on A and on B: B is *not* zero, so W != W0 at initialisation), so
``apply_lora_to_ViT`` / ``unfreeze_lora_layers`` and a training loop written for the reference work unchanged.

The reference's quirk, reproduced as it is: ``.weight`` is ``W0 + (B @ A) * s`` with ``B @ A`` [in, out]
added to ``W0`` [out, in] *without* a transpose.  It is defined only for in == out and is not the weight
``forward`` applies (that one is ``W0 + s * (B @ A)^T``): ``F.linear(x, layer.weight)`` differs from
``layer(x)``.  ``nn.MultiheadAttention`` reads ``out_proj.weight`` (quirk Q5, as for DoRA), so on the
CLIP-HBA path ``W0 + s * (B @ A)`` is the weight that trains.  Its build and backward are HIP kernels
(csrc/lora.hip); ``forward(x)`` is the reference's formula on the HIP GEMMs (never reached on the CLIP path,
but part of the class's surface).
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from . import _lib as L
from . import ops
from ._lib import call, ptr
from .dora import _LinearF32Fn

MAX_R = 64


def _check(W0, A, Bm):
    if W0.dim() != 2 or W0.shape[0] != W0.shape[1]:
        raise ValueError(f"lora_weight: W0 + (B @ A) * s adds [in, out] to [out, in] without a transpose (the "
                         f"reference's LoRALayer.weight), so it needs in == out; got W0 {tuple(W0.shape)}")
    n = W0.shape[0]
    r = A.shape[0] if A.dim() == 2 else -1
    if not 1 <= r <= MAX_R:
        raise ValueError(f"lora_weight: rank {r} outside 1..{MAX_R}")
    if tuple(A.shape) != (r, n) or tuple(Bm.shape) != (n, r):
        raise ValueError(f"lora_weight: A {tuple(A.shape)} / B {tuple(Bm.shape)} do not fit W0 [{n}, {n}], r = {r}")
    return n, r


class _LoraWeightFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, W0, A, Bm, scaling):
        n, r = A.shape[1], A.shape[0]
        dev = W0.device
        W = torch.empty(n, n, dtype=torch.float32, device=dev)
        W0_ = W0.detach().float().contiguous()
        A_, B_ = A.detach().float().contiguous(), Bm.detach().float().contiguous()
        call("vit_lora_weight_fwd", n, r, ptr(W0_), ptr(A_), ptr(B_), float(scaling), ptr(W),
             L.stream_ptr(dev))
        ctx.save_for_backward(A_, B_)
        ctx.scaling = scaling
        return W

    @staticmethod
    def backward(ctx, gW):
        A, Bm = ctx.saved_tensors
        r, n = A.shape
        dev = A.device
        ng = ctx.needs_input_grad
        dA = dB = None
        if ng[1] or ng[2]:
            g = gW.contiguous().float()
            dA, dB = torch.empty_like(A), torch.empty_like(Bm)
            nfl = L.lib().vit_lora_weight_bwd_ws_floats(n, r)
            if nfl <= 0:
                raise L.HipError(f"vit_lora_weight_bwd: no workspace size for n = {n}, r = {r}")
            ws = ops.workspace(f"lora_bwd:{L.stream_ptr(dev)}", nfl * 4, dev)
            call("vit_lora_weight_bwd", n, r, ptr(A), ptr(Bm), ptr(g), float(ctx.scaling), ptr(dA), ptr(dB), ptr(ws),
                 L.stream_ptr(dev))
        return (gW if ng[0] else None), (dA if ng[1] else None), (dB if ng[2] else None), None


def lora_weight(W0, A, Bm, scaling):
    """W [n, n] = W0 + (B @ A) * s, the reference's ``LoRALayer.weight`` (NEWP:330-332) with its missing
    transpose (module docstring): W0 [n, n], A [r, n], B [n, r], f32, 1 <= r <= 64.  Gradients: dA = s B^T gW,
    dB = s gW A^T, and dW0 = gW only when W0 asks for it.  ``ValueError`` before anything is queued when W0
    is not square or r is out of range."""
    _check(W0, A, Bm)
    L.require_gpu(W0)
    return _LoraWeightFn.apply(W0, A, Bm, scaling)


class LoRALayer(nn.Module):
    def __init__(self, original_layer, r=8, lora_alpha=16, lora_dropout=0.1):
        super().__init__()
        self.original_layer = original_layer
        self.r = r
        self.lora_alpha = lora_alpha
        self.lora_dropout = nn.Dropout(p=lora_dropout)
        self.lora_A = nn.Parameter(torch.randn(self.r, original_layer.out_features))
        self.lora_B = nn.Parameter(torch.zeros(original_layer.in_features, self.r))
        self.scaling = self.lora_alpha / self.r
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.kaiming_uniform_(self.lora_A, a=math.sqrt(5))
        nn.init.kaiming_uniform_(self.lora_B, a=math.sqrt(5))

    @property
    def weight(self):
        """``W0 + (B @ A) * s`` (no transpose: in == out only, module docstring), what MHA reads."""
        return lora_weight(self.original_layer.weight, self.lora_A, self.lora_B, self.scaling)

    @property
    def bias(self):
        return self.original_layer.bias

    def forward(self, x):
        """NEWP:325-328: ``original_layer(x) + (lora_dropout(x) @ B @ A) * s``, f32 on the HIP GEMMs."""
        L.require_gpu(x)
        base = self.original_layer
        shp = x.shape
        x2 = x.reshape(-1, shp[-1]).float().contiguous()
        xd = self.lora_dropout(x).reshape(-1, shp[-1]).float().contiguous()
        y = _LinearF32Fn.apply(x2, base.weight.float(), None if base.bias is None else base.bias.float())
        # x @ B and (.) @ A as F.linear on the transposed factors ([r, in] and [out, r], tiny copies)
        u = _LinearF32Fn.apply(xd, self.lora_B.float().t().contiguous(), None)
        v = _LinearF32Fn.apply(u, self.lora_A.float().t().contiguous(), None)
        return (y + v * self.scaling).reshape(*shp[:-1], y.shape[-1])
