"""Attention test cases with a float64 reference (test infrastructure only: imported by tests/).

``make_case`` draws q, k, v = randn * 1.5 per (b, h), reshapes them by ``kind`` into the score
distributions that trained ViT / CLIP towers show and random draws do not (peaked rows, a large common
score offset, single outlier keys, a running maximum that moves in every chunk, all-zero rows), rounds the
inputs to the storage dtype and evaluates plain ``softmax(q k^T * scale) v`` with autograd in float64 on
the rounded inputs.  ``emulate_bf16`` restates, again in float64, the roundings a correct bf16 kernel
cannot avoid (P and dS to bf16 before their MFMAs, o and the gradients stored as bf16): the error it
makes against the reference is the floor under every bf16 bound, found without reading the library.
``torch_f32`` evaluates the same formula in torch float32 on the CPU: the yardstick for the f32 bounds.

Layouts are the library's: qkv [B*N, 3*H*64] with q at column h*64, k at D + h*64, v at 2D + h*64
(D = H*64, row b*N + n); o and do [B*N, D]; lse [B*H*N] (natural log of the scaled scores);
grads [B*N, 3D] = [dq | dk | dv]; colsum [3D] = the qkv bias gradient.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

KINDS = ("base", "peaked", "offset", "outlier", "rising", "falling", "zerorows")
# ``offset`` made milder (q, k += 4: lse ~ 110..160) for the f32 MFMA backward, whose scores are a chain of 64
# sequential f32 FMAs at the raw magnitude q.k ~ 2400 (tests/test_gpu_attention_conformance.py)
MILDER = {"offset": "offset4"}

# the project's bf16 bounds, relative to the reference's largest magnitude (tests/test_gpu_kernels._close)
BF16_O, BF16_LSE, BF16_GRAD = 1.5e-2, 2e-3, 3e-2
BF16_LSE_ABS = 2e-2   # what BF16_LSE admits at lse ~ 10 (randn * 1.5); held on every kind
BF16_ROW = 1.5e-2     # worst single row of a single (b, h): |err_row| / |ref_row|, o and dv
F32_O, F32_LSE, F32_GRAD = 1e-5, 1e-5, 1e-4


@dataclass
class Case:
    kind: str
    B: int
    H: int
    N: int
    dtype: torch.dtype
    causal: bool
    scale: float
    qkv: torch.Tensor     # [B*N, 3D] dtype
    do: torch.Tensor      # [B*N, D] dtype
    o: torch.Tensor       # [B*N, D] float64
    lse: torch.Tensor     # [B*H*N] float64
    grads: torch.Tensor   # [B*N, 3D] float64
    colsum: torch.Tensor  # [3D] float64

    @property
    def D(self):
        return self.H * 64


def pack(t):
    """[B, H, N, 64] -> [B*N, H*64]"""
    B, H, N, d = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * N, H * d)


def unpack(x, B, H, N):
    """[B*N, H*64] -> [B, H, N, 64]"""
    return x.reshape(B, N, H, 64).permute(0, 2, 1, 3)


def split_qkv(qkv, B, H, N):
    """[B*N, 3D] -> q, k, v [B, H, N, 64]"""
    D = H * 64
    return tuple(unpack(qkv[:, i * D:(i + 1) * D], B, H, N) for i in range(3))


def _shape_inputs(kind, q, k, v, g):
    B, H, N, _ = q.shape
    if kind == "base":
        pass
    elif kind == "peaked":
        q *= 8 / 3
        k *= 8 / 3
    elif kind in ("offset", "offset4"):
        q += 6 if kind == "offset" else 4
        k += 6 if kind == "offset" else 4
    elif kind == "outlier":
        k[:, :, N - 1] = 8 * torch.sign(q[:, :, 0])
        v[:, :, N - 1] *= 20
    elif kind in ("rising", "falling"):
        u = torch.randn(B, H, 1, 64, generator=g, dtype=torch.float64)
        u = u / u.norm(dim=-1, keepdim=True)
        ramp = torch.linspace(0, 1, N, dtype=torch.float64) if N > 1 else torch.ones(1, dtype=torch.float64)
        if kind == "falling":
            ramp = ramp.flip(0)
        q += 16 * u
        k += 20 * ramp[None, None, :, None] * u
    elif kind == "zerorows":
        q[:, :, ::3] = 0
        k[:, :, 1::5] = 0
        v[:, :, 2::7] = 0
    else:
        raise ValueError(f"unknown kind {kind!r}")


def _mask(N):
    return torch.ones(N, N, dtype=torch.bool).triu(1)


def _sdpa_autograd(q, k, v, do, scale, causal):
    """softmax(q k^T * scale) v and its gradients in the dtype of q; q, k, v, do [B, H, N, 64]."""
    q, k, v = (t.clone().requires_grad_(True) for t in (q, k, v))
    s = (q @ k.transpose(-1, -2)) * scale
    if causal:
        s = s.masked_fill(_mask(q.shape[2]), -math.inf)
    lse = torch.logsumexp(s, -1)
    o = torch.softmax(s, -1) @ v
    o.backward(do)
    return o.detach(), lse.detach(), q.grad, k.grad, v.grad


def make_case(kind, B, H, N, dtype, causal=False, seed=34, scale=0.125):
    """Inputs of one (kind, shape), rounded to ``dtype``, and the float64 reference on the rounded inputs."""
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(B, H, N, 64, generator=g, dtype=torch.float64) * 1.5 for _ in range(3))
    do = torch.randn(B, H, N, 64, generator=g, dtype=torch.float64)
    _shape_inputs(kind, q, k, v, g)
    qkv = torch.cat([pack(q), pack(k), pack(v)], 1).to(dtype).contiguous()
    do = pack(do).to(dtype).contiguous()
    q, k, v = split_qkv(qkv.double(), B, H, N)
    o, lse, dq, dk, dv = _sdpa_autograd(q, k, v, unpack(do.double(), B, H, N), scale, causal)
    grads = torch.cat([pack(dq), pack(dk), pack(dv)], 1)
    return Case(kind, B, H, N, dtype, causal, scale, qkv, do, pack(o), lse.reshape(-1), grads, grads.sum(0))


def torch_f32(case):
    """The same formula in torch float32 on the CPU: (o, lse, grads, colsum), each as float64."""
    B, H, N = case.B, case.H, case.N
    q, k, v = split_qkv(case.qkv.float(), B, H, N)
    o, lse, dq, dk, dv = _sdpa_autograd(q, k, v, unpack(case.do.float(), B, H, N), case.scale, case.causal)
    grads = torch.cat([pack(dq), pack(dk), pack(dv)], 1)
    return pack(o).double(), lse.reshape(-1).double(), grads.double(), grads.sum(0).double()


def _bf16(x):
    return x.float().to(torch.bfloat16).double()


def emulate_bf16(case):
    """What a correct bf16 kernel must round, in float64 otherwise: (o, lse, grads, colsum).

    Forward: p = exp(s - rowmax) as f32, its row sum taken unrounded, p rounded to bf16 for P V, o rounded
    to bf16.  Backward (from the reference's o rounded to bf16 and the reference's lse as f32, as the tests
    feed it): P = exp(s - lse) and dS = p * (dP - delta) rounded to bf16 before dV = P^T dO,
    dQ = dS K * scale and dK = dS^T Q * scale; the three stored as bf16; colsum sums the stored values."""
    B, H, N = case.B, case.H, case.N
    q, k, v = split_qkv(case.qkv.double(), B, H, N)
    do = unpack(case.do.double(), B, H, N)
    s = (q @ k.transpose(-1, -2)) * case.scale
    masked = _mask(N) if case.causal else None
    if masked is not None:
        s = s.masked_fill(masked, -math.inf)
    m = s.amax(-1, keepdim=True)
    p = torch.exp(s - m).float().double()
    l = p.sum(-1, keepdim=True)
    o = _bf16((_bf16(p) @ v) / l)
    lse = (m + torch.log(l)).squeeze(-1).float().double()

    o_in = unpack(_bf16(case.o), B, H, N)
    lse_in = case.lse.float().double().reshape(B, H, N, 1)
    p = torch.exp(s - lse_in)
    delta = (do * o_in).sum(-1, keepdim=True)
    ds = p * (do @ v.transpose(-1, -2) - delta)
    if masked is not None:
        ds = ds.masked_fill(masked, 0.0)
    pb, dsb = _bf16(p), _bf16(ds)
    dq = _bf16((dsb @ k) * case.scale)
    dk = _bf16((dsb.transpose(-1, -2) @ q) * case.scale)
    dv = _bf16(pb.transpose(-1, -2) @ do)
    grads = torch.cat([pack(dq), pack(dk), pack(dv)], 1)
    return pack(o), lse.reshape(-1), grads, grads.sum(0)


# ---------------------------------------------------------------------------- error measures

def rel_max(got, ref, whole=None):
    """max |got - ref| / max |ref|: the measure of the project's bounds (_close).  Where ``ref`` is
    identically zero (dq and dk of a one-token sequence: softmax over one key is constant) the measure has
    no scale of its own and takes that of ``whole``, the [dq | dk | dv] the block belongs to."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    scale = ref.abs().max()
    if scale == 0 and whole is not None:
        scale = whole.detach().double().abs().max()
    return ((got - ref).abs().max() / (scale + 1e-12)).item()


def abs_max(got, ref):
    return (got.detach().double().cpu() - ref.detach().double().cpu()).abs().max().item()


def row_rel(got, ref, B, H, N):
    """Worst |err_row| / |ref_row| over the 64-wide rows of single (b, h) items; got, ref [B*N, H*64]."""
    got, ref = unpack(got.detach().double().cpu(), B, H, N), unpack(ref.detach().double().cpu(), B, H, N)
    return ((got - ref).norm(dim=-1) / ref.norm(dim=-1).clamp_min(1e-300)).max().item()


def item_rel(got, ref, B, H, N):
    """Worst |err_item| / |ref_item| over (b, h) items, each item its dq, dk and dv together (what
    test_sdpa_bwd_large_grid computes); got, ref [B*N, 3*H*64]."""
    def items(x):
        return x.detach().double().cpu().reshape(B, N, 3, H, 64).permute(0, 3, 2, 1, 4).reshape(B * H, -1)
    err, scl = items(got) - items(ref), items(ref)
    return (err.norm(dim=1) / scl.norm(dim=1).clamp_min(1e-6)).max().item()


# ---------------------------------------------------------------------------- what the kinds claim

def probabilities(case):
    """softmax of the reference's scaled scores, [B, H, N, N] float64."""
    q, k, _ = split_qkv(case.qkv.double(), case.B, case.H, case.N)
    s = (q @ k.transpose(-1, -2)) * case.scale
    if case.causal:
        s = s.masked_fill(_mask(case.N), -math.inf)
    return torch.softmax(s, -1)
