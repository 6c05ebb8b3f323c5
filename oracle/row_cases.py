"""Cases for the row kernels (LayerNorm, cross-entropy, SGD, casts, CLIP pieces) with float64 references
(test infrastructure only: imported by tests/).

Every builder draws its inputs from a seeded generator, shapes them by ``kind``, rounds them to the storage
dtype and evaluates the operation in float64 on the rounded inputs (autograd for the backward passes).
``torch_f32`` members hold the same formula evaluated in torch float32 on the CPU: the yardstick of the f32
bounds, never the kernel's own output.

LayerNorm kinds: ``base`` randn * 2; ``offset`` 100 + randn (a one-pass variance E[x^2] - mean^2 loses every
digit here); ``tiny`` randn * 1e-3 (variance ~ eps, so a wrong eps shows); ``const`` every element 3.25 (sums
of 3.25 are exact in f32 up to D = 2048, so the mean is exact, x - mean is 0 and y is the bias bit for bit);
``outlier`` randn with one element of 1e4 per row.

Cross-entropy kinds: ``base`` randn * 3; ``wide`` randn * 30; ``spike``, ``equal`` and ``low`` are ``base`` with
row 0 replaced by a single +80 among values near -80, by one value repeated, and by -90 everywhere (without the
max subtraction ``wide`` overflows exp and the last sinks into the denormals: log 0 once they are flushed).
Targets hold class 0 and class C - 1.

Bounds are the project's own (tests/test_gpu_kernels.py), relative to the reference's largest magnitude:
f32 in and out 1e-5, bf16 out 8e-3 (LayerNorm) / 1e-2, optimizers 1e-6, copies and single adds 0.  On the
kinds where f32 arithmetic itself exceeds 1e-5 (``offset``, ``outlier``, ``wide``: a two-pass f32 LayerNorm at
offset 100 is 4e-6..5e-6 of scale away from float64) the bound of an output is four times the error torch
float32 makes on that output of that case -- the factor covers another summation order and the hardware
rsqrt / exp -- and never below the project's bound: on an output torch happens to get exactly right (a mean of
few terms, an identically zero gradient) four times nothing would ask for bits, which no bound here means.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import torch

F32 = 1e-5       # f32 in, f32 out
BF16_LN = 8e-3   # bf16 out, LayerNorm
BF16 = 1e-2      # bf16 out, elsewhere
OPT = 1e-6       # optimizers against torch's
HARD_FACTOR = 4.0

LN_KINDS = ("base", "offset", "tiny", "const", "outlier")
LN_HARD = ("offset", "outlier")
CE_KINDS = ("base", "wide", "spike", "equal", "low")
CE_HARD = ("wide",)
CONST = 3.25

# ---------------------------------------------------------------------------- the shapes the GPU tests run
LN_FWD_VEC_D = (256, 512, 768, 1024, 1536, 2048)
LN_FWD_SCALAR_D = (1280, 1792, 8, 33, 64, 200, 1000)
LN_FWD_ROWS = (1, 3, 4, 5, 37)
LN_KIND_D = (768, 200)
LN_EPS = {"tiny": (1e-6, 1e-5)}  # every other kind: 1e-6
LN_MAX_D = 2048
LN_FWD_LAST_SLOT = (2048, 2050)  # (D, ldx): ld % 4 != 0 sends the widest D to the scalar kernel
ADD_LN_D = tuple(256 * k for k in range(1, 9))
ADD_LN_ROWS = (1, 5, 37)
ADD_LN_KINDS = ("offset", "tiny")
LN_BWD_PIPE_D = (768, 1024)
LN_BWD_SCALAR_D = (256, 1280, 2048, 200, 33)
# a wave of a 32-row block owns 0..3 rows (1, 4, 5, 8, 9, 12, 13), one full block (32), ragged second (33, 37) and
# fifth (130) blocks
LN_BWD_ROWS = (1, 4, 5, 8, 9, 12, 13, 32, 33, 37, 130)
LN_BWD_RES_EVERY = (5, (13, 37))
LN_BWD_COMPACT_NP = (4, (15, 35))
LN_BWD_ODD_LD = 2  # lddy = D + 2: ld % 4 != 0
CE_SHAPES = ((1, 1), (1, 10), (3, 63), (4, 64), (5, 65), (9, 1001), (37, 1000))
CE_LD_PAD = 3
CAST_N = (1, 3, 4, 5, 1023, 1024, 1025, 4099)
POS_B = (1, 7, 8, 9, 31, 32, 33, 40)
POS_SD = ((5, 64), (17, 192), (3, 6), (2, 1))
UNFOLD_PS = (16, 14, 8, 6)
SGD_N = (1, 3, 4, 5, 4095, 4096, 4097, 8193)
EMBED_D = (4, 128, 260, 768)
ROWS_D = (1, 63, 64, 65, 200)
ROWNORM_D = (1, 63, 64, 65, 66, 768)
ROWNORM_SCALES = (1.0, 1e-6, 1e6)
MSE_N = (1, 63, 1023, 1024, 1025, 4224, 70001)


def rel_max(got, ref):
    """max |got - ref| / max |ref|: the measure of the project's bounds (``_close``)."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    if ref.numel() == 0:
        return 0.0
    return ((got - ref).abs().max() / (ref.abs().max() + 1e-12)).item()


def row_rel_max(got, ref, scale=None):
    """The worst row of max |got_row - ref_row| / max |ref_row| (rows of very different magnitude); ``scale``
    [rows] replaces max |ref_row| where a row of the reference may be identically zero."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    scale = ref.abs().amax(-1) if scale is None else scale.detach().double().cpu()
    return ((got - ref).abs().amax(-1) / (scale + 1e-300)).max().item()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


# ---------------------------------------------------------------------------- LayerNorm

def ln_input(kind, rows, D, g):
    """x [rows, D] float64 of one kind (before rounding to the storage dtype)."""
    if kind == "base":
        return _randn(g, rows, D) * 2
    if kind == "offset":
        return 100 + _randn(g, rows, D)
    if kind == "tiny":
        return _randn(g, rows, D) * 1e-3
    if kind == "const":
        return torch.full((rows, D), CONST, dtype=torch.float64)
    if kind == "outlier":
        x = _randn(g, rows, D)
        x[torch.arange(rows), torch.randint(0, D, (rows,), generator=g)] = 1e4
        return x
    raise ValueError(f"unknown LayerNorm kind {kind!r}")


def ln_fwd(x, w, b, eps):
    """F.layer_norm over the last dim, written out, in the dtype of x: (y, mean, rstd)."""
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    rstd = (d * d).mean(-1, keepdim=True).add(eps).rsqrt()
    return d * rstd * w + b, mean.squeeze(-1), rstd.squeeze(-1)


def ln_bwd(x, dy, w, mean, rstd):
    """The LayerNorm backward from given statistics, in the dtype of x: (dx, dgamma, dbeta)."""
    xh = (x - mean[:, None]) * rstd[:, None]
    g = dy * w
    dx = rstd[:, None] * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    return dx, (dy * xh).sum(0), dy.sum(0)


class _Bounded:
    """``bound(name)``: the project's bound, or on a hard kind 4x torch float32's own error on that output of
    this case if that is larger."""
    hard = ()

    def bound(self, name, base=F32):
        if self.kind not in self.hard:
            return base
        if name not in self._err:
            self._err[name] = rel_max(self.torch_f32[name], self.ref[name])
        return max(base, HARD_FACTOR * self._err[name])


@dataclass
class LnCase(_Bounded):
    hard = LN_HARD
    kind: str
    rows: int
    D: int
    eps: float
    x: torch.Tensor        # [rows, D] storage dtype
    dy: torch.Tensor       # [rows, D] storage dtype
    w: torch.Tensor        # [D] f32
    b: torch.Tensor        # [D] f32
    ref: dict              # y, mean, rstd, dx (LN'(dy) alone), dgamma, dbeta, dsum (column sums of dx): float64
    torch_f32: dict        # the same names, evaluated in torch float32 (as float64 tensors)
    _err: dict = field(default_factory=dict)

    def stats_f32(self):
        """mean, rstd of the float64 reference rounded to f32: what the backward tests feed the kernel, so that
        an error of the forward kernel cannot cancel one of the backward."""
        return self.ref["mean"].float(), self.ref["rstd"].float()


@functools.lru_cache(maxsize=None)
def ln_case(kind, rows, D, xdt=torch.float32, dyt=torch.float32, eps=1e-6, seed=71):
    g = _gen(seed + 1000 * LN_KINDS.index(kind) + rows + 7 * D)
    x = ln_input(kind, rows, D, g).to(xdt)
    w = (1 + _randn(g, D) * 0.2).float()
    b = (_randn(g, D) * 0.1).float()
    dy = _randn(g, rows, D).to(dyt)
    ref, f32 = {}, {}
    # float64, backward by autograd
    xd = x.double().requires_grad_(True)
    wd, bd = w.double().requires_grad_(True), b.double().requires_grad_(True)
    y, mean, rstd = ln_fwd(xd, wd, bd, eps)
    y.backward(dy.double())
    ref.update(y=y.detach(), mean=mean.detach(), rstd=rstd.detach(), dx=xd.grad, dgamma=wd.grad, dbeta=bd.grad,
               dsum=xd.grad.sum(0))
    # torch float32: the forward from x, the backward from the reference's statistics rounded to f32
    yf, mf, rf = ln_fwd(x.float(), w, b, eps)
    dxf, dgf, dbf = ln_bwd(x.float(), dy.float(), w, ref["mean"].float(), ref["rstd"].float())
    f32.update(y=yf, mean=mf, rstd=rf, dx=dxf, dgamma=dgf, dbeta=dbf, dsum=dxf.sum(0))
    return LnCase(kind, rows, D, eps, x, dy, w, b, ref, {k: v.double() for k, v in f32.items()})


@dataclass
class AddLnCase(_Bounded):
    hard = LN_HARD
    kind: str
    rows: int
    D: int
    eps: float
    x: torch.Tensor        # [rows, D] f32, the residual stream
    r: torch.Tensor        # [rows, D] f32 or bf16, the branch output
    s: torch.Tensor        # x + r as one f32 add: what xs must hold bit for bit
    w: torch.Tensor
    b: torch.Tensor
    ref: dict              # y, mean, rstd of LayerNorm(s): float64
    torch_f32: dict
    _err: dict = field(default_factory=dict)


@functools.lru_cache(maxsize=None)
def add_ln_case(kind, rows, D, rdt=torch.bfloat16, eps=1e-6, seed=79):
    """x of ``kind`` plus a branch output r of the kind's own spread (randn; randn * 1e-3 on ``tiny``)."""
    g = _gen(seed + 1000 * LN_KINDS.index(kind) + rows + 7 * D)
    x = ln_input(kind, rows, D, g).float()
    r = (_randn(g, rows, D) * (1e-3 if kind == "tiny" else 1.0)).to(rdt)
    w = (1 + _randn(g, D) * 0.2).float()
    b = (_randn(g, D) * 0.1).float()
    s = x + r.float()
    names = ("y", "mean", "rstd")
    ref = dict(zip(names, ln_fwd(s.double(), w.double(), b.double(), eps)))
    f32 = {k: v.double() for k, v in zip(names, ln_fwd(s, w, b, eps))}
    return AddLnCase(kind, rows, D, eps, x, r, s, w, b, ref, f32)


def spread_rows(compact, every, rows):
    """[ceil(rows / every), D] -> [rows, D], zero but for rows 0, every, 2 * every, ... (the compact residual
    gradient of vit_layer_norm_bwd_cls as the dense one it stands for)."""
    out = torch.zeros(rows, compact.shape[1], dtype=compact.dtype)
    out[::every] = compact[:(rows + every - 1) // every]
    return out


def compact_rows(dx, np_):
    """Drop row 0 of every (np_ + 1)-row image: the compact_np copy of the LayerNorm backward.  A ragged last
    image keeps the rows it has."""
    keep = torch.arange(dx.shape[0]) % (np_ + 1) != 0
    return dx[keep]


# ---------------------------------------------------------------------------- cross-entropy

def ce_fwd(logits, target):
    """(mean loss, row_lse) in the dtype of logits, with the max subtracted as every stable form does."""
    m = logits.amax(-1, keepdim=True)
    lse = (m + (logits - m).exp().sum(-1, keepdim=True).log()).squeeze(-1)
    return (lse - logits.gather(1, target[:, None]).squeeze(1)).mean(), lse


@dataclass
class CeCase(_Bounded):
    hard = CE_HARD
    kind: str
    B: int
    C: int
    logits: torch.Tensor   # [B, C] f32
    target: torch.Tensor   # [B] int64
    ref: dict              # loss, lse, d (dlogits for grad_loss = 1): float64
    torch_f32: dict
    _err: dict = field(default_factory=dict)


@functools.lru_cache(maxsize=None)
def ce_case(kind, B, C, seed=83):
    g = _gen(seed + 1000 * CE_KINDS.index(kind) + 31 * B + C)
    x = _randn(g, B, C) * (30 if kind == "wide" else 3)
    if kind == "spike":
        x[0] = -80 + _randn(g, C) * 0.5
        x[0, C // 2] = 80
    elif kind == "equal":
        x[0] = 1.75
    elif kind == "low":
        x[0] = -90
    elif kind not in ("base", "wide"):
        raise ValueError(f"unknown cross-entropy kind {kind!r}")
    target = torch.randint(0, C, (B,), generator=g)
    target[-1] = C - 1
    if B > 1:
        target[0] = 0
    logits = x.float()
    out = {}
    for dt in (torch.float64, torch.float32):
        l = logits.to(dt).clone().requires_grad_(True)
        loss, lse = ce_fwd(l, target)
        loss.backward()
        out[dt] = dict(loss=loss.detach().double().reshape(1), lse=lse.detach().double(), d=l.grad.double())
    return CeCase(kind, B, C, logits, target, out[torch.float64], out[torch.float32])


# ---------------------------------------------------------------------------- SGD, MSE, rownorm, cast, pos_grad

def sgd_steps(p, grads, lr, momentum, wd):
    """torch.optim.SGD (dampening 0, nesterov off) over a list of gradients, in the dtype of p: the parameter
    after every step."""
    buf, out = None, []
    for gr in grads:
        d = gr.to(p.dtype) + wd * p
        buf = d.clone() if buf is None else momentum * buf + d
        p = p - lr * buf
        out.append(p)
    return out


def sgd_inputs(n, steps=3, seed=97):
    g = _gen(seed + n)
    return torch.randn(n, generator=g), [torch.randn(n, generator=g) for _ in range(steps)]


def mse(p, t):
    """(loss, dloss/dp for grad_loss = 1) of nn.MSELoss() in the dtype of p."""
    d = p - t
    return (d * d).mean().reshape(1), 2 * d / d.numel()


def mse_inputs(n, seed=101):
    g = _gen(seed + n)
    return torch.randn(n, generator=g), torch.randn(n, generator=g)


def rownorm_inputs(n, D, scale, seed=103):
    g = _gen(seed + 17 * n + D)
    return (torch.randn(n, D, generator=g, dtype=torch.float64) * scale).float(), torch.randn(n, D, generator=g)


def rownorm(x, dy, log_scale):
    """y = exp(log_scale) * x / |x|, rnorm = 1 / |x| and dx by autograd, in the dtype of x."""
    x = x.clone().requires_grad_(True)
    rn = 1 / x.norm(dim=1, keepdim=True)
    y = x * rn * (torch.tensor(log_scale, dtype=x.dtype).exp() if log_scale is not None else 1.0)
    y.backward(dy.to(x.dtype))
    return y.detach(), rn.detach().squeeze(1), x.grad


def rownorm_dx_scale(rn, dy, log_scale):
    """[rows]: exp(log_scale) / |x| * max |dy_row|, the size of a row of dx before the projection takes the
    component along x out (at D = 1 it takes everything: dx is identically zero)."""
    k = torch.tensor(log_scale, dtype=torch.float64).exp() if log_scale is not None else 1.0
    return k * rn.double() * dy.double().abs().amax(1)


def _f32_bits(*words):
    return torch.tensor([w - (1 << 32) if w >= (1 << 31) else w for w in words], dtype=torch.int32).view(torch.float32)


CAST_SPECIALS = _f32_bits(
    0x3F808000,  # 1 + 2^-8: a tie, rounds down to the even 0x3F80
    0x3F818000,  # a tie above an odd mantissa: rounds up to the even 0x3F82
    0xBF808000, 0xBF818000,  # the same ties, negative
    0x3F808001, 0x3F817FFF,  # just past / just short of a tie
    0x00000000, 0x80000000,  # +0, -0
    0x00000001, 0x807FFFFF, 0x00008000, 0x00018000,  # denormals, two of them ties
    0x7F7F0000,  # the largest finite bf16
    0x7F7F8000, 0x7F7FFFFF, 0xFF7FFFFF,  # finite f32 that round to +-inf
    0x7F800000, 0xFF800000,  # +-inf
    0x7FC00000, 0x7F800001, 0xFFC12345, 0x7FFFFFFF,  # NaNs: quiet, signalling with a low payload, negative, all ones
)


def cast_input(n, seed=107):
    """f32 [n]: the special values first (as many as fit), randn * 3 spread over many exponents after them."""
    g = _gen(seed + n)
    x = torch.randn(n, generator=g) * 3 * torch.exp2(torch.randint(-20, 20, (n,), generator=g).float())
    k = min(n, CAST_SPECIALS.numel())
    x[:k] = CAST_SPECIALS[:k]
    return x


def pos_grad_inputs(B, S, D, seed=109):
    return torch.randn(B, S, D, generator=_gen(seed + 1000 * B + 10 * S + D))
