"""Cases for the GEMM family (csrc/gemm.hip, gemm_g4.hip, gemm_w4.inc, gemm_f32.inc) whose results are exact
(test infrastructure only: imported by tests/).

Every operand is chosen so that each value a kernel forms is exactly representable where the kernel holds it.
The result then does not depend on tile shape, k order, split count or reduction tree, and one float64
reference serves every dispatch path bit for bit.

  operands      small integers (``int``: p in {-2..2}, q in {-1, 0, 1}; reductions past 512 thin q out to one
                non-zero in four) or quarters of them (``quarter``: p in {-2..2} / 4).  Products and partial sums
                are multiples of 1/4 below 2^22: f32 accumulation is exact on MFMA and FMA alike.
  bf16 outputs  |acc + bias| <= 256 with integer bias (integers up to 256 are bf16 values), or for the
                activation pairs quarter-step bias and |pre| < 64 (multiples of 1/4 below 64 are bf16 values),
                so that pre = bf16(acc + bias) is exact.  ``quarter`` spreads pre over about [-8, 8]: both
                tails and the middle of GELU.
  GELU' dgrad   aux holds multiples of 1/16 in [0, 1.25]; acc * aux is exact in f32 and the stored value is the
                single rounding bf16(acc * aux).  Stored values and unrounded products are all multiples of
                1/16 below 2^9, so their f32 column sums over a few hundred rows are exact in any order -- and
                the two sums differ, which is how a test tells "column sums of dX as stored" from "column sums
                of the f32 products".
  residual, patch, accumulate   dyadic values (multiples of 1/8), exact.

Activation values (GELU, GELU', QuickGELU and its derivative) cannot be exact.  They are held per element
against float64 on the exact pre:

    |got - ref| <= eps * |ref| + 2e-6 * max(1, |pre|)      eps = 2^-8 (bf16 out), 2^-23 (f32 out)

The first term is one rounding to the output type.  The second comes from the code, not from a measurement of
it: erf_fast is Abramowitz-Stegun 7.1.26 with |error| <= 1.5e-7, v_rcp and v_exp add about an ulp each (1.2e-7
at 1), the cdf error is multiplied by |pre| in act = pre * cdf, and the whole carries a fivefold margin.
tests/test_gemm_cases_host.py asserts that an f32 restatement of gelu_fast_both / quick_gelu_both and torch's
own f32 erf GELU stay inside the bound on every case listed here.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import torch

F32, BF = torch.float32, torch.bfloat16
RC, CR = 0, 1

# ---------------------------------------------------------------------------- the activation bound (the one tolerance)
ACT_ABS = 2e-6


def act_eps(out_dtype):
    return 2.0 ** -8 if out_dtype == BF else 2.0 ** -23


def act_bound(ref, pre, out_dtype):
    """Per-element bound on |got - ref| (float64 tensors in, float64 out)."""
    return act_eps(out_dtype) * ref.abs() + ACT_ABS * pre.abs().clamp_min(1.0)


def act_fraction(got, ref, pre, out_dtype):
    """The worst |got - ref| / bound over the elements: <= 1 passes.  A non-finite ``got`` gives inf."""
    got, ref, pre = got.detach().double().cpu(), ref.double().cpu(), pre.double().cpu()
    if not bool(torch.isfinite(got).all()):
        return math.inf
    return ((got - ref).abs() / act_bound(ref, pre, out_dtype)).max().item()


_RSQRT2, _RSQRT2PI = 0.70710678118654752, 0.39894228040143268


def gelu_both(pre):
    """(gelu_erf(pre), gelu_erf'(pre)) in the dtype of pre (float64 for the reference)."""
    cdf = 0.5 * (1.0 + torch.erf(pre * _RSQRT2))
    return pre * cdf, cdf + pre * _RSQRT2PI * torch.exp(-0.5 * pre * pre)


def qgelu_both(pre):
    """QuickGELU x * sigmoid(1.702 x) and its derivative, in the dtype of pre."""
    s = torch.sigmoid(1.702 * pre)
    return pre * s, s + 1.702 * pre * s * (1.0 - s)


def gelu_fast_both_f32(pre):
    """csrc/common.hpp's gelu_fast_both restated in torch float32 (fused multiply-adds as two roundings: the
    restatement is a yardstick of the bound, not a model of the bits)."""
    x = pre.float()
    z = x * _RSQRT2
    az = z.abs()
    t = 1.0 / (0.3275911 * az + 1.0)
    p = 1.061405429 * t - 1.453152027
    p = p * t + 1.421413741
    p = p * t - 0.284496736
    p = p * t + 0.254829592
    e = torch.exp(-az * az)
    cdf = 0.5 + 0.5 * torch.copysign(1.0 - p * t * e, z)
    return x * cdf, (x * _RSQRT2PI) * e + cdf


def qgelu_both_f32(pre):
    x = pre.float()
    s = 1.0 / (1.0 + torch.exp(-1.702 * x))
    return x * s, s + 1.702 * x * s * (1.0 - s)


ACTS = {"gelu": (gelu_both, gelu_fast_both_f32), "qgelu": (qgelu_both, qgelu_both_f32)}

# ---------------------------------------------------------------------------- builders


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


@dataclass
class MmCase:
    """C [M, N] = p [M, R] q [N, R]^T (+ bias [N]).  The forward reads X = p, W = q; the input gradient reads
    dY = p and W = ``qT`` [R, N] (its Linear has R outputs and N inputs)."""
    kind: str
    M: int
    N: int
    R: int
    p: torch.Tensor      # [M, R] storage dtype
    q: torch.Tensor      # [N, R] storage dtype
    qT: torch.Tensor     # [R, N] storage dtype, contiguous
    bias: torch.Tensor   # [N] f32
    acc: torch.Tensor    # [M, N] float64, p q^T
    pre: torch.Tensor    # [M, N] float64, acc + bias


@functools.lru_cache(maxsize=None)
def mm_case(M, N, R, dtype=BF, kind="int", seed=211):
    g = _gen(seed + 100003 * M + 1009 * N + R + (7 if kind == "quarter" else 0))
    p = _ints(g, -2, 2, M, R)
    q = _ints(g, -1, 1, N, R)
    if R > 512:  # a long reduction: one weight in four keeps |acc| inside the bf16 integers
        q = q * (torch.rand(N, R, generator=g) < 0.25)
    if kind == "quarter":
        p = p / 4
        bias = _ints(g, -8, 8, N) / 4
    elif kind == "int":
        bias = _ints(g, -3, 3, N)
    else:
        raise ValueError(f"unknown kind {kind!r}")
    acc = p @ q.T
    return MmCase(kind, M, N, R, p.to(dtype), q.to(dtype), q.T.contiguous().to(dtype), bias.float(), acc, acc + bias)


def sixteenths(M, N, dtype=BF, seed=223):
    """A saved act' stand-in: multiples of 1/16 in [0, 1.25]."""
    return (_ints(_gen(seed + 31 * M + N), 0, 20, M, N) / 16).to(dtype)


def eighths(M, N, seed=227):
    """A residual stream / pos_embed stand-in: f32 multiples of 1/8 in [-4, 4]."""
    return (_ints(_gen(seed + 31 * M + N), -32, 32, M, N) / 8).float()


def act_bwd_ref(acc, aux, out_dtype):
    """The GELU' / QuickGELU' input gradient on exact data: (stored, column sums of the stored values, column
    sums of the unrounded f32 products), the sums in float64.  acc * aux is formed in f32 (exact), so a zero
    keeps the sign the kernel's multiply gives it."""
    prod = acc.float() * aux.float()
    assert torch.equal(prod.double(), acc * aux.double()), "acc * aux is not exact in f32"
    stored = prod.to(out_dtype)
    return stored, stored.double().sum(0), prod.double().sum(0)


@dataclass
class WgCase:
    """dW [N, K] = dy [M, N]^T x [M, K]."""
    M: int
    N: int
    K: int
    dy: torch.Tensor
    x: torch.Tensor
    dW: torch.Tensor     # float64


@functools.lru_cache(maxsize=None)
def wg_case(M, N, K, dtype=BF, seed=229):
    g = _gen(seed + 100003 * M + 1009 * N + K)
    dy, x = _ints(g, -2, 2, M, N), _ints(g, -1, 1, M, K)
    return WgCase(M, N, K, dy.to(dtype), x.to(dtype), dy.T @ x)


@dataclass
class PatchCase:
    """Token rows b * (np + 1) + 1 + p of x [B * (np + 1), D] = U [B * np, K] W [D, K]^T + bias + pos[1 + p]."""
    B: int
    np: int
    D: int
    K: int
    U: torch.Tensor
    W: torch.Tensor
    bias: torch.Tensor
    pos: torch.Tensor    # [np + 1, D] f32
    rows: torch.Tensor   # [B, np, D] float64


@functools.lru_cache(maxsize=None)
def patch_case(B, np_, D, K, dtype=BF, seed=233):
    g = _gen(seed + 1009 * D + K)
    U, W, bias = _ints(g, -2, 2, B * np_, K), _ints(g, -1, 1, D, K), _ints(g, -3, 3, D)
    pos = eighths(np_ + 1, D, seed)
    rows = (U @ W.T + bias).view(B, np_, D) + pos.double()[1:]
    return PatchCase(B, np_, D, K, U.to(dtype), W.to(dtype), bias.float(), pos, rows)


# ---------------------------------------------------------------------------- the host's dispatch rules, restated
# From include/vit_hip.h and the comments of csrc/gemm.hip's dispatcher; tests/test_gemm_cases_host.py holds every
# shape list below against them, so a shape edit cannot silently lose a branch.  Row strides are taken as
# 16-byte multiples and bases as aligned (the misaligned cases are listed apart).
CUS = 256              # MI355X; stream-K slots = 2 * CUS
F32_BM = F32_BN = 128
F32_BK = 32


def bf16_mfma_ok(pl, ql, M, N, R):
    """fast_ok: a CR operand's extent % 8, N % 4, R % 32."""
    return not ((pl == CR and M % 8) or (ql == CR and N % 8) or N % 4 or R % 32 or R <= 0)


def g4_takes(N, R, act_bwd=False):
    """g4_launch: R % 64, N % 8; the GELU' form needs two k-steps."""
    return R > 0 and R % 64 == 0 and N >= 8 and N % 8 == 0 and (not act_bwd or R >= 128)


def bf16_branch(cls, M, N, R, epi="store", csum=False, g4_gelu=1):
    """The kernel the default dispatch runs for a bf16 GEMM of class fwd / dgrad / wgrad: g4, v5, v1, v3, pp
    (the ping-pong weight-gradient kernel) or gen."""
    pl, ql = {"fwd": (RC, RC), "dgrad": (RC, CR), "wgrad": (CR, CR)}[cls]
    if not bf16_mfma_ok(pl, ql, M, N, R):
        return "gen"
    if cls == "wgrad":
        return "pp"
    if epi == "store" and not csum and g4_takes(N, R):
        return "g4"
    if epi == "pair" and cls == "fwd" and (g4_gelu & 2) and not csum and g4_takes(N, R):
        return "g4"
    if epi == "act_bwd" and cls == "dgrad" and (g4_gelu & 1) and g4_takes(N, R, True):
        return "g4"
    if cls == "fwd":
        return "v5" if R % 64 == 0 else "v1"
    return "v1" if (epi == "act_bwd" or (N <= 1024 and R <= 1024)) else "v3"


def f32_tiles(M, N):
    return -(-M // F32_BM) * -(-N // F32_BN)


def f32_branch(pl, ql, M, N, R, split=1, streamk_ws=False):
    """mfma, streamk or gen for an f32 GEMM: operands as fast_f32_ok asks, at least 64 tiles x splits, and
    stream-K when a registered workspace meets a ragged last round of 2 x CUs slots."""
    ok = not ((pl == CR and M % 4) or (ql == CR and N % 4) or N % 4 or R % F32_BK or R <= 0)
    if not ok or f32_tiles(M, N) * max(split, 1) < 64:
        return "gen"
    t, G = f32_tiles(M, N), 2 * CUS
    if streamk_ws and split <= 1 and t >= G and 1.0 - t / (-(-t // G) * G) > 0.03:
        return "streamk"
    return "mfma"


def gen_tile(M, N, nz=1):
    """The generic kernel's tile: 32 while 64-tiles x chunks stay under 256 workgroups."""
    return 32 if -(-N // 64) * -(-M // 64) * nz < 256 else 64


def wgrad_nslabs(M, split, bk=64):
    """vit_linear_wgrad_nslabs: chunks of ceil(R0 / split) rounded up to the k-step over the R0 = M - M % 32 rows."""
    R0 = M - M % 32
    if R0 <= 0:
        return 1
    chunk = -(-(-(-R0 // max(split, 1))) // bk) * bk
    return -(-R0 // chunk)


def dgrad_partial_floats(M, K):
    rows = -(-M // 64)
    return rows * K + (-(-rows // 64) * K if rows > 64 else 0)


# ---------------------------------------------------------------------------- the shapes the GPU tests run
# (M, N, R): output rows, output columns, reduction.
G4_SHAPES = (
    (1, 8, 64),        # g4: one row, the narrowest output it takes, one k-step
    (257, 136, 192),   # g4: a 1-row second row tile, a ragged 136-column tile, three k-steps (odd)
    (300, 264, 128),   # g4: a second column tile 8 columns wide
    (513, 256, 64),    # g4: three row tiles, a full column tile
)
G4_WALKS = ((1, 1, 0, 0), (0, 0, 1, 0))   # vit_gemm_g4_config: row bands; the stride walk on ONE workgroup
PAIR_SHAPES = ((257, 136, 192), (300, 264, 128))   # v5 by default (R % 64 == 0), g4 under vit_gemm_g4_gelu(3)
V1_FWD = (257, 136, 96)      # v1: R % 64 != 0 keeps g4 and the BK = 64 tiles out
ACT_BWD_SHAPES = ((70, 136, 128), (300, 136, 128))  # v1 under vit_gemm_g4_gelu(0), g4 under (3): 2 and 5 partial
                                                    # rows, the last one ragged; two k-steps, the least g4's form takes
N_MOD8_4 = (257, 132, 192)   # v5 forward, generic input gradient (a CR extent % 8): N % 8 == 4 passes N % 4 while
                             # g4, the permlane pairs and the bf16 image decline it
V3_DGRAD = (64, 136, 1088)  # v3: column sums keep g4 out, R > 1024 picks the 256-row tile
RESID_SHAPE = (257, 136, 192)  # v5, f32 out
GROUP_BANDS = (3, 3)         # vit_gemm_group on the 257-row shapes
MISALIGNED = (257, 136, 192)  # the g4 forward shape of the alignment cases: C, aux and bias off by 4 and by 1 element
WGRAD_NK = ((264, 136), (256, 256))
WGRAD_ROWS = ((32, 1), (96, 1), (160, 3), (50, 1), (19, 1))  # (M, split): one k-step half full; 64 + 32; three
                                                             # slabs; 32 MFMA rows + 18 generic; every row generic
WGRAD_F32 = ((64, 512, 512, 4), (64, 40, 24, 1), (70, 5, 7, 3))  # (M, N, K, split): mfma by the 64-tile rule;
                                                                 # generic; generic split with N * K % 4 != 0
F32_MFMA = (1000, 1004, 96)     # 8 x 8 = 64 tiles, ragged both ways
F32_STREAMK = (8300, 1024, 32)  # 65 x 8 = 520 tiles on 512 slots
GEN_SHAPES = ((37, 1000, 70), (3, 5, 7), (5, 9, 1))  # 32-tiles over a wide ragged output; one tile; K = 1
PATCH = ((2, 5, 136, 64), (2, 5, 136, 40))  # (B, np, D, K): mfma (v5), generic (K % 32 != 0)
SPLITK = (24, 40, 512)       # vit_gemm_splitk: 2 tiles, split = R / 128 = 4
COLSUM = (300, 136)
