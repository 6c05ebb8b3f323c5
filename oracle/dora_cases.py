"""Cases for the DoRA weight build and its backward (csrc/dora.hip) with float64 references and bounds of every
stage (test infrastructure only: imported by tests/).

    Dn = D + (B @ A) * s [* noise]      D, noise [in, out], B [in, r], A [r, out]
    nu[o] = ||Dn[:, o]||,  n = nu + 1e-8,  W[o][i] = Dn[i][o] * (m[o] / n[o])
    c[o] = gW[o] . DnT[o],  dm = c / n
    sdDnT = s * (m/n * gW - m c / (n^2 nu) * DnT) [* noise^T]       (second term 0 where nu == 0)
    dB = sdDnT^T-by-A,  dA = B^T-by-sdDnT^T

Stages.  The kernels store DnT, nu, W (forward), dm, sdDnT, dB, dA (backward).  The float64 reference of a stage
is evaluated on what the previous stage actually stored (f32 values, exact in float64), never on the previous
stage's reference, so an error shows in the stage that makes it and only there: ``stage_fractions``.

Bounds, per element, with u = 2^-24 the unit roundoff of f32 and U = 2u = 2^-23.  Each is the first-order bound of
the kernel's own arithmetic (every operation rounds once, relative error <= u; division and sqrtf are correctly
rounded in this build; a contracted fma only removes roundings), doubled, in the style of ``_within`` of
tests/test_gpu_lora.py:

  DnT   the rank product is r terms (r roundings on a term at most, in any order), then one multiply by s, one by
        the noise, and the add to D rounds the sum:  u ((r + 2) s |noise| (|B| @ |A|) + |Dn|).
        Bound  U ((r + 2) s |noise| (|B| @ |A|) + |Dn|)^T.
  nu    a sum of ``in`` squares, all positive, so a summation of depth d (the longest chain of additions a term
        goes through, plus one for the rounding of the square) is within d u of its value.  The kernels add
        16 squares in a thread, four threads as (a + b) + (c + d), ceil(tiles / 64) tiles in a lane and six levels
        of a wave tree: d = NU_DEPTH(in) = 16 + 2 + ceil(tiles / 64) + 6 + 1, whatever ``in``.  sqrtf halves
        the relative error and rounds once:  u (d / 2 + 1) nu.   Bound  U (d / 2 + 1) nu.
  W     n = nu + 1e-8, f = m / n, W = DnT * f: three roundings (1e-8f is 6e-9 off 1e-8: a tenth of one).
        Bound  3 U |W|.
  dm    c is a lane's chain of ceil(in / 64) fmas and the six-level tree: depth d = C_DEPTH(in) = ceil(in / 64)
        + 6 + 1, so |c - c64| <= d u (|gW| . |DnT|); n and the division round once each.
        Bound  U (d + 2) (|gW| . |DnT|) / n.
  sdDnT with a = m / n, b = m c / (n^2 nu):  a gW carries 3 roundings (n, /, *), b DnT 7 (m c, n, n n, (n n) nu,
        /, * and n again in the square) plus the error of c; the subtraction, s and the noise add one each to
        both:  u s |noise| (6 |a gW| + 10 |b DnT| + d m / (n^2 nu) (|gW| . |DnT|) |DnT|), d = C_DEPTH.
        Bound: that with U for u.  The last term is the error of c carried into the second term.
  dB, dA  a dot product of length R in any order, split or not:  Bound  (R + 2) U |.| @ |.|  (LoRA's), R = out
        for dB [in, r] and R = in for dA [r, out].

``torch_f32`` holds the same stages in torch float32 on the CPU (``f32_stages``), each fed by its own previous
stage, the two reductions summed in the kernels' order (the depth bounds of nu and dm hold for that order, not
for any order).  It is the yardstick of the bounds -- tests/test_dora_cases_host.py asserts that it is inside
every one -- and never an expected value.

End to end: ``ref`` is float64 autograd of ``oracle.vit_ref.dora_weight`` (with the noise factor) on the f32
inputs.  Columns of ``zero_col`` and ``tiny_col`` differ in scale by 1e8, so the comparison is per column of Dn:
per row of W, DnT and sdDnT, per element of nu and dm, per column of dA, each relative to that column's largest
reference magnitude (``e2e_fraction``); dB mixes all columns and is held through its stage bound only.  Bounds
are the project's: 1e-5 forward, 1e-4 gradients.  Where ``torch_f32`` itself is further away than that on an
output of a case (dm is c / n with c a sum that can cancel), the bound of that output is HARD_FACTOR = 4 times
torch_f32's own figure, and never below the project's (the rule of oracle/row_cases.py).

Kinds: ``base`` D with unit columns of a random weight, m its column norms times (1 + 0.1 randn), A and B 0.3
randn, s = 16 / r; ``init`` what DoRALayer.__init__ makes of a seeded nn.Linear; ``masked`` base with a
Dropout(p = 0.5) of ones as noise (0 and 2); ``zero_delta`` B = 0 (DnT is D^T bit for bit, dA exactly zero) and
``zero_delta_noise0`` the same with an all-zero noise; ``zero_col`` column 1 and the last column of D and A zero
(nu, W, dm exact zeros there, sdDnT = s m / 1e-8 gW, everything finite); ``tiny_col`` columns 2 and out - 2 of D
scaled to norm 3e-8 with A zero there (1e-8 is a quarter of n); ``index`` the exact kind: B = 0, D[:, o] = 2^a at
one row pi(o), m = k in 1..7, A and gW small integers, s = 2, so that every stored value is exact in f32 and
``index_expected`` gives closed forms to compare bit for bit.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass, field

import torch

from oracle import vit_ref as R

U = 2.0 ** -23
EPS = 1e-8
FWD, GRAD = 1e-5, 1e-4   # the project's bounds (tests/test_gpu_kernels.py)
HARD_FACTOR = 4.0

# (in, out, r): each the smallest that hits its edge (tests/test_dora_cases_host.py states which)
SHAPES = ((1, 1, 1), (3, 5, 2), (63, 65, 8), (65, 63, 1), (64, 64, 64), (96, 80, 8), (130, 257, 33), (257, 130, 5),
          (256, 320, 8), (260, 333, 5), (768, 768, 32), (1024, 1024, 32))
KIND_SHAPES = ((96, 80, 8), (130, 257, 33))
SPLIT_SHAPES = ((256, 320, 8), (260, 333, 5))
KINDS = ("base", "init", "masked", "zero_delta", "zero_delta_noise0", "zero_col", "tiny_col", "index")
STAGES = ("DnT", "nu", "W", "dm", "sdDnT", "dB", "dA")
E2E = {"W": FWD, "DnT": FWD, "nu": FWD, "dm": GRAD, "sdDnT": GRAD, "dA": GRAD}
TINY_NORM = 3e-8


def cases():
    """Every (in, out, r, kind) the GPU test runs stage by stage."""
    out = [(i, o, r, "base") for i, o, r in SHAPES]
    out += [(i, o, r, k) for i, o, r in KIND_SHAPES for k in KINDS[1:]]
    out += [(i, o, r, "index") for i, o, r in SPLIT_SHAPES]
    return out


def nu_depth(fin):
    return 16 + 2 + -(-((fin + 63) // 64) // 64) + 6 + 1


def c_depth(fin):
    return (fin + 63) // 64 + 6 + 1


def zero_cols(fout):
    return sorted({1 % fout, fout - 1})


def tiny_cols(fout):
    return sorted({2 % fout, (fout - 2) % fout})


def index_row(o, fin):
    """pi(o): the one non-zero row of column o of the ``index`` kind."""
    return (5 * o + 2) % fin


# ---------------------------------------------------------------------------- float64 stage references and bounds
# every function takes float64 tensors (the f32 values a kernel stored, widened) and returns (reference, bound)

def _nz(noise, like):
    return torch.ones_like(like) if noise is None else noise


def ref_DnT(A, Bm, D, s, noise):
    prod, absprod = Bm @ A, Bm.abs() @ A.abs()
    nz = _nz(noise, D)
    Dn = D + prod * s * nz
    return Dn.T.contiguous(), (U * ((A.shape[0] + 2) * s * nz.abs() * absprod + Dn.abs())).T.contiguous()


def ref_nu(DnT):
    nu = DnT.pow(2).sum(1).sqrt()
    return nu, U * (nu_depth(DnT.shape[1]) / 2 + 1) * nu


def ref_W(DnT, nu, m):
    W = DnT * (m / (nu + EPS))[:, None]
    return W, 3 * U * W.abs()


def ref_dm(gW, DnT, nu):
    n = nu + EPS
    return (gW * DnT).sum(1) / n, U * (c_depth(DnT.shape[1]) + 2) * (gW.abs() * DnT.abs()).sum(1) / n


def ref_sdDnT(gW, DnT, nu, m, s, noise):
    n = nu + EPS
    c, cabs = (gW * DnT).sum(1), (gW.abs() * DnT.abs()).sum(1)
    a = m / n
    k = torch.where(nu > 0, m / (n * n * nu.clamp_min(1e-300)), torch.zeros_like(nu))   # b = k c; 0 on a zero column
    nzT = _nz(None if noise is None else noise.T, DnT)
    t1, t2 = a[:, None] * gW, (k * c)[:, None] * DnT
    ref = s * (t1 - t2) * nzT
    bound = U * s * nzT.abs() * (6 * t1.abs() + 10 * t2.abs() + c_depth(DnT.shape[1]) * (k.abs() * cabs)[:, None] * DnT.abs())
    return ref, bound


def ref_dB(sdDnT, A):
    return sdDnT.T @ A.T, (sdDnT.shape[0] + 2) * U * (sdDnT.abs().T @ A.abs().T)


def ref_dA(sdDnT, Bm):
    return Bm.T @ sdDnT.T, (sdDnT.shape[1] + 2) * U * (Bm.abs().T @ sdDnT.abs().T)


def fraction(got, ref, bound):
    """The worst |got - ref| / bound over the elements: <= 1 passes.  Zero error on a zero bound is 0, any other
    error on it, and a non-finite ``got``, is inf."""
    got = got.detach().double().cpu().reshape(ref.shape)
    if not bool(torch.isfinite(got).all()):
        return math.inf
    err = (got - ref).abs()
    f = torch.where(err == 0, torch.zeros_like(err), err / bound)      # x / 0 = inf in IEEE division
    return float(f.max()) if f.numel() else 0.0


def stage_fractions(case, got):
    """{stage: worst err / bound} of the stored values ``got`` (DnT, nu, W, dm, sdDnT, dB, dA; any subset that
    holds what its stages read), each stage against float64 of the values ``got`` holds for the stage before."""
    d = lambda t: None if t is None else t.detach().double().cpu()
    m, A, Bm, D, gW, nz, s = d(case.m), d(case.A), d(case.B), d(case.D), d(case.gW), d(case.noise), case.s
    g = {k: d(v) for k, v in got.items()}
    fin, fout = case.fin, case.fout
    out = {}
    if "DnT" in g:
        g["DnT"] = g["DnT"].reshape(fout, fin)
        out["DnT"] = fraction(g["DnT"], *ref_DnT(A, Bm, D, s, nz))
    if "nu" in g:
        out["nu"] = fraction(g["nu"], *ref_nu(g["DnT"]))
    if "W" in g:
        out["W"] = fraction(g["W"], *ref_W(g["DnT"], g["nu"], m))
    if "dm" in g:
        out["dm"] = fraction(g["dm"], *ref_dm(gW, g["DnT"], g["nu"]))
    if "sdDnT" in g:
        g["sdDnT"] = g["sdDnT"].reshape(fout, fin)
        out["sdDnT"] = fraction(g["sdDnT"], *ref_sdDnT(gW, g["DnT"], g["nu"], m, s, nz))
    if "dB" in g:
        out["dB"] = fraction(g["dB"], *ref_dB(g["sdDnT"], A))
    if "dA" in g:
        out["dA"] = fraction(g["dA"], *ref_dA(g["sdDnT"], Bm))
    return out


# ---------------------------------------------------------------------------- the f32 restatement (the yardstick)

def _wave_tree(v):
    """[..., 64] -> [...]: the xor butterfly of wave_sum (v[l] += v[l ^ 32], 16, ... 1), of which every lane
    holds the same value; adding the upper half onto the lower at each level forms that value."""
    for h in (32, 16, 8, 4, 2, 1):
        v = v[..., :h] + v[..., h:2 * h]
    return v[..., 0]


def _lane_strided(x, fma_with=None):
    """[rows, L] -> [rows]: lane l adds x[l], x[l + 64], ... in that order from zero, then the wave tree."""
    rows, L = x.shape
    k = (L + 63) // 64
    pad = lambda t: torch.nn.functional.pad(t, (0, k * 64 - L)).view(rows, k, 64)
    x = pad(x)
    y = None if fma_with is None else pad(fma_with)
    acc = torch.zeros(rows, 64, dtype=x.dtype)
    for j in range(k):
        acc = acc + (x[:, j] if y is None else x[:, j] * y[:, j])
    return _wave_tree(acc)


def f32_colsq(DnT):
    """Column sums of squares [out] of DnT [out, in] f32 in the order of dora_tile_kernel / dora_finish_kernel."""
    fout, fin = DnT.shape
    nt = (fin + 63) // 64
    x = torch.nn.functional.pad(DnT, (0, nt * 64 - fin)).view(fout, nt, 4, 16)
    sq = torch.zeros(fout, nt, 4, dtype=DnT.dtype)
    for u in range(16):
        sq = sq + x[..., u] * x[..., u]
    tile = (sq[..., 0] + sq[..., 1]) + (sq[..., 2] + sq[..., 3])
    return _lane_strided(tile)


PLANTS = ("no_eps", "n_for_nu", "no_guard", "skip_rank_term", "norm_skips_last_row", "noise_as_out_in",
          "bwd_unmasked", "W_untransposed")


def f32_stages(case, plant=None):
    """Every stage in torch float32 on the CPU, each from the values the previous one stored; ``plant`` names one
    deliberate error (PLANTS) for the sharpness test."""
    assert plant is None or plant in PLANTS
    f = torch.float32
    m, A, Bm, D, gW, nz = case.m, case.A, case.B, case.D, case.gW, case.noise
    s = torch.tensor(case.s, dtype=f)
    eps = torch.tensor(0.0 if plant == "no_eps" else EPS, dtype=f)
    fin, fout = case.fin, case.fout
    prod = (Bm[:, :-1] @ A[:-1]) if plant == "skip_rank_term" else Bm @ A
    delta = prod * s
    if nz is not None:
        delta = delta * (nz.flatten().view(fout, fin).T if plant == "noise_as_out_in" else nz)
    DnT = (D + delta).T.contiguous()
    sq_of = DnT.clone()
    if plant == "norm_skips_last_row":
        sq_of[:, fin - 1] = 0
    nu = f32_colsq(sq_of).sqrt()
    n = nu + eps
    W = DnT * (m / n)[:, None]
    if plant == "W_untransposed":
        W = W.T.contiguous().view(fout, fin)
    c = _lane_strided(gW, DnT)
    dm = c / n
    a = m / n
    den = n * n * (n if plant == "n_for_nu" else nu)
    b = m * c / den
    if plant != "no_guard":
        b = torch.where(nu > 0, b, torch.zeros_like(b))
    sd = s * (a[:, None] * gW - b[:, None] * DnT)
    if nz is not None and plant != "bwd_unmasked":
        sd = sd * nz.T
    return dict(DnT=DnT, nu=nu, W=W, dm=dm, sdDnT=sd, dB=sd.T @ A.T, dA=Bm.T @ sd.T)


# ---------------------------------------------------------------------------- end to end

def e2e_ref(m, A, Bm, D, s, noise, gW):
    """float64 autograd of oracle.vit_ref.dora_weight (its formula with the noise factor when there is one) on
    the f32 inputs: W, DnT, nu, dm, dA, dB and sdDnT = s * dL/dDn^T [* noise^T]."""
    m, A, Bm = (t.double().clone().requires_grad_(True) for t in (m, A, Bm))
    D, gW = D.double(), gW.double()
    if noise is None:
        W = R.dora_weight(m, A, Bm, D, s)
        Dn = D + (Bm @ A) * s
        nzT = 1.0
    else:
        Dn = D + (Bm @ A) * s * noise.double()
        W = ((Dn / (torch.norm(Dn, dim=0, keepdim=True) + EPS)) * m).T
        nzT = noise.double().T
    W.backward(gW)
    # dL/dDn by a second pass with Dn as the leaf
    Dl = Dn.detach().clone().requires_grad_(True)
    ((Dl / (torch.norm(Dl, dim=0, keepdim=True) + EPS)) * m.detach()).T.backward(gW)
    return dict(W=W.detach(), DnT=Dn.detach().T.contiguous(), nu=torch.norm(Dn.detach(), dim=0), dm=m.grad,
                dA=A.grad, dB=Bm.grad, sdDnT=(s * Dl.grad.T * nzT).contiguous())


def col_rel(name, got, ref):
    """[out]: per column of Dn, max |got - ref| / max |ref| (0 / 0 = 0, anything else over 0 = inf)."""
    got = got.detach().double().cpu().reshape(ref.shape)
    if not bool(torch.isfinite(got).all()):
        return torch.full((1,), math.inf, dtype=torch.float64)
    err, mag = (got - ref).abs(), ref.abs()
    if name in ("W", "DnT", "sdDnT"):
        err, mag = err.amax(1), mag.amax(1)
    elif name == "dA":
        err, mag = err.amax(0), mag.amax(0)
    return torch.where(err == 0, torch.zeros_like(err), err / mag.clamp_min(1e-300))


@dataclass
class DoraCase:
    kind: str
    fin: int
    fout: int
    r: int
    s: float
    m: torch.Tensor          # [out] f32
    A: torch.Tensor          # [r, out] f32
    B: torch.Tensor          # [in, r] f32
    D: torch.Tensor          # [in, out] f32
    noise: torch.Tensor      # [in, out] f32 or None
    gW: torch.Tensor         # [out, in] f32
    ref: dict                # end to end, float64: W, DnT, nu, dm, dA, dB, sdDnT
    torch_f32: dict          # f32_stages(case): the yardstick
    _e2e: dict = field(default_factory=dict)

    def e2e_bound(self, name):
        """The project's bound of output ``name``, or HARD_FACTOR times torch_f32's own worst column if larger."""
        if name not in self._e2e:
            own = float(col_rel(name, self.torch_f32[name], self.ref[name]).max())
            self._e2e[name] = max(E2E[name], HARD_FACTOR * own)
        return self._e2e[name]

    def e2e_fraction(self, name, got):
        """The worst column's relative error of ``got`` over e2e_bound(name): <= 1 passes."""
        return float(col_rel(name, got, self.ref[name]).max()) / self.e2e_bound(name)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _base_inputs(fin, fout, r, g):
    Wt = torch.randn(fin, fout, generator=g, dtype=torch.float64)
    S = Wt.norm(dim=0)
    D = (Wt / S).float()
    m = (S * (1 + 0.1 * torch.randn(fout, generator=g, dtype=torch.float64))).float()
    A = (torch.randn(r, fout, generator=g) * 0.3)
    Bm = (torch.randn(fin, r, generator=g) * 0.3)
    gW = torch.randn(fout, fin, generator=g)
    return m, A, Bm, D, gW, 16.0 / r


def init_inputs(fin, fout, r, seed):
    """(m, A, B, D, scaling) as DoRALayer.__init__(nn.Linear(in, out), r, dora_alpha=16) makes them under
    torch.manual_seed(seed), the module's RNG order; the global generator is put back."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        lin = torch.nn.Linear(fin, fout)
        Wt = lin.weight.data.clone().T
        S = torch.norm(Wt, dim=0)
        A, Bm = torch.zeros(r, fout), torch.zeros(fin, r)
        torch.nn.init.kaiming_uniform_(A, a=math.sqrt(5))
        torch.nn.init.kaiming_uniform_(Bm, a=math.sqrt(5))
    return S, A, Bm, Wt / S, 16 / r


def index_inputs(fin, fout, r, g):
    o = torch.arange(fout)
    D = torch.zeros(fin, fout)
    D[index_row(o, fin), o] = torch.exp2((o % 3).float())
    m = (1 + o % 7).float()
    A = torch.randint(-3, 4, (r, fout), generator=g).float()
    gW = torch.randint(-4, 5, (fout, fin), generator=g).float()
    return m, A, torch.zeros(fin, r), D, gW, 2.0


def index_expected(case):
    """The closed forms of the ``index`` kind (float64; every one an f32 value): what the kernels must store bit
    for bit, up to the sign of a zero."""
    fin, fout = case.fin, case.fout
    o = torch.arange(fout)
    pi = index_row(o, fin)
    k, p2 = case.m.double(), torch.exp2((o % 3).double())
    gW = case.gW.double()
    W = torch.zeros(fout, fin, dtype=torch.float64)
    W[o, pi] = k
    sd = case.s * (k / p2)[:, None] * gW
    sd[o, pi] = 0
    return dict(DnT=case.D.double().T.contiguous(), nu=p2, W=W, dm=gW[o, pi], sdDnT=sd,
                dB=sd.T @ case.A.double().T, dA=torch.zeros(case.r, fout, dtype=torch.float64))


@functools.lru_cache(maxsize=None)
def case(fin, fout, r, kind="base", seed=131):
    g = _gen(seed + 100003 * KINDS.index(kind) + 1009 * fin + 31 * fout + r)
    noise = None
    if kind == "init":
        m, A, Bm, D, s = init_inputs(fin, fout, r, seed + fin + fout + r)
        gW = torch.randn(fout, fin, generator=g)
    elif kind == "index":
        m, A, Bm, D, gW, s = index_inputs(fin, fout, r, g)
    else:
        m, A, Bm, D, gW, s = _base_inputs(fin, fout, r, g)
        if kind == "masked":
            with torch.random.fork_rng(devices=[]):
                torch.manual_seed(seed + fin * fout)
                noise = torch.nn.functional.dropout(torch.ones(fin, fout), 0.5, True)
        elif kind in ("zero_delta", "zero_delta_noise0"):
            Bm = torch.zeros_like(Bm)
            noise = torch.zeros(fin, fout) if kind == "zero_delta_noise0" else None
        elif kind == "zero_col":
            D[:, zero_cols(fout)] = 0
            A[:, zero_cols(fout)] = 0
        elif kind == "tiny_col":
            D[:, tiny_cols(fout)] *= TINY_NORM
            A[:, tiny_cols(fout)] = 0
        elif kind != "base":
            raise ValueError(f"unknown DoRA kind {kind!r}")
    c = DoraCase(kind, fin, fout, r, float(s), m, A, Bm, D, noise, gW, e2e_ref(m, A, Bm, D, float(s), noise, gW), {})
    c.torch_f32 = f32_stages(c)
    return c
