"""GPU: every attention kernel family against the float64 reference of oracle/attn_cases.py -- every resident
tile count NT = ceil(N / 16) in 1..18, the hard softmax inputs (peaked rows, a large common score offset, an
outlier in the last key, a running maximum that moves in every chunk or never, all-zero rows), operands that
are views, and scales other than 0.125.

Families: ``res-bf16-fused`` (attn_fwd_mfma + attn_bwd_fused, NT <= 14), ``res-bf16-two`` (attn_fwd_mfma +
attn_bwd_dq / attn_bwd_dkv), ``res-f32`` (attn_*_f32mfma), ``stream-bf16`` / ``stream-f32`` (past 288 tokens),
``generic-bf16`` / ``generic-f32`` (reached through a qkv row stride of 3D + 2) and ``cls`` (the class-token
forward).  B = H = 2 throughout: the batch and the head offsets are both non-zero.  The backward is fed the
reference's o (rounded to the dtype) and lse, so a forward error cannot leak into the gradient check.

Bounds, all against the float64 reference:
  * bf16: the project's (o 1.5e-2, lse 2e-3, dq / dk / dv / qkv-bias gradient 3e-2, each of the reference's
    largest magnitude), lse also 2e-2 absolute (what 2e-3 admits at lse ~ 10; on ``offset`` 2e-3 alone would
    admit 0.7), single rows of single (b, h) items 1.5e-2 for o and dv (not dq / dk: their rows are
    legitimately near zero on peaked inputs), single (b, h) items 3e-2 as test_sdpa_bwd_large_grid computes it.
    tests/test_attention_cases_host.py shows that the roundings a correct bf16 kernel cannot avoid stay at
    least 1.6x inside each of them on every kind.
  * f32: the project's (o, lse 1e-5; gradients 1e-4; rows and items likewise) or 4x the error that torch's own
    float32 CPU evaluation of the same formula makes on the same inputs in the same measure, whichever is
    larger: on ``offset`` (scores ~ 300, one f32 ulp of a score is 3e-5) torch itself is 3.5e-5 off in o, and
    no f32 kernel can hold 1e-5 there; the factor 4 covers another summation order and the hardware exp2 /
    log2, each of the size of torch's own error.

At N = 1 (NT = 1's first token count) the reference's dq and dk are identically zero; their error is then
measured against the largest magnitude of [dq | dk | dv] (``AC.rel_max``).

Every figure is printed as a ``FIG`` line (family, case, measure, error, bound, and for f32 the ratio to
torch's error) before it is asserted."""
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import attn_cases as AC  # noqa: E402
from vit_amd import _lib as L  # noqa: E402
from vit_amd import ops  # noqa: E402

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
B, H = 2, 2
D = H * 64
HARD = [k for k in AC.KINDS if k != "base"]
SENT = -12288.0  # exact in bf16


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    L.load()
    L.lib().vit_sdpa_long_config(-1)
    L.lib().vit_sdpa_bwd_variant(-1)


def _dt(dtype):
    return "bf16" if dtype == BF16 else "f32"


_CASES = {}


def _case(kind, N, dtype, causal=False, scale=0.125):
    """The case, its device operands (with the backward's o and lse from the reference) and, for f32, torch's
    float32 evaluation; computed once per key and left unchanged."""
    key = (kind, N, dtype, causal, scale)
    if key not in _CASES:
        c = AC.make_case(kind, B, H, N, dtype, causal=causal, scale=scale)
        d = SimpleNamespace(qkv=c.qkv.to(DEV), do=c.do.to(DEV), o_in=c.o.to(dtype).to(DEV),
                            lse_in=c.lse.float().to(DEV))
        _CASES[key] = (c, d, AC.torch_f32(c) if dtype == F32 else None)
    return _CASES[key]


def _label(c):
    return f"{c.kind} N={c.N} {_dt(c.dtype)}{' causal' if c.causal else ''} scale={c.scale}"


class _Report:
    """Prints one FIG line per figure and collects the ones past their bound."""

    def __init__(self, fam, c):
        self.head, self.bad = f"FIG {fam} | {_label(c)}", []

    def add(self, what, err, bound, torch_err=None):
        ratio = "" if torch_err is None else f" | x torch-f32 {err / max(torch_err, 1e-30):.2f} ({torch_err:.2e})"
        print(f"{self.head} | {what} {err:.3e} (bound {bound:.1e}){ratio}")
        if not err <= bound:  # a NaN is past every bound
            self.bad.append(f"{what} {err:.3e} > {bound:.1e}")

    def done(self):
        assert not self.bad, f"{self.head}: " + "; ".join(self.bad)


def _bound(dtype, project, torch_err):
    return project if dtype == BF16 else max(project, 4 * torch_err)


def _check_fwd(rep, c, tf, o, lse):
    N, bf = c.N, c.dtype == BF16
    to, tl = (AC.BF16_O, AC.BF16_LSE) if bf else (AC.F32_O, AC.F32_LSE)
    for what, fn, got, ref, tref, tol in (
            ("o", AC.rel_max, o, c.o, tf and tf[0], to),
            ("o row", lambda a, b: AC.row_rel(a, b, B, H, N), o, c.o, tf and tf[0], AC.BF16_ROW if bf else to),
            ("lse", AC.rel_max, lse, c.lse, tf and tf[1], tl)):
        te = None if bf else fn(tref, ref)
        rep.add(what, fn(got, ref), _bound(c.dtype, tol, te or 0.0), te)
    if bf:
        rep.add("lse abs", AC.abs_max(lse, c.lse), AC.BF16_LSE_ABS)


def _check_bwd(rep, c, tf, dqkv, dbias):
    N, bf = c.N, c.dtype == BF16
    tg = AC.BF16_GRAD if bf else AC.F32_GRAD
    g = dqkv.detach().double().cpu()
    blk = lambda x, i: x[:, i * D:(i + 1) * D]
    for i, name in enumerate(("dq", "dk", "dv")):
        te = None if bf else AC.rel_max(blk(tf[2], i), blk(c.grads, i), c.grads)
        rep.add(name, AC.rel_max(blk(g, i), blk(c.grads, i), c.grads), _bound(c.dtype, tg, te or 0.0), te)
    te = None if bf else AC.row_rel(blk(tf[2], 2), blk(c.grads, 2), B, H, N)
    rep.add("dv row", AC.row_rel(blk(g, 2), blk(c.grads, 2), B, H, N),
            _bound(c.dtype, AC.BF16_ROW if bf else tg, te or 0.0), te)
    te = None if bf else AC.item_rel(tf[2], c.grads, B, H, N)
    rep.add("dqkv item", AC.item_rel(g, c.grads, B, H, N), _bound(c.dtype, tg, te or 0.0), te)
    te = None if bf else AC.rel_max(tf[3], c.colsum)
    rep.add("qkv bias grad", AC.rel_max(dbias, c.colsum), _bound(c.dtype, tg, te or 0.0), te)


def _fwd(c, d, qkv=None, o=None):
    return ops.sdpa_fwd(d.qkv if qkv is None else qkv, B, H, c.N, o=o, scale=c.scale, causal=c.causal)


def _bwd(c, d, qkv=None, o_in=None, do=None, dqkv=None, variant=-1, reduce_on=None):
    """The backward from the reference's o and lse, with dbias, under ``vit_sdpa_bwd_variant(variant)``."""
    dbias = torch.full((3 * D,), float("nan"), device=DEV)
    lib = L.lib()
    try:
        assert lib.vit_sdpa_bwd_variant(variant) == 0
        dqkv = ops.sdpa_bwd(d.qkv if qkv is None else qkv, d.o_in if o_in is None else o_in,
                            d.do if do is None else do, d.lse_in, B, H, c.N, dqkv=dqkv, scale=c.scale, dbias=dbias,
                            causal=c.causal, reduce_on=reduce_on)
    finally:
        lib.vit_sdpa_bwd_variant(-1)
    return dqkv, dbias


def _misaligned(x):
    """x as a view whose row stride is 2 elements wider: no vector width divides it, so the generic kernels run."""
    w = torch.full((x.shape[0], x.shape[1] + 2), SENT, dtype=x.dtype, device=x.device)
    v = w[:, :x.shape[1]]
    v.copy_(x)
    assert v.stride(0) % 4 == 2
    return v


def _counts():
    lib = L.lib()
    return lib.vit_sdpa_long_count(0), lib.vit_sdpa_long_f32_count(0)


# family -> (dtype, backward variant, generic, the streamed counters' advance over one forward + one backward)
FAMILIES = {
    "res-bf16-fused": (BF16, 1, False, (0, 0)),
    "res-bf16-two": (BF16, 2, False, (0, 0)),
    "res-f32": (F32, -1, False, (0, 0)),
    "stream-bf16": (BF16, -1, False, (2, 0)),
    "stream-f32": (F32, -1, False, (0, 2)),
    "generic-bf16": (BF16, -1, True, (0, 0)),
    "generic-f32": (F32, -1, True, (0, 0)),
}


def _run_family(fam, kind, N, causal=False, scale=0.125, fwd=True, bwd=True):
    """One forward and one backward (unless ``fwd`` / ``bwd`` is False) of the family on the case, every figure
    held to its bound, and the streamed counters to what the family implies."""
    dtype, variant, generic, adv = FAMILIES[fam]
    assert (N > 288) == fam.startswith("stream") or generic
    assert fam != "res-bf16-fused" or N <= 224
    c, d, tf = _case(kind, N, dtype, causal, scale)
    qkv = _misaligned(d.qkv) if generic else None
    rep = _Report(fam, c)
    c0 = _counts()
    if fwd:
        o, lse = _fwd(c, d, qkv=qkv)
        _check_fwd(rep, c, tf, o, lse)
    if bwd:
        dqkv, dbias = _bwd(c, d, qkv=qkv, variant=variant)
        _check_bwd(rep, c, tf, dqkv, dbias)
    c1 = _counts()
    want = tuple(a // 2 * (fwd + bwd) for a in adv)
    assert (c1[0] - c0[0], c1[1] - c0[1]) == want, f"{fam}: streamed counters advanced by {c1} - {c0}"
    rep.done()


# ---------------------------------------------------------------------------- 1. every resident tile count

def _nt_cases():
    out = []
    for nt in range(1, 19):
        for N, causal in ((16 * nt - 15, False), (16 * nt, False), (16 * nt - 15, True)):
            for fam in ("res-bf16-fused", "res-bf16-two", "res-f32"):
                if fam == "res-bf16-fused" and nt > 14:
                    continue
                out.append(pytest.param(fam, N, causal, id=f"{fam}-NT{nt}-N{N}{'-causal' if causal else ''}"))
    return out


@pytest.mark.parametrize("fam,N,causal", _nt_cases())
def test_every_resident_tile_count(fam, N, causal):
    """NT = 1..18 at its first and last token count, and causal at the first: forward and backward with dbias.
    (The bf16 forward is one kernel for both backward forms; it runs with the two-kernel family.)"""
    _run_family(fam, "base", N, causal=causal, fwd=fam != "res-bf16-fused")


@pytest.mark.parametrize("N", [n for nt in range(1, 19) for n in (16 * nt - 15, 16 * nt)],
                         ids=lambda n: f"NT{(n + 15) // 16}-N{n}")
def test_cls_forward_every_tile_count(N):
    """sdpa_fwd_cls: rows 0..15 of each image bit for bit sdpa_fwd's (and within the bounds of the reference),
    every other row o = 0 and lse = +inf, whatever the buffers held."""
    c, d, _ = _case("base", N, BF16)
    lib = L.lib()
    o, lse = _fwd(c, d)
    n0 = lib.vit_sdpa_cls_count(0)
    oc, lc = ops.sdpa_fwd_cls(d.qkv, B, H, N, o=torch.full((B * N, D), 7.0, dtype=BF16, device=DEV), scale=c.scale,
                              lse=torch.full((B * H * N,), 7.0, device=DEV))
    torch.cuda.synchronize()
    assert lib.vit_sdpa_cls_count(0) - n0 == 1
    R = min(16, N)
    o3, oc3 = o.reshape(B, N, D), oc.reshape(B, N, D)
    l3, lc3 = lse.reshape(B * H, N), lc.reshape(B * H, N)
    assert torch.equal(oc3[:, :R], o3[:, :R]) and torch.equal(lc3[:, :R], l3[:, :R])
    assert (oc3[:, R:] == 0).all() and (lc3[:, R:] == float("inf")).all()
    rep = _Report("cls", c)
    rep.add("o", AC.rel_max(oc3[:, :R], c.o.reshape(B, N, D)[:, :R]), AC.BF16_O)
    rep.add("lse", AC.rel_max(lc3[:, :R], c.lse.reshape(B * H, N)[:, :R]), AC.BF16_LSE)
    rep.add("lse abs", AC.abs_max(lc3[:, :R], c.lse.reshape(B * H, N)[:, :R]), AC.BF16_LSE_ABS)
    rep.done()


def test_cls_forward_f32_runs_every_row():
    """Anything but resident bf16 runs sdpa_fwd on all rows and leaves the counter alone."""
    c, d, _ = _case("base", 33, F32)
    n0 = L.lib().vit_sdpa_cls_count(0)
    o, lse = _fwd(c, d)
    oc, lc = ops.sdpa_fwd_cls(d.qkv, B, H, 33, scale=c.scale)
    assert L.lib().vit_sdpa_cls_count(0) == n0
    assert torch.equal(o, oc) and torch.equal(lse, lc)


# ---------------------------------------------------------------------------- 2. hard inputs on every family

# 193 = 12 * 16 + 1 and 225 = 14 * 16 + 1: one key in the last tile; 321 = 5 * 64 + 1: five full chunks plus one
# key, and a ragged third query block; causal 77: only the last query sees ``outlier``'s key
HARD_SHAPES = [("res-bf16-fused", 193, False), ("res-bf16-two", 225, False), ("res-f32", 193, False),
               ("stream-bf16", 321, False), ("stream-f32", 321, False),
               ("generic-bf16", 50, False), ("generic-bf16", 321, False),
               ("generic-f32", 50, False), ("generic-f32", 321, False),
               ("res-bf16-fused", 77, True), ("res-bf16-two", 77, True), ("res-f32", 77, True)]


# A kind made milder (the issue's rule for a bound too tight for a kernel that is right): the f32 MFMA backward on
# ``offset`` at 193 / 321 tokens.  Measured with q, k += 6: dq 1.76e-4 (resident) and 1.43e-4 (streamed) of max|dq|,
# 5.4x and 4.8x torch-f32's error, past max(1e-4, 4 x torch); the generic f32 kernels on the same inputs 5.8e-5
# (1.9x).  The cause is the order in which the raw scores q.k ~ 2400 are summed, and a float64 restatement with
# only that sum in f32 reproduces each figure: 64 sequential FMAs (v_mfma_f32_16x16x4_f32, 16 in a chain) give dq
# 1.37e-4 / 1.26e-4, the generic kernels' 4 chains of 16 and a tree 4.7e-5 / 5.5e-5; every other f32 figure on
# ``offset``, the forward's included, holds.  sum_j dS_ij = 0 makes dq the one output that turns a score's
# rounding (one f32 ulp at 2400 is 2.4e-4, 3e-5 in the exponent) into an error 6 |dS| wide.  With q, k += 4
# the same kernels hold the bounds; the forward keeps ``offset`` as it is.
MILDER_BWD = {("res-f32", "offset", False), ("stream-f32", "offset", False)}


@pytest.mark.parametrize("kind", HARD)
@pytest.mark.parametrize("fam,N,causal", HARD_SHAPES,
                         ids=[f"{f}-N{n}{'-causal' if c else ''}" for f, n, c in HARD_SHAPES])
def test_hard_inputs(fam, N, causal, kind):
    if (fam, kind, causal) in MILDER_BWD:
        _run_family(fam, kind, N, bwd=False)
        _run_family(fam, AC.MILDER[kind], N)
    else:
        _run_family(fam, kind, N, causal=causal)


# ---------------------------------------------------------------------------- 4. views

def _view_operands(c, d):
    """qkv from column 8 of a [B*N, 3D + 16] buffer; o, do and dqkv in buffers 8 columns wider; sentinels around."""
    dtype, R = c.dtype, B * c.N
    w = SimpleNamespace(qkv=torch.full((R, 3 * D + 16), SENT, dtype=dtype, device=DEV),
                        o=torch.full((R, D + 8), SENT, dtype=dtype, device=DEV),
                        o_in=torch.full((R, D + 8), SENT, dtype=dtype, device=DEV),
                        do=torch.full((R, D + 8), SENT, dtype=dtype, device=DEV),
                        dqkv=torch.full((R, 3 * D + 8), SENT, dtype=dtype, device=DEV))
    v = SimpleNamespace(qkv=w.qkv[:, 8:8 + 3 * D], o=w.o[:, :D], o_in=w.o_in[:, :D], do=w.do[:, :D],
                        dqkv=w.dqkv[:, :3 * D])
    v.qkv.copy_(d.qkv)
    v.o_in.copy_(d.o_in)
    v.do.copy_(d.do)
    for t in vars(v).values():  # what the dispatch asks of an MFMA family
        assert t.stride(0) % 8 == 0 and t.data_ptr() % 16 == 0 and not t.is_contiguous()
    return w, v


def _sentinels_intact(w, c, d):
    assert (w.qkv[:, :8] == SENT).all() and (w.qkv[:, 8 + 3 * D:] == SENT).all()
    assert torch.equal(w.qkv[:, 8:8 + 3 * D], d.qkv)
    for name, width in (("o", D), ("o_in", D), ("do", D), ("dqkv", 3 * D)):
        assert (getattr(w, name)[:, width:] == SENT).all(), f"{name}: written outside the view"
    assert torch.equal(w.o_in[:, :D], d.o_in) and torch.equal(w.do[:, :D], d.do)


@pytest.mark.parametrize("fam,N", [("res-bf16-fused", 197), ("res-bf16-two", 197), ("res-f32", 197),
                                   ("stream-bf16", 321)], ids=lambda x: str(x))
def test_views_match_contiguous(fam, N):
    """Operands that are views give the contiguous call's bits and leave every element outside them alone.  That
    the MFMA kernels ran: past 288 tokens the streamed counter; resident bf16 takes the partial-only bias mode,
    which every other path below 289 tokens refuses; resident f32 has no counter -- its dispatch reads only the
    strides asserted in ``_view_operands``, and the generic kernels sum in another order."""
    dtype, variant, _, adv = FAMILIES[fam]
    c, d, _ = _case("base", N, dtype)
    c0 = _counts()
    o0, lse0 = _fwd(c, d)
    dq0, db0 = _bwd(c, d, variant=variant)
    w, v = _view_operands(c, d)
    o1, lse1 = _fwd(c, d, qkv=v.qkv, o=v.o)
    dq1, db1 = _bwd(c, d, qkv=v.qkv, o_in=v.o_in, do=v.do, dqkv=v.dqkv, variant=variant)
    torch.cuda.synchronize()
    c1 = _counts()
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (2 * adv[0], 2 * adv[1])
    assert o1.data_ptr() == w.o.data_ptr() and dq1.data_ptr() == w.dqkv.data_ptr()
    for a, b, name in ((o0, o1, "o"), (lse0, lse1, "lse"), (dq0, dq1, "dqkv"), (db0, db1, "dbias")):
        assert torch.equal(a, b), f"{name}: the call on views and the contiguous call differ"
    _sentinels_intact(w, c, d)
    if fam.startswith("res-bf16"):
        rb = ops.ColBatch()
        dq2, db2 = _bwd(c, d, qkv=v.qkv, o_in=v.o_in, do=v.do, dqkv=v.dqkv, variant=variant, reduce_on=rb)
        rb.launch()
        torch.cuda.synchronize()
        assert torch.equal(dq2, dq0)
        assert AC.rel_max(db2, db0) <= 2e-4  # test_sdpa_long_partial_only_mode's bound between the two reductions
        _sentinels_intact(w, c, d)


def test_views_cls_forward():
    N = 197
    c, d, _ = _case("base", N, BF16)
    lib = L.lib()
    n0 = lib.vit_sdpa_cls_count(0)
    o0, lse0 = ops.sdpa_fwd_cls(d.qkv, B, H, N, scale=c.scale)
    w, v = _view_operands(c, d)
    o1, lse1 = ops.sdpa_fwd_cls(v.qkv, B, H, N, o=v.o, scale=c.scale)
    torch.cuda.synchronize()
    assert lib.vit_sdpa_cls_count(0) - n0 == 2
    assert torch.equal(o0, o1) and torch.equal(lse0, lse1)
    assert (w.o[:, D:] == SENT).all()
    _sentinels_intact(w, c, d)


# ---------------------------------------------------------------------------- 5. scale

@pytest.mark.parametrize("scale", [0.05, 0.3])
@pytest.mark.parametrize("fam,N", [("res-bf16-fused", 193), ("res-bf16-two", 225), ("res-f32", 193),
                                   ("stream-bf16", 321), ("generic-bf16", 50), ("generic-f32", 50)],
                         ids=lambda x: str(x))
def test_scale(fam, N, scale):
    """A scale other than 64 ** -0.5 reaches the forward's exponent and the backward's -lse / scale alike."""
    _run_family(fam, "base", N, scale=scale)
