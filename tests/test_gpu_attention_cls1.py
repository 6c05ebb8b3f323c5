"""GPU: the one-query attention kernels (attn_cls1_fwd / attn_cls1_bwd behind vit_sdpa_cls1_fwd /
vit_sdpa_cls1_bwd) against a float64 evaluation of the same formula.

Inputs are those of oracle/attn_cases.make_case, rounded to the storage dtype; the reference is query row 0 of every
(b, h) against all keys and values in float64, and its gradients for a dO that is zero except in row 0.  The backward
is fed the reference's o (rounded to the dtype) and lse, so a forward error cannot leak into the gradient check.

Bounds: those tests/test_gpu_attention_conformance.py applies to the full kernels of the same dtype, none fitted to
these kernels -- bf16: o 1.5e-2, lse 2e-3 and 2e-2 absolute, dq / dk / dv 3e-2, each of the reference's largest
magnitude; f32: o and lse 1e-5, gradients 1e-4, or 4x the error torch's own float32 CPU evaluation of the same
one-query formula makes on the same inputs, whichever is larger (on ``offset`` one f32 ulp of a score is 3e-5, and
no f32 kernel can hold 1e-5 there).  The f32 backward on ``offset`` runs on ``offset4`` (its MILDER substitution);
the forward keeps ``offset``.  At N = 1 dq and dk are identically zero and their error is measured against the
largest magnitude of [dq | dk | dv].

B = H = 2: two heads exercise the head column offsets, two images the row strides.  Outputs are pre-filled with NaN
(an unwritten element shows), a guard band behind each output buffer must stay untouched, and dq rows 1 .. N-1 are
compared with ``== 0``.  Every figure is printed as a ``FIG`` line before it is asserted."""
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import attn_cases as AC  # noqa: E402
from vit_amd import _lib as L  # noqa: E402
from vit_amd import ops  # noqa: E402

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
DTYPES, IDS = [BF16, F32], ["bf16", "f32"]
B, H = 2, 2
SENT = -12288.0  # exact in bf16
GUARD = 256      # elements behind each output buffer
TOKENS = list(range(1, 81)) + [127, 128, 129, 197, 257, 289, 577, 785]


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    L.load()


def _one_query(q, k, v, do, scale):
    """Query row 0 against all keys, in the dtype of q: (o [B, D], lse [B*H], grads [B*N, 3D] for a dO that is
    zero except row 0).  q, k, v, do [B, H, N, 64]."""
    q0 = q[:, :, :1].clone().requires_grad_(True)
    k, v = k.clone().requires_grad_(True), v.clone().requires_grad_(True)
    s = (q0 @ k.transpose(-1, -2)) * scale
    lse = torch.logsumexp(s, -1)
    o = torch.softmax(s, -1) @ v
    o.backward(do[:, :, :1])
    dq = torch.zeros_like(q)
    dq[:, :, :1] = q0.grad
    grads = torch.cat([AC.pack(dq), AC.pack(k.grad), AC.pack(v.grad)], 1)
    return AC.pack(o.detach()).double(), lse.detach().reshape(-1).double(), grads.double()


_CASES = {}


def _case(kind, N, dtype, Bn=B, Hn=H):
    """The case, its float64 one-query reference, torch's float32 evaluation (f32 only) and the device operands;
    computed once per key and left unchanged."""
    key = (kind, N, dtype, Bn, Hn)
    if key not in _CASES:
        c = AC.make_case(kind, Bn, Hn, N, dtype)
        D = Hn * 64
        parts = lambda cast: tuple(t for t in AC.split_qkv(cast(c.qkv), Bn, Hn, N)) + (AC.unpack(cast(c.do), Bn, Hn, N),)
        ref = _one_query(*parts(lambda t: t.double()), c.scale)
        tf = _one_query(*parts(lambda t: t.float()), c.scale) if dtype == F32 else None
        d = SimpleNamespace(qkv=c.qkv.to(DEV), do=c.do.reshape(Bn, N, D)[:, 0].contiguous().to(DEV),
                            o_in=ref[0].to(dtype).to(DEV), lse_in=ref[1].float().to(DEV))
        _CASES[key] = (c, ref, tf, d)
    return _CASES[key]


class _Report:
    def __init__(self, c):
        self.head, self.bad = f"FIG cls1 | {c.kind} N={c.N} {'bf16' if c.dtype == BF16 else 'f32'}", []

    def add(self, what, err, bound, torch_err=None):
        ratio = "" if torch_err is None else f" | x torch-f32 {err / max(torch_err, 1e-30):.2f} ({torch_err:.2e})"
        print(f"{self.head} | {what} {err:.3e} (bound {bound:.1e}){ratio}")
        if not err <= bound:  # a NaN is past every bound
            self.bad.append(f"{what} {err:.3e} > {bound:.1e}")

    def done(self):
        assert not self.bad, f"{self.head}: " + "; ".join(self.bad)


def _bound(dtype, project, torch_err):
    return project if dtype == BF16 else max(project, 4 * torch_err)


def _guarded(rows, cols, dtype):
    """A NaN-filled [rows, cols] output with a sentinel guard band behind it, as (view, whole buffer)."""
    buf = torch.full((rows * cols + GUARD,), SENT, dtype=dtype, device=DEV)
    view = buf[:rows * cols].view(rows, cols)
    view.fill_(float("nan"))
    return view, buf


def _guard_intact(buf, n):
    return bool((buf[n:] == SENT).all())


def _run_fwd(rep, kind, N, dtype, Bn=B, Hn=H):
    c, ref, tf, d = _case(kind, N, dtype, Bn, Hn)
    D = Hn * 64
    o, obuf = _guarded(Bn, D, dtype)
    lse, lbuf = _guarded(1, Bn * Hn, F32)
    ops.sdpa_cls1_fwd(d.qkv, Bn, Hn, N, o=o, lse=lse.view(-1), scale=c.scale)
    torch.cuda.synchronize()
    assert _guard_intact(obuf, Bn * D) and _guard_intact(lbuf, Bn * Hn), "written behind an output buffer"
    bf = dtype == BF16
    for what, got, i, tol in (("o", o, 0, AC.BF16_O if bf else AC.F32_O),
                              ("lse", lse.view(-1), 1, AC.BF16_LSE if bf else AC.F32_LSE)):
        te = None if bf else AC.rel_max(tf[i], ref[i])
        rep.add(what, AC.rel_max(got, ref[i]), _bound(dtype, tol, te or 0.0), te)
    if bf:
        rep.add("lse abs", AC.abs_max(lse.view(-1), ref[1]), AC.BF16_LSE_ABS)
    return o, lse.view(-1)


def _run_bwd(rep, kind, N, dtype, Bn=B, Hn=H):
    c, ref, tf, d = _case(kind, N, dtype, Bn, Hn)
    D = Hn * 64
    dqkv, buf = _guarded(Bn * N, 3 * D, dtype)
    ops.sdpa_cls1_bwd(d.qkv, d.o_in, d.do, d.lse_in, Bn, Hn, N, dqkv=dqkv, scale=c.scale)
    torch.cuda.synchronize()
    assert _guard_intact(buf, Bn * N * 3 * D), "written behind dqkv"
    assert not torch.isnan(dqkv).any(), "an element of dqkv was not written"
    assert (dqkv.view(Bn, N, 3 * D)[:, 1:, :D] == 0).all(), "dq rows 1 .. N-1 are not exact zeros"
    bf = dtype == BF16
    tg = AC.BF16_GRAD if bf else AC.F32_GRAD
    g = dqkv.double().cpu()
    blk = lambda x, i: x[:, i * D:(i + 1) * D]
    for i, name in enumerate(("dq", "dk", "dv")):
        te = None if bf else AC.rel_max(blk(tf[2], i), blk(ref[2], i), ref[2])
        rep.add(name, AC.rel_max(blk(g, i), blk(ref[2], i), ref[2]), _bound(dtype, tg, te or 0.0), te)
    return dqkv


def _run(kind, N, dtype):
    """Forward and backward on the case; the f32 backward on ``offset`` takes its MILDER substitution."""
    rep = _Report(_case(kind, N, dtype)[0])
    _run_fwd(rep, kind, N, dtype)
    bk = AC.MILDER.get(kind, kind) if dtype == F32 else kind
    if bk != kind:
        rep.head += f" (backward on {bk})"
    _run_bwd(rep, bk, N, dtype)
    rep.done()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("N", TOKENS)
def test_every_token_count(N, dtype):
    _run("base", N, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("N", [17, 257, 577])
@pytest.mark.parametrize("kind", AC.KINDS)
def test_every_kind(kind, N, dtype):
    _run(kind, N, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_views(dtype):
    """B = 3, H = 16, N = 50: qkv a column-offset view of a wider buffer, o_cls written into the dense o
    (ld_o = N * D), dqkv a view: the contiguous call's bits, within the bounds, nothing outside the views touched."""
    Bn, Hn, N = 3, 16, 50
    D = Hn * 64
    c, ref, tf, d = _case("base", N, dtype, Bn, Hn)
    rep = _Report(c)
    o0, lse0 = _run_fwd(rep, "base", N, dtype, Bn, Hn)
    dq0 = _run_bwd(rep, "base", N, dtype, Bn, Hn)
    rep.done()
    wq = torch.full((Bn * N, 3 * D + 16), SENT, dtype=dtype, device=DEV)
    qkv = wq[:, 8:8 + 3 * D]
    qkv.copy_(d.qkv)
    o_dense = torch.full((Bn * N, D), float("nan"), dtype=dtype, device=DEV)
    o_cls = o_dense.view(Bn, N * D)[:, :D]
    wd = torch.full((Bn * N, 3 * D + 8), SENT, dtype=dtype, device=DEV)
    dqkv = wd[:, :3 * D]
    assert qkv.stride(0) > 3 * D and o_cls.stride(0) == N * D and not dqkv.is_contiguous()
    _, lse1 = ops.sdpa_cls1_fwd(qkv, Bn, Hn, N, o=o_cls, scale=c.scale)
    # the backward from the forward's own o in the dense tensor and a strided dO
    do_dense = torch.full((Bn * N, D), SENT, dtype=dtype, device=DEV)
    do_dense.view(Bn, N * D)[:, :D].copy_(d.do)
    o_in = torch.full((Bn * N, D), SENT, dtype=dtype, device=DEV)
    o_in.view(Bn, N * D)[:, :D].copy_(d.o_in)
    ops.sdpa_cls1_bwd(qkv, o_in.view(Bn, N * D)[:, :D], do_dense.view(Bn, N * D)[:, :D], d.lse_in, Bn, Hn, N, dqkv=dqkv,
                      scale=c.scale)
    torch.cuda.synchronize()
    assert torch.equal(o_cls, o0) and torch.equal(lse1, lse0) and torch.equal(dqkv, dq0)
    assert torch.isnan(o_dense.view(Bn, N, D)[:, 1:]).all(), "o: written outside the class rows"
    assert (wq[:, :8] == SENT).all() and (wq[:, 8 + 3 * D:] == SENT).all() and torch.equal(qkv, d.qkv)
    assert (wd[:, 3 * D:] == SENT).all(), "dqkv: written outside the view"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_two_calls_are_bitwise_equal_and_counted(dtype):
    N = 257
    c, ref, tf, d = _case("base", N, dtype)
    lib = L.lib()
    n0 = lib.vit_sdpa_cls1_count(0)
    outs = []
    for _ in range(2):
        o, lse = ops.sdpa_cls1_fwd(d.qkv, B, H, N, scale=c.scale)
        dqkv = ops.sdpa_cls1_bwd(d.qkv, d.o_in, d.do, d.lse_in, B, H, N, scale=c.scale)
        outs.append((o, lse, dqkv))
    torch.cuda.synchronize()
    assert lib.vit_sdpa_cls1_count(0) - n0 == 4  # each launch of either kernel
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert lib.vit_sdpa_cls1_count(1) >= 4 and lib.vit_sdpa_cls1_count(0) == 0  # reset


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_rejected_arguments_queue_nothing(dtype):
    """head_dim 32, N = 0, a row stride that is not a multiple of 16 bytes and N past the bound: an error code, the
    counter unmoved and the NaN fill intact."""
    N, D = 17, H * 64
    c, ref, tf, d = _case("base", N, dtype)
    lib, dt, st = L.lib(), L.dt(d.qkv), L.stream_ptr()
    o = torch.full((B, D), float("nan"), dtype=dtype, device=DEV)
    lse = torch.full((B * H,), float("nan"), device=DEV)
    dqkv = torch.full((B * N, 3 * D), float("nan"), dtype=dtype, device=DEV)
    p = lambda t: t.data_ptr()
    n0 = lib.vit_sdpa_cls1_count(0)

    def fwd(n=N, hd=64, ldq=3 * D, ldo=D):
        return lib.vit_sdpa_cls1_fwd(dt, B, H, n, hd, p(d.qkv), ldq, p(o), ldo, p(lse), c.scale, st)

    def bwd(n=N, hd=64, ldq=3 * D, ldo=D, ldd=D, ldg=3 * D):
        return lib.vit_sdpa_cls1_bwd(dt, B, H, n, hd, p(d.qkv), ldq, p(d.o_in), ldo, p(d.do), ldd, p(d.lse_in), p(dqkv),
                                     ldg, c.scale, st)

    for rc in (fwd(hd=32), fwd(n=0), fwd(ldq=3 * D + 2), fwd(ldo=D + 2), fwd(n=ops.CLS1_MAX_TOKENS + 1),
               bwd(hd=32), bwd(n=0), bwd(ldq=3 * D + 2), bwd(ldo=D + 2), bwd(ldd=D + 2), bwd(ldg=3 * D + 2),
               bwd(n=ops.CLS1_MAX_TOKENS + 1)):
        assert rc != 0
    torch.cuda.synchronize()
    assert lib.vit_sdpa_cls1_count(0) == n0
    assert torch.isnan(o).all() and torch.isnan(lse).all() and torch.isnan(dqkv).all()
    assert fwd() == 0 and bwd() == 0  # the same operands with valid arguments launch
    torch.cuda.synchronize()
    assert lib.vit_sdpa_cls1_count(0) == n0 + 2 and not torch.isnan(o).any() and not torch.isnan(dqkv).any()
