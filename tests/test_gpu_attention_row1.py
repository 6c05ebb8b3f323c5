"""GPU: the one-query attention forward at a row per sequence (attn_row1_fwd behind vit_sdpa_row1_fwd, DESIGN
§4.21) against a float64 evaluation of the same formula.

Inputs are those of oracle/attn_cases.make_case, rounded to the storage dtype; the reference is, per sequence b,
query row qrow[b] of every head against keys and values 0 .. nk - 1 (nk = qrow[b] + 1 under the causal mask, else
N) in float64.

Bounds: those tests/test_gpu_attention_conformance.py and tests/test_gpu_attention_cls1.py apply to the kernels of
the same dtype, none fitted to this kernel -- bf16: o 1.5e-2, lse 2e-3 and 2e-2 absolute, each of the reference's
largest magnitude; f32: o and lse 1e-5, or 4x the error torch's own float32 CPU evaluation of the same one-query
formula makes on the same inputs, whichever is larger.  The agreement with sdpa_fwd(causal=True) at row qrow[b] is
held to the same bounds.

B = 3, H = 2; the token counts cross one key, 8 keys a wave and 32 keys a step; qrow is mixed per sequence from
{0, 1, N/2, N-1}.  Outputs are pre-filled with NaN inside sentinel-filled buffers.  Every figure is printed as a
``FIG`` line before it is asserted.  The bit equalities follow from the shared device body: the class-token kernel
is the qrow = 0, unmasked case, and the mask is a shorter key loop."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import attn_cases as AC  # noqa: E402
from vit_amd import _lib as L  # noqa: E402
from vit_amd import ops  # noqa: E402

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
DTYPES, IDS = [BF16, F32], ["bf16", "f32"]
B, H, D = 3, 2, 128
SENT = -12288.0  # exact in bf16
TOKENS = [1, 2, 7, 8, 9, 31, 32, 33, 63, 64, 65, 77, 257]


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    L.load()


def _mixes(N):
    """Two assignments of {0, 1, N/2, N-1} to the three sequences (positions past a short sequence fold in)."""
    c = lambda v: min(v, N - 1)
    return [[N - 1, c(N // 2), 0], [c(1), N - 1, c(N // 2)]]


def _one_query(qkv, N, qrow, causal, scale):
    """(o [B, D], lse [B * H]) of query row qrow[b] against keys 0 .. nk - 1, in the dtype of qkv (a CPU tensor)."""
    q, k, v = AC.split_qkv(qkv, B, H, N)
    o, lse = torch.empty(B, D, dtype=qkv.dtype), torch.empty(B * H, dtype=qkv.dtype)
    for b, e in enumerate(qrow):
        nk = e + 1 if causal else N
        s = (q[b, :, e:e + 1] @ k[b, :, :nk].transpose(-1, -2)) * scale  # [H, 1, nk]
        lse[b * H:(b + 1) * H] = torch.logsumexp(s, -1).reshape(H)
        o[b] = (torch.softmax(s, -1) @ v[b, :, :nk]).reshape(D)
    return o, lse


_CASES = {}


def _case(kind, N, dtype):
    """The case and its device qkv; computed once per key and left unchanged."""
    key = (kind, N, dtype)
    if key not in _CASES:
        c = AC.make_case(kind, B, H, N, dtype)
        _CASES[key] = (c, c.qkv.to(DEV))
    return _CASES[key]


class _Report:
    def __init__(self, head):
        self.head, self.bad = "FIG row1 | " + head, []

    def add(self, what, err, bound, torch_err=None):
        ratio = "" if torch_err is None else f" | x torch-f32 {err / max(torch_err, 1e-30):.2f} ({torch_err:.2e})"
        print(f"{self.head} | {what} {err:.3e} (bound {bound:.1e}){ratio}")
        if not err <= bound:  # a NaN is past every bound
            self.bad.append(f"{what} {err:.3e} > {bound:.1e}")

    def done(self):
        assert not self.bad, f"{self.head}: " + "; ".join(self.bad)


def _bound(dtype, project, torch_err):
    return project if dtype == BF16 else max(project, 4 * torch_err)


def _poisoned(dtype):
    """o_row and lse_row as strided / offset views, NaN-filled, inside sentinel-filled buffers:
    (o view, o buffer, lse view, lse buffer)."""
    ld = 2 * D + 8  # 16-byte multiples in both dtypes
    obuf = torch.full((B + 2, ld), SENT, dtype=dtype, device=DEV)
    o = obuf[1:1 + B, 8:8 + D]
    o.fill_(float("nan"))
    lbuf = torch.full((B * H + 16,), SENT, dtype=F32, device=DEV)
    lse = lbuf[8:8 + B * H]
    lse.fill_(float("nan"))
    return o, obuf, lse, lbuf


def _outside_intact(o, obuf, lse, lbuf):
    ob, lb = obuf.clone(), lbuf.clone()
    ob[1:1 + B, 8:8 + D] = SENT
    lb[8:8 + B * H] = SENT
    return bool((ob == SENT).all()) and bool((lb == SENT).all())


def _rows(qrow):
    return torch.tensor(qrow, dtype=torch.int64, device=DEV)


def _run(kind, N, dtype, causal):
    c, qkv = _case(kind, N, dtype)
    bf = dtype == BF16
    for qrow in _mixes(N):
        rep = _Report(f"{kind} N={N} {IDS[not bf]} causal={int(causal)} qrow={qrow}")
        ref = _one_query(c.qkv.double(), N, qrow, causal, c.scale)
        tf = None if bf else _one_query(c.qkv.float(), N, qrow, causal, c.scale)
        o, obuf, lse, lbuf = _poisoned(dtype)
        assert o.stride(0) == 2 * D + 8 and not o.is_contiguous()
        ops.sdpa_row1_fwd(qkv, _rows(qrow), B, H, N, causal=causal, o=o, lse=lse, scale=c.scale)
        torch.cuda.synchronize()
        assert _outside_intact(o, obuf, lse, lbuf), "written outside the output views"
        assert not torch.isnan(o).any() and not torch.isnan(lse).any(), "an output element was not written"
        for what, got, i, tol in (("o", o, 0, AC.BF16_O if bf else AC.F32_O),
                                  ("lse", lse, 1, AC.BF16_LSE if bf else AC.F32_LSE)):
            te = None if bf else AC.rel_max(tf[i], ref[i])
            rep.add(what, AC.rel_max(got, ref[i]), _bound(dtype, tol, te or 0.0), te)
        if bf:
            rep.add("lse abs", AC.abs_max(lse, ref[1]), AC.BF16_LSE_ABS)
        if causal:
            # the dense causal forward at the same rows, held to the same bounds (scale: the reference's magnitude)
            od, ld = ops.sdpa_fwd(qkv, B, H, N, causal=True, scale=c.scale)
            torch.cuda.synchronize()
            od = torch.stack([od.view(B, N, D)[b, e] for b, e in enumerate(qrow)])
            ld = torch.stack([ld.view(B, H, N)[b, :, e] for b, e in enumerate(qrow)]).reshape(-1)
            so, sl = ref[0].abs().max().item() + 1e-12, ref[1].abs().max().item() + 1e-12
            te_o = None if bf else AC.rel_max(tf[0], ref[0])
            te_l = None if bf else AC.rel_max(tf[1], ref[1])
            rep.add("o vs sdpa_fwd", AC.abs_max(o, od) / so, _bound(dtype, AC.BF16_O if bf else AC.F32_O, te_o or 0.0),
                    te_o)
            rep.add("lse vs sdpa_fwd", AC.abs_max(lse, ld) / sl,
                    _bound(dtype, AC.BF16_LSE if bf else AC.F32_LSE, te_l or 0.0), te_l)
        rep.done()


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("N", TOKENS)
def test_every_token_count(N, dtype, causal):
    _run("base", N, dtype, causal)


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", [k for k in AC.KINDS if k != "base"])
def test_every_kind(kind, dtype, causal):
    _run(kind, 77, dtype, causal)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("N", [1, 9, 33, 77, 257])
def test_row_zero_unmasked_is_the_class_token_kernel(N, dtype):
    c, qkv = _case("base", N, dtype)
    o0, l0 = ops.sdpa_cls1_fwd(qkv, B, H, N, scale=c.scale)
    o1, l1 = ops.sdpa_row1_fwd(qkv, _rows([0, 0, 0]), B, H, N, causal=False, scale=c.scale)
    torch.cuda.synchronize()
    assert torch.equal(o1, o0) and torch.equal(l1, l0)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("N", [2, 9, 33, 77, 257])
def test_causal_is_the_unmasked_call_on_the_rows_in_front(N, dtype):
    """Causal with qrow = e equals the unmasked call on the first e + 1 rows of the sequence (a view, N = e + 1)."""
    c, qkv = _case("base", N, dtype)
    for qrow in _mixes(N):
        o, lse = ops.sdpa_row1_fwd(qkv, _rows(qrow), B, H, N, causal=True, scale=c.scale)
        for b, e in enumerate(qrow):
            head = qkv[b * N:b * N + e + 1]
            ob, lb = ops.sdpa_row1_fwd(head, _rows([e]), 1, H, e + 1, causal=False, scale=c.scale)
            torch.cuda.synchronize()
            assert torch.equal(ob[0], o[b]) and torch.equal(lb, lse[b * H:(b + 1) * H]), (qrow, b)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_two_calls_are_bitwise_equal_and_counted(dtype):
    N = 77
    c, qkv = _case("base", N, dtype)
    lib = L.lib()
    rows = _rows(_mixes(N)[0])
    n0 = lib.vit_sdpa_row1_count(0)
    n1 = lib.vit_sdpa_cls1_count(0)
    a = ops.sdpa_row1_fwd(qkv, rows, B, H, N, causal=True, scale=c.scale)
    b = ops.sdpa_row1_fwd(qkv, rows, B, H, N, causal=True, scale=c.scale)
    torch.cuda.synchronize()
    assert lib.vit_sdpa_row1_count(0) - n0 == 2, "a silent fallback: the one-query kernel did not run"
    assert lib.vit_sdpa_cls1_count(0) == n1  # its own counter
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert lib.vit_sdpa_row1_count(1) >= 2 and lib.vit_sdpa_row1_count(0) == 0  # reset


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("N", [9, 77])
def test_causal_isolation_and_clamped_positions(N, dtype):
    """K and V rows past qrow[b] are NaN: o and lse keep their bits.  A position of -5 or N + 5 is 0 or N - 1."""
    c, qkv = _case("base", N, dtype)
    for qrow in _mixes(N):
        o0, l0 = ops.sdpa_row1_fwd(qkv, _rows(qrow), B, H, N, causal=True, scale=c.scale)
        bad = qkv.clone().view(B, N, 3 * D)
        for b, e in enumerate(qrow):
            bad[b, e + 1:, D:] = float("nan")
        o1, l1 = ops.sdpa_row1_fwd(bad.view(B * N, 3 * D), _rows(qrow), B, H, N, causal=True, scale=c.scale)
        torch.cuda.synchronize()
        assert not torch.isnan(o1).any() and not torch.isnan(l1).any(), "a masked K / V row was read"
        assert torch.equal(o1, o0) and torch.equal(l1, l0)
    for causal in (False, True):  # finite data everywhere
        want = ops.sdpa_row1_fwd(qkv, _rows([0, N - 1, 0]), B, H, N, causal=causal, scale=c.scale)
        got = ops.sdpa_row1_fwd(qkv, _rows([-5, N + 5, -(1 << 40)]), B, H, N, causal=causal, scale=c.scale)
        torch.cuda.synchronize()
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), causal


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_rejected_arguments_queue_nothing(dtype):
    N = 17
    c, qkv = _case("base", N, dtype)
    lib, dt, st = L.lib(), L.dt(qkv), L.stream_ptr()
    o = torch.full((B, D), float("nan"), dtype=dtype, device=DEV)
    lse = torch.full((B * H,), float("nan"), device=DEV)
    rows = _rows([0, 3, 16])
    p = lambda t: t.data_ptr()
    n0 = lib.vit_sdpa_row1_count(0)

    def fwd(n=N, hd=64, ldq=3 * D, ldo=D, r=p(rows)):
        return lib.vit_sdpa_row1_fwd(dt, B, H, n, hd, p(qkv), ldq, r, 1, p(o), ldo, p(lse), c.scale, st)

    for rc in (fwd(hd=32), fwd(n=0), fwd(ldq=3 * D + 2), fwd(ldo=D + 2), fwd(n=ops.CLS1_MAX_TOKENS + 1), fwd(r=None)):
        assert rc != 0
    torch.cuda.synchronize()
    assert lib.vit_sdpa_row1_count(0) == n0
    assert torch.isnan(o).all() and torch.isnan(lse).all()
    assert fwd() == 0  # the same operands with valid arguments launch
    torch.cuda.synchronize()
    assert lib.vit_sdpa_row1_count(0) == n0 + 1 and not torch.isnan(o).any() and not torch.isnan(lse).any()
