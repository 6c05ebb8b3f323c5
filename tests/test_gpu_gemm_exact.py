"""GPU: the GEMM family bit for bit, inside poisoned, strided views.

Cases come from oracle/gemm_cases.py: operands whose products and sums are exact wherever a kernel holds them, so
one float64 reference serves every tile shape, k order, split count and reduction tree.  Store-type outputs (plain
stores, residual and accumulate adds, patch rows, slab totals, column sums) are compared bitwise; the activation
values are held per element to gemm_cases.act_bound, the only tolerance here.

Every operand and output is a view in the interior of a larger allocation: a row stride past the extent, a
16-byte-aligned offset in front and 256 rows behind.  Input padding is NaN (a kernel that loads past an edge and
multiplies by zero shows), output padding a sentinel.  After each call the outputs are finite, everything outside
each output view and every input buffer is bitwise unchanged, and vit_gemm_g4_count says which kernel ran.
"""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import gemm_cases as G  # noqa: E402
from vit_amd import _lib as L  # noqa: E402

DEV = "cuda"
F32, BF = torch.float32, torch.bfloat16
SENT = 640.0       # exact in f32 and bf16, outside every value the cases produce
TAIL_ROWS = 256    # one full tile of rows behind every view
OFF = 72           # elements in front of a view: 144 bytes of bf16, 288 of f32, both 16-byte multiples
INVALID = 1        # hipErrorInvalidValue
WORST = {"f": 0.0, "what": "none"}


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    L.load()


def _raw(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


class Buf:
    """A [rows, cols] view with row stride ``ld`` that starts ``off`` elements into a buffer filled with NaN (an
    input: ``src`` given) or the sentinel (an output), with ``tail`` elements (256 rows) behind the view."""

    def __init__(self, rows, cols, dtype, src=None, ld=None, off=OFF, tail=None, fill=None):
        self.rows, self.cols, self.ld, self.off = rows, cols, cols if ld is None else ld, off
        assert self.ld >= cols
        tail = TAIL_ROWS * self.ld if tail is None else tail
        fill = (float("nan") if src is not None else SENT) if fill is None else fill
        self.fill = fill
        self.buf = torch.full((off + rows * self.ld + tail,), fill, dtype=dtype, device=DEV)
        self.v = self.buf[off:off + rows * self.ld].view(rows, self.ld)[:, :cols]
        if src is not None:
            self.v.copy_(src.reshape(rows, cols))
        self.snap = self.buf.clone() if src is not None else None

    @property
    def ptr(self):
        return self.v.data_ptr()

    def set(self, src):
        """Give an output view a starting value (accumulate / in-place residual)."""
        self.v.copy_(src.reshape(self.rows, self.cols))

    def unchanged(self, what):
        assert torch.equal(_raw(self.buf), _raw(self.snap)), f"{what}: an input buffer changed"

    def outside_untouched(self, what):
        m = torch.ones(self.buf.numel(), dtype=torch.bool, device=DEV)
        m[self.off:self.off + self.rows * self.ld].view(self.rows, self.ld)[:, :self.cols] = False
        assert bool((self.buf[m] == self.fill).all()), f"{what}: wrote outside its [{self.rows}, {self.cols}] view"

    def all_untouched(self, what):
        assert bool((self.buf == self.fill).all()), f"{what}: wrote into a buffer no kernel may touch"


def _vec(n, src=None, off=4, dtype=F32):
    return Buf(1, n, dtype, src, off=off, tail=4096)


def _stream():
    return L.stream_ptr(DEV)


def _exact(out, ref64, what):
    """Bitwise: the float64 reference is exact in the output's dtype."""
    ref = ref64.to(out.v.dtype)
    assert torch.equal(ref.double(), ref64.double()), f"{what}: the reference is not exact in {out.v.dtype}"
    got = out.v.cpu().contiguous()
    assert bool(torch.isfinite(got.float()).all()), f"{what}: non-finite output"
    nbad = int((_raw(got) != _raw(ref.reshape(got.shape).contiguous())).sum())
    assert nbad == 0, f"{what}: {nbad} of {got.numel()} elements differ from the exact result"


def _act(out, ref64, pre64, what):
    f = G.act_fraction(out.v, ref64, pre64, out.v.dtype)
    if f > WORST["f"]:
        WORST.update(f=f, what=what)
    print(f"{what}: {f:.3f} of the activation bound")
    assert f <= 1.0, f"{what}: {f:.3f} of the activation bound"


def _settle(what, outs=(), ins=(), idle=()):
    torch.cuda.synchronize()
    for b in outs:
        b.outside_untouched(what)
    for b in ins:
        b.unchanged(what)
    for b in idle:
        b.all_untouched(what)


def _g4(reset=1):
    return L.lib().vit_gemm_g4_count(reset)


@contextlib.contextmanager
def hooks(variant=None, g4_gelu=None, g4_cfg=None, group=None):
    lib, prev = L.lib(), None
    try:
        if variant is not None:
            lib.vit_gemm_variant(variant)
        if g4_gelu is not None:
            prev = lib.vit_gemm_g4_gelu(g4_gelu)
        if g4_cfg is not None:
            lib.vit_gemm_g4_config(*g4_cfg)
        if group is not None:
            lib.vit_gemm_group(*group)
        yield
    finally:
        lib.vit_gemm_variant(-1)
        if prev is not None:
            lib.vit_gemm_g4_gelu(prev)
        if g4_cfg is not None:
            lib.vit_gemm_g4_config(0, 2, 0, 1)
        if group is not None:
            lib.vit_gemm_group(-2, -2)


# ---------------------------------------------------------------------------- forward / input gradient runners

def _fwd(c, epi=L.EPI_STORE, odt=BF, bias=True, pad=8, c_off=OFF, bias_off=4, resid=None, resid_off=OFF,
         in_place=False, two=False, what=""):
    """vit_linear_fwd over strided views; returns (Y, act_out).  ``resid`` [M, N] f32 shares Y's row stride."""
    M, N, K = c.M, c.N, c.R
    x = Buf(M, K, c.p.dtype, c.p, ld=K + pad)
    w = Buf(N, K, c.q.dtype, c.q)                    # the ABI takes W contiguous
    b = _vec(N, c.bias, off=bias_off) if bias else None
    y = Buf(M, N, odt, ld=N + pad, off=c_off)
    a = Buf(M, N, odt, ld=N + pad) if two else None
    r = None
    if in_place:
        y.set(resid)
    elif resid is not None:
        r = Buf(M, N, F32, resid, ld=N + pad, off=resid_off)
    rp = y.ptr if in_place else (r.ptr if r is not None else None)
    L.call("vit_linear_fwd", L.dt(c.p), L.dt(y.v), epi, M, N, K, x.ptr, x.ld, w.ptr, b.ptr if b else None, y.ptr, y.ld,
           rp, a.ptr if a else None, _stream())
    _settle(what, outs=[t for t in (y, a) if t is not None], ins=[t for t in (x, w, b, r) if t is not None])
    return y, a


def _dgrad(c, epi=L.EPI_STORE, odt=BF, aux=None, pad=8, dx_off=OFF, aux_off=OFF, dbias=False, defer=0, part_off=4,
           what=""):
    """vit_linear_dgrad: dX [M, N] = dY [M, R] W [R, N] (* aux); returns (dX, dbias or None, partial or None)."""
    M, Nl, Kl = c.M, c.R, c.N
    dy = Buf(M, Nl, c.p.dtype, c.p, ld=Nl + pad)
    w = Buf(Nl, Kl, c.qT.dtype, c.qT)
    dx = Buf(M, Kl, odt, ld=Kl + pad, off=dx_off)
    ax = Buf(M, Kl, aux.dtype, aux, ld=Kl + pad, off=aux_off) if aux is not None else None
    db = part = None
    pf = 0
    if dbias:
        pf = L.lib().vit_linear_dgrad_partial_floats(M, Kl)
        assert pf == G.dgrad_partial_floats(M, Kl)
        db, part = _vec(Kl), _vec(pf, off=part_off)
    L.call("vit_linear_dgrad", L.dt(c.p), L.dt(dx.v), epi, M, Nl, Kl, dy.ptr, dy.ld, w.ptr, dx.ptr, dx.ld,
           ax.ptr if ax else None, db.ptr if db else None, part.ptr if part else None, pf, defer, _stream())
    outs = [dx] + ([part] if dbias else []) + ([db] if dbias and not defer else [])
    _settle(what, outs=outs, ins=[t for t in (dy, w, ax) if t is not None], idle=[db] if dbias and defer else [])
    return dx, db, part


# ---------------------------------------------------------------------------- g4: the default plain bf16 path

@pytest.mark.parametrize("walk", [None] + list(G.G4_WALKS), ids=["default", "bands", "one-wg"])
@pytest.mark.parametrize("shape", G.G4_SHAPES, ids=str)
def test_g4_forward_and_input_gradient(shape, walk):
    c = G.mm_case(*shape)
    with hooks(g4_cfg=walk):
        _g4()
        y, _ = _fwd(c, what=f"g4 fwd {shape} walk {walk}")
        assert _g4() == 1, "the forward did not run on g4"
        _exact(y, c.pre, f"g4 fwd {shape} walk {walk}")
        y, _ = _fwd(c, bias=False, pad=24, what=f"g4 fwd no bias {shape}")
        assert _g4() == 1
        _exact(y, c.acc, f"g4 fwd no bias {shape} walk {walk}")
        dx, _, _ = _dgrad(c, what=f"g4 dgrad {shape} walk {walk}")
        assert _g4() == 1, "the input gradient did not run on g4"
        _exact(dx, c.acc, f"g4 dgrad {shape} walk {walk}")


def test_g4_and_v5_in_bands_of_three_row_tiles():
    c, cq = G.mm_case(*G.G4_SHAPES[1]), G.mm_case(*G.PAIR_SHAPES[0], BF, "quarter")
    with hooks(group=G.GROUP_BANDS):
        _g4()
        y, _ = _fwd(c, what="g4 fwd bands of 3")
        _exact(y, c.pre, "g4 fwd bands of 3")
        dx, _, _ = _dgrad(c, what="g4 dgrad bands of 3")
        _exact(dx, c.acc, "g4 dgrad bands of 3")
        assert _g4() == 2
        _pair(cq, "gelu", "bands of 3")
        y, _ = _fwd(c, L.EPI_RESID, F32, resid=G.eighths(c.M, c.N), what="v5 resid bands of 3")
        _exact(y, c.pre + G.eighths(c.M, c.N).double(), "v5 resid bands of 3")
        assert _g4() == 0


# ---------------------------------------------------------------------------- 8-wave kernels of the default dispatch

def _pair(c, act, tag, odt=BF):
    pair_epi, fwd_epi = {"gelu": (L.EPI_BIAS_GELU, L.EPI_BIAS_GELU_FWD), "qgelu": (L.EPI_BIAS_QGELU, L.EPI_BIAS_QGELU_FWD)}[act]
    ra, rd = G.ACTS[act][0](c.pre)
    what = f"{act} pair {c.M}x{c.N}x{c.R} {odt} {tag}"
    d, a = _fwd(c, pair_epi, odt, two=True, what=what)
    _act(a, ra, c.pre, what + " act")
    _act(d, rd, c.pre, what + " act'")
    only, _ = _fwd(c, fwd_epi, odt, what=what + " act-only")
    assert torch.equal(_raw(only.v.contiguous()), _raw(a.v.contiguous())), what + ": act-only differs from the pair's act_out"
    return d, a


@pytest.mark.parametrize("act", ["gelu", "qgelu"])
@pytest.mark.parametrize("shape", G.PAIR_SHAPES, ids=str)
def test_activation_pairs_on_v5_and_g4(shape, act):
    c = G.mm_case(*shape, BF, "quarter")
    with hooks(g4_gelu=1):
        _g4()
        d5, a5 = _pair(c, act, "v5")
        assert _g4() == 0, "the pair left the 8-wave kernel"
    if act == "gelu":  # the erf GELU pair is the one g4 has a form for
        with hooks(g4_gelu=3):
            ra, rd = G.gelu_both(c.pre)
            d, a = _fwd(c, L.EPI_BIAS_GELU, BF, two=True, what=f"gelu pair g4 {shape}")
            assert _g4() == 1, "the GELU pair did not run on g4"
            _act(a, ra, c.pre, f"gelu pair g4 {shape} act")
            _act(d, rd, c.pre, f"gelu pair g4 {shape} act'")


def test_v1_forward_at_k_96():
    c = G.mm_case(*G.V1_FWD)
    _g4()
    y, _ = _fwd(c, what="v1 fwd K=96")
    _exact(y, c.pre, "v1 fwd K=96")
    y, _ = _fwd(c, odt=F32, what="v1 fwd K=96 f32 out")
    _exact(y, c.pre, "v1 fwd K=96 f32 out")
    assert _g4() == 0


def test_bf16_output_width_that_is_no_multiple_of_8():
    """N % 8 == 4 passes the MFMA operand rules (N % 4) while g4, the permlane pairs and the bf16 image all
    decline it; the bf16 row sweeps store 8 columns at a time, so the last 4 columns must not take 4 more with
    them."""
    c = G.mm_case(*G.N_MOD8_4)
    _g4()
    for pad in (12, 4):   # ld % 8 == 0, and ld = N + 4 where a second half of a 16-byte store would land
        y, _ = _fwd(c, pad=pad, what=f"bf16 fwd N=132 pad {pad}")
        _exact(y, c.pre, f"bf16 fwd N=132 pad {pad}")
        dx, _, _ = _dgrad(c, pad=pad, what=f"bf16 dgrad N=132 pad {pad}")
        _exact(dx, c.acc, f"bf16 dgrad N=132 pad {pad}")
    y, _ = _fwd(c, odt=F32, pad=12, what="f32-out fwd N=132")
    _exact(y, c.pre, "f32-out fwd N=132")
    assert _g4() == 0


@pytest.mark.parametrize("in_place", [False, True], ids=["out-of-place", "in-place"])
def test_residual_epilogue_to_f32(in_place):
    c, r = G.mm_case(*G.RESID_SHAPE), G.eighths(*G.RESID_SHAPE[:2])
    y, _ = _fwd(c, L.EPI_RESID, F32, resid=r, in_place=in_place, what=f"resid in_place={in_place}")
    _exact(y, c.pre + r.double(), f"resid in_place={in_place}")


# ---------------------------------------------------------------------------- dbias: what each path sums

@pytest.mark.parametrize("path", ["v1", "g4"])
@pytest.mark.parametrize("epi", [L.EPI_GELU_BWD, L.EPI_QGELU_BWD], ids=["gelu'", "qgelu'"])
@pytest.mark.parametrize("shape", G.ACT_BWD_SHAPES, ids=str)
def test_act_bwd_input_gradient_with_fused_dbias(shape, epi, path):
    """The MFMA epilogues (8-wave V1 and g4) sum the f32 products acc * aux BEFORE they are rounded to the stored
    bf16: dbias is the column sum of the unrounded products, exactly, fused or through vit_colreduce."""
    c, aux = G.mm_case(*shape), G.sixteenths(*shape[:2])
    stored, s_stored, s_prod = G.act_bwd_ref(c.acc, aux, BF)
    assert not torch.equal(s_stored, s_prod)
    rows = -(-c.M // 64)
    with hooks(g4_gelu=3 if path == "g4" else 0):
        _g4()
        what = f"{path} act' dgrad {shape} epi {epi}"
        dx, db, part = _dgrad(c, epi, aux=aux, dbias=True, what=what + " fused")
        assert _g4() == (1 if path == "g4" else 0)
        _exact(dx, stored.double(), what)
        _exact(db, s_prod, what + " dbias = column sums of the f32 products")
        assert torch.equal(part.v.view(-1)[:rows * c.N].view(rows, c.N).double().sum(0).cpu(), s_prod)
        dx, db, part = _dgrad(c, epi, aux=aux, dbias=True, defer=1, what=what + " deferred")
        _exact(dx, stored.double(), what + " deferred")
        out = _vec(c.N)
        L.call("vit_colreduce", part.ptr, rows, c.N, out.ptr, 0, None, _stream())
        _settle(what + " colreduce", outs=[out, part])
        _exact(out, s_prod, what + " deferred dbias")
        dx, _, _ = _dgrad(c, epi, aux=aux, what=what + " no dbias")
        _exact(dx, stored.double(), what + " no dbias")


@pytest.mark.parametrize("which", ["dX", "partial", "aux"])
def test_act_bwd_on_the_generic_path_sums_the_stored_values(which):
    """dX or aux off the 16-byte grid sends the input gradient to the generic kernel; a misaligned partial buffer
    alone keeps the GEMM on g4 but takes the fused sums away.  Either way colsum_partial_kernel reads dX back, so
    dbias is the column sum of the STORED values."""
    shape = G.ACT_BWD_SHAPES[0]
    c, aux = G.mm_case(*shape), G.sixteenths(*shape[:2])
    stored, s_stored, _ = G.act_bwd_ref(c.acc, aux, BF)
    for delta in (1, 4):
        kw = {"dX": dict(dx_off=OFF + delta), "partial": dict(part_off=4 + delta), "aux": dict(aux_off=OFF + delta)}[which]
        aligned = which == "partial" and delta == 4
        with hooks(g4_gelu=3):
            _g4()
            what = f"act' dgrad, {which} off by {delta}"
            dx, db, _ = _dgrad(c, L.EPI_GELU_BWD, aux=aux, dbias=True, what=what, **kw)
            assert _g4() == (1 if which == "partial" else 0)
            _exact(dx, stored.double(), what)
            _exact(db, G.act_bwd_ref(c.acc, aux, BF)[2] if aligned else s_stored, what + " dbias")


def test_v3_input_gradient_over_a_long_reduction_with_dbias():
    c = G.mm_case(*G.V3_DGRAD)
    _g4()
    dx, db, _ = _dgrad(c, dbias=True, what="v3 dgrad R=1088")
    assert _g4() == 0
    _exact(dx, c.acc, "v3 dgrad R=1088")
    _exact(db, c.acc.sum(0), "v3 dgrad R=1088 dbias")   # integers: stored and unrounded sums coincide


# ---------------------------------------------------------------------------- alignment: what the dispatcher now asks

@pytest.mark.parametrize("delta", [1, 4])
@pytest.mark.parametrize("which", ["C", "bias", "resid"])
def test_misaligned_epilogue_operands_take_the_generic_kernel(which, delta):
    """C, bias or the residual off the 16-byte grid: the dispatcher leaves g4 / the MFMA kernels for the generic
    kernel, and exact data makes its answer the same bits.  (bias and the residual are f32: 4 elements are 16
    bytes and keep the fast path.)"""
    c = G.mm_case(*G.MISALIGNED)
    what = f"{which} off by {delta}"
    _g4()
    if which == "resid":
        r = G.eighths(c.M, c.N)
        y, _ = _fwd(c, L.EPI_RESID, F32, resid=r, resid_off=OFF + delta, what=what)
        _exact(y, c.pre + r.double(), what)
        assert _g4() == 0
        return
    y, _ = _fwd(c, what=what, **({"c_off": OFF + delta} if which == "C" else {"bias_off": 4 + delta}))
    _exact(y, c.pre, what)
    assert _g4() == (1 if (which == "bias" and delta == 4) else 0)


# ---------------------------------------------------------------------------- weight gradient

def _wg_bufs(c, pad=8):
    return Buf(c.M, c.N, c.dy.dtype, c.dy, ld=c.N + pad), Buf(c.M, c.K, c.x.dtype, c.x, ld=c.K + 2 * pad)


def _wgrad_all(c, split, what):
    lib, n = L.lib(), c.N * c.K
    dt = L.dt(c.dy)
    dy, x = _wg_bufs(c)
    dW = _vec(n)
    ws = _vec(split * n) if split > 1 else None
    L.call("vit_linear_wgrad", dt, c.M, c.N, c.K, dy.ptr, dy.ld, x.ptr, x.ld, dW.ptr, split, ws.ptr if ws else None,
           split * n * 4 if ws else 0, _stream())
    _settle(what, outs=[dW] + ([ws] if ws else []), ins=[dy, x])
    _exact(dW, c.dW.reshape(1, n), what + " wgrad")
    return dy, x


@pytest.mark.parametrize("variant", [-1, 11], ids=["default", "w4"])
@pytest.mark.parametrize("N,K", G.WGRAD_NK)
def test_weight_gradient_bf16(N, K, variant):
    lib = L.lib()
    with hooks(variant=variant):
        for M, split in G.WGRAD_ROWS:
            c = G.wg_case(M, N, K)
            what = f"wgrad {M}x{N}x{K} split {split} variant {variant}"
            dy, x = _wgrad_all(c, split, what)
            n = N * K
            nz = lib.vit_linear_wgrad_nslabs(L.BF16, M, N, K, split)
            assert nz == G.wgrad_nslabs(M, split)
            slabs = _vec(nz * n)
            L.call("vit_linear_wgrad_partials", L.BF16, M, N, K, dy.ptr, dy.ld, x.ptr, x.ld, split, slabs.ptr, nz * n * 4,
                   _stream())
            _settle(what + " partials", outs=[slabs], ins=[dy, x])
            # every slab holds exact integers, so their float64 total is dW itself
            assert torch.equal(slabs.v.view(nz, n).double().sum(0).cpu(), c.dW.reshape(n)), what + ": slab total"
            assert bool(torch.isfinite(slabs.v).all())


@pytest.mark.parametrize("variant", [-1, 11], ids=["default", "w4"])
def test_weight_gradient_pairs_in_one_launch(variant):
    lib = L.lib()
    (Na, Ka), (Nb, Kb) = G.WGRAD_NK
    with hooks(variant=variant):
        for M, split in ((32, 1), (96, 1), (160, 3)):
            a, b = G.wg_case(M, Na, Ka), G.wg_case(M, Nb, Kb)
            (dya, xa), (dyb, xb) = _wg_bufs(a), _wg_bufs(b, pad=16)
            nz = lib.vit_linear_wgrad_nslabs(L.BF16, M, Na, Ka, split)
            sa, sb = _vec(nz * Na * Ka), _vec(nz * Nb * Kb)
            L.call("vit_linear_wgrad_partials2", M, split, Na, Ka, dya.ptr, dya.ld, xa.ptr, xa.ld, sa.ptr, nz * Na * Ka * 4,
                   Nb, Kb, dyb.ptr, dyb.ld, xb.ptr, xb.ld, sb.ptr, nz * Nb * Kb * 4, _stream())
            what = f"partials2 M={M} split {split} variant {variant}"
            _settle(what, outs=[sa, sb], ins=[dya, xa, dyb, xb])
            for s, c_, n in ((sa, a, Na * Ka), (sb, b, Nb * Kb)):
                assert bool(torch.isfinite(s.v).all())
                assert torch.equal(s.v.view(nz, n).double().sum(0).cpu(), c_.dW.reshape(n)), what + ": slab total"


@pytest.mark.parametrize("M,N,K,split", G.WGRAD_F32)
def test_weight_gradient_f32(M, N, K, split):
    c = G.wg_case(M, N, K, F32)
    _wgrad_all(c, split, f"f32 wgrad {M}x{N}x{K} split {split}")
    if (N * K) % 4 == 0 and G.f32_branch(G.CR, G.CR, N, K, M, split) == "mfma":
        lib, n = L.lib(), N * K
        dy, x = _wg_bufs(c)
        nz = lib.vit_linear_wgrad_nslabs(L.F32, M, N, K, split)
        assert nz == G.wgrad_nslabs(M, split, G.F32_BK)
        slabs = _vec(nz * n)
        L.call("vit_linear_wgrad_partials", L.F32, M, N, K, dy.ptr, dy.ld, x.ptr, x.ld, split, slabs.ptr, nz * n * 4, _stream())
        _settle("f32 partials", outs=[slabs], ins=[dy, x])
        assert torch.equal(slabs.v.view(nz, n).double().sum(0).cpu(), c.dW.reshape(n))


# ---------------------------------------------------------------------------- f32 MFMA

def test_f32_mfma_forward_epilogues():
    shape = G.F32_MFMA
    c = G.mm_case(*shape, F32)
    y, _ = _fwd(c, odt=F32, pad=4, what="f32 fwd")
    _exact(y, c.pre, "f32 fwd")
    r = G.eighths(c.M, c.N)
    y, _ = _fwd(c, L.EPI_RESID, F32, pad=4, resid=r, what="f32 resid")
    _exact(y, c.pre + r.double(), "f32 resid")
    cq = G.mm_case(*shape, F32, "quarter")
    _pair(cq, "gelu", "f32 mfma", F32)
    _pair(cq, "qgelu", "f32 mfma", F32)


def test_f32_mfma_input_gradient_with_dbias():
    c = G.mm_case(*G.F32_MFMA, F32)
    aux = G.sixteenths(c.M, c.N, F32)
    stored, s_stored, s_prod = G.act_bwd_ref(c.acc, aux, F32)
    dx, db, _ = _dgrad(c, L.EPI_GELU_BWD, F32, aux=aux, pad=4, dbias=True, what="f32 act' dgrad")
    _exact(dx, stored.double(), "f32 act' dgrad")
    _exact(db, s_prod, "f32 act' dgrad dbias")   # f32 out stores the product: both readings coincide
    dx, _, _ = _dgrad(c, odt=F32, pad=4, what="f32 dgrad")
    _exact(dx, c.acc, "f32 dgrad")


def _gemm_layouts(c, odt, pad, c_off=OFF, allow_fast=1, what=""):
    """All four layouts through vit_gemm: a CR operand is the transposed matrix, its extent contiguous."""
    M, N, R = c.M, c.N, c.R
    for pl in (G.RC, G.CR):
        for ql in (G.RC, G.CR):
            P = Buf(M, R, c.p.dtype, c.p, ld=R + pad) if pl == G.RC else Buf(R, M, c.p.dtype, c.p.T.contiguous(), ld=M + pad)
            Q = Buf(N, R, c.q.dtype, c.q, ld=R + pad) if ql == G.RC else Buf(R, N, c.q.dtype, c.qT, ld=N + pad)
            b = _vec(N, c.bias)
            C = Buf(M, N, odt, ld=N + pad, off=c_off)
            L.call("vit_gemm", L.dt(c.p), L.dt(C.v), pl, ql, L.EPI_STORE, M, N, R, P.ptr, P.ld, Q.ptr, Q.ld, C.ptr, C.ld,
                   b.ptr, None, 0, None, allow_fast, _stream())
            w = f"{what} layouts {pl}{ql} {M}x{N}x{R} pad {pad}"
            _settle(w, outs=[C], ins=[P, Q, b])
            _exact(C, c.pre, w)


def test_f32_mfma_every_layout():
    _gemm_layouts(G.mm_case(*G.F32_MFMA, F32), F32, 4, what="f32 mfma")


def test_f32_stream_k_and_the_plain_launch_after_removing_the_workspace():
    c = G.mm_case(*G.F32_STREAMK, F32)
    M, N, K = c.M, c.N, c.R
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    g = 2 * cus
    side = torch.cuda.Stream()
    part = torch.zeros(g * 2 * 128 * 128, dtype=F32, device=DEV)
    cnt = torch.zeros(g, dtype=torch.int32, device=DEV)
    x, w, b = Buf(M, K, F32, c.p, ld=K + 4), Buf(N, K, F32, c.q), _vec(N, c.bias)
    ref = c.pre.float().to(DEV)
    torch.cuda.synchronize()
    try:
        for registered in (True, False):
            if registered:
                L.call("vit_gemm_streamk_workspace", side.cuda_stream, part.data_ptr(), part.numel() * 4, cnt.data_ptr(), g)
            else:
                L.call("vit_gemm_streamk_workspace", side.cuda_stream, None, 0, None, 0)
            y = Buf(M, N, F32, ld=N + 4)
            torch.cuda.synchronize()   # the fill ran on the current stream, the GEMM runs on `side`
            L.call("vit_linear_fwd", L.F32, L.F32, L.EPI_STORE, M, N, K, x.ptr, x.ld, w.ptr, b.ptr, y.ptr, y.ld, None, None,
                   side.cuda_stream)
            what = f"stream-K case, workspace registered={registered}"
            _settle(what, outs=[y], ins=[x, w, b])
            assert torch.equal(_raw(y.v.contiguous()), _raw(ref)), what + ": not the exact result"
            assert int(cnt.abs().sum()) == 0, "the stream-K counters must come back zero"
    finally:
        L.call("vit_gemm_streamk_workspace", side.cuda_stream, None, 0, None, 0)


# ---------------------------------------------------------------------------- generic kernel

@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("shape", G.GEN_SHAPES, ids=str)
def test_generic_kernel_every_layout_odd_strides_and_bases(shape, dtype):
    c = G.mm_case(*shape, dtype)
    _gemm_layouts(c, dtype, 3, c_off=OFF + 1, what="generic")
    _gemm_layouts(c, F32, 5, what="generic f32 out")
    _gemm_layouts(G.mm_case(*G.G4_SHAPES[1], dtype) if shape == G.GEN_SHAPES[1] else c, dtype, 8, allow_fast=0,
                  what="generic by allow_fast=0")


# ---------------------------------------------------------------------------- patch embedding

@pytest.mark.parametrize("B,np_,D,K", G.PATCH)
def test_patch_embedding_skips_the_class_token_rows(B, np_, D, K):
    """ABI 7's contract keeps ZEROS in the pad columns of U and W (they are part of the reduction on the padded
    MFMA path); rows past the operands and the space around them are NaN."""
    c = G.patch_case(B, np_, D, K)
    ldu = K + 8
    U, W = Buf(B * np_, K, BF, c.U, ld=ldu), Buf(D, K, BF, c.W, ld=ldu)
    for t in (U, W):
        t.buf[t.off:t.off + t.rows * t.ld].view(t.rows, t.ld)[:, K:] = 0
        t.snap = t.buf.clone()
    b, pos = _vec(D, c.bias), Buf(np_ + 1, D, F32, c.pos)
    x = Buf(B * (np_ + 1), D, F32)
    L.call("vit_patch_embed_fwd_ld", L.BF16, B, np_, D, K, U.ptr, U.ld, W.ptr, W.ld, b.ptr, pos.ptr, x.ptr, _stream())
    what = f"patch embed K={K}"
    _settle(what, outs=[x], ins=[U, W, b, pos])
    tok = x.v.view(B, np_ + 1, D)
    assert bool((tok[:, 0] == SENT).all()), what + ": a class-token row was written"
    got = tok[:, 1:].cpu()
    assert torch.equal(_raw(got.contiguous()), _raw(c.rows.float().contiguous())), what + ": patch rows"


# ---------------------------------------------------------------------------- vit_gemm_splitk, vit_colsum

def test_splitk_with_strided_operands():
    c = G.mm_case(*G.SPLITK, F32)
    M, N, R = G.SPLITK
    for pl, ql in ((G.CR, G.CR), (G.RC, G.RC)):
        P = Buf(M, R, F32, c.p, ld=R + 4) if pl == G.RC else Buf(R, M, F32, c.p.T.contiguous(), ld=M + 4)
        Q = Buf(N, R, F32, c.q, ld=R + 4) if ql == G.RC else Buf(R, N, F32, c.qT, ld=N + 4)
        C, slabs = Buf(M, N, F32), _vec(4 * M * N)
        L.call("vit_gemm_splitk", pl, ql, M, N, R, P.ptr, P.ld, Q.ptr, Q.ld, C.ptr, slabs.ptr, 4 * M * N, _stream())
        _settle(f"splitk {pl}{ql}", outs=[C, slabs], ins=[P, Q])
        _exact(C, c.acc, f"splitk {pl}{ql}")
        assert torch.equal(slabs.v.view(4, M * N).double().sum(0).cpu(), c.acc.reshape(-1)), "slab total"


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
def test_colsum_with_a_partial_buffer_of_exactly_the_documented_size(dtype):
    M, N = G.COLSUM
    xs = G.sixteenths(M, N, dtype)
    ref = xs.double().sum(0)
    for S in (1, 5, 300):   # partial rows the buffer has room for: S * N floats, then the guard
        x, out, part = Buf(M, N, dtype, xs, ld=N + 8), _vec(N), _vec(S * N)
        L.call("vit_colsum", L.dt(xs), M, N, x.ptr, x.ld, out.ptr, part.ptr, S * N, 0, _stream())
        _settle(f"colsum S={S}", outs=[out, part], ins=[x])
        _exact(out, ref, f"colsum S={S}")
        out.set(torch.full((N,), 2.0))
        L.call("vit_colsum", L.dt(xs), M, N, x.ptr, x.ld, out.ptr, part.ptr, S * N, 1, _stream())
        _settle(f"colsum accumulate S={S}", outs=[out, part], ins=[x])
        _exact(out, ref + 2.0, f"colsum accumulate S={S}")


# ---------------------------------------------------------------------------- contracts that launch nothing

def test_refused_calls_launch_nothing():
    lib, s = L.lib(), _stream()
    c = G.wg_case(50, *G.WGRAD_NK[0])
    (dy, x), n = _wg_bufs(c), c.N * c.K
    sa, sb = _vec(n), _vec(n)
    assert lib.vit_linear_wgrad_partials2(50, 1, c.N, c.K, dy.ptr, dy.ld, x.ptr, x.ld, sa.ptr, n * 4, c.N, c.K, dy.ptr, dy.ld,
                                          x.ptr, x.ld, sb.ptr, n * 4, s) == INVALID
    dW, ws = _vec(n), _vec(3 * n)
    assert lib.vit_linear_wgrad(L.BF16, 50, c.N, c.K, dy.ptr, dy.ld, x.ptr, x.ld, dW.ptr, 3, ws.ptr, 3 * n * 4 - 4, s) == INVALID
    assert lib.vit_linear_wgrad(L.BF16, 50, c.N, c.K, dy.ptr, dy.ld, x.ptr, x.ld, dW.ptr, 3, None, 0, s) == INVALID
    m = G.mm_case(*G.ACT_BWD_SHAPES[0])
    aux = G.sixteenths(m.M, m.N)
    p, qT, ax = Buf(m.M, m.R, BF, m.p), Buf(m.R, m.N, BF, m.qT), Buf(m.M, m.N, BF, aux)
    dx, db = Buf(m.M, m.N, BF), _vec(m.N)
    pf = lib.vit_linear_dgrad_partial_floats(m.M, m.N)
    part = _vec(pf)
    assert lib.vit_linear_dgrad(L.BF16, L.BF16, L.EPI_GELU_BWD, m.M, m.R, m.N, p.ptr, p.ld, qT.ptr, dx.ptr, dx.ld, ax.ptr,
                                db.ptr, part.ptr, pf - 1, 0, s) == INVALID
    y = Buf(m.M, m.N, BF)
    b = _vec(m.N, m.bias)
    q = Buf(m.N, m.R, BF, m.q)
    for pl, ql in ((G.RC, G.CR), (G.CR, G.CR), (G.CR, G.RC)):
        for epi in (L.EPI_BIAS_GELU_FWD, L.EPI_BIAS_QGELU_FWD):
            assert lib.vit_gemm(L.BF16, L.BF16, pl, ql, epi, m.M, m.N, m.R, p.ptr, p.ld, q.ptr, q.ld, y.ptr, y.ld, b.ptr, None, 0,
                                None, 1, s) == INVALID
    # empty problems: 0, nothing written
    assert lib.vit_linear_fwd(L.BF16, L.BF16, L.EPI_STORE, 0, m.N, m.R, p.ptr, p.ld, q.ptr, b.ptr, y.ptr, y.ld, None, None, s) == 0
    assert lib.vit_linear_fwd(L.BF16, L.BF16, L.EPI_STORE, m.M, 0, m.R, p.ptr, p.ld, q.ptr, b.ptr, y.ptr, y.ld, None, None, s) == 0
    assert lib.vit_linear_dgrad(L.BF16, L.BF16, L.EPI_STORE, 0, m.R, m.N, p.ptr, p.ld, qT.ptr, dx.ptr, dx.ld, None, None, None,
                                0, 0, s) == 0
    _settle("refused calls", ins=[dy, x, p, q, qT, ax, b], idle=[sa, sb, dW, ws, dx, db, part, y])


def test_zz_worst_fraction_of_the_activation_bound():
    print(f"worst fraction of the activation bound: {WORST['f']:.3f} ({WORST['what']})")
    assert WORST["f"] <= 1.0
