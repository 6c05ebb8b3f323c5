"""GPU: the row kernels of norm.hip, misc.hip and clip.hip and the SGD kernel on every dispatch branch, against
the float64 references of oracle/row_cases.py.

Bounds are the project's (f32 1e-5 of the reference's largest magnitude, bf16 out 8e-3 for LayerNorm and 1e-2
elsewhere, 1e-6 for the optimizer, 0 for copies and single f32 adds); on the ``offset`` / ``outlier`` / ``wide``
kinds an output's bound is 4x the error torch float32 makes on it if that is larger (row_cases, asserted reachable
in tests/test_row_cases_host.py).  Every strided or offset case lives in a buffer filled with a sentinel, and
everything outside the view must come back bitwise unchanged.  The LayerNorm backward is fed the reference's mean
and rstd rounded to f32, not the forward kernel's.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import row_cases as RC  # noqa: E402
from vit_amd import _lib as L  # noqa: E402
from vit_amd import ops  # noqa: E402
from vit_amd._lib import call, ptr  # noqa: E402

DEV = "cuda"
F32, BF = torch.float32, torch.bfloat16
SENT = 640.0   # exact in f32 and bf16, far from every value the cases produce
PAD = 5        # sentinel elements after the last row


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    L.load()


class Buf:
    """A [rows, cols] view with row stride ``ld`` that starts ``off`` elements into a sentinel-filled buffer."""

    def __init__(self, rows, cols, ld=None, off=0, dtype=F32, src=None):
        self.rows, self.cols, self.ld, self.off = rows, cols, cols if ld is None else ld, off
        assert self.ld >= cols
        self.buf = torch.full((off + rows * self.ld + PAD,), SENT, dtype=dtype, device=DEV)
        self.v = self.buf[off:off + rows * self.ld].view(rows, self.ld)[:, :cols]
        if src is not None:
            self.v.copy_(src.reshape(rows, cols))

    @property
    def flat(self):
        """The view as a 1-D tensor (one row, or contiguous rows)."""
        assert self.rows == 1 or self.ld == self.cols
        return self.buf[self.off:self.off + self.rows * self.cols]

    def outside_untouched(self, what=""):
        m = torch.ones(self.buf.numel(), dtype=torch.bool, device=DEV)
        m[self.off:self.off + self.rows * self.ld].view(self.rows, self.ld)[:, :self.cols] = False
        assert bool((self.buf[m] == SENT).all()), f"{what}: wrote outside its [{self.rows}, {self.cols}] view"


def _stream():
    return L.stream_ptr(DEV)


def _rand(seed, *shape, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def _same_bits(got, want, what=""):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert torch.equal(_bits(got), _bits(want)), f"{what}: not bitwise equal"


def _within(got, ref, bound, what):
    e = RC.rel_max(got, ref)
    print(f"{what}: {e:.2e} (bound {bound:.1e})")
    assert e <= bound, f"{what}: {e:.3e} > {bound:.1e}"


# ---------------------------------------------------------------------------- LayerNorm forward

def _ln_fwd(c, ydt=F32, ldx=None, ldy=None, offx=0, offy=0, need_stats=True, what=""):
    x = Buf(c.rows, c.D, ldx, offx, c.x.dtype, c.x)
    y = Buf(c.rows, c.D, ldy, offy, ydt)
    mean, rstd = Buf(1, c.rows), Buf(1, c.rows)
    xin = x.buf.clone()
    ops.layer_norm_fwd(x.v, c.w.to(DEV), c.b.to(DEV), c.eps, ydt, rows=c.rows, ldx=x.ld, out=y.v,
                       need_stats=need_stats, mean=mean.flat if need_stats else None,
                       rstd=rstd.flat if need_stats else None)
    torch.cuda.synchronize()
    what = f"ln fwd {c.kind} {c.rows}x{c.D} {c.x.dtype}->{ydt} eps {c.eps} {what}"
    _within(y.v, c.ref["y"], c.bound("y", RC.F32 if ydt == F32 else RC.BF16_LN), what + " y")
    if need_stats:
        _within(mean.flat, c.ref["mean"], c.bound("mean"), what + " mean")
        _within(rstd.flat, c.ref["rstd"], c.bound("rstd"), what + " rstd")
    else:
        assert bool((mean.buf == SENT).all()) and bool((rstd.buf == SENT).all())
    if c.kind == "const":
        _same_bits(y.v, c.b.to(ydt).expand(c.rows, c.D), what + " const y == b")
        if need_stats:
            assert bool((mean.flat == RC.CONST).all())
            _within(rstd.flat, torch.full((c.rows,), c.eps ** -0.5, dtype=torch.float64), RC.F32, what + " eps^-1/2")
    for b_, n in ((y, "y"), (mean, "mean"), (rstd, "rstd")):
        b_.outside_untouched(what + " " + n)
    assert torch.equal(x.buf, xin), what + ": the input changed"
    return y


@pytest.mark.parametrize("D", RC.LN_FWD_VEC_D + RC.LN_FWD_SCALAR_D)
def test_ln_fwd_every_width_and_row_count(D):
    """NV = 1, 2, 3, 4, 6, 8 and the scalar kernel (NV 5 and 7 have no forward instance; ragged D), with 1 to 37
    rows: a last workgroup of 1, 3 and 4 waves."""
    for rows in RC.LN_FWD_ROWS:
        _ln_fwd(RC.ln_case("base", rows, D))


@pytest.mark.parametrize("D", RC.LN_KIND_D)
@pytest.mark.parametrize("xdt,ydt", [(F32, F32), (F32, BF), (BF, BF), (BF, F32)])
def test_ln_fwd_dtype_pairs(D, xdt, ydt):
    _ln_fwd(RC.ln_case("base", 5, D, xdt, xdt), ydt)


@pytest.mark.parametrize("D", RC.LN_KIND_D)
@pytest.mark.parametrize("kind", RC.LN_KINDS)
def test_ln_fwd_hard_inputs(kind, D):
    for eps in RC.LN_EPS.get(kind, (1e-6,)):
        for xdt, ydt in ((F32, F32), (BF, BF)):
            _ln_fwd(RC.ln_case(kind, 5, D, xdt, xdt, eps), ydt)


@pytest.mark.parametrize("D", RC.LN_KIND_D)
def test_ln_fwd_strided_views(D):
    """The class-token call (rows = B, ldx = N * D), a padded output, a stride that is no multiple of 4 (scalar
    kernel at a vector width) and need_stats=False."""
    c = RC.ln_case("base", 5, D)
    _ln_fwd(c, ldx=3 * D, what="ldx=3D")
    _ln_fwd(c, ldy=D + 4, what="ldy=D+4")
    _ln_fwd(c, BF, ldx=3 * D, ldy=D + 8, what="both")
    _ln_fwd(c, ldx=D + 2, what="ldx=D+2")
    _ln_fwd(c, BF, ldy=D + 2, what="ldy=D+2")
    _ln_fwd(c, need_stats=False, what="no stats")
    _ln_fwd(RC.ln_case("base", 5, D, BF, BF), BF, ldx=3 * D, need_stats=False, what="bf16 no stats")


def test_ln_fwd_widest_row_on_the_scalar_kernel_and_past_it():
    D, ld = RC.LN_FWD_LAST_SLOT
    _ln_fwd(RC.ln_case("base", 5, D), ldx=ld, what="last scalar slot")
    w = torch.ones(RC.LN_MAX_D + 1, device=DEV)
    x = torch.zeros(2, RC.LN_MAX_D + 1, device=DEV)
    with pytest.raises(L.HipError):
        ops.layer_norm_fwd(x, w, w, 1e-6, F32)


@pytest.mark.parametrize("xdt,ydt", [(F32, F32), (BF, BF)])
def test_ln_fwd_offset_base_pointers(xdt, ydt):
    """A base pointer one element into an aligned buffer, strides still multiples of 4: the scalar kernel, same
    bounds."""
    c = RC.ln_case("base", 5, 768, xdt, xdt)
    _ln_fwd(c, ydt, ldx=772, offx=1, what="x+1")
    _ln_fwd(c, ydt, ldy=772, offy=1, what="y+1")
    _ln_fwd(c, ydt, offx=3, offy=2, what="x+3 y+2")
    # gamma / beta one element in
    wb = Buf(1, 768, off=1, src=c.w), Buf(1, 768, off=1, src=c.b)
    for w_, b_ in ((wb[0].flat, c.b.to(DEV)), (c.w.to(DEV), wb[1].flat)):
        y, mean, rstd = ops.layer_norm_fwd(c.x.to(DEV), w_, b_, c.eps, ydt)
        _within(y, c.ref["y"], RC.F32 if ydt == F32 else RC.BF16_LN, "ln fwd w/b+1")
        _within(mean, c.ref["mean"], RC.F32, "ln fwd w/b+1 mean")
        _within(rstd, c.ref["rstd"], RC.F32, "ln fwd w/b+1 rstd")


# ---------------------------------------------------------------------------- residual add + LayerNorm

def _add_ln(c, ydt=BF, ld=(None,) * 4, inplace=False, add_only=False, what=""):
    ldx, ldr, ldxs, ldy = ld
    x = Buf(c.rows, c.D, ldx, 0, F32, c.x)
    r = Buf(c.rows, c.D, ldr, 0, c.r.dtype, c.r)
    xs = x if inplace else Buf(c.rows, c.D, ldxs)
    y = Buf(c.rows, c.D, ldy, 0, ydt)
    mean, rstd = Buf(1, c.rows), Buf(1, c.rows)
    if add_only:
        ops.add_layer_norm_fwd(x.v, r.v, xs.v)
    else:
        ops.add_layer_norm_fwd(x.v, r.v, xs.v, c.w.to(DEV), c.b.to(DEV), c.eps, out=y.v, mean=mean.flat, rstd=rstd.flat)
    torch.cuda.synchronize()
    what = f"add_ln {c.kind} {c.rows}x{c.D} r {c.r.dtype} y {ydt} {what}"
    _same_bits(xs.v, c.s, what + " sum")
    if add_only:
        assert bool((y.buf == SENT).all()) and bool((mean.buf == SENT).all())
    else:
        _within(y.v, c.ref["y"], c.bound("y", RC.F32 if ydt == F32 else RC.BF16_LN), what + " y")
        _within(mean.flat, c.ref["mean"], c.bound("mean"), what + " mean")
        _within(rstd.flat, c.ref["rstd"], c.bound("rstd"), what + " rstd")
    for b_, n in ((xs, "xs"), (y, "y"), (mean, "mean"), (rstd, "rstd"), (r, "r")):
        b_.outside_untouched(what + " " + n)
    if not inplace:
        _same_bits(x.v, c.x, what + " x")


@pytest.mark.parametrize("D", RC.ADD_LN_D)
def test_add_ln_every_width(D):
    for rows in RC.ADD_LN_ROWS:
        _add_ln(RC.add_ln_case("base", rows, D, BF))
    for rdt, ydt in ((BF, F32), (F32, BF), (F32, F32)):
        _add_ln(RC.add_ln_case("base", 5, D, rdt), ydt)
    for kind in RC.ADD_LN_KINDS:
        _add_ln(RC.add_ln_case(kind, 5, D, F32), F32)
        _add_ln(RC.add_ln_case(kind, 5, D, BF), BF)


@pytest.mark.parametrize("D", [768, 1280])
def test_add_ln_strides_in_place_and_add_only(D):
    c = RC.add_ln_case("base", 5, D, BF)
    for i in range(4):
        _add_ln(c, ld=tuple(D + 4 * (j + 1) if j == i else None for j in range(4)), what=f"ld[{i}]")
    _add_ln(c, ld=(3 * D, D + 8, 3 * D, D + 4), inplace=True, what="in place")
    _add_ln(c, inplace=True, add_only=True, what="in place, add only")
    _add_ln(c, ld=(None, D + 4, D + 8, None), add_only=True, what="add only")


def test_add_ln_rejects_what_it_has_no_kernel_for():
    """No scalar kernel here: another width, a stride that is no multiple of 4 and a misaligned base are errors."""
    c = RC.add_ln_case("base", 5, 200, BF)
    with pytest.raises(L.HipError):
        _add_ln(c)
    c = RC.add_ln_case("base", 5, 768, BF)
    for i in range(4):
        with pytest.raises(L.HipError):
            _add_ln(c, ld=tuple(768 + 2 if j == i else None for j in range(4)))
    mean, rstd = torch.empty(5, device=DEV), torch.empty(5, device=DEV)
    for which in ("x", "r", "xs", "y", "w", "b"):
        off = {k: int(k == which) for k in ("x", "r", "xs", "y", "w", "b")}
        x, r = Buf(5, 768, 772, off["x"], F32, c.x), Buf(5, 768, 772, off["r"], BF, c.r)
        xs, y = Buf(5, 768, 772, off["xs"]), Buf(5, 768, 772, off["y"], BF)
        w_, b_ = Buf(1, 768, off=off["w"], src=c.w), Buf(1, 768, off=off["b"], src=c.b)
        with pytest.raises(L.HipError):
            ops.add_layer_norm_fwd(x.v, r.v, xs.v, w_.flat, b_.flat, c.eps, out=y.v, mean=mean, rstd=rstd)
        torch.cuda.synchronize()
        assert bool((xs.buf == SENT).all()) and bool((y.buf == SENT).all()), which
    with pytest.raises(L.HipError):  # add only: x, r and xs still count
        ops.add_layer_norm_fwd(Buf(5, 768, 772, 1, F32, c.x).v, c.r.to(DEV), torch.empty(5, 768, device=DEV))


# ---------------------------------------------------------------------------- LayerNorm backward

def _bwd_rows():
    """Row counts that give a wave of one block 0, 1, 2 and 3 rows (odd and even trips of the 2x unrolled loop,
    its break in the middle), one full block, and ragged second and fifth blocks."""
    R = ops.ln_bwd_rows_per()
    if R == 32:
        return RC.LN_BWD_ROWS
    return (1, 4, 5, 8, 9, 12, 13, R, R + 1, R + 5, 4 * R + 2)


class _Inline:
    """A reduce_on object: runs the deferred reduction at once, on the current stream."""

    def __init__(self):
        self.calls = 0

    def run(self, fn):
        self.calls += 1
        fn()


def _ln_bwd(c, copy_dt=BF, dres=None, res_every=0, compact_np=0, outs=("dgamma", "dbeta", "dsum"), ldx=None,
            lddy=None, lddx=None, ld_copy=None, ldres=None, off=None, reduce_on=None, what=""):
    rows, D = c.rows, c.D
    off = off or {}
    x = Buf(rows, D, ldx, off.get("x", 0), c.x.dtype, c.x)
    dy = Buf(rows, D, lddy, off.get("dy", 0), c.dy.dtype, c.dy)
    mean, rstd = (t.to(DEV) for t in c.stats_f32())
    w = Buf(1, D, off=off.get("w", 0), src=c.w)
    dres_full = torch.zeros(rows, D, dtype=torch.float64)
    res = None
    if dres == "dense":
        r = _rand(61 + rows, rows, D)
        res = Buf(rows, D, ldres, off.get("dres", 0), F32, r)
        dres_full = r.double()
    elif dres == "compact":
        nr = (rows + res_every - 1) // res_every
        r = _rand(62 + rows, nr, D)
        res = Buf(nr, D, ldres, off.get("dres", 0), F32, r)
        dres_full = RC.spread_rows(r, res_every, rows).double()
    dx = Buf(rows, D, lddx, off.get("dx", 0))
    dx_ref = c.ref["dx"] + dres_full
    copy_ref = RC.compact_rows(dx_ref, compact_np) if compact_np else dx_ref
    copy = Buf(copy_ref.shape[0], D, ld_copy, off.get("copy", 0), copy_dt) if copy_dt is not None else None
    red = {n: Buf(1, D) for n in ("dgamma", "dbeta", "dsum")}
    ins = [(b_, b_.buf.clone()) for b_ in (x, dy, w) + ((res,) if res is not None else ())]
    ops.layer_norm_bwd(x.v, x.ld, dy.v, w.flat, mean, rstd, dx.v, dx.ld, rows,
                       dres=res.v if res is not None else None, ldres=res.ld if res is not None else 0,
                       dx_copy=copy.v if copy is not None else None, ld_copy=copy.ld if copy is not None else 0,
                       compact_np=compact_np, dgamma=red["dgamma"].flat if "dgamma" in outs else None,
                       dbeta=red["dbeta"].flat if "dbeta" in outs else None,
                       dsum=red["dsum"].flat if "dsum" in outs else None, reduce_on=reduce_on, res_every=res_every)
    torch.cuda.synchronize()
    what = (f"ln bwd {c.kind} {rows}x{D} x {c.x.dtype} dy {c.dy.dtype} copy {copy_dt} dres {dres} every {res_every} "
            f"np {compact_np} outs {outs} {what}")
    plain = dres is None
    _within(dx.v, dx_ref, c.bound("dx") if plain else RC.F32, what + " dx")
    if copy is not None:
        _within(copy.v, copy_ref, (c.bound("dx", RC.F32 if copy_dt == F32 else RC.BF16_LN) if plain
                                   else RC.F32 if copy_dt == F32 else RC.BF16_LN), what + " copy")
        got_dx = dx.v.cpu()
        _same_bits(copy.v, (RC.compact_rows(got_dx, compact_np) if compact_np else got_dx).to(copy_dt),
                   what + " copy is dx in its dtype")
        copy.outside_untouched(what + " copy")
    for n in ("dgamma", "dbeta", "dsum"):
        if n in outs:
            ref = dx_ref.sum(0) if n == "dsum" else c.ref[n]
            _within(red[n].flat, ref, c.bound(n) if plain or n != "dsum" else RC.F32, what + " " + n)
            red[n].outside_untouched(what + " " + n)
        else:
            assert bool((red[n].buf == SENT).all()), what + f": wrote {n} unasked"
    dx.outside_untouched(what + " dx")
    for b_, before in ins:
        assert torch.equal(b_.buf, before), what + ": an input changed"


@pytest.mark.parametrize("variant", [1, 0])
@pytest.mark.parametrize("D", RC.LN_BWD_PIPE_D)
def test_ln_bwd_vector_kernels_every_row_count(D, variant):
    try:
        L.lib().vit_layer_norm_bwd_variant(variant)
        for rows in _bwd_rows():
            _ln_bwd(RC.ln_case("base", rows, D), dres="dense", what=f"variant {variant}")
    finally:
        L.lib().vit_layer_norm_bwd_variant(1)


@pytest.mark.parametrize("D", RC.LN_BWD_SCALAR_D)
def test_ln_bwd_scalar_kernel_every_row_count(D):
    for rows in _bwd_rows():
        _ln_bwd(RC.ln_case("base", rows, D), dres="dense")


@pytest.mark.parametrize("variant", [1, 0])
@pytest.mark.parametrize("D", RC.LN_KIND_D)
def test_ln_bwd_dtype_triples(D, variant):
    try:
        L.lib().vit_layer_norm_bwd_variant(variant)
        for xdt in (F32, BF):
            for dyt in (F32, BF):
                for cdt in (F32, BF):
                    _ln_bwd(RC.ln_case("base", 13, D, xdt, dyt), cdt, dres="dense")
    finally:
        L.lib().vit_layer_norm_bwd_variant(1)


@pytest.mark.parametrize("D", RC.LN_KIND_D)
@pytest.mark.parametrize("kind", RC.LN_KINDS)
def test_ln_bwd_hard_inputs(kind, D):
    for eps in RC.LN_EPS.get(kind, (1e-6,)):
        _ln_bwd(RC.ln_case(kind, 13, D, F32, F32, eps), F32)
        _ln_bwd(RC.ln_case(kind, 13, D, BF, BF, eps), BF)


@pytest.mark.parametrize("variant", [1, 0])
@pytest.mark.parametrize("D", RC.LN_KIND_D)
def test_ln_bwd_residual_forms_and_output_subsets(D, variant):
    """dres absent / dense with a padded stride / compact (res_every = 5 at 13 and 37 rows: a ragged last image);
    compact_np = 4 at 15 and 35 rows with the reductions on; the four output subsets, where ``dsum`` alone puts its
    partials behind the two absent matrices."""
    try:
        L.lib().vit_layer_norm_bwd_variant(variant)
        c = RC.ln_case("base", 37, D)
        _ln_bwd(c)
        _ln_bwd(c, dres="dense", ldres=D + 4)
        _ln_bwd(c, copy_dt=None, dres="dense")
        every, at = RC.LN_BWD_RES_EVERY
        for rows in at:
            _ln_bwd(RC.ln_case("base", rows, D), dres="compact", res_every=every)
            _ln_bwd(RC.ln_case("base", rows, D), F32, dres="compact", res_every=every, ldres=D + 8, outs=("dsum",))
        np_, at = RC.LN_BWD_COMPACT_NP
        for rows in at:
            _ln_bwd(RC.ln_case("base", rows, D), compact_np=np_, dres="dense")
            _ln_bwd(RC.ln_case("base", rows, D), F32, compact_np=np_, dres="compact", res_every=np_ + 1)
        for outs in (("dgamma", "dbeta", "dsum"), ("dgamma", "dbeta"), ("dsum",), ()):
            _ln_bwd(c, dres="dense", outs=outs)
            _ln_bwd(RC.ln_case("base", 37, D, BF, BF), F32, outs=outs)
    finally:
        L.lib().vit_layer_norm_bwd_variant(1)


@pytest.mark.parametrize("D", RC.LN_KIND_D)
def test_ln_bwd_strided_views_and_deferred_reduce(D):
    """The class-token layout (ldx = lddx = ld_copy = 3 * D, 7 rows), lddy = D + 2 (the scalar kernel at a vector
    width) and the reductions issued through a reduce_on object."""
    c = RC.ln_case("base", 7, D, BF, BF)
    _ln_bwd(c, BF, dres="dense", ldx=3 * D, lddx=3 * D, ld_copy=3 * D, what="class-token layout")
    _ln_bwd(RC.ln_case("base", 7, D), F32, dres="dense", ldx=3 * D, lddx=3 * D, ld_copy=3 * D, ldres=3 * D)
    _ln_bwd(RC.ln_case("base", 37, D), dres="dense", lddy=D + RC.LN_BWD_ODD_LD, what="lddy=D+2")
    _ln_bwd(RC.ln_case("base", 37, D), dres="dense", ld_copy=D + 2, lddx=D + 4, what="ld_copy=D+2")
    for outs in (("dgamma", "dbeta", "dsum"), ("dsum",)):
        r = _Inline()
        _ln_bwd(RC.ln_case("base", 37, D), dres="dense", outs=outs, reduce_on=r, what="reduce_on")
        assert r.calls == 1


@pytest.mark.parametrize("which,dt", [("x", F32), ("x", BF), ("dy", F32), ("dy", BF), ("copy", F32), ("copy", BF),
                                      ("w", F32), ("dres", F32), ("dx", F32)])
def test_ln_bwd_offset_base_pointers(which, dt):
    """One base pointer one element into an aligned buffer, strides multiples of 4: the scalar kernel, same bounds."""
    c = RC.ln_case("base", 37, 768, dt, dt)
    _ln_bwd(c, dt, dres="dense", ldx=772, lddy=772, lddx=772, ld_copy=772, ldres=772, off={which: 1},
            what=f"{which}+1")


# ---------------------------------------------------------------------------- cross-entropy

def _ce_bwd(c, logits, tgt, lse, g, odt, ldd):
    d = Buf(c.B, c.C, ldd, 0, odt)
    call("vit_cross_entropy_bwd", L.dt(d.v), c.B, c.C, ptr(logits.v), logits.ld, ptr(tgt), ptr(lse),
         ptr(g), ptr(d.v), d.ld, _stream())
    torch.cuda.synchronize()
    d.outside_untouched("dlogits")
    return d.v


@pytest.mark.parametrize("B,C", RC.CE_SHAPES)
@pytest.mark.parametrize("kind", RC.CE_KINDS)
def test_cross_entropy_every_kind_and_shape(kind, B, C):
    c = RC.ce_case(kind, B, C)
    tgt = c.target.to(DEV)
    lse_ref = c.ref["lse"].float().to(DEV)
    for ld in (C, C + RC.CE_LD_PAD):
        logits = Buf(B, C, ld, 0, F32, c.logits)
        loss, lse = ops.cross_entropy_fwd(logits.v, tgt)
        what = f"ce {kind} {B}x{C} ld {ld}"
        _within(loss.reshape(1), c.ref["loss"], c.bound("loss"), what + " loss")
        _within(lse, c.ref["lse"], c.bound("lse"), what + " lse")
        for g in (0.5, None):
            gt = torch.tensor(g, device=DEV) if g is not None else None
            ref = c.ref["d"] * (g if g is not None else 1.0)
            # through the wrapper (contiguous gradient) with the kernel's own lse, as the model does
            _within(ops.cross_entropy_bwd(logits.v, tgt, lse, gt), ref, c.bound("d"), what + f" d g {g}")
            # the backward alone, from the reference's lse, into a padded gradient
            for odt, bound in ((F32, c.bound("d")), (BF, c.bound("d", RC.BF16))):
                for ldd in (C, C + 5):
                    d = _ce_bwd(c, logits, tgt, lse_ref, gt, odt, ldd)
                    _within(d, ref, bound, what + f" d {odt} ldd {ldd} g {g}")
        logits.outside_untouched(what)
        _same_bits(logits.v, c.logits, what + " logits")


# ---------------------------------------------------------------------------- cast, pos_grad, fills, unfold

@pytest.mark.parametrize("n", RC.CAST_N)
@pytest.mark.parametrize("offs", [(0, 0), (1, 0), (0, 1), (3, 3)])
def test_cast_f32_bf16_is_round_to_nearest_even(n, offs):
    """Bitwise ``x.to(bfloat16)`` on ties, zeros, denormals, the overflow to inf, infs and NaNs; aligned (vector
    kernel and its tail) and with the source / the destination / both one or three elements in (scalar kernel)."""
    x = RC.cast_input(n)
    src = Buf(1, n, off=offs[0], src=x)
    dst = Buf(1, n, off=offs[1], dtype=BF)
    ops.cast_bf16(src.flat, dst.flat)
    torch.cuda.synchronize()
    want, got = x.to(BF), dst.flat.cpu()
    nan = torch.isnan(x)
    assert torch.equal(torch.isnan(got.float()), nan), "NaN must stay NaN and nothing else become one"
    _same_bits(torch.where(nan, torch.zeros_like(got), got), torch.where(nan, torch.zeros_like(want), want), f"cast {n}")
    dst.outside_untouched(f"cast {n} {offs}")
    _same_bits(src.flat, x, "cast source")


@pytest.mark.parametrize("S,D", RC.POS_SD)
def test_pos_grad_every_batch_split(S, D):
    """The 8 waves and the four-accumulator stride of 32 images; (3, 6) and (2, 1) take the scalar kernel."""
    for B in RC.POS_B:
        dx = RC.pos_grad_inputs(B, S, D)
        ref = dx.double().sum(0).reshape(-1)
        dxd = dx.to(DEV)
        for with_cls in (True, False):
            runs = []
            for _ in range(2):
                dpos, dcls = Buf(1, S * D), Buf(1, D)
                ops.pos_grad(dxd, B, S, D, dpos.flat, dcls.flat if with_cls else None)
                torch.cuda.synchronize()
                dpos.outside_untouched("dpos")
                dcls.outside_untouched("dcls")
                runs.append((dpos.flat.clone(), dcls.buf.clone()))
            _within(runs[0][0], ref, RC.F32, f"pos_grad B {B} S {S} D {D}")
            if with_cls:
                _same_bits(runs[0][1][:D], runs[0][0][:D], "dcls is dpos[0]")
            else:
                assert bool((runs[0][1] == SENT).all())
            _same_bits(runs[0][0], runs[1][0], "pos_grad twice")
            _same_bits(runs[0][1], runs[1][1], "dcls twice")


def test_cls_pos_fill_writes_row_zero_of_each_image():
    B, S, D = 3, 5, 200
    cls, pos = _rand(3, D), _rand(4, S, D)
    x = Buf(B * S, D)
    cls_d, pos_d = cls.to(DEV), pos.to(DEV)  # held: a temporary's memory is handed to the next one
    call("vit_cls_pos_fill", B, S, D, ptr(x.v), ptr(cls_d), ptr(pos_d), _stream())
    torch.cuda.synchronize()
    want = torch.full((B, S, D), SENT)
    want[:, 0] = cls + pos[0]
    _same_bits(x.v.reshape(B, S, D), want, "cls_pos_fill")
    x.outside_untouched("cls_pos_fill")


@pytest.mark.parametrize("dt", [F32, BF])
def test_pad_cols_pads_with_exact_zeros(dt):
    for rows, cols, ld_src, ld in ((5, 37, 41, 64), (3, 64, 200, 64), (1, 1, 3, 2), (7, 147, 147, 192)):
        w = _rand(5 + cols, rows, cols).to(dt)
        src = Buf(rows, cols, ld_src, 0, dt, w)
        out = Buf(rows, ld, dtype=dt)
        ops.pad_cols(src.v, ld, out=out.v)
        torch.cuda.synchronize()
        want = torch.zeros(rows, ld, dtype=dt)
        want[:, :cols] = w
        _same_bits(out.v, want, f"pad_cols {rows}x{cols}->{ld}")
        out.outside_untouched("pad_cols")


@pytest.mark.parametrize("ps", RC.UNFOLD_PS)
@pytest.mark.parametrize("dt", [F32, BF])
def test_patch_unfold_every_branch(ps, dt):
    """ps = 16 (bf16: the 16-byte stores), 8 (ps % 4 == 0), 14 and 6 (scalar), rows K wide and padded to 64."""
    B, C, Hi, Wi = 2, 3, 2 * ps, 3 * ps
    img = _rand(9 + ps, B, C, Hi, Wi)
    K = C * ps * ps
    want = img.unfold(2, ps, ps).unfold(3, ps, ps).permute(0, 2, 3, 1, 4, 5).reshape(B * 6, K).to(dt)
    img_d = img.to(DEV)
    for ld in (K, (K + 63) // 64 * 64 + (64 if K % 64 == 0 else 0)):
        U = Buf(B * 6, ld, dtype=dt)
        call("vit_patch_unfold_ld", L.dt(U.v), B, C, Hi, Wi, ps, ld, ptr(img_d), ptr(U.v), _stream())
        torch.cuda.synchronize()
        _same_bits(U.v[:, :K], want, f"unfold ps {ps} ld {ld}")
        assert bool((U.v[:, K:] == 0).all()), "padding columns must be exactly zero"
        U.outside_untouched("unfold")
    _same_bits(ops.patch_unfold(img_d, ps, dt), want, "ops.patch_unfold")


# ---------------------------------------------------------------------------- SGD

def _sgd_run(n, offp, offg, offs):
    from vit_amd.optim import FusedSGD
    p0, grads = RC.sgd_inputs(n)
    pb, gb, sb = Buf(1, n, off=offp, src=p0), Buf(1, n, off=offg), Buf(1, n, off=offs, dtype=BF)
    q = torch.nn.Parameter(pb.flat)
    assert q.data_ptr() == pb.flat.data_ptr()
    q._vit_shadow = sb.flat
    opt = FusedSGD([q], lr=0.1, momentum=0.9, weight_decay=1e-4)
    steps = []
    for g in grads:
        gb.flat.copy_(g)
        q.grad = gb.flat
        opt.step()
        torch.cuda.synchronize()
        assert q.grad.data_ptr() == gb.flat.data_ptr()
        _same_bits(sb.flat, pb.flat.to(BF), "shadow is p in bf16")
        steps.append((pb.flat.cpu().clone(), sb.flat.cpu().clone()))
        _same_bits(gb.flat, g, "the gradient is read only")
    buf = opt.state[q]["momentum_buffer"]
    assert buf.data_ptr() % 16 == 0  # as FusedSGD makes it: from the allocator
    for b_ in (pb, gb, sb):
        b_.outside_untouched(f"sgd n {n} offsets {offp, offg, offs}")
    return steps, buf.cpu().clone()


@pytest.mark.parametrize("n", RC.SGD_N)
def test_sgd_misaligned_views_match_aligned_bitwise(n):
    """The scalar branch of sgd_kernel (any of p, grad, shadow not aligned to 4 elements) runs the same rounded
    operations as the vector branch: bitwise equal, and both within 1e-6 of torch.optim.SGD."""
    p0, grads = RC.sgd_inputs(n)
    p = torch.nn.Parameter(p0.clone())
    ref_opt = torch.optim.SGD([p], lr=0.1, momentum=0.9, weight_decay=1e-4)
    ref = []
    for g in grads:
        p.grad = g.clone()
        ref_opt.step()
        ref.append(p.detach().clone())
    base, base_buf = _sgd_run(n, 0, 0, 0)
    for (got, _), want in zip(base, ref):
        _within(got, want, RC.OPT, f"sgd n {n} aligned")
    for offs in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (4, 4, 2)):
        steps, buf = _sgd_run(n, *offs)
        for k, ((got, sh), (bp, bsh), want) in enumerate(zip(steps, base, ref)):
            _same_bits(got, bp, f"sgd n {n} offsets {offs} step {k}")
            _same_bits(sh, bsh, f"sgd shadow n {n} offsets {offs} step {k}")
            _within(got, want, RC.OPT, f"sgd n {n} offsets {offs} step {k}")
        _same_bits(buf, base_buf, "momentum buffer")


# ---------------------------------------------------------------------------- CLIP kernels

@pytest.mark.parametrize("D", RC.EMBED_D)
@pytest.mark.parametrize("off", [0, 1])
def test_token_embed_clamps_ids_and_takes_offset_tables(D, off):
    """7 rows over 3 positions; ids -1 and ``vocab`` read the table's first and last row; a table one element into
    its buffer takes the element-wise kernel."""
    rows, Lq, V = 7, 3, 11
    tok = torch.tensor([3, -1, V, 0, V - 1, 5, -7], dtype=torch.int64)
    table, pos = _rand(20 + D, V, D), _rand(21 + D, Lq, D)
    tb = Buf(V, D, off=off, src=table)
    x = Buf(rows, D)
    tok_d, pos_d, table_d = tok.to(DEV), pos.to(DEV), table.to(DEV)
    call("vit_token_embed", rows, Lq, D, V, ptr(tok_d), ptr(tb.v), ptr(pos_d), ptr(x.v), _stream())
    torch.cuda.synchronize()
    want = table[tok.clamp(0, V - 1)] + pos[torch.arange(rows) % Lq]
    _same_bits(x.v, want, f"token_embed D {D} off {off}")
    x.outside_untouched("token_embed")
    if off:  # pos and the output one element in
        pb, xo = Buf(Lq, D, off=1, src=pos), Buf(rows, D, off=1)
        call("vit_token_embed", rows, Lq, D, V, ptr(tok_d), ptr(table_d), ptr(pb.v), ptr(xo.v), _stream())
        torch.cuda.synchronize()
        _same_bits(xo.v, want, "token_embed pos+1 x+1")
        xo.outside_untouched("token_embed x+1")


def test_token_embed_rejects_a_width_that_is_no_multiple_of_4():
    tok = torch.zeros(2, 2, dtype=torch.int64, device=DEV)
    with pytest.raises(L.HipError):
        ops.token_embed(tok, torch.zeros(5, 6, device=DEV), torch.zeros(2, 6, device=DEV))


@pytest.mark.parametrize("D", RC.ROWS_D)
@pytest.mark.parametrize("n", [1, 5])
def test_gather_and_scatter_rows_in_padded_views(D, n):
    rows = 9
    srcv = _rand(30 + D, rows, D)
    idx = torch.tensor([7, 0, 8, 3, 4][:n], dtype=torch.int64)
    src = Buf(rows, D, D + 3, 0, F32, srcv)
    out = Buf(n, D, D + 5)
    ops.gather_rows(src.v, idx.to(DEV), out=out.v)
    torch.cuda.synchronize()
    _same_bits(out.v, srcv[idx], f"gather D {D} n {n}")
    out.outside_untouched("gather")
    packed = Buf(n, D, D + 2, 0, F32, srcv[:n])
    dst = Buf(rows, D, D + 7)
    ops.scatter_rows(packed.v, idx.to(DEV), dst.v)
    torch.cuda.synchronize()
    want = torch.full((rows, D), SENT)
    want[idx] = srcv[:n]
    _same_bits(dst.v, want, f"scatter D {D} n {n}")
    dst.outside_untouched("scatter")


@pytest.mark.parametrize("D", RC.ROWNORM_D)
@pytest.mark.parametrize("n", [1, 5])
def test_rownorm_fwd_bwd(D, n):
    """Widths around the 64 lanes, 66 (the width CLIP-HBA runs it at); rows scaled by 1e-6 and 1e6 each against
    its own magnitude; the backward from the reference's rnorm."""
    for scale in RC.ROWNORM_SCALES:
        for ls in (2.3, None):
            x, dy = RC.rownorm_inputs(n, D, scale)
            y_ref, rn_ref, dx_ref = RC.rownorm(x.double(), dy, ls)
            lsd = torch.tensor([ls], device=DEV) if ls is not None else None
            y, rn = ops.rownorm_fwd(x.to(DEV), lsd)
            what = f"rownorm {n}x{D} scale {scale} ls {ls}"
            _within(y, y_ref, RC.F32, what + " y")
            e = RC.row_rel_max(rn[:, None], rn_ref[:, None])
            assert e <= RC.F32, (what, "rnorm", e)
            dx = ops.rownorm_bwd(x.to(DEV), dy.to(DEV), rn_ref.float().to(DEV), lsd)
            e = RC.row_rel_max(dx, dx_ref, RC.rownorm_dx_scale(rn_ref, dy, ls))
            print(f"{what} dx: {e:.2e}")
            assert e <= RC.F32, (what, "dx", e)


@pytest.mark.parametrize("n", RC.MSE_N)
def test_mse_fwd_bwd(n):
    """One workgroup of 1024 lanes: under one pass, exactly one, just past it, 4224 (64 x 66) and 70001."""
    p, t = RC.mse_inputs(n)
    loss_ref, d_ref = RC.mse(p.double(), t.double())
    pd, td = p.to(DEV), t.to(DEV)
    _within(ops.mse_fwd(pd, td).reshape(1), loss_ref, RC.F32, f"mse {n}")
    for g in (0.7, None):
        gt = torch.tensor(g, device=DEV) if g is not None else None
        d = Buf(1, n)
        call("vit_mse_bwd", n, ptr(pd), ptr(td), ptr(gt), ptr(d.v), _stream())
        torch.cuda.synchronize()
        _within(d.flat, d_ref * (g if g is not None else 1.0), RC.F32, f"mse bwd {n} g {g}")
        d.outside_untouched("mse bwd")
        _within(ops.mse_bwd(pd, td, gt), d_ref * (g if g is not None else 1.0), RC.F32, f"ops.mse_bwd {n}")
