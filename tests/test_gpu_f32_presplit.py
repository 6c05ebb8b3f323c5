"""GPU: pre-split weight images for the fp32 "high" GEMMs (gemm_f32.inc SPLIT = 2, namespace f32w).

A GEMM that reads the image issues the MFMAs of the in-loop split on the same operand bits in the same order, so
every comparison here is ``torch.equal`` on raw bits against the in-loop "high" result computed in the same test from
the same buffers.  Operands are randn scaled into |x| in [2^-20, 2^20] and not bf16-valued: lo != 0, and a form that
dropped or misplaced lo differs in most elements.  Buffers are the poisoned, strided views of
tests/test_gpu_gemm_exact.py; the image restatement is tests/test_f32_presplit_host.py's.

  1. the image pass, plain and transposed, against the restatement, and what it refuses;
  2. the forward with every epilogue: equal to vit_linear_fwd, counted, and reading the image alone (W = NaN);
  3. stream-K with a cut tile, registered and unregistered;
  4. the input gradient with its act' epilogues and fused column sums;
  5. GEMMs that do not take the MFMA path fall back with today's bits;
  6. a stale image is rebuilt after an in-place update and after a fused optimizer step;
  7. a two-block fp32 CLIP-HBA train step and a small all-trainable f32 VisionTransformer, bit for bit.

Every test leaves the process in "highest" with pre-splitting off.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_f32_presplit_host as PH  # noqa: E402
import test_gpu_gemm_exact as GE  # noqa: E402
from vit_amd import _lib as L  # noqa: E402

DEV = "cuda"
F32 = torch.float32
INVALID = 1  # hipErrorInvalidValue
Buf, _vec, _settle, _raw, _stream = GE.Buf, GE._vec, GE._settle, GE._raw, GE._stream
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    L.load()


@pytest.fixture(autouse=True)
def _restore_highest():
    yield
    from vit_amd import ops
    ops.set_float32_matmul_precision("highest")


def _mode(high):
    L.lib().vit_gemm_f32_precision(1 if high else 0)


def _counts(reset=1):
    """(f32 MFMA-path launches, of those bf16x3, of those reading an image)"""
    lib = L.lib()
    return lib.vit_gemm_f32_count(reset), lib.vit_gemm_f32_split_count(reset), lib.vit_gemm_f32_presplit_count(reset)


def _same(a, b, what):
    a, b = a.contiguous(), b.contiguous()
    assert bool(torch.isfinite(a).all()), what + ": non-finite"
    n = int((_raw(a) != _raw(b)).sum())
    assert n == 0, f"{what}: {n} of {a.numel()} elements differ from the in-loop split"


def _image(w, transposed=False):
    """The image of a contiguous weight view, built by the pre-pass into a poisoned buffer of its own."""
    N, K = w.rows, w.cols
    img = Buf(K, N, F32) if transposed else Buf(N, K, F32)
    L.call("vit_gemm_f32_weight_image", N, K, w.ptr, w.ld, int(transposed), img.ptr, _stream())
    _settle("image", outs=[img], ins=[w])
    img.snap = img.buf.clone()  # an input from here on
    return img


# ---------------------------------------------------------------------------- 1. the image pass

@pytest.mark.parametrize("transposed", [False, True], ids=["plain", "transposed"])
@pytest.mark.parametrize("shape", [(128, 32, 0), (136, 96, 4), (64, 1024, 0)], ids=str)
def test_image_pass(shape, transposed):
    rows, red, pad = shape   # the image's rows and reduction extent; the transposed form reads W [red][rows]
    a = PH.scaled_randn(rows, red, seed=3 + rows)
    src = a.T.contiguous() if transposed else a
    N, K = src.shape
    w = Buf(N, K, F32, src, ld=K + pad)
    img = Buf(rows, red, F32)
    L.call("vit_gemm_f32_weight_image", N, K, w.ptr, w.ld, int(transposed), img.ptr, _stream())
    _settle(f"image {shape} transposed={transposed}", outs=[img], ins=[w])
    ref = PH.image_ref(a)
    assert torch.equal(_raw(img.v.cpu().contiguous()), _raw(ref)), "the image is not the restatement's"


def test_image_pass_refuses_what_does_not_qualify():
    src = PH.scaled_randn(64, 72, seed=9)
    w = Buf(64, 72, F32, src, ld=76)
    img = Buf(72, 72, F32)
    s = _stream()
    call = L.lib().vit_gemm_f32_weight_image
    assert call(64, 40, w.ptr, w.ld, 0, img.ptr, s) == INVALID          # K % 32 != 0
    assert call(40, 64, w.ptr, w.ld, 1, img.ptr, s) == INVALID          # transposed: N % 32 != 0
    assert call(64, 64, w.ptr + 4, w.ld, 0, img.ptr, s) == INVALID      # misaligned W
    assert call(64, 64, w.ptr, 75, 0, img.ptr, s) == INVALID            # rows not 16-byte aligned
    assert call(64, 64, w.ptr, 32, 0, img.ptr, s) == INVALID            # a row stride under the extent
    assert call(64, 64, w.ptr, w.ld, 0, img.ptr + 8, s) == INVALID      # misaligned image
    assert call(64, 64, w.ptr, w.ld, 1, None, s) == INVALID
    _settle("refused image calls", ins=[w], idle=[img])


# ---------------------------------------------------------------------------- 2. forward

FWD_EPIS = {"store": L.EPI_STORE, "resid": L.EPI_RESID, "gelu": L.EPI_BIAS_GELU, "qgelu": L.EPI_BIAS_QGELU,
            "gelu_fwd": L.EPI_BIAS_GELU_FWD, "qgelu_fwd": L.EPI_BIAS_QGELU_FWD}


def _fwd(entry, epi, M, N, K, x, w, b, resid, wimg, stream=None, what=""):
    pair = epi in (L.EPI_BIAS_GELU, L.EPI_BIAS_QGELU)
    y = Buf(M, N, F32, ld=N + 4)
    a = Buf(M, N, F32, ld=N + 4) if pair else None
    r = Buf(M, N, F32, resid, ld=N + 4) if epi == L.EPI_RESID else None
    args = [L.F32, L.F32, epi, M, N, K, x.ptr, x.ld, w.ptr, b.ptr, y.ptr, y.ld, r.ptr if r else None,
            a.ptr if a else None]
    st = _stream() if stream is None else stream
    if entry == "wimg":
        L.call("vit_linear_fwd_wimg", *args, wimg.ptr if wimg is not None else None, st)
    else:
        L.call("vit_linear_fwd", *args, st)
    _settle(what, outs=[t for t in (y, a) if t is not None], ins=[t for t in (x, w, b, r, wimg) if t is not None])
    return y, a


@pytest.fixture(scope="module")
def fwd_operands():
    out = {}
    for M, N, K in ((1024, 1024, 64), (1032, 1028, 96)):
        src = [PH.scaled_randn(M, K, 1), PH.scaled_randn(N, K, 2), PH.scaled_randn(1, N, 3), PH.scaled_randn(M, N, 4)]
        x, w, b = Buf(M, K, F32, src[0], ld=K + 4), Buf(N, K, F32, src[1]), _vec(N, src[2])
        wnan = Buf(N, K, F32, torch.full((N, K), NAN))
        out[(M, N, K)] = (x, w, b, src[3], wnan, _image(w))
    return out


@pytest.mark.parametrize("epi", list(FWD_EPIS))
@pytest.mark.parametrize("shape", [(1024, 1024, 64), (1032, 1028, 96)], ids=str)
def test_forward_reads_the_image_alone(fwd_operands, shape, epi):
    M, N, K = shape
    x, w, b, resid, wnan, img = fwd_operands[shape]
    e = FWD_EPIS[epi]
    what = f"fwd {shape} {epi}"
    _mode(True)
    _counts()
    ref = _fwd("plain", e, M, N, K, x, w, b, resid, None, what=what + " in-loop")
    assert _counts() == (1, 1, 0)
    got = _fwd("wimg", e, M, N, K, x, w, b, resid, img, what=what + " image")
    assert _counts() == (1, 1, 1), "the pre-split count equals the launches"
    blind = _fwd("wimg", e, M, N, K, x, wnan, b, resid, img, what=what + " image, W = NaN")
    assert _counts() == (1, 1, 1)
    for r, g, n in zip(ref, got, blind):
        if r is not None:
            _same(g.v, r.v, what)
            _same(n.v, r.v, what + " with W = NaN: W was read")
    # lo matters: the image of hi alone (lo = 0) is another result
    assert float((PH.image_inverse(img.v.cpu())[1] != 0).float().mean()) > 0.9
    # without an image, or in "highest", it is vit_linear_fwd
    none = _fwd("wimg", e, M, N, K, x, w, b, resid, None, what=what + " no image")
    assert _counts() == (1, 1, 0)
    _same(none[0].v, ref[0].v, what + " Wimg = NULL")
    _mode(False)
    ref0 = _fwd("plain", e, M, N, K, x, w, b, resid, None, what=what + " highest")
    got0 = _fwd("wimg", e, M, N, K, x, w, b, resid, img, what=what + " highest, image given")
    assert _counts() == (2, 0, 0)
    for r, g in zip(ref0, got0):
        if r is not None:
            _same(g.v, r.v, what + " in highest")
    assert not torch.equal(_raw(ref0[0].v.contiguous()), _raw(ref[0].v.contiguous()))


# ---------------------------------------------------------------------------- 3. stream-K

def test_stream_k_cut_tile_reads_the_image():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    M, N, K = (2 * cus // 8 + 1) * 128, 1024, 64   # MI355X: 65 x 8 = 520 tiles on 512 slots, a tile cut between workgroups
    g = 2 * cus
    side = torch.cuda.Stream()
    part = torch.zeros(g * 2 * 128 * 128, dtype=F32, device=DEV)
    cnt = torch.zeros(g, dtype=torch.int32, device=DEV)
    x = Buf(M, K, F32, PH.scaled_randn(M, K, 21), ld=K + 4)
    w, b = Buf(N, K, F32, PH.scaled_randn(N, K, 22)), _vec(N, PH.scaled_randn(1, N, 23))
    img = _image(w)
    torch.cuda.synchronize()
    _mode(True)
    _counts()
    try:
        for registered in (True, False):
            if registered:
                L.call("vit_gemm_streamk_workspace", side.cuda_stream, part.data_ptr(), part.numel() * 4, cnt.data_ptr(), g)
            else:
                L.call("vit_gemm_streamk_workspace", side.cuda_stream, None, 0, None, 0)
            what = f"stream-K, workspace registered={registered}"
            ref, _ = _fwd("plain", L.EPI_STORE, M, N, K, x, w, b, None, None, stream=side.cuda_stream, what=what)
            got, _ = _fwd("wimg", L.EPI_STORE, M, N, K, x, w, b, None, img, stream=side.cuda_stream, what=what + " image")
            _same(got.v, ref.v, what)
            assert int(cnt.abs().sum()) == 0, "the stream-K counters must come back zero"
    finally:
        L.call("vit_gemm_streamk_workspace", side.cuda_stream, None, 0, None, 0)
    assert _counts() == (4, 4, 2)


# ---------------------------------------------------------------------------- 4. input gradient

def _dgrad(entry, epi, M, N, K, dy, w, pre, wimg, what=""):
    dx = Buf(M, K, F32, ld=K + 4)
    ax = Buf(M, K, F32, pre, ld=K + 4) if epi != L.EPI_STORE else None
    pf = L.lib().vit_linear_dgrad_partial_floats(M, K)
    db, part = _vec(K), _vec(pf)
    args = [L.F32, L.F32, epi, M, N, K, dy.ptr, dy.ld, w.ptr, dx.ptr, dx.ld, ax.ptr if ax else None, db.ptr, part.ptr,
            pf, 0]
    if entry == "wimg":
        L.call("vit_linear_dgrad_wimg", *args, wimg.ptr if wimg is not None else None, _stream())
    else:
        L.call("vit_linear_dgrad", *args, _stream())
    _settle(what, outs=[dx, db, part], ins=[t for t in (dy, w, ax, wimg) if t is not None])
    return dx, db


@pytest.mark.parametrize("epi", ["store", "gelu_bwd", "qgelu_bwd"])
@pytest.mark.parametrize("N", [64, 96])
def test_input_gradient_reads_the_transposed_image(N, epi):
    M, K = 1024, 1024   # dX [M, K] = dY [M, N] W [N, K]: 64 output tiles, reduced over N
    e = {"store": L.EPI_STORE, "gelu_bwd": L.EPI_GELU_BWD, "qgelu_bwd": L.EPI_QGELU_BWD}[epi]
    dy = Buf(M, N, F32, PH.scaled_randn(M, N, 31), ld=N + 4)
    w = Buf(N, K, F32, PH.scaled_randn(N, K, 32))
    wnan = Buf(N, K, F32, torch.full((N, K), NAN))
    pre = PH.scaled_randn(M, K, 33)
    img = _image(w, transposed=True)
    what = f"dgrad N={N} {epi}"
    _mode(True)
    _counts()
    rdx, rdb = _dgrad("plain", e, M, N, K, dy, w, pre, None, what + " in-loop")
    assert _counts() == (1, 1, 0)
    gdx, gdb = _dgrad("wimg", e, M, N, K, dy, w, pre, img, what + " image")
    ndx, ndb = _dgrad("wimg", e, M, N, K, dy, wnan, pre, img, what + " image, W = NaN")
    assert _counts() == (2, 2, 2)
    for g_, r_ in ((gdx, rdx), (gdb, rdb), (ndx, rdx), (ndb, rdb)):
        _same(g_.v, r_.v, what)
    odx, odb = _dgrad("wimg", e, M, N, K, dy, w, pre, None, what + " no image")
    assert _counts() == (1, 1, 0)
    _same(odx.v, rdx.v, what + " Wimg = NULL")
    _same(odb.v, rdb.v, what + " Wimg = NULL, dbias")


# ---------------------------------------------------------------------------- 5. off the MFMA path

def test_small_and_misaligned_gemms_fall_back():
    _mode(True)
    # under 64 tiles
    M, N, K = 256, 256, 64
    x, w = Buf(M, K, F32, PH.scaled_randn(M, K, 41), ld=K + 4), Buf(N, K, F32, PH.scaled_randn(N, K, 42))
    b = _vec(N, PH.scaled_randn(1, N, 43))
    img = _image(w)
    _counts()
    ref, _ = _fwd("plain", L.EPI_STORE, M, N, K, x, w, b, None, None, what="small in-loop")
    got, _ = _fwd("wimg", L.EPI_STORE, M, N, K, x, w, b, None, img, what="small image")
    assert _counts() == (0, 0, 0)
    _same(got.v, ref.v, "a GEMM under 64 tiles")
    # a misaligned X
    M, N, K = 1024, 1024, 64
    x = Buf(M, K, F32, PH.scaled_randn(M, K, 44), ld=K + 4, off=GE.OFF + 1)
    w, b = Buf(N, K, F32, PH.scaled_randn(N, K, 45)), _vec(N, PH.scaled_randn(1, N, 46))
    img = _image(w)
    _counts()
    ref, _ = _fwd("plain", L.EPI_STORE, M, N, K, x, w, b, None, None, what="misaligned in-loop")
    got, _ = _fwd("wimg", L.EPI_STORE, M, N, K, x, w, b, None, img, what="misaligned image")
    assert _counts() == (0, 0, 0)
    _same(got.v, ref.v, "a GEMM with a misaligned X")


# ---------------------------------------------------------------------------- 6. staleness

def test_a_stale_image_is_rebuilt():
    import vit_amd
    from vit_amd import ops
    from vit_amd.model import _Shadowed
    p = torch.nn.Parameter(PH.scaled_randn(1024, 64, 51).to(DEV))
    reg = _Shadowed()
    reg.add(p, F32)
    x = PH.scaled_randn(1024, 64, 52).to(DEV)
    assert ops.weight_image(p) is None            # the switch is off
    vit_amd.set_float32_matmul_precision("high", presplit_weights=True)

    def step(update, what):
        img0, v0 = ops.weight_image(p), p._vit_wimg_version
        assert img0 is p._vit_wimg and ops.weight_image(p) is img0   # built once per version
        _counts()
        stale = ops.linear_fwd(x, p.detach(), wimg=img0)
        assert _counts() == (1, 1, 1)
        update()
        img1 = ops.weight_image(p)
        assert p._vit_wimg_version != v0 and img1 is not img0, what + ": the image version did not change"
        fresh = ops.linear_fwd(x, p.detach(), wimg=img1)
        ref = ops.linear_fwd(x, p.detach())
        torch.cuda.synchronize()
        assert _counts() == (2, 2, 1)
        _same(fresh, ref, what)
        assert not torch.equal(_raw(fresh), _raw(stale)), what + ": the stale result"

    def add():
        with torch.no_grad():
            p.add_(PH.scaled_randn(1024, 64, 53).to(DEV) * 0.125)

    opt = vit_amd.FusedAdamW([p], lr=1e-2)

    def adamw():
        p.grad = PH.scaled_randn(1024, 64, 54).to(DEV)
        opt.step()

    step(add, "after an in-place add_")
    step(adamw, "after a FusedAdamW step")
    assert ops.weight_image_bytes([p]) == 1024 * 64 * 4
    vit_amd.set_float32_matmul_precision("high")
    reg.refresh()                                  # switching off drops the images at the next refresh
    assert ops.weight_image_bytes([p]) == 0 and ops.weight_image(p) is None


# ---------------------------------------------------------------------------- 7. models

def _train_step(m, x, y):
    import vit_amd
    m.clip_model._text_cache = None
    for q in m.parameters():
        q.grad = None
    pred = m(x)
    loss = vit_amd.mse_loss(pred, y)
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: q.grad.clone() for k, q in m.named_parameters() if q.requires_grad}
    return pred.detach().clone(), loss.detach().clone(), grads


def test_clip_hba_step_is_bit_equal_and_shares_the_prefix_cache(monkeypatch):
    import test_gpu_f32_split as FS
    import vit_amd
    from vit_amd import ops
    torch.manual_seed(0)
    m, _, _ = FS._model()
    m = m.to(DEV)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(FS.MB, 3, 224, 224, generator=g).to(DEV)
    y = (torch.randn(FS.MB, FS.MT, generator=g) * 0.5 + 1.0).to(DEV)
    vit_amd.set_float32_matmul_precision("high")
    _counts()
    pred0, loss0, grads0 = _train_step(m, x, y)
    n0, s0, i0 = _counts()
    assert n0 > 0 and s0 == n0 and i0 == 0 and ops.weight_image_bytes(m) == 0
    cache = vit_amd.VisualPrefixCache.build(m, x, batch_size=FS.MB)

    # which weights went without an image: only computed ones (not registered parameters) may
    registered = {p.data_ptr() for p in m.parameters() if getattr(p, "_vit_wimg_ok", False)}
    assert registered
    bare = []
    fwd, dgrad = ops.linear_fwd, ops.linear_dgrad
    monkeypatch.setattr(ops, "linear_fwd", lambda x2, w, *a, **k: (bare.append(w.data_ptr()) if k.get("wimg") is None
                                                                  else None, fwd(x2, w, *a, **k))[1])
    monkeypatch.setattr(ops, "linear_dgrad", lambda d2, w, *a, **k: (bare.append(w.data_ptr()) if k.get("wimg") is None
                                                                    else None, dgrad(d2, w, *a, **k))[1])
    vit_amd.set_float32_matmul_precision("high", presplit_weights=True)
    assert cache.ensure(m, x, batch_size=FS.MB) is False, "a cache filled in-loop was rebuilt under pre-splitting"
    _counts()
    pred1, loss1, grads1 = _train_step(m, x, y)
    n1, s1, i1 = _counts()
    assert (n1, s1) == (n0, s0) and 0 < i1 < n1, (n0, s0, n1, s1, i1)
    assert bare and not registered & set(bare), "a registered weight parameter ran without its image"
    _same(pred1, pred0, "predictions")
    _same(loss1.view(1), loss0.view(1), "loss")
    assert grads1.keys() == grads0.keys() and len(grads1) == 6
    for k in grads0:
        _same(grads1[k], grads0[k], k)
    held = ops.weight_image_bytes(m)
    assert held > 0 and held % 4 == 0
    fresh = vit_amd.VisualPrefixCache.build(m, x, batch_size=FS.MB)   # built from images: the in-loop rows
    idx = torch.arange(FS.MB)
    _same(fresh.take(idx), cache.take(idx), "prefix rows")
    vit_amd.set_float32_matmul_precision("high")
    assert fresh.ensure(m, x, batch_size=FS.MB) is False
    with torch.no_grad():
        m(x)
    assert ops.weight_image_bytes(m) == 0, "switching off frees the images at the next forward"


def test_all_trainable_f32_vit_refreshes_its_images_every_step():
    import vit_amd
    from vit_amd import ops
    g = torch.Generator().manual_seed(61)
    x = torch.randn(16, 3, 224, 224, generator=g).to(DEV)   # 16 x 197 rows: every block Linear has 64 tiles
    y = torch.randint(0, 10, (16,), generator=g).to(DEV)

    def run(presplit):
        torch.manual_seed(1)
        m = vit_amd.VisionTransformer(img_size=224, patch_size=16, embed_dim=512, depth=2, num_heads=8, num_classes=10,
                                      compute_dtype=F32).to(DEV)
        opt = vit_amd.FusedSGD(m.parameters(), lr=0.1, momentum=0.9)
        vit_amd.set_float32_matmul_precision("high", presplit_weights=presplit)
        _counts()
        losses, versions = [], []
        for _ in range(2):
            opt.zero_grad()
            loss = vit_amd.cross_entropy(m(x), y)
            loss.backward()
            opt.step()
            losses.append(loss.detach().clone())
            versions.append(getattr(m.blocks[0].mlp.fc1.weight, "_vit_wimg_version", None))
        torch.cuda.synchronize()
        return losses, {k: v.detach().clone() for k, v in m.state_dict().items()}, _counts(), versions, ops.weight_image_bytes(m)

    l0, sd0, c0, v0, held0 = run(False)
    l1, sd1, c1, v1, held1 = run(True)
    assert c0[2] == 0 and held0 == 0 and v0 == [None, None]
    assert c1[:2] == c0[:2] and c1[2] > 0, (c0, c1)
    assert v1[0] is not None and v1[0] != v1[1], "the images were not rebuilt after the optimizer step"
    # both images of the four block weights of each block
    assert held1 == 2 * sum(p.numel() * 4 for b in m_blocks(sd1) for p in b)
    for a, b in zip(l0, l1):
        _same(b.view(1), a.view(1), "loss")
    for k in sd0:
        _same(sd1[k], sd0[k], k)


def m_blocks(sd):
    """The GEMM weights of each block in a state dict."""
    names = ("attn.qkv.weight", "attn.proj.weight", "mlp.fc1.weight", "mlp.fc2.weight")
    depth = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
    return [[sd[f"blocks.{i}.{n}"] for n in names] for i in range(depth)]
