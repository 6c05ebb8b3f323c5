"""GPU: pre-split activation images for the fp32 "high" GEMMs (gemm_f32.inc SPLIT = 3, namespace f32a).

An activation image holds the hi / lo packs split8 forms from the f32 values, so a GEMM that reads one issues the
MFMAs of the in-loop split on the same bits in the same order, and a producer that writes one writes what
``vit_gemm_f32_weight_image`` makes of the f32 tensor it would have written.  Every comparison is on raw bits, against
the f32-operand call made in the same test from the same buffers (helpers and the image restatement are
tests/test_gpu_f32_presplit.py's and tests/test_f32_presplit_host.py's).

  1. consumer: ``vit_linear_fwd_wimg`` with X as an image, the four epilogues, one / odd k-step counts, ragged tiles,
     a strided poisoned X, stream-K with a cut tile;
  2. refusals: ``hipErrorInvalidValue``, nothing counted, the output untouched;
  3. the image-writing epilogue against the image of the f32 output, strided, ragged rows, stream-K;
  4. the LayerNorm producers, both entry points, part-filled blocks of waves;
  5. the fc1 -> fc2 chain on images end to end.  (4096 rows, not the 1024 the issue names: with 1024 rows fc2
     [1024 x 256] has 16 output tiles, and under 64 tiles a GEMM is off the MFMA path, where an image is refused);
  6. the two-block fp32 CLIP-HBA model: no-grad predictions, prefix caches across modes, a training step; which
     GEMMs received an image;
  7. two runs of 6 are bitwise equal;
  8. models whose width the LayerNorm vector kernels do not cover (384; 1280 on the plain entry): the pass runs, no
     LayerNorm is asked for an image, the bits are the weights-only pass's.

The image X has no f32 twin in the call (the dtype code says what X holds), so "the image alone is read" is shown the
way §4.25's test shows it for W: the f32 W handed in beside the weight image is all NaN.

Every test leaves the process in "highest" with both pre-split switches off.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_f32_presplit_host as PH  # noqa: E402
import test_gpu_f32_presplit as PS  # noqa: E402
import test_gpu_gemm_exact as GE  # noqa: E402
from vit_amd import _lib as L  # noqa: E402

DEV = "cuda"
F32 = torch.float32
INVALID = 1  # hipErrorInvalidValue
NAN = float("nan")
Buf, _vec, _settle, _raw, _stream, _same, _image, _mode = (GE.Buf, GE._vec, GE._settle, GE._raw, GE._stream, PS._same,
                                                           PS._image, PS._mode)
EPIS = {"store": L.EPI_STORE, "resid": L.EPI_RESID, "gelu_fwd": L.EPI_BIAS_GELU_FWD, "qgelu_fwd": L.EPI_BIAS_QGELU_FWD}
OUT_EPIS = ("store", "gelu_fwd", "qgelu_fwd")


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


def _counts(reset=1):
    """(f32 MFMA-path launches, of those bf16x3, of those reading a weight image, of those reading an activation image)"""
    lib = L.lib()
    return (lib.vit_gemm_f32_count(reset), lib.vit_gemm_f32_split_count(reset), lib.vit_gemm_f32_presplit_count(reset),
            lib.vit_gemm_f32_presplit_act_count(reset))


def _bits_equal(a, b, what):
    a, b = _raw(a.contiguous()), _raw(b.contiguous())
    n = int((a != b).sum())
    assert n == 0, f"{what}: {n} of {a.numel()} cells differ"


def _strided_image(x, pad=4):
    """The image of the f32 view x, in a row-strided view (pitch > K) of a NaN-filled buffer."""
    img = _image(x)
    out = Buf(x.rows, x.cols, F32, img.v, ld=x.cols + pad)
    return out


def _fwd(epi, M, N, K, x, w, b, resid, wimg, xdt=L.F32, odt=L.F32, stream=None, what="", expect=0, y=None):
    y = Buf(M, N, F32, ld=N + 4) if y is None else y
    r = Buf(M, N, F32, resid, ld=N + 4) if epi == L.EPI_RESID else None
    rc = L.lib().vit_linear_fwd_wimg(xdt, odt, epi, M, N, K, x.ptr, x.ld, w.ptr, b.ptr, y.ptr, y.ld,
                                     r.ptr if r else None, None, wimg.ptr if wimg is not None else None,
                                     _stream() if stream is None else stream)
    assert rc == expect, f"{what}: returned {rc}"
    ins = [t for t in (x, w, b, r, wimg) if t is not None]
    if expect:
        _settle(what, ins=ins, idle=[y])
    else:
        _settle(what, outs=[y], ins=ins)
    return y


def _image_of(y):
    """vit_gemm_f32_weight_image of a (strided) f32 view: the tests' reference for every produced image."""
    img = Buf(y.rows, y.cols, F32)
    L.call("vit_gemm_f32_weight_image", y.rows, y.cols, y.ptr, y.ld, 0, img.ptr, _stream())
    _settle("reference image", outs=[img])
    return img


# ---------------------------------------------------------------------------- 1. consumer

SHAPES = [(1024, 1024, 32), (1024, 1024, 96), (1032, 1028, 96)]


@pytest.fixture(scope="module")
def operands():
    out = {}
    for M, N, K in SHAPES:
        x = Buf(M, K, F32, PH.scaled_randn(M, K, 101), ld=K + 4)
        w, b = Buf(N, K, F32, PH.scaled_randn(N, K, 102)), _vec(N, PH.scaled_randn(1, N, 103))
        wnan = Buf(N, K, F32, torch.full((N, K), NAN))
        out[(M, N, K)] = (x, w, b, PH.scaled_randn(M, N, 104), wnan, _image(w), _strided_image(x))
    return out


@pytest.mark.parametrize("epi", list(EPIS))
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_forward_reads_the_activation_image(operands, shape, epi):
    M, N, K = shape
    x, w, b, resid, wnan, wimg, ximg = operands[shape]
    e = EPIS[epi]
    what = f"fwd {shape} {epi}"
    assert float((PH.image_inverse(_image(x).v.cpu())[1] != 0).float().mean()) > 0.9   # lo matters
    _mode(True)
    _counts()
    ref = _fwd(e, M, N, K, x, w, b, resid, wimg, what=what + " f32 X")
    assert _counts() == (1, 1, 1, 0)
    got = _fwd(e, M, N, K, ximg, wnan, b, resid, wimg, xdt=L.F32_SPLIT, what=what + " image X, W = NaN")
    assert _counts() == (1, 1, 1, 1), "an activation-image launch counts once in each counter"
    _same(got.v, ref.v, what)


def test_stream_k_cut_tile_reads_the_activation_image():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    M, N, K = (2 * cus // 8 + 1) * 128, 1024, 64   # a tile cut between workgroups (tests/test_gpu_f32_presplit.py)
    g = 2 * cus
    side = torch.cuda.Stream()
    part = torch.zeros(g * 2 * 128 * 128, dtype=F32, device=DEV)
    cnt = torch.zeros(g, dtype=torch.int32, device=DEV)
    x = Buf(M, K, F32, PH.scaled_randn(M, K, 21), ld=K + 4)
    w, b = Buf(N, K, F32, PH.scaled_randn(N, K, 22)), _vec(N, PH.scaled_randn(1, N, 23))
    wimg, ximg = _image(w), _strided_image(x)
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
            for e in (L.EPI_STORE, L.EPI_BIAS_GELU_FWD):
                ref = _fwd(e, M, N, K, x, w, b, None, wimg, stream=side.cuda_stream, what=what)
                got = _fwd(e, M, N, K, ximg, w, b, None, wimg, xdt=L.F32_SPLIT, stream=side.cuda_stream,
                           what=what + " image X")
                _same(got.v, ref.v, what)
                # 3. the cut tile's combine ends in the image epilogue too
                yimg = _fwd(e, M, N, K, ximg, w, b, None, wimg, xdt=L.F32_SPLIT, odt=L.F32_SPLIT,
                            stream=side.cuda_stream, what=what + " image X, image Y")
                _bits_equal(yimg.v, _image_of(ref).v, what + " image Y")
                yimg = _fwd(e, M, N, K, x, w, b, None, wimg, odt=L.F32_SPLIT, stream=side.cuda_stream,
                            what=what + " f32 X, image Y")
                _bits_equal(yimg.v, _image_of(ref).v, what + " image Y from an f32 X")
            assert int(cnt.abs().sum()) == 0, "the stream-K counters must come back zero"
    finally:
        L.call("vit_gemm_streamk_workspace", side.cuda_stream, None, 0, None, 0)
    assert _counts() == (16, 16, 16, 8)


# ---------------------------------------------------------------------------- 2. refusals

def test_an_image_the_kernels_cannot_read_is_refused(operands):
    x, w, b, resid, wnan, wimg, ximg = operands[(1024, 1024, 96)]
    _mode(True)
    _counts()
    S = L.F32_SPLIT

    def refused(what, M=1024, N=1024, K=96, x=ximg, wimg=wimg, xdt=S, odt=L.F32, epi=L.EPI_STORE):
        _fwd(epi, M, N, K, x, w, b, resid, wimg, xdt=xdt, odt=odt, what=what, expect=INVALID)
        assert _counts() == (0, 0, 0, 0), what

    # 7 x 9 = 63 output tiles, with operands of its own (the shared ones have 1024 weight rows)
    M63, N63 = 896, 1152
    x63 = Buf(M63, 96, F32, PH.scaled_randn(M63, 96, 111), ld=100)
    w63, b63 = Buf(N63, 96, F32, PH.scaled_randn(N63, 96, 112)), _vec(N63, PH.scaled_randn(1, N63, 113))
    _fwd(L.EPI_STORE, M63, N63, 96, _strided_image(x63), w63, b63, None, _image(w63), xdt=S, what="63 tiles",
         expect=INVALID)
    assert _counts() == (0, 0, 0, 0)
    refused("K = 48", K=48)
    off = Buf(1024, 96, F32, ximg.v, ld=100, off=GE.OFF + 1)
    refused("a misaligned X", x=off)
    refused("Wimg = NULL", wimg=None)
    refused("a pair epilogue", epi=L.EPI_BIAS_GELU)
    refused("an image output behind the residual epilogue", odt=S, epi=L.EPI_RESID)
    _mode(False)
    refused("mode 0")
    refused("mode 0, image output", xdt=L.F32, x=x, odt=S)


def test_an_image_output_needs_whole_k_blocks(operands):
    x, w, b, resid, wnan, wimg, ximg = operands[(1032, 1028, 96)]
    _mode(True)
    _counts()
    for xdt, xx in ((L.F32, x), (L.F32_SPLIT, ximg)):
        _fwd(L.EPI_STORE, 1032, 1028, 96, xx, w, b, None, wimg, xdt=xdt, odt=L.F32_SPLIT, what="N = 1028", expect=INVALID)
    assert _counts() == (0, 0, 0, 0)


# ---------------------------------------------------------------------------- 3. epilogue producer

@pytest.mark.parametrize("epi", OUT_EPIS)
@pytest.mark.parametrize("shape", [(1024, 1024, 64), (1032, 1024, 96)], ids=str)
def test_epilogue_writes_the_image_of_its_f32_output(shape, epi):
    M, N, K = shape
    e = EPIS[epi]
    x = Buf(M, K, F32, PH.scaled_randn(M, K, 121), ld=K + 4)
    w, b = Buf(N, K, F32, PH.scaled_randn(N, K, 122)), _vec(N, PH.scaled_randn(1, N, 123))
    wimg, ximg = _image(w), _strided_image(x)
    what = f"image output {shape} {epi}"
    _mode(True)
    _counts()
    ref = _fwd(e, M, N, K, x, w, b, None, wimg, what=what + " f32")
    want = _image_of(ref)
    assert _counts() == (1, 1, 1, 0)
    # pitch > N in a poisoned buffer: _fwd checks that nothing outside the view was written
    got = _fwd(e, M, N, K, x, w, b, None, wimg, odt=L.F32_SPLIT, what=what + " from an f32 X")
    assert _counts() == (1, 1, 1, 0)
    _bits_equal(got.v, want.v, what)
    got = _fwd(e, M, N, K, ximg, w, b, None, wimg, xdt=L.F32_SPLIT, odt=L.F32_SPLIT, y=Buf(M, N, F32, ld=N + 36),
               what=what + " from an image X")
    assert _counts() == (1, 1, 1, 1)
    _bits_equal(got.v, want.v, what + ", image X")
    hi, lo = PH.image_inverse(got.v.cpu().contiguous())
    assert torch.equal(hi, ref.v.cpu().to(torch.bfloat16).float()) and float((lo != 0).float().mean()) > 0.5


# ---------------------------------------------------------------------------- 4. LayerNorm producers

def _ln(entry, rows, D, x, r, w, b, ydt, what, expect=0):
    y, mean, rstd = Buf(rows, D, F32, ld=D + 8), _vec(rows), _vec(rows)
    xs = Buf(rows, D, F32, ld=D + 4) if entry == "add" else None
    lib = L.lib()
    if entry == "add":
        rc = lib.vit_add_layer_norm_fwd(L.F32, ydt, rows, D, x.ptr, x.ld, r.ptr, r.ld, xs.ptr, xs.ld, y.ptr, y.ld, w.ptr,
                                        b.ptr, mean.ptr, rstd.ptr, 1e-5, _stream())
    else:
        rc = lib.vit_layer_norm_fwd(L.F32, ydt, rows, D, x.ptr, x.ld, y.ptr, y.ld, w.ptr, b.ptr, mean.ptr, rstd.ptr, 1e-5,
                                    _stream())
    assert rc == expect, f"{what}: returned {rc}"
    outs = [t for t in (y, mean, rstd, xs) if t is not None]
    if expect:
        _settle(what, ins=[x, w, b], idle=outs)
    else:
        _settle(what, outs=outs, ins=[t for t in (x, r, w, b) if t is not None])
    return y, mean, rstd, xs


@pytest.mark.parametrize("entry", ["ln", "add"])
@pytest.mark.parametrize("D", [256, 768, 1024, 2048])
@pytest.mark.parametrize("rows", [1, 5, 9])
def test_layer_norm_writes_the_image_of_its_f32_output(rows, D, entry):
    x = Buf(rows, D, F32, PH.scaled_randn(rows, D, 131), ld=D + 4)
    r = Buf(rows, D, F32, PH.scaled_randn(rows, D, 132), ld=D + 12) if entry == "add" else None
    w, b = _vec(D, PH.scaled_randn(1, D, 133)), _vec(D, PH.scaled_randn(1, D, 134))
    what = f"{entry} rows={rows} D={D}"
    ref = _ln(entry, rows, D, x, r, w, b, L.F32, what + " f32")
    got = _ln(entry, rows, D, x, r, w, b, L.F32_SPLIT, what + " image")
    _bits_equal(got[0].v, _image_of(ref[0]).v, what)
    for g_, r_, name in zip(got[1:], ref[1:], ("mean", "rstd", "xs")):
        if r_ is not None:
            _same(g_.v, r_.v, f"{what} {name}")
    hi, _ = PH.image_inverse(got[0].v.cpu().contiguous())
    assert torch.equal(hi, ref[0].v.cpu().to(torch.bfloat16).float())


def test_the_element_wise_layer_norm_has_no_image_form():
    rows, D = 5, 96
    x = Buf(rows, D, F32, PH.scaled_randn(rows, D, 141), ld=D + 4)
    w, b = _vec(D, PH.scaled_randn(1, D, 142)), _vec(D, PH.scaled_randn(1, D, 143))
    _ln("ln", rows, D, x, None, w, b, L.F32_SPLIT, "D = 96", expect=INVALID)
    _ln("add", rows, D, x, x, w, b, L.F32_SPLIT, "add, D = 96", expect=INVALID)
    _ln("ln", rows, D, x, None, w, b, L.F32, "D = 96 as f32")   # the f32 form still runs


# ---------------------------------------------------------------------------- 5. chain

def test_mlp_chain_on_images_end_to_end():
    from vit_amd import ops
    import vit_amd
    M, D, F = 4096, 256, 1024   # fc1 32 x 8 tiles, fc2 32 x 2 = 64 tiles
    xm = PH.scaled_randn(M, D, 151).to(DEV)
    nw, nb = PH.scaled_randn(1, D, 152).to(DEV).view(D), PH.scaled_randn(1, D, 153).to(DEV).view(D)
    w1, b1 = (PH.scaled_randn(F, D, 154) * 0.05).to(DEV), PH.scaled_randn(1, F, 155).to(DEV).view(F)
    w2, b2 = (PH.scaled_randn(D, F, 156) * 0.05).to(DEV), PH.scaled_randn(1, D, 157).to(DEV).view(D)
    vit_amd.set_float32_matmul_precision("high", presplit_weights=True, presplit_activations=True)
    i1, i2 = ops.weight_image_raw(w1), ops.weight_image_raw(w2)

    def chain(images, add):
        h2, act, xo = torch.empty(M, D, device=DEV), torch.empty(M, F, device=DEV), torch.empty(M, D, device=DEV)
        m2, r2 = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
        if add:
            xs = torch.empty(M, D, device=DEV)
            ops.add_layer_norm_fwd(xm, xm, xs, nw, nb, 1e-5, out=h2, mean=m2, rstd=r2, out_image=images)
        else:
            xs = xm
            ops.layer_norm_fwd(xm, nw, nb, 1e-5, F32, out=h2, mean=m2, rstd=r2, out_image=images)
        if images:
            assert ops.linear_fwd_takes_image(h2, w1, i1) and ops.linear_fwd_takes_image(act, w2, i2)
        ops.linear_fwd(h2, w1, b1, epi=L.EPI_BIAS_QGELU_FWD, out=act, wimg=i1, x_image=images, out_image=images)
        ops.linear_fwd(act, w2, b2, epi=L.EPI_RESID, resid=xs, out=xo, wimg=i2, x_image=images)
        torch.cuda.synchronize()
        return xo

    for add in (False, True):
        _counts()
        ref = chain(False, add)
        assert _counts() == (2, 2, 2, 0)
        got = chain(True, add)
        assert _counts() == (2, 2, 2, 2)
        _same(got, ref, f"MLP chain, add={add}")
    assert not ops.linear_fwd_takes_image(torch.empty(1024, F, device=DEV), w2, i2)   # 16 tiles: asked before produced


# ---------------------------------------------------------------------------- 6, 7. model

def _model_case():
    """The whole of case 6, returning every tensor it compared (for case 7)."""
    import test_gpu_f32_split as FS
    import vit_amd
    from vit_amd import ops
    torch.manual_seed(0)
    m, _, _ = FS._model()
    m = m.to(DEV)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(FS.MB, 3, 224, 224, generator=g).to(DEV)
    y = (torch.randn(FS.MB, FS.MT, generator=g) * 0.5 + 1.0).to(DEV)
    idx = torch.arange(FS.MB)
    act_count = L.lib().vit_gemm_f32_presplit_act_count

    def predict():
        m.clip_model._text_cache = None
        with torch.no_grad():
            out = m(x).detach().clone()
        torch.cuda.synchronize()
        return out

    vit_amd.set_float32_matmul_precision("high", presplit_weights=True)
    act_count(1)
    pred2 = predict()
    cache2 = vit_amd.VisualPrefixCache.build(m, x, batch_size=FS.MB)
    step2 = PS._train_step(m, x, y)
    assert act_count(1) == 0

    vit_amd.set_float32_matmul_precision("high", presplit_weights=True, presplit_activations=True)
    assert cache2.ensure(m, x, batch_size=FS.MB) is False, "a cache built from f32 activations was rebuilt under images"
    pred3 = predict()
    n_pred = act_count(1)
    assert n_pred > 0, "no frozen block read an activation image"
    _same(pred3, pred2, "no-grad predictions")
    cache3 = vit_amd.VisualPrefixCache.build(m, x, batch_size=FS.MB)
    assert act_count(1) > 0
    _same(cache3.take(idx), cache2.take(idx), "prefix rows")

    # which GEMMs received an image X: the qkv, fc1 and fc2 of the frozen visual block 0 and nothing else
    frozen = m.clip_model.visual.transformer.resblocks[0].block_params()
    seen, fwd = [], ops.linear_fwd

    def spy(x2, w, *a, **k):
        if k.get("x_image") or k.get("out_image"):
            seen.append((w.data_ptr(), bool(k.get("x_image")), bool(k.get("out_image"))))
        return fwd(x2, w, *a, **k)

    ops.linear_fwd = spy
    try:
        step3 = PS._train_step(m, x, y)
    finally:
        ops.linear_fwd = fwd
    n_step = act_count(1)
    assert n_step == 3 and sorted(seen) == sorted([(frozen[2].data_ptr(), True, False), (frozen[8].data_ptr(), True, True),
                                                   (frozen[10].data_ptr(), True, False)]), (n_step, seen)
    _same(step3[0], step2[0], "predictions")
    _same(step3[1].view(1), step2[1].view(1), "loss")
    assert step3[2].keys() == step2[2].keys() and len(step3[2]) == 6
    for k in step2[2]:
        _same(step3[2][k], step2[2][k], k)

    vit_amd.set_float32_matmul_precision("high", presplit_weights=True)
    assert cache3.ensure(m, x, batch_size=FS.MB) is False, "a cache built from images was rebuilt without them"
    pred2b = predict()
    assert act_count(1) == 0, "switching off still handed an image to a GEMM"
    _same(pred2b, pred2, "predictions after switching off")
    vit_amd.set_float32_matmul_precision("highest")
    return [pred3, cache3.take(idx).clone(), step3[0], step3[1].view(1)] + [step3[2][k] for k in sorted(step3[2])]


@pytest.fixture(scope="module")
def first_run():
    return _model_case()


def test_clip_hba_model_is_bit_equal_with_activation_images(first_run):
    assert len(first_run) == 4 + 6


def test_the_model_case_repeats_bit_for_bit(first_run):
    again = _model_case()
    assert len(again) == len(first_run)
    for i, (a, b) in enumerate(zip(again, first_run)):
        _same(a, b, f"run 2 against run 1, tensor {i}")



# ---------------------------------------------------------------------------- 8. widths off the LayerNorm vector kernels

@pytest.mark.parametrize("width,heads,fused", [(384, 6, False), (1280, 20, False), (1280, 20, True)])
def test_a_width_the_layer_norm_cannot_image_keeps_f32_activations(monkeypatch, width, heads, fused):
    """D = 384 has no vector LayerNorm at all; D = 1280 has one on the fused add + LayerNorm entry alone (the plain
    entry runs its element-wise kernel there).  The GEMMs of either qualify (16 x 197 rows, K % 32 == 0, >= 64 tiles),
    so only the producer's side of the decision keeps h1 / h2 in f32.  act still travels as an image: its producer
    is fc1's epilogue, not a LayerNorm."""
    import vit_amd
    from vit_amd import model as M, ops
    monkeypatch.setattr(M, "_FUSED_RESID_F32", [fused])
    torch.manual_seed(3)
    m = vit_amd.VisionTransformer(img_size=224, patch_size=16, embed_dim=width, depth=2, num_heads=heads, num_classes=10,
                                  compute_dtype=F32).to(DEV)
    x = torch.randn(16, 3, 224, 224, generator=torch.Generator().manual_seed(4)).to(DEV)
    asked = {"ln": 0, "gemm": 0}
    ln, aln, fwd = ops.layer_norm_fwd, ops.add_layer_norm_fwd, ops.linear_fwd

    def spy(fn, key):
        def wrapped(*a, **k):
            asked[key] += bool(k.get("out_image") if key == "ln" else k.get("x_image"))
            return fn(*a, **k)
        return wrapped

    monkeypatch.setattr(ops, "layer_norm_fwd", spy(ln, "ln"))
    monkeypatch.setattr(ops, "add_layer_norm_fwd", spy(aln, "ln"))
    monkeypatch.setattr(ops, "linear_fwd", spy(fwd, "gemm"))

    def predict():
        with torch.no_grad():
            out = m(x).detach().clone()
        torch.cuda.synchronize()
        return out

    vit_amd.set_float32_matmul_precision("high", presplit_weights=True)
    ref = predict()
    assert asked == {"ln": 0, "gemm": 0}
    vit_amd.set_float32_matmul_precision("high", presplit_weights=True, presplit_activations=True)
    _counts()
    got = predict()
    n = _counts()[3]
    _same(got, ref, f"width {width}, fused={fused}")
    assert n == asked["gemm"] >= 1, (n, asked)                       # fc2 reads fc1's image at every width
    assert (asked["ln"] > 0) == (width == 1280 and fused), asked     # ... and a LayerNorm writes one only where it can
