"""GPU: pre-split images through fp32 "high" attention (attn_fwd_image_x3, attn_fwd_image_stream).

``vit_sdpa_fwd_image`` reads ``qkv`` as a §4.26 activation image and writes ``o`` as one.  The image holds the hi / lo
packs that the f32 kernels form with split8, so the image kernels issue the same MFMAs on the same bits: ``o`` is the
image of the f32 kernel's ``o`` and ``lse`` its ``lse``, bit for bit.  Every comparison is on raw bits, against the
f32-operand "high" call made in the same test from the same values (helpers are tests/test_gpu_f32_presplit_act.py's).

  1. resident kernels, N in {1, 16, 17, 33, 77, 257, 288}, causal at 17 / 33 / 77, strided poisoned views;
  2. streamed kernel (long switch), N in {289, 320, 321, 577};
  3. hard softmax input (scores ~ 300), one resident and one streamed shape;
  4. refusals: hipErrorInvalidValue, the output's poison intact, no counter moved, the host query false;
  5. qkv -> attention -> proj on images against the same three launches with f32 qkv / o;
  6. the two-block fp32 CLIP-HBA model; 6b. two runs are bitwise equal;
  7. a model one end of which cannot take an image: the pass runs on f32 tensors, the switch-off pass's bits.

Every test leaves the process in "highest" with all switches off.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_f32_presplit_host as PH  # noqa: E402
import test_gpu_f32_presplit as PS  # noqa: E402
import test_gpu_f32_presplit_act as PA  # noqa: E402
import test_gpu_gemm_exact as GE  # noqa: E402
from oracle import attn_cases as AC  # noqa: E402
from vit_amd import _lib as L  # noqa: E402

DEV = "cuda"
F32 = torch.float32
INVALID = 1  # hipErrorInvalidValue
Buf, _vec, _settle, _raw, _stream, _same = GE.Buf, GE._vec, GE._settle, GE._raw, GE._stream, PS._same
_image_of, _bits_equal, _strided_image = PA._image_of, PA._bits_equal, PA._strided_image
B, H = 2, 2
D = H * 64


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
    ops.set_float32_attention_precision("highest")


def _counts(reset=1):
    """(image launches, resident bf16x3 calls, streamed f32 calls, streamed bf16x3 calls)"""
    lib = L.lib()
    return (lib.vit_sdpa_f32_image_count(reset), lib.vit_sdpa_f32_split_count(reset), lib.vit_sdpa_long_f32_count(reset),
            lib.vit_sdpa_long_f32_split_count(reset))


def _high(long=False):
    lib = L.lib()
    lib.vit_sdpa_f32_precision(1)
    lib.vit_sdpa_f32_long_precision(1 if long else 0)


def _takes(qkv, o, lse, N, causal, heads=H, head_dim=64, batch=B):
    return L.lib().vit_sdpa_fwd_takes_image(batch, heads, N, head_dim, int(causal), qkv.ld | o.ld,
                                            qkv.ptr | o.ptr)


def _attn(qkv, N, causal, image, what, scale=0.125, expect=0, o_ld=D + 4, heads=H, head_dim=64):
    """One forward into a strided poisoned o and a poisoned lse; qkv is an input Buf (f32 values or their image)."""
    o, lse = Buf(B * N, heads * head_dim, F32, ld=o_ld), _vec(B * heads * N)
    lib = L.lib()
    if image:
        assert bool(_takes(qkv, o, lse, N, causal, heads, head_dim)) == (expect == 0), what + ": the host query"
        rc = lib.vit_sdpa_fwd_image(B, heads, N, head_dim, qkv.ptr, qkv.ld, o.ptr, o.ld, lse.ptr, scale, int(causal),
                                    _stream())
    else:
        rc = lib.vit_sdpa_fwd(L.F32, B, heads, N, head_dim, qkv.ptr, qkv.ld, o.ptr, o.ld, lse.ptr, scale, int(causal),
                              _stream())
    assert rc == expect, f"{what}: returned {rc}"
    if expect:
        _settle(what, ins=[qkv], idle=[o, lse])
    else:
        _settle(what, outs=[o, lse], ins=[qkv])
    return o, lse


def _compare(values, N, causal, long, what, scale=0.125):
    """The f32 "high" call and the image call on the same values: o_img = image(o_f32), lse equal, counters."""
    qkv = Buf(B * N, 3 * D, F32, values, ld=3 * D + 4)
    qimg = _strided_image(qkv)
    assert float((PH.image_inverse(PS._image(qkv).v.cpu())[1] != 0).float().mean()) > 0.9   # lo matters
    _high(long)
    _counts()
    o, lse = _attn(qkv, N, causal, False, what + " f32", scale=scale)
    want = (0, 0, 1, 1) if N > 288 else (0, 1, 0, 0)
    assert _counts() == want, what + ": the f32 call did not take the bf16x3 kernels"
    oi, lsei = _attn(qimg, N, causal, True, what + " image", scale=scale)
    assert _counts() == (1,) + want[1:], what + ": one image launch, counted where the f32 form counts"
    assert bool(torch.isfinite(o.v).all()) and bool(torch.isfinite(lse.v).all()), what
    _bits_equal(oi.v, _image_of(o).v, what + " o")
    _same(lsei.v, lse.v, what + " lse")
    hi, _ = PH.image_inverse(oi.v.cpu().contiguous())
    assert torch.equal(hi, o.v.cpu().to(torch.bfloat16).float()), what + ": hi of the o image"


# ---------------------------------------------------------------------------- 1, 2. kernels

RESIDENT = [(N, False) for N in (1, 16, 17, 33, 77, 257, 288)] + [(N, True) for N in (17, 33, 77)]


@pytest.mark.parametrize("N,causal", RESIDENT, ids=lambda v: str(v))
def test_resident_kernel_reads_and_writes_images(N, causal):
    _compare(PH.scaled_randn(B * N, 3 * D, 200 + N), N, causal, False, f"resident N={N} causal={causal}")


@pytest.mark.parametrize("N", [289, 320, 321, 577])
def test_streamed_kernel_reads_and_writes_images(N):
    _compare(PH.scaled_randn(B * N, 3 * D, 300 + N), N, False, True, f"streamed N={N}")


# ---------------------------------------------------------------------------- 3. hard softmax input

@pytest.mark.parametrize("N,long", [(77, False), (321, True)], ids=["resident", "streamed"])
def test_scores_of_magnitude_300(N, long):
    c = AC.make_case("offset", B, H, N, F32)   # q, k += 6: scores ~ 64 * 36 * 0.125 ~ 300
    q, k, _ = AC.split_qkv(c.qkv.double(), B, H, N)
    assert float((q @ k.transpose(-1, -2)).mean()) * c.scale > 200
    _compare(c.qkv, N, False, long, f"offset N={N}", scale=c.scale)


# ---------------------------------------------------------------------------- 4. refusals

def test_what_the_image_kernels_cannot_run_is_refused():
    lib = L.lib()

    def refused(what, N=77, causal=False, heads=H, head_dim=64, pad=4, o_ld=None):
        w = heads * head_dim
        qimg = Buf(B * N, 3 * w, F32, PH.scaled_randn(B * N, 3 * w, 400), ld=3 * w + pad)   # never read
        _attn(qimg, N, causal, True, what, expect=INVALID, heads=heads, head_dim=head_dim,
              o_ld=w + 4 if o_ld is None else o_ld)
        assert _counts() == (0, 0, 0, 0), what

    _high(long=False)
    _counts()
    refused("N = 289 without the long switch", N=289)
    refused("head_dim 32", heads=4, head_dim=32)
    refused("a qkv pitch that is no multiple of 4 floats", pad=3)
    refused("an o pitch that is no multiple of 4 floats", o_ld=D + 2)
    _high(long=True)
    refused("causal at N = 289", N=289, causal=True)
    prev = lib.vit_sdpa_long_config(0)
    try:
        refused("N = 289 with the streamed kernels off", N=289)
    finally:
        lib.vit_sdpa_long_config(prev)
    lib.vit_sdpa_f32_precision(0)
    refused('"highest"')
    refused('"highest", long', N=289)


# ---------------------------------------------------------------------------- 5. chain

def test_qkv_attention_proj_on_images_end_to_end():
    from vit_amd import ops
    import vit_amd
    Bc, Hc, N = 16, 4, 257          # 4112 rows: proj [4112 x 256] has 33 x 2 = 66 output tiles, on the MFMA path
    Dc, M = Hc * 64, Bc * N
    x = PH.scaled_randn(M, Dc, 501).to(DEV)
    h1 = PH.scaled_randn(M, Dc, 502).to(DEV)
    wq, bq = (PH.scaled_randn(3 * Dc, Dc, 503) * 0.05).to(DEV), PH.scaled_randn(1, 3 * Dc, 504).to(DEV).view(3 * Dc)
    wp, bp = (PH.scaled_randn(Dc, Dc, 505) * 0.05).to(DEV), PH.scaled_randn(1, Dc, 506).to(DEV).view(Dc)
    vit_amd.set_float32_matmul_precision("high", presplit_weights=True, presplit_activations=True)
    vit_amd.set_float32_attention_precision("high", presplit=True)
    assert vit_amd.get_float32_attention_presplit()
    iq, ip = ops.weight_image_raw(wq), ops.weight_image_raw(wp)
    h1img = ops.weight_image_raw(h1)   # an activation image is the row-by-row image of the matrix
    act_count = L.lib().vit_gemm_f32_presplit_act_count

    def chain(images):
        qkv, o, xm = torch.empty(M, 3 * Dc, device=DEV), torch.empty(M, Dc, device=DEV), torch.empty(M, Dc, device=DEV)
        lse = torch.empty(Bc * Hc * N, device=DEV)
        if images:
            assert ops.linear_fwd_takes_image(h1img, wq, iq) and ops.linear_fwd_takes_image(o, wp, ip)
            assert ops.sdpa_fwd_takes_image(qkv, Bc, Hc, N, o, lse)
        ops.linear_fwd(h1img, wq, bq, out=qkv, wimg=iq, x_image=True, out_image=images)
        ops.sdpa_fwd(qkv, Bc, Hc, N, o=o, lse=lse, image=images)
        ops.linear_fwd(o, wp, bp, epi=L.EPI_RESID, resid=x, out=xm, wimg=ip, x_image=images)
        torch.cuda.synchronize()
        return xm, lse

    act_count(1)
    _counts()
    ref, lse0 = chain(False)
    assert act_count(1) == 1 and _counts() == (0, 1, 0, 0)
    got, lse1 = chain(True)
    assert act_count(1) == 2 and _counts() == (1, 1, 0, 0)
    _same(got, ref, "proj output of the image chain")
    _same(lse1, lse0, "lse of the image chain")


# ---------------------------------------------------------------------------- 6. model

def _model_case():
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
    img_count = L.lib().vit_sdpa_f32_image_count

    def predict():
        m.clip_model._text_cache = None
        with torch.no_grad():
            out = m(x).detach().clone()
        torch.cuda.synchronize()
        return out

    def gemm_mode():
        vit_amd.set_float32_matmul_precision("high", presplit_weights=True, presplit_activations=True)

    gemm_mode()
    vit_amd.set_float32_attention_precision("high", presplit=False)
    img_count(1)
    pred0 = predict()
    cache0 = vit_amd.VisualPrefixCache.build(m, x, batch_size=FS.MB)
    step0 = PS._train_step(m, x, y)
    assert img_count(1) == 0

    vit_amd.set_float32_attention_precision("high", presplit=True)
    assert cache0.ensure(m, x, batch_size=FS.MB) is False, "a cache built on f32 qkv / o was rebuilt under images"
    # which launches carried an image through attention
    seen, attn = [], []
    fwd, sdpa = ops.linear_fwd, ops.sdpa_fwd

    def spy(x2, w, *a, **k):
        if k.get("x_image") or k.get("out_image"):
            seen.append((w.data_ptr(), bool(k.get("x_image")), bool(k.get("out_image"))))
        return fwd(x2, w, *a, **k)

    def spy_attn(*a, **k):
        attn.append(bool(k.get("image")))
        return sdpa(*a, **k)

    frozen = m.clip_model.visual.transformer.resblocks[0].block_params()
    qkv_w, proj_w, fc1_w, fc2_w = (frozen[i].data_ptr() for i in (2, 4, 8, 10))
    ops.linear_fwd, ops.sdpa_fwd = spy, spy_attn
    try:
        pred1 = predict()
        n_pred = img_count(1)
        # the forward-only dense blocks both ends of which can take an image, counted from the model, not from what
        # the chain chose: of the two visual blocks the second has a DoRA-computed proj weight (no weight image), and
        # the text tower's 12 x 16 = 192 rows put its GEMMs under 64 tiles, off the MFMA path.  That leaves visual
        # block 0: one image launch; its qkv wrote an image and its proj read one, while block 1's qkv, still on the
        # activation-image chain, wrote f32.
        blocks = m.clip_model.visual.transformer.resblocks
        assert len(blocks) == 2 and FS.MT * FS.MCFG.context_length == 192
        assert n_pred == 1 and sum(attn) == 1, (n_pred, attn)
        qkv_w1 = blocks[1].block_params()[2].data_ptr()
        assert (qkv_w, True, True) in seen and (proj_w, True, False) in seen, seen
        assert (qkv_w1, True, False) in seen and (qkv_w1, True, True) not in seen, seen
        assert {w for w, xi, oi in seen if oi} == {qkv_w, fc1_w, blocks[1].block_params()[8].data_ptr()}, seen
        del seen[:], attn[:]
        step1 = PS._train_step(m, x, y)
        n_step = img_count(1)
    finally:
        ops.linear_fwd, ops.sdpa_fwd = fwd, sdpa
    # the frozen visual block 0 alone: its four GEMMs, proj counted as reading an activation image; the training
    # blocks' attention is not counted
    assert n_step == 1 and sum(attn) == 1, (n_step, attn)
    assert sorted(seen) == sorted([(qkv_w, True, True), (proj_w, True, False), (fc1_w, True, True),
                                   (fc2_w, True, False)]), seen
    _same(pred1, pred0, "no-grad predictions")
    cache1 = vit_amd.VisualPrefixCache.build(m, x, batch_size=FS.MB)
    assert img_count(1) >= 1
    _same(cache1.take(idx), cache0.take(idx), "prefix rows")
    _same(step1[0], step0[0], "predictions")
    _same(step1[1].view(1), step0[1].view(1), "loss")
    assert step1[2].keys() == step0[2].keys() and len(step1[2]) == 6
    for k in step0[2]:
        _same(step1[2][k], step0[2][k], k)

    vit_amd.set_float32_attention_precision("high", presplit=False)
    assert cache1.ensure(m, x, batch_size=FS.MB) is False, "a cache built from images was rebuilt without them"
    pred0b = predict()
    assert img_count(1) == 0, "switching off still ran an image kernel"
    _same(pred0b, pred0, "predictions after switching off")
    vit_amd.set_float32_matmul_precision("highest")
    vit_amd.set_float32_attention_precision("highest")
    return [pred1, cache1.take(idx).clone(), step1[0], step1[1].view(1)] + [step1[2][k] for k in sorted(step1[2])]


@pytest.fixture(scope="module")
def first_run():
    return _model_case()


def test_clip_hba_model_is_bit_equal_with_attention_images(first_run):
    assert len(first_run) == 4 + 6


def test_the_model_case_repeats_bit_for_bit(first_run):
    again = _model_case()
    assert len(again) == len(first_run)
    for i, (a, b) in enumerate(zip(again, first_run)):
        _same(a, b, f"run 2 against run 1, tensor {i}")


# ---------------------------------------------------------------------------- 7. one end cannot

def test_a_block_whose_proj_cannot_read_an_image_keeps_f32_attention(monkeypatch):
    """Both ends or neither: with proj refused an image (the query patched to say no for its weight) the qkv GEMM is
    not asked for one and attention runs the f32 entry; without the patch the same model runs the image kernels."""
    import vit_amd
    from vit_amd import ops
    torch.manual_seed(3)
    m = vit_amd.VisionTransformer(img_size=224, patch_size=16, embed_dim=512, depth=2, num_heads=8, num_classes=10,
                                  compute_dtype=F32).to(DEV)
    x = torch.randn(16, 3, 224, 224, generator=torch.Generator().manual_seed(4)).to(DEV)
    projs = {blk.attn.proj.weight.data_ptr() for blk in m.blocks}
    img_count = L.lib().vit_sdpa_f32_image_count

    def predict():
        with torch.no_grad():
            out = m(x).detach().clone()
        torch.cuda.synchronize()
        return out

    vit_amd.set_float32_matmul_precision("high", presplit_weights=True, presplit_activations=True)
    vit_amd.set_float32_attention_precision("high", presplit=False)
    img_count(1)
    ref = predict()
    assert img_count(1) == 0
    vit_amd.set_float32_attention_precision("high", presplit=True)
    ctl = predict()
    assert img_count(1) >= 1, "the unpatched model ran no image kernel: the case below would show nothing"
    _same(ctl, ref, "unpatched")
    real = ops.linear_fwd_takes_image
    asked = []

    def no_proj(x2d, w, wimg):
        return False if w.data_ptr() in projs else real(x2d, w, wimg)

    fwd = ops.linear_fwd

    def spy(x2, w, *a, **k):
        asked.append(bool(k.get("out_image")) and w.shape[0] == 3 * 512)   # a qkv GEMM asked for an image
        return fwd(x2, w, *a, **k)

    monkeypatch.setattr(ops, "linear_fwd_takes_image", no_proj)
    monkeypatch.setattr(ops, "linear_fwd", spy)
    got = predict()
    assert img_count(1) == 0 and not any(asked), "an image kernel ran although proj cannot read an image"
    _same(got, ref, "proj refused")
