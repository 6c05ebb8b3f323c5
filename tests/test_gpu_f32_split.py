"""GPU: the fp32 "high" GEMM mode (bf16x3 on the f32 MFMA path; f32m SPLIT = 1).

  1. exact cases: the f32 cases tests/test_gpu_gemm_exact.py drives through the MFMA path (forward with every
     epilogue, input gradient, weight gradient with its split-K partials, every layout) and an f32 padded patch
     embedding, run again in "high" inside the same poisoned, strided views: their operands are bf16 values, so
     lo = 0 and the result is the float64 reference bit for bit;
  2. stream-K in "high": a cut tile on a registered workspace equals the reference and the plain launch;
  3. cross terms: 9-bit integer operands make hi*lo and lo*hi non-zero and every sum exact, so the result is
     sum(p q - p_lo q_lo) bit for bit: three products, not the f32 form and not bf16;
  4. the bound (3 * 2^-18 + (R + 3) * 2^-24) |P||Q|^T on randn operands in all four layouts, and
     (R + 3) * 2^-24 |P||Q|^T in "highest";
  5. what the switch must not touch: bf16 GEMMs, f32 attention, GEMMs under 64 tiles;
  6. a two-block CLIP-HBA model in fp32: the 1e-3 gate of the fp32 path against the float64 oracle in both
     modes, the prefix cache rebuilt across the switch, RSA within +-0.005.

The restatement of the split rule lives in tests/test_f32_split_host.py (CPU-checked against the bound).
Every test leaves the process in "highest".
"""
import functools
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_f32_split_host as H  # noqa: E402
import test_gpu_gemm_exact as GE  # noqa: E402
from oracle import clip_ref as CR  # noqa: E402
from oracle import gemm_cases as G  # noqa: E402
from vit_amd import _lib as L  # noqa: E402

DEV = "cuda"
F32, BF = torch.float32, torch.bfloat16
Buf, _vec, _exact, _settle, _raw, _stream = GE.Buf, GE._vec, GE._exact, GE._settle, GE._raw, GE._stream


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    L.load()


@pytest.fixture(autouse=True)
def _restore_highest():
    yield
    L.lib().vit_gemm_f32_precision(0)


def _mode(high):
    L.lib().vit_gemm_f32_precision(1 if high else 0)


def _counts(reset=1):
    lib = L.lib()
    return lib.vit_gemm_f32_count(reset), lib.vit_gemm_f32_split_count(reset)


def _all_split(what):
    n, ns = _counts()
    assert n > 0 and ns == n, f"{what}: {ns} of {n} f32 MFMA-path launches ran the split form"
    return n


# ---------------------------------------------------------------------------- 1. exact cases

def test_exact_forward_epilogues_in_high():
    _mode(True)
    _counts()
    GE.test_f32_mfma_forward_epilogues()   # store, residual, GELU / QuickGELU pairs and their act-only forms
    assert _all_split("forward epilogues") == 6   # store, residual, two pairs, two act-only


def test_exact_input_gradient_in_high():
    _mode(True)
    _counts()
    GE.test_f32_mfma_input_gradient_with_dbias()
    _all_split("input gradient")


def test_exact_every_layout_in_high():
    _mode(True)
    _counts()
    GE.test_f32_mfma_every_layout()
    assert _all_split("layouts") == 4


def test_exact_weight_gradient_and_partials_in_high():
    M, N, K, split = G.WGRAD_F32[0]
    assert G.f32_branch(G.CR, G.CR, N, K, M, split) == "mfma"
    _mode(True)
    _counts()
    GE.test_weight_gradient_f32(M, N, K, split)
    _all_split("weight gradient")


def test_exact_padded_patch_embedding_in_high():
    """An f32 patch embedding with 64 output tiles and a padded reduction (zeros in the pad columns)."""
    B, np_, D, K = 2, 512, 1024, 64
    assert G.f32_branch(G.RC, G.RC, B * np_, D, K) == "mfma"
    c = G.patch_case(B, np_, D, K, F32)
    ldu = K + 8
    U, W = Buf(B * np_, K, F32, c.U, ld=ldu), Buf(D, K, F32, c.W, ld=ldu)
    for t in (U, W):
        t.buf[t.off:t.off + t.rows * t.ld].view(t.rows, t.ld)[:, K:] = 0
        t.snap = t.buf.clone()
    b, pos = _vec(D, c.bias), Buf(np_ + 1, D, F32, c.pos)
    got = {}
    for high in (True, False):
        _mode(high)
        _counts()
        x = Buf(B * (np_ + 1), D, F32)
        L.call("vit_patch_embed_fwd_ld", L.F32, B, np_, D, K, U.ptr, U.ld, W.ptr, W.ld, b.ptr, pos.ptr, x.ptr, _stream())
        what = f"f32 patch embed high={high}"
        _settle(what, outs=[x], ins=[U, W, b, pos])
        assert _counts() == (1, 1 if high else 0), what
        tok = x.v.view(B, np_ + 1, D)
        assert bool((tok[:, 0] == GE.SENT).all()), what + ": a class-token row was written"
        got[high] = tok[:, 1:].cpu().contiguous()
        assert torch.equal(_raw(got[high]), _raw(c.rows.float().contiguous())), what + ": patch rows"


# ---------------------------------------------------------------------------- 2. stream-K

def test_stream_k_cut_tile_in_high():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    M, N, K = (2 * cus // 8 + 1) * 128, 1024, 64   # MI355X: 65 x 8 = 520 tiles on 512 slots, the persistent form
    if cus == G.CUS:                                # with a tile cut between workgroups
        assert M == 65 * 128 and G.f32_branch(G.RC, G.RC, M, N, K, streamk_ws=True) == "streamk"
    c = G.mm_case(M, N, K, F32)
    g = 2 * cus
    side = torch.cuda.Stream()
    part = torch.zeros(g * 2 * 128 * 128, dtype=F32, device=DEV)
    cnt = torch.zeros(g, dtype=torch.int32, device=DEV)
    x, w, b = Buf(M, K, F32, c.p, ld=K + 4), Buf(N, K, F32, c.q), _vec(N, c.bias)
    ref = c.pre.float().to(DEV)
    assert torch.equal(ref.double().cpu(), c.pre)
    torch.cuda.synchronize()
    _mode(True)
    _counts()
    outs = []
    try:
        for registered in (True, False):
            if registered:
                L.call("vit_gemm_streamk_workspace", side.cuda_stream, part.data_ptr(), part.numel() * 4, cnt.data_ptr(), g)
            else:
                L.call("vit_gemm_streamk_workspace", side.cuda_stream, None, 0, None, 0)
            y = Buf(M, N, F32, ld=N + 4)
            torch.cuda.synchronize()
            L.call("vit_linear_fwd", L.F32, L.F32, L.EPI_STORE, M, N, K, x.ptr, x.ld, w.ptr, b.ptr, y.ptr, y.ld, None, None,
                   side.cuda_stream)
            what = f"stream-K in high, workspace registered={registered}"
            _settle(what, outs=[y], ins=[x, w, b])
            assert torch.equal(_raw(y.v.contiguous()), _raw(ref)), what + ": not the exact result"
            assert int(cnt.abs().sum()) == 0, "the stream-K counters must come back zero"
            outs.append(y.v.contiguous())
    finally:
        L.call("vit_gemm_streamk_workspace", side.cuda_stream, None, 0, None, 0)
    assert torch.equal(_raw(outs[0]), _raw(outs[1]))
    assert _all_split("stream-K") == 2


# ---------------------------------------------------------------------------- 3. cross terms

VARIANTS = {"p9": (True, False), "q9": (False, True), "both": (True, True)}


def _case(p, q):
    return types.SimpleNamespace(M=p.shape[0], N=q.shape[0], R=p.shape[1], p=p, q=q, qT=q.T.contiguous(),
                                 bias=torch.zeros(q.shape[0]))


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_cross_terms_forward_and_input_gradient(variant):
    p9, q9 = VARIANTS[variant]
    p, q = H.nine_bit_case(1024, 1024, 128, p9, q9)
    ref, full = H.x3_f64(p, q), p.double() @ q.double().T
    (ph, _), (qh, _) = H.split(p), H.split(q)
    assert (variant == "both") == (not torch.equal(ref, full))
    assert not torch.equal(ref, ph.double() @ qh.double().T)
    c = _case(p, q)
    _mode(True)
    _counts()
    y, _ = GE._fwd(c, odt=F32, bias=False, pad=4, what=f"9-bit fwd {variant}")
    _exact(y, ref, f"9-bit fwd {variant}")
    dx, _, _ = GE._dgrad(c, odt=F32, pad=4, what=f"9-bit dgrad {variant}")
    _exact(dx, ref, f"9-bit dgrad {variant}")
    assert _all_split(f"9-bit {variant}") == 2
    if variant == "both":
        assert not torch.equal(y.v.cpu().double(), full)
        _mode(False)   # and "highest" gives the full product on the same views
        y, _ = GE._fwd(c, odt=F32, bias=False, pad=4, what="9-bit fwd highest")
        _exact(y, full, "9-bit fwd highest")
        assert _counts() == (1, 0)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_cross_terms_weight_gradient(variant):
    """dW [N, K] = dy [M, N]^T x [M, K]: the reduction is the M = 128 rows, x thinned to one row in four."""
    p9, q9 = VARIANTS[variant]
    M, N, K = 128, 1024, 1024
    pT, qT = H.nine_bit_case(N, K, M, p9, q9)   # [N, M], [K, M]: the operands as the reduction sees them
    ref = H.x3_f64(pT, qT)
    dy, x = Buf(M, N, F32, pT.T.contiguous(), ld=N + 8), Buf(M, K, F32, qT.T.contiguous(), ld=K + 16)
    dW = _vec(N * K)
    _mode(True)
    _counts()
    L.call("vit_linear_wgrad", L.F32, M, N, K, dy.ptr, dy.ld, x.ptr, x.ld, dW.ptr, 1, None, 0, _stream())
    _settle(f"9-bit wgrad {variant}", outs=[dW], ins=[dy, x])
    _exact(dW, ref.reshape(1, N * K), f"9-bit wgrad {variant}")
    _all_split(f"9-bit wgrad {variant}")
    if variant == "both":
        assert not torch.equal(dW.v.cpu().double().view(N, K), pT.double() @ qT.double().T)


# ---------------------------------------------------------------------------- 4. the bound

@functools.lru_cache(maxsize=None)
def _randn_case(R):
    g = torch.Generator().manual_seed(41 + R)
    M = N = 1024

    def draw(rows):  # |x| kept in [2^-20, 2^20]: lo cannot underflow
        x = torch.randn(rows, R, generator=g)
        return torch.copysign(x.abs().clamp(2.0 ** -20, 2.0 ** 20), x)

    p, q = draw(M), draw(N)
    ref = p.double() @ q.double().T
    return p, q, ref, H.bound(p, q, True), H.bound(p, q, False)


@pytest.mark.parametrize("R", [32, 1024, 4096])
def test_bound_on_randn_in_every_layout(R):
    p, q, ref, b_high, b_highest = _randn_case(R)
    M, N = p.shape[0], q.shape[0]
    pd, qd = p.to(DEV), q.to(DEV)
    ops_ = {G.RC: (pd, qd), G.CR: (pd.T.contiguous(), qd.T.contiguous())}
    for high, bnd in ((True, b_high), (False, b_highest)):
        _mode(high)
        _counts()
        for pl in (G.RC, G.CR):
            for ql in (G.RC, G.CR):
                P, Q = ops_[pl][0], ops_[ql][1]
                C = torch.empty(M, N, dtype=F32, device=DEV)
                L.call("vit_gemm", L.F32, L.F32, pl, ql, L.EPI_STORE, M, N, R, P.data_ptr(), P.stride(0), Q.data_ptr(),
                       Q.stride(0), C.data_ptr(), N, None, None, 0, None, 1, _stream())
                torch.cuda.synchronize()
                got = C.cpu().double()
                assert bool(torch.isfinite(got).all())
                frac = ((got - ref).abs() / bnd).max().item()
                rms = ((got - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()
                print(f"R={R} layouts {pl}{ql} high={high}: {frac:.3f} of the bound, rms relative error {rms:.2e}")
                assert frac <= 1.0, (R, pl, ql, high, frac)
        assert _counts() == (4, 4 if high else 0)


# ---------------------------------------------------------------------------- 5. what the switch must not touch

def test_switch_leaves_bf16_gemm_f32_attention_and_small_gemms_alone():
    from vit_amd import ops
    g = torch.Generator().manual_seed(3)
    xb = torch.randn(1024, 256, generator=g).to(BF).to(DEV)
    wb = torch.randn(1024, 256, generator=g).to(BF).to(DEV)
    bias = torch.randn(1024, generator=g).to(DEV)
    B, Hh, N = 2, 2, 197
    qkv = torch.randn(B * N, 3 * Hh * 64, generator=g).to(DEV)
    ps, qs = torch.randn(256, 64, generator=g).to(DEV), torch.randn(256, 64, generator=g).to(DEV)  # 4 tiles
    assert G.f32_branch(G.RC, G.RC, 256, 256, 64) == "gen"
    got = {}
    for high in (False, True):
        _mode(high)
        _counts()
        y = ops.linear_fwd(xb, wb, bias)
        o, lse = ops.sdpa_fwd(qkv, B, Hh, N)
        c = torch.empty(256, 256, dtype=F32, device=DEV)
        L.call("vit_gemm", L.F32, L.F32, G.RC, G.RC, L.EPI_STORE, 256, 256, 64, ps.data_ptr(), 64, qs.data_ptr(), 64,
               c.data_ptr(), 256, None, None, 0, None, 1, _stream())
        torch.cuda.synchronize()
        assert _counts() == (0, 0), "a bf16 GEMM, an attention or a small GEMM moved the f32 MFMA-path counters"
        got[high] = (y, o, lse, c)
    for a, b in zip(got[False], got[True]):
        assert bool(torch.isfinite(a.float()).all()) and torch.equal(_raw(a.contiguous()), _raw(b.contiguous()))


# ---------------------------------------------------------------------------- 6. model level

MCFG = CR.CLIPConfig(image_resolution=224, vision_patch=16, vision_width=512, vision_layers=2, vision_heads=8,
                     embed_dim=256, context_length=16, vocab_size=512, text_width=512, text_layers=2, text_heads=8)
MB, MT, MR = 16, 12, 8   # 16 x 197 = 3152 token rows: every Linear of a visual block has at least 64 tiles


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _model():
    import vit_amd
    from vit_amd import clip
    p = CR.init_params(MCFG, seed=5)
    prompts = CR.synthetic_prompts(MT, MCFG, seed=6)
    cm = clip.build_model(p, compute_dtype=F32)
    m = vit_amd.CLIPHBA([f"c{i}" for i in range(MT)], "ViT-L/14", pos_embedding=True, clip_model=cm,
                        tokenized_prompts=prompts)
    vit_amd.apply_dora_to_ViT(m, n_vision_layers=1, n_transformer_layers=1, r=MR)
    vit_amd.switch_dora_layers(m, freeze_all=True, dora_state=True)
    return m, p, prompts


@pytest.fixture(scope="module")
def model_and_oracle():
    """The product model on the GPU and the float64 oracle step on the CPU, computed once for both modes."""
    torch.manual_seed(0)
    m, p, prompts = _model()
    sd = m.state_dict()
    d = CR.init_dora(p, MCFG, r=MR, seed=0, n_vision_layers=1, n_transformer_layers=1)
    for k in list(d):
        if not k.endswith(".scaling"):
            d[k] = sd[k].detach().clone().float()
    g = torch.Generator().manual_seed(7)
    x = torch.randn(MB, 3, 224, 224, generator=g)
    y = torch.randn(MB, MT, generator=g) * 0.5 + 1.0
    dbl = lambda t: t.double() if torch.is_tensor(t) and t.is_floating_point() else t
    p64 = {k: dbl(v) for k, v in p.items()}
    d64 = {k: dbl(v) for k, v in d.items()}
    ref_loss, ref_pred, ref_grads = CR.train_step(p64, d64, {}, x.double(), prompts, y.double(), MCFG, lr=3e-4,
                                                  pos_embedding=True)
    assert ref_pred.dtype == torch.float64
    return m.to(DEV), x.to(DEV), y.to(DEV), ref_loss, ref_pred, ref_grads


@pytest.mark.parametrize("mode", ["highest", "high"])
def test_model_step_matches_the_float64_oracle(model_and_oracle, mode):
    import vit_amd
    m, x, y, ref_loss, ref_pred, ref_grads = model_and_oracle
    vit_amd.set_float32_matmul_precision(mode)
    m.clip_model._text_cache = None
    for q in m.parameters():
        q.grad = None
    _counts()
    pred = m(x)
    loss = vit_amd.mse_loss(pred, y)
    loss.backward()
    torch.cuda.synchronize()
    n, ns = _counts()
    assert n > 0 and ns == (n if mode == "high" else 0), (mode, n, ns)
    grads = {k: q.grad for k, q in m.named_parameters() if q.requires_grad}
    assert len(grads) == len(ref_grads) == 6
    worst = {"pred": _rel(pred, ref_pred), "loss": abs(float(loss.detach()) - ref_loss) / abs(ref_loss)}
    worst.update({k: _rel(grads[k], rg) for k, rg in ref_grads.items()})
    print(mode, {k.split("clip_model.")[-1]: f"{v:.2e}" for k, v in worst.items()})
    for k, v in worst.items():
        assert v < 1e-3, (mode, k, v)


def test_prefix_cache_is_rebuilt_across_the_switch_and_rsa_stays(model_and_oracle):
    import vit_amd
    from vit_amd import sweep as S
    m = model_and_oracle[0]
    imgs = torch.randn(48, 3, 224, 224, generator=torch.Generator().manual_seed(3)).to(DEV)
    a = np.random.default_rng(1).random((48, 48))
    rdm = (a + a.T) / 2
    np.fill_diagonal(rdm, 0)
    idx = torch.arange(16)
    cache = vit_amd.VisualPrefixCache.build(m, imgs, batch_size=16)
    assert cache.ensure(m, imgs, batch_size=16) is False
    rows_highest = cache.take(idx).clone()
    rho_highest, _ = S.behavioral_rsa(m, imgs, rdm)
    vit_amd.set_float32_matmul_precision("high")
    assert not cache.valid_for(m, imgs)
    _counts()
    assert cache.ensure(m, imgs, batch_size=16) is True and cache.builds == 2
    _all_split("the rebuilt prefix")
    fresh = vit_amd.VisualPrefixCache.build(m, imgs, batch_size=16)
    rows_high = cache.take(idx)
    assert torch.equal(_raw(rows_high), _raw(fresh.take(idx)))
    assert not torch.equal(_raw(rows_high), _raw(rows_highest)), "the rebuilt rows are the other mode's"
    rho_high, _ = S.behavioral_rsa(m, imgs, rdm)
    rho_cached, _ = S.behavioral_rsa(m, imgs, rdm, cache_visual_prefix=cache)
    print(f"rho highest {rho_highest:.6f} high {rho_high:.6f} high, cached {rho_cached:.6f}")
    assert abs(rho_high - rho_highest) <= 0.005, (rho_high, rho_highest)
    assert abs(rho_cached - rho_highest) <= 0.005, (rho_cached, rho_highest)
    vit_amd.set_float32_matmul_precision("highest")
    assert cache.ensure(m, imgs, batch_size=16) is True   # and back: rebuilt again, the first rows return
    assert torch.equal(_raw(cache.take(idx)), _raw(rows_highest))
