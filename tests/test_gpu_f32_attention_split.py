"""GPU: the fp32 "high" attention mode (resident f32 attention as three bf16 MFMA products) against
the float64 reference of oracle/attn_cases.py, every figure held to the bound tests/test_f32_attention_split_host.py
derives: max(project f32 bound, 4 x torch-f32 error) + 2 x (the float64 restatement's own error on the case).

B = H = 2 throughout, forward and backward with dbias; the backward is fed the reference's o and lse.  The split
counter (``vit_sdpa_f32_split_count``) shows which kernels ran.  Every figure is printed as a ``FIG`` line before it
is asserted."""
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import attn_cases as AC  # noqa: E402
from oracle import clip_ref as CR  # noqa: E402
from vit_amd import _lib as L  # noqa: E402
from vit_amd import ops  # noqa: E402

import test_f32_attention_split_host as HS  # noqa: E402

DEV = "cuda"
F32 = torch.float32
B, H = 2, 2
D = H * 64
HARD = [k for k in AC.KINDS if k != "base"]
SENT = -12288.0


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    L.load()
    L.lib().vit_sdpa_long_config(-1)
    L.lib().vit_sdpa_bwd_variant(-1)


@pytest.fixture(autouse=True)
def _restore_highest():
    yield
    ops.set_float32_attention_precision("highest")
    ops.set_float32_matmul_precision("highest")


def _count(reset=0):
    return L.lib().vit_sdpa_f32_split_count(reset)


_CASES = {}


def _case(kind, N, causal=False, scale=0.125):
    key = (kind, N, causal, scale)
    if key not in _CASES:
        c = AC.make_case(kind, B, H, N, F32, causal=causal, scale=scale)
        d = SimpleNamespace(qkv=c.qkv.to(DEV), do=c.do.to(DEV), o_in=c.o.float().to(DEV), lse_in=c.lse.float().to(DEV))
        _CASES[key] = (c, d)
    return _CASES[key]


def _fwd(c, d, qkv=None, o=None):
    return ops.sdpa_fwd(d.qkv if qkv is None else qkv, B, H, c.N, o=o, scale=c.scale, causal=c.causal)


def _bwd(c, d, qkv=None, o_in=None, do=None, dqkv=None):
    dbias = torch.full((3 * D,), float("nan"), device=DEV)
    dqkv = ops.sdpa_bwd(d.qkv if qkv is None else qkv, d.o_in if o_in is None else o_in, d.do if do is None else do,
                        d.lse_in, B, H, c.N, dqkv=dqkv, scale=c.scale, dbias=dbias, causal=c.causal)
    return dqkv, dbias


def _run_high(kind, N, causal=False, scale=0.125, fwd=True, bwd=True):
    """One forward and one backward in "high" on the case: the counter advances by one per call and every figure
    stays inside its derived bound."""
    c, d = _case(kind, N, causal, scale)
    bd = HS.bounds(c)
    ops.set_float32_attention_precision("high")
    n0 = _count()
    got = {}
    if fwd:
        o, lse = _fwd(c, d)
        got.update(HS.figures(c, o=o, lse=lse))
    if bwd:
        dqkv, dbias = _bwd(c, d)
        got.update(HS.figures(c, grads=dqkv, colsum=dbias))
    torch.cuda.synchronize()
    assert _count() - n0 == fwd + bwd, "a call did not take the bf16x3 kernels"
    bad = []
    for k, err in got.items():
        bound, te, re_ = bd[k]
        print(f"FIG f32x3 | {kind} N={N}{' causal' if causal else ''} scale={scale} | {k} {err:.3e} (bound {bound:.1e}; "
              f"torch-f32 {te:.1e}, restatement {re_:.1e})")
        if not err <= bound:  # a NaN is past every bound
            bad.append(f"{k} {err:.3e} > {bound:.1e}")
    assert not bad, f"{kind} N={N} causal={causal} scale={scale}: " + "; ".join(bad)


# ---------------------------------------------------------------------------- every tile count

def _nt_cases():
    return [pytest.param(N, causal, id=f"NT{nt}-N{N}{'-causal' if causal else ''}") for nt in range(1, 19)
            for N, causal in ((16 * nt - 15, False), (16 * nt, False), (16 * nt - 15, True))]


@pytest.mark.parametrize("N,causal", _nt_cases())
def test_every_resident_tile_count(N, causal):
    _run_high("base", N, causal=causal)


# ---------------------------------------------------------------------------- hard kinds, scales

@pytest.mark.parametrize("kind", HARD)
@pytest.mark.parametrize("N,causal", [(257, False), (77, True)], ids=["N257", "N77-causal"])
def test_hard_inputs(N, causal, kind):
    """As tests/test_gpu_attention_conformance.py runs ``res-f32``: the non-causal backward on ``offset`` takes the
    milder ``offset4`` (the f32 accumulation of raw scores ~ 2400, not this mode, is what misses there)."""
    if kind in AC.MILDER and not causal:
        _run_high(kind, N, bwd=False)
        _run_high(AC.MILDER[kind], N)
    else:
        _run_high(kind, N, causal=causal)


@pytest.mark.parametrize("scale", [0.05, 0.3])
def test_scale(scale):
    _run_high("base", 193, scale=scale)


# ---------------------------------------------------------------------------- views

def test_views_match_contiguous():
    """Operands that are views inside poisoned, wider buffers: the contiguous call's bits, the poison intact."""
    N = 197
    c, d = _case("base", N)
    ops.set_float32_attention_precision("high")
    n0 = _count()
    o0, lse0 = _fwd(c, d)
    dq0, db0 = _bwd(c, d)
    R = B * N
    w = SimpleNamespace(qkv=torch.full((R, 3 * D + 16), SENT, device=DEV), o=torch.full((R, D + 8), SENT, device=DEV),
                        o_in=torch.full((R, D + 8), SENT, device=DEV), do=torch.full((R, D + 8), SENT, device=DEV),
                        dqkv=torch.full((R, 3 * D + 8), SENT, device=DEV))
    v = SimpleNamespace(qkv=w.qkv[:, 8:8 + 3 * D], o=w.o[:, :D], o_in=w.o_in[:, :D], do=w.do[:, :D],
                        dqkv=w.dqkv[:, :3 * D])
    v.qkv.copy_(d.qkv)
    v.o_in.copy_(d.o_in)
    v.do.copy_(d.do)
    for t in vars(v).values():
        assert t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0 and not t.is_contiguous()
    o1, lse1 = _fwd(c, d, qkv=v.qkv, o=v.o)
    dq1, db1 = _bwd(c, d, qkv=v.qkv, o_in=v.o_in, do=v.do, dqkv=v.dqkv)
    torch.cuda.synchronize()
    assert _count() - n0 == 4
    assert o1.data_ptr() == w.o.data_ptr() and dq1.data_ptr() == w.dqkv.data_ptr()
    for a, b, name in ((o0, o1, "o"), (lse0, lse1, "lse"), (dq0, dq1, "dqkv"), (db0, db1, "dbias")):
        assert torch.equal(a, b), f"{name}: the call on views and the contiguous call differ"
    assert (w.qkv[:, :8] == SENT).all() and (w.qkv[:, 8 + 3 * D:] == SENT).all()
    assert torch.equal(w.qkv[:, 8:8 + 3 * D], d.qkv)
    for name, width in (("o", D), ("o_in", D), ("do", D), ("dqkv", 3 * D)):
        assert (getattr(w, name)[:, width:] == SENT).all(), f"{name}: written outside the view"
    assert torch.equal(w.o_in[:, :D], d.o_in) and torch.equal(w.do[:, :D], d.do)


# ---------------------------------------------------------------------------- the lo terms, exactly

def test_lo_terms_of_pv_are_present_and_carry_the_right_sign():
    """q = 0 makes every p exactly 1, and integer v with |v| <= 511 keeps every partial sum an integer below 2^24:
    "high" must return the bits of "highest", which a P V without its v_lo term (v rounded to bf16) does not."""
    N = 257
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(B * N, 3 * D, generator=g)
    qkv[:, :D] = 0
    qkv[:, 2 * D:] = torch.randint(-511, 512, (B * N, D), generator=g).float()
    rounded = qkv.clone()
    rounded[:, 2 * D:] = qkv[:, 2 * D:].to(torch.bfloat16).float()
    assert not torch.equal(rounded, qkv)
    qkv, rounded = qkv.to(DEV), rounded.to(DEV)
    o_highest, lse_highest = ops.sdpa_fwd(qkv, B, H, N)
    o_bf16v, _ = ops.sdpa_fwd(rounded, B, H, N)
    ops.set_float32_attention_precision("high")
    n0 = _count()
    o_high, lse_high = ops.sdpa_fwd(qkv, B, H, N)
    torch.cuda.synchronize()
    assert _count() - n0 == 1
    assert torch.equal(o_high, o_highest) and torch.equal(lse_high, lse_highest)
    assert not torch.equal(o_high, o_bf16v)
    want = AC.pack(AC.unpack(qkv[:, 2 * D:].double().cpu(), B, H, N).mean(2, keepdim=True).expand(B, H, N, 64))
    assert AC.rel_max(o_high, want) <= AC.F32_O


def test_high_differs_from_highest_and_highest_returns():
    """On ``base`` at 257 tokens the two modes differ in bits; after switching back "highest" gives the bits it gave
    before and the counter stands still."""
    c, d = _case("base", 257)
    before = _fwd(c, d) + _bwd(c, d)
    ops.set_float32_attention_precision("high")
    high = _fwd(c, d) + _bwd(c, d)
    ops.set_float32_attention_precision("highest")
    n0 = _count()
    after = _fwd(c, d) + _bwd(c, d)
    torch.cuda.synchronize()
    assert _count() == n0
    for a, b, h, name in zip(before, after, high, ("o", "lse", "dqkv", "dbias")):
        assert torch.equal(a, b), f"{name}: highest after the switch is not highest before it"
        assert not torch.equal(a, h), f"{name}: high gave the bits of highest"


# ---------------------------------------------------------------------------- what stays exact f32

def _misaligned(x):
    w = torch.full((x.shape[0], x.shape[1] + 2), SENT, dtype=x.dtype, device=x.device)
    v = w[:, :x.shape[1]]
    v.copy_(x)
    assert v.stride(0) % 4 == 2
    return v


@pytest.mark.parametrize("path", ["streamed", "generic"])
def test_fallbacks_stay_exact_under_high(path):
    """Past 288 tokens (the streamed f32 kernels) and with a misaligned row stride (the generic kernels) the mode
    changes nothing: the counter stands still and the bits are those of "highest"."""
    N = 289 if path == "streamed" else 50
    c, d = _case("base", N)
    qkv = _misaligned(d.qkv) if path == "generic" else None
    lib = L.lib()
    s0 = lib.vit_sdpa_long_f32_count(0)
    a = _fwd(c, d, qkv=qkv) + _bwd(c, d, qkv=qkv)
    ops.set_float32_attention_precision("high")
    n0 = _count()
    b = _fwd(c, d, qkv=qkv) + _bwd(c, d, qkv=qkv)
    torch.cuda.synchronize()
    assert _count() == n0
    assert lib.vit_sdpa_long_f32_count(0) - s0 == (4 if path == "streamed" else 0)
    for x, y, name in zip(a, b, ("o", "lse", "dqkv", "dbias")):
        assert torch.equal(x, y), name


# ---------------------------------------------------------------------------- model level

MB, MT, MR = 4, 5, 4


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.fixture(scope="module")
def model_and_oracle():
    """A CLIP_TINY CLIP-HBA model on the GPU and the float64 oracle step on the CPU, computed once."""
    import vit_amd
    from vit_amd import clip
    cfg = CR.CLIP_TINY
    torch.manual_seed(0)
    p = CR.init_params(cfg, seed=5)
    prompts = CR.synthetic_prompts(MT, cfg, seed=6)
    cm = clip.build_model(p, compute_dtype=F32)
    m = vit_amd.CLIPHBA([f"c{i}" for i in range(MT)], "ViT-L/14", pos_embedding=True, clip_model=cm,
                        tokenized_prompts=prompts)
    vit_amd.apply_dora_to_ViT(m, n_vision_layers=1, n_transformer_layers=1, r=MR)
    vit_amd.switch_dora_layers(m, freeze_all=True, dora_state=True)
    sd = m.state_dict()
    d = CR.init_dora(p, cfg, r=MR, seed=0, n_vision_layers=1, n_transformer_layers=1)
    for k in list(d):
        if not k.endswith(".scaling"):
            d[k] = sd[k].detach().clone().float()
    g = torch.Generator().manual_seed(7)
    x = torch.randn(MB, 3, cfg.image_resolution, cfg.image_resolution, generator=g)
    y = torch.randn(MB, MT, generator=g) * 0.5 + 1.0
    dbl = lambda t: t.double() if torch.is_tensor(t) and t.is_floating_point() else t
    ref_loss, ref_pred, ref_grads = CR.train_step({k: dbl(v) for k, v in p.items()}, {k: dbl(v) for k, v in d.items()},
                                                  {}, x.double(), prompts, y.double(), cfg, lr=3e-4, pos_embedding=True)
    assert ref_pred.dtype == torch.float64
    return m.to(DEV), x.to(DEV), y.to(DEV), ref_loss, ref_pred, ref_grads


@pytest.mark.parametrize("gemm", ["highest", "high"])
def test_model_step_matches_the_float64_oracle(model_and_oracle, gemm):
    import vit_amd
    m, x, y, ref_loss, ref_pred, ref_grads = model_and_oracle
    vit_amd.set_float32_matmul_precision(gemm)
    vit_amd.set_float32_attention_precision("high")
    m.clip_model._text_cache = None
    for q in m.parameters():
        q.grad = None
    _count(1)
    pred = m(x)
    loss = vit_amd.mse_loss(pred, y)
    loss.backward()
    torch.cuda.synchronize()
    assert _count() > 0, "no attention of the step took the bf16x3 kernels"
    grads = {k: q.grad for k, q in m.named_parameters() if q.requires_grad}
    assert len(grads) == len(ref_grads) == 6
    worst = {"pred": _rel(pred, ref_pred), "loss": abs(float(loss.detach()) - ref_loss) / abs(ref_loss)}
    worst.update({k: _rel(grads[k], rg) for k, rg in ref_grads.items()})
    print(gemm, {k.split("clip_model.")[-1]: f"{v:.2e}" for k, v in worst.items()})
    for k, v in worst.items():
        assert v < 1e-3, (gemm, k, v)


def test_prefix_cache_is_rebuilt_across_the_attention_switch(model_and_oracle):
    import vit_amd
    m = model_and_oracle[0]
    raw = lambda t: t.contiguous().view(torch.int32)
    imgs = torch.randn(8, 3, 32, 32, generator=torch.Generator().manual_seed(3)).to(DEV)
    idx = torch.arange(4)
    cache = vit_amd.VisualPrefixCache.build(m, imgs, batch_size=4)
    assert cache.ensure(m, imgs, batch_size=4) is False
    rows_highest = cache.take(idx).clone()
    vit_amd.set_float32_attention_precision("high")
    assert not cache.valid_for(m, imgs)
    _count(1)
    assert cache.ensure(m, imgs, batch_size=4) is True and cache.builds == 2
    assert _count() > 0
    rows_high = cache.take(idx)
    assert not torch.equal(raw(rows_high), raw(rows_highest)), "the rebuilt rows are the other mode's"
    assert _rel(rows_high, rows_highest) < 1e-3
    vit_amd.set_float32_attention_precision("highest")
    assert cache.ensure(m, imgs, batch_size=4) is True  # and back: rebuilt again, the first rows return
    assert torch.equal(raw(cache.take(idx)), raw(rows_highest))
