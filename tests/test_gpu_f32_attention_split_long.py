"""GPU: streamed f32 attention past 288 tokens as three bf16 MFMA products
(``set_float32_attention_precision("high", long_sequences=True)``: attn_fwd_stream_x3, attn_bwd_dq_stream_x3,
attn_bwd_dkv_stream_x3) against the float64 reference of oracle/attn_cases.py.  Every figure is held
to the bound tests/test_f32_attention_split_host.py derives for the case -- max(project f32 bound, 4 x torch-f32
error) + 2 x (the float64 restatement's own error) -- which tests/test_f32_attention_split_long_host.py shows to
hold for the streamed (chunked) form and to be at least 10x below a kernel without its ``lo`` terms.

B = H = 2 throughout, forward and backward with dbias; the backward is fed the reference's o and lse.  Three counters
show which kernels ran: ``vit_sdpa_long_f32_split_count`` (the new kernels), ``vit_sdpa_long_f32_count`` (every
streamed f32 call) and ``vit_sdpa_f32_split_count`` (the resident bf16x3 kernels, which must stand still).  Every
figure is printed as a ``FIG`` line before it is asserted."""
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
NAMES = ("o", "lse", "dqkv", "dbias")


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
    L.lib().vit_sdpa_long_config(-1)


def _high_long():
    ops.set_float32_attention_precision("high", long_sequences=True)


def _counts():
    """(the new kernels, every streamed f32 call, the resident bf16x3 kernels)"""
    lib = L.lib()
    return lib.vit_sdpa_long_f32_split_count(0), lib.vit_sdpa_long_f32_count(0), lib.vit_sdpa_f32_split_count(0)


def _advance(c0):
    return tuple(a - b for a, b in zip(_counts(), c0))


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


def _run_long(kind, N, scale=0.125, fwd=True, bwd=True):
    """One forward and one backward in high + long on the case: per call the new counter and the streamed f32
    counter advance by one and the resident counter stands still; every figure stays inside its derived bound."""
    c, d = _case(kind, N, scale=scale)
    bd = HS.bounds(c)
    _high_long()
    got = {}
    if fwd:
        c0 = _counts()
        o, lse = _fwd(c, d)
        assert _advance(c0) == (1, 1, 0), "the forward did not take the streamed bf16x3 kernel"
        got.update(HS.figures(c, o=o, lse=lse))
    if bwd:
        c0 = _counts()
        dqkv, dbias = _bwd(c, d)
        assert _advance(c0) == (1, 1, 0), "the backward did not take the streamed bf16x3 kernels"
        got.update(HS.figures(c, grads=dqkv, colsum=dbias))
    torch.cuda.synchronize()
    bad = []
    for k, err in got.items():
        bound, te, re_ = bd[k]
        print(f"FIG stream x3 | {kind} N={N} scale={scale} | {k} {err:.3e} (bound {bound:.1e}; torch-f32 {te:.1e}, "
              f"restatement {re_:.1e})")
        if not err <= bound:  # a NaN is past every bound
            bad.append(f"{k} {err:.3e} > {bound:.1e}")
    assert not bad, f"{kind} N={N} scale={scale}: " + "; ".join(bad)


# ---------------------------------------------------------------------------- chunk and block edges

# 289: last chunk 33 rows, last query block 33; 320: exactly 5 chunks; 321: a 1-row last chunk; 384: 3 full blocks;
# 385: a 1-query last block; 577: the 336-pixel workload's count
@pytest.mark.parametrize("N", [289, 320, 321, 384, 385, 577])
def test_chunk_and_block_edges(N):
    _run_long("base", N)


# ---------------------------------------------------------------------------- hard kinds, scales

@pytest.mark.parametrize("kind", HARD)
def test_hard_inputs(kind):
    """As tests/test_gpu_attention_conformance.py runs ``stream-f32``: the backward on ``offset`` takes the milder
    ``offset4`` (the f32 accumulation of raw scores ~ 2400, not this mode, is what misses there)."""
    if kind in AC.MILDER:
        _run_long(kind, 321, bwd=False)
        _run_long(AC.MILDER[kind], 321)
    else:
        _run_long(kind, 321)


@pytest.mark.parametrize("scale", [0.05, 0.3])
def test_scale(scale):
    _run_long("base", 321, scale=scale)


# ---------------------------------------------------------------------------- views

def test_views_match_contiguous():
    """Operands that are views inside poisoned, wider buffers: the contiguous call's bits, the poison intact."""
    N = 321
    c, d = _case("base", N)
    _high_long()
    c0 = _counts()
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
    assert _advance(c0) == (4, 4, 0)
    assert o1.data_ptr() == w.o.data_ptr() and dq1.data_ptr() == w.dqkv.data_ptr()
    for a, b, name in zip((o0, lse0, dq0, db0), (o1, lse1, dq1, db1), NAMES):
        assert torch.equal(a, b), f"{name}: the call on views and the contiguous call differ"
    assert (w.qkv[:, :8] == SENT).all() and (w.qkv[:, 8 + 3 * D:] == SENT).all()
    assert torch.equal(w.qkv[:, 8:8 + 3 * D], d.qkv)
    for name, width in (("o", D), ("o_in", D), ("do", D), ("dqkv", 3 * D)):
        assert (getattr(w, name)[:, width:] == SENT).all(), f"{name}: written outside the view"
    assert torch.equal(w.o_in[:, :D], d.o_in) and torch.equal(w.do[:, :D], d.do)


# ---------------------------------------------------------------------------- the lo terms, exactly

def test_lo_terms_of_pv_are_present_and_carry_the_right_sign():
    """q = 0 makes every score 0, the running maximum 0 and every p exactly 1 in every chunk, and integer v with
    |v| <= 511 keeps every partial sum an integer below 2^24: high + long must return the bits of "highest", which a
    P V without its v_lo term (v rounded to bf16) does not."""
    N = 321
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
    _high_long()
    c0 = _counts()
    o_long, lse_long = ops.sdpa_fwd(qkv, B, H, N)
    torch.cuda.synchronize()
    assert _advance(c0) == (1, 1, 0)
    assert torch.equal(o_long, o_highest) and torch.equal(lse_long, lse_highest)
    assert not torch.equal(o_long, o_bf16v)
    want = AC.pack(AC.unpack(qkv[:, 2 * D:].double().cpu(), B, H, N).mean(2, keepdim=True).expand(B, H, N, 64))
    assert AC.rel_max(o_long, want) <= AC.F32_O


# ---------------------------------------------------------------------------- three states, repeatability

def test_high_alone_is_highest_and_high_long_differs_and_highest_returns():
    c, d = _case("base", 321)
    run = lambda: _fwd(c, d) + _bwd(c, d)
    before = run()
    ops.set_float32_attention_precision("high")
    c0 = _counts()
    high = run()
    assert _advance(c0) == (0, 2, 0), '"high" alone left the exact streamed kernels'
    _high_long()
    c0 = _counts()
    long_ = run()
    assert _advance(c0) == (2, 2, 0)
    ops.set_float32_attention_precision("highest")
    c0 = _counts()
    after = run()
    torch.cuda.synchronize()
    assert _advance(c0) == (0, 2, 0)
    for a, h, x, b, name in zip(before, high, long_, after, NAMES):
        assert torch.equal(a, h), f'{name}: "high" alone changed streamed attention'
        assert not torch.equal(a, x), f"{name}: high + long gave the bits of highest"
        assert torch.equal(a, b), f"{name}: highest after the switch is not highest before it"


def test_two_runs_are_bitwise_equal():
    c, d = _case("base", 577)
    _high_long()
    c0 = _counts()
    a = _fwd(c, d) + _bwd(c, d)
    b = _fwd(c, d) + _bwd(c, d)
    torch.cuda.synchronize()
    assert _advance(c0) == (4, 4, 0)
    for x, y, name in zip(a, b, NAMES):
        assert torch.equal(x, y), f"{name}: two runs in high + long differ"


# ---------------------------------------------------------------------------- what stays exact f32

def _misaligned(x):
    w = torch.full((x.shape[0], x.shape[1] + 2), SENT, dtype=x.dtype, device=x.device)
    v = w[:, :x.shape[1]]
    v.copy_(x)
    assert v.stride(0) % 4 == 2
    return v


@pytest.mark.parametrize("path", ["causal", "misaligned", "long_config0"])
def test_generic_fallbacks_stay_exact_under_high_long(path):
    """Causal, a misaligned row stride and vit_sdpa_long_config(0) at 289 tokens keep the generic kernels: the bits
    of "highest", and no counter of a streamed or bf16x3 family moves."""
    N = 289
    c, d = _case("base", N, causal=path == "causal")
    qkv = _misaligned(d.qkv) if path == "misaligned" else None
    if path == "long_config0":
        L.lib().vit_sdpa_long_config(0)
    a = _fwd(c, d, qkv=qkv) + _bwd(c, d, qkv=qkv)
    _high_long()
    c0 = _counts()
    b = _fwd(c, d, qkv=qkv) + _bwd(c, d, qkv=qkv)
    torch.cuda.synchronize()
    assert _advance(c0) == (0, 0, 0)
    for x, y, name in zip(a, b, NAMES):
        assert torch.equal(x, y), name


# ---------------------------------------------------------------------------- model level

def _rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return (a - b).abs().max().item() / (b.abs().max().item() + 1e-30)


def test_clip_hba_290_tokens_matches_oracle_in_high_long():
    """The step of tests/test_gpu_attention_long_f32.py::test_clip_hba_290_tokens_matches_oracle (CLIP-HBA + DoRA on
    a tiny CLIP with 290 visual tokens, fp32, B = 3) in high + long: predictions, loss and all nine DoRA gradients
    within that test's 1e-3 of oracle.clip_ref's CPU step; the new kernels ran; a visual prefix cache built with the
    long switch off is not valid once it is on."""
    import vit_amd
    from vit_amd import clip
    t = CR.CLIP_TINY
    cfg = CR.CLIPConfig(image_resolution=136, vision_patch=8, vision_width=128, vision_layers=3, vision_heads=2,
                        embed_dim=t.embed_dim, context_length=t.context_length, vocab_size=t.vocab_size,
                        text_width=t.text_width, text_layers=t.text_layers, text_heads=t.text_heads)
    assert cfg.vision_tokens == 290
    MB, T, r = 3, 5, 8
    p = CR.init_params(cfg, seed=15)
    prompts = CR.synthetic_prompts(T, cfg, seed=16)
    cm = clip.build_model(p, compute_dtype=F32)
    m = vit_amd.CLIPHBA([f"c{i}" for i in range(T)], "ViT-L/14", pos_embedding=True, clip_model=cm,
                        tokenized_prompts=prompts)
    vit_amd.apply_dora_to_ViT(m, n_vision_layers=2, n_transformer_layers=1, r=r)
    vit_amd.switch_dora_layers(m, freeze_all=True, dora_state=True)
    sd = m.state_dict()
    d = CR.init_dora(p, cfg, r=r, seed=0)
    for k in list(d):
        if not k.endswith(".scaling"):  # the oracle's parameters with the product's own A / B draw
            d[k] = sd[k].detach().clone().float()
    g = torch.Generator().manual_seed(17)
    x = torch.randn(MB, 3, 136, 136, generator=g)
    y = torch.randn(MB, T, generator=g) * 0.5 + 1.0
    ref_loss, ref_pred, ref_grads = CR.train_step(p, d, {}, x, prompts, y, cfg, lr=3e-4, pos_embedding=True)

    m = m.cuda()
    xg = x.cuda()
    ops.set_float32_attention_precision("high")
    cache = vit_amd.VisualPrefixCache.build(m, xg, batch_size=MB)
    assert cache.valid_for(m, xg)
    _high_long()
    assert not cache.valid_for(m, xg), "rows built with the long switch off would be read with it on"
    c0 = _counts()
    pred = m(xg)
    loss = vit_amd.mse_loss(pred, y.cuda())
    loss.backward()
    torch.cuda.synchronize()
    adv = _advance(c0)
    assert adv[0] > 0 and adv[0] == adv[1], f"the step's visual attention did not take the new kernels: {adv}"
    grads = {n: q.grad.detach().cpu() for n, q in m.named_parameters() if q.requires_grad}
    assert len(grads) == 9 and sorted(grads) == sorted(ref_grads)
    print("FIG pred rel", _rel(pred, ref_pred), "loss", float(loss.detach()), ref_loss)
    assert _rel(pred, ref_pred) < 1e-3
    assert abs(float(loss.detach()) - ref_loss) <= 1e-3 * abs(ref_loss)
    for k, rg in ref_grads.items():
        print("FIG", k, _rel(grads[k], rg))
        assert _rel(grads[k], rg) < 1e-3, (k, _rel(grads[k], rg))
