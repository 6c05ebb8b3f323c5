"""GPU: the class-token tail (the last block under ``forward()`` computed for the class rows alone) against
the dense block and the fp64 oracle.

Contract: logits bit for bit the dense path's.  Gradients: where the tail's row-padded backward lines up with
the dense launches (at least 64 tokens, the weight gradients' M % 32 == 0 rule met and split-K slab boundaries
on image boundaries -- the benchmark's shape) every gradient is bit for bit the dense block's; elsewhere the
same terms may be summed in another order, and every parameter gradient's error against the fp64 oracle is at
most 2x the dense path's error on the same inputs plus a floor of two f32 ulps of the gradient's scale (2^-22
relative: a parameter whose dense error happens to be ~0 may still move by a rounding).
Errors are max |got - ref| / max |ref| per parameter."""
from collections import OrderedDict

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import vit_ref as R  # noqa: E402

DEV = "cuda"
FLOOR = 2.0 ** -22

# depth 2, D = 128, 2 heads: N = 17 (img 64 / patch 16) and N = 197 (img 224 / patch 16); B = 3
CFGS = {
    17: R.ViTConfig(img_size=64, patch_size=16, embed_dim=128, depth=2, num_heads=2, num_classes=10),
    197: R.ViTConfig(img_size=224, patch_size=16, embed_dim=128, depth=2, num_heads=2, num_classes=10),
}
B = 3
_REF = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _case(n):
    """Parameters, inputs and the fp64 oracle's logits / gradients for the N = n model (computed once)."""
    if n not in _REF:
        cfg = CFGS[n]
        p = R.init_params(cfg, seed=31 + n, random_affine=True)
        g = torch.Generator().manual_seed(32 + n)
        x = torch.randn(B, cfg.in_chans, cfg.img_size, cfg.img_size, generator=g)
        y = torch.randint(0, cfg.num_classes, (B,), generator=g)
        leaf = OrderedDict((k, v.double().requires_grad_(True)) for k, v in p.items())
        logits = R.forward(leaf, x.double(), cfg)
        R.cross_entropy(logits, y).backward()
        _REF[n] = (cfg, p, x, y, logits.detach(), OrderedDict((k, v.grad.detach()) for k, v in leaf.items()))
    return _REF[n]


def _model(cfg, params, dtype):
    import vit_amd
    m = vit_amd.VisionTransformer(img_size=cfg.img_size, patch_size=cfg.patch_size, in_chans=cfg.in_chans,
                                  num_classes=cfg.num_classes, embed_dim=cfg.embed_dim, depth=cfg.depth,
                                  num_heads=cfg.num_heads, mlp_ratio=cfg.mlp_ratio, eps=cfg.eps,
                                  compute_dtype=dtype)
    m.load_state_dict(params)
    return m.to(DEV)


def _run(n, dtype, tail, flat=False):
    """logits and gradients of one forward + backward with the tail on / off."""
    import vit_amd
    cfg, p, x, y = _case(n)[:4]
    prev = vit_amd.set_cls_tail(tail)
    try:
        m = _model(cfg, p, dtype)
        if flat:  # the bench configuration: flat gradient buffer, side stream joined at the backward's end
            m.use_flat_grads(True)
            m.set_deferred_grad_join(True)
        logits = m(x.to(DEV))
        vit_amd.cross_entropy(logits, y.to(DEV)).backward()
        torch.cuda.synchronize()
        grads = OrderedDict((k, q.grad.detach().double().cpu()) for k, q in m.named_parameters())
    finally:
        vit_amd.set_cls_tail(prev)
    return logits.detach().cpu(), grads


def _err(got, ref):
    return (got - ref).abs().max().item() / (ref.abs().max().item() + 1e-300)


def _check(n, dtype, flat=False):
    ref = _case(n)[5]
    l_off, g_off = _run(n, dtype, False, flat)
    l_on, g_on = _run(n, dtype, True, flat)
    assert torch.equal(l_on, l_off)
    bad = []
    for k in ref:
        e_off, e_on = _err(g_off[k], ref[k]), _err(g_on[k], ref[k])
        print(f"N={n} {dtype} {k}: dense {e_off:.3e} tail {e_on:.3e}")
        if not e_on <= 2.0 * e_off + FLOOR:
            bad.append((k, e_off, e_on))
    assert not bad, bad


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("n", [17, 197])
def test_tail_matches_dense_and_oracle(n, dtype):
    _check(n, dtype)


@pytest.mark.parametrize("join", ["block", "end"])
def test_tail_under_both_join_modes(join, monkeypatch):
    from vit_amd import model
    monkeypatch.setattr(model, "_FWD_JOIN", [join])
    monkeypatch.setattr(model, "_BWD_JOIN", [join])
    _check(17, torch.bfloat16, flat=True)
    _check(197, torch.bfloat16, flat=True)


def test_head_receives_the_compact_block_output():
    """With the switch on, forward() hands the head a [B, 1, D] block output; forward_features() never does."""
    import vit_amd
    from vit_amd import model
    cfg, p, x = _case(17)[:3]
    m = _model(cfg, p, torch.bfloat16)
    seen = []
    orig = model._HeadFn.forward

    def spy(ctx, xx, *a):
        seen.append(tuple(xx.shape))
        return orig(ctx, xx, *a)

    prev = vit_amd.set_cls_tail(True)
    try:
        model._HeadFn.forward = staticmethod(spy)
        m(x.to(DEV))
        vit_amd.set_cls_tail(False)
        m(x.to(DEV))
    finally:
        model._HeadFn.forward = staticmethod(orig)
        vit_amd.set_cls_tail(prev)
    assert seen == [(B, 1, cfg.embed_dim), (B, 17, cfg.embed_dim)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_forward_features_unchanged_by_the_switch(dtype):
    import vit_amd
    from vit_amd import model
    cfg, p, x = _case(17)[:3]
    m = _model(cfg, p, dtype)
    out = []
    prev = model.cls_tail_enabled()
    try:
        for on in (True, False):
            vit_amd.set_cls_tail(on)
            with torch.no_grad():
                out.append(m.forward_features(x.to(DEV)).cpu())
            out.append(m.forward_features(x.to(DEV)).detach().cpu())
    finally:
        vit_amd.set_cls_tail(prev)
    assert out[0].shape == (B, 17, cfg.embed_dim)
    for o in out[1:]:
        assert torch.equal(o, out[0])


@pytest.mark.parametrize("D", [128, 768])
def test_layer_norm_bwd_compact_residual_is_the_dense_form(D):
    """vit_layer_norm_bwd_cls at rows = 3 * 17: bitwise the dense kernel over a residual gradient that is zero
    outside every 17th row (the same adds), in dx, its bf16 copy and the three column sums."""
    from vit_amd import ops
    Bn, N = 3, 17
    rows = Bn * N
    g = torch.Generator().manual_seed(5 + D)
    x = torch.randn(rows, D, generator=g).to(DEV)
    dy = torch.randn(rows, D, generator=g).to(DEV).to(torch.bfloat16)
    w = torch.randn(D, generator=g).to(DEV)
    mean = x.mean(1).contiguous()
    rstd = (x.var(1, unbiased=False) + 1e-6).rsqrt().contiguous()
    cres = torch.randn(Bn, D, generator=g).to(DEV)
    dense = torch.zeros(rows, D, device=DEV)
    dense[::N] = cres
    res = []
    for kw in (dict(dres=dense, ldres=D), dict(dres=cres, ldres=D, res_every=N)):
        dx = torch.empty(rows, D, device=DEV)
        dxc = torch.empty(rows, D, dtype=torch.bfloat16, device=DEV)
        dg, db, ds = (torch.empty(D, device=DEV) for _ in range(3))
        ops.layer_norm_bwd(x, D, dy, w, mean, rstd, dx, D, rows, dx_copy=dxc, ld_copy=D, dgamma=dg, dbeta=db, dsum=ds,
                           **kw)
        torch.cuda.synchronize()
        res.append((dx, dxc, dg, db, ds))
    for a, b in zip(*res):
        assert torch.equal(a.view(torch.int32 if a.dtype == torch.float32 else torch.int16),
                           b.view(torch.int32 if b.dtype == torch.float32 else torch.int16))


def test_tail_gradients_are_bitwise_the_dense_block_where_slabs_align(monkeypatch):
    """128 images of 197 tokens with the weight gradients split in two: each split-K slab holds 64 images in
    the dense block (12 608 rows) and in the tail's padded layout (4 096 rows), every 64-row column-sum
    group, LayerNorm partial block and 32-row k-tile at most one class row -- the same terms in the same
    order, so every gradient keeps its bits (as at the benchmark's 256 x 197)."""
    import vit_amd
    from vit_amd import ops
    monkeypatch.setattr(ops, "_WGRAD_WGS", [6])  # fc2 + fc1: 4 tiles, proj + qkv: 3 tiles -> split 2 for both pairs
    cfg = CFGS[197]
    Bn = 128
    assert ops.pair_split(Bn * 197, 128, 512, 512, 128) == 2 and ops.pair_split(Bn * 197, 128, 128, 384, 128) == 2
    p = _case(197)[1]
    g = torch.Generator(device=DEV).manual_seed(9)
    x = torch.randn(Bn, 3, cfg.img_size, cfg.img_size, generator=g, device=DEV)
    y = torch.randint(0, cfg.num_classes, (Bn,), generator=g, device=DEV)
    res = []
    prev = vit_amd.set_cls_tail(False)
    try:
        for on in (False, True):
            vit_amd.set_cls_tail(on)
            m = _model(cfg, p, torch.bfloat16)
            logits = m(x)
            vit_amd.cross_entropy(logits, y).backward()
            torch.cuda.synchronize()
            res.append((logits.detach(), {k: q.grad.detach() for k, q in m.named_parameters()}))
    finally:
        vit_amd.set_cls_tail(prev)
    assert torch.equal(res[0][0], res[1][0])
    assert [k for k in res[0][1] if not torch.equal(res[0][1][k], res[1][1][k])] == []


# (B, H, N): one tile, a ragged second tile, the ViT-B/16 token count (odd tile count), and two counts past
# the resident kernels' 288 tokens (the fallback route: the full streamed kernels)
ATTN_CASES = [(2, 2, 16), (3, 2, 17), (2, 3, 197), (1, 2, 257), (1, 1, 577)]
_ATTN = {}


def _attn_case(shape, dtype):
    """qkv (rounded to dtype), the class rows' dO, and in fp64: o and lse of query 0, and the dqkv / bias
    gradient of sum(o[:, 0] * dO)."""
    key = (shape, dtype)
    if key not in _ATTN:
        Bn, H, N = shape
        D = H * 64
        g = torch.Generator().manual_seed(7 + N)
        qkv = torch.randn(Bn * N, 3 * D, generator=g).to(dtype)
        do = torch.randn(Bn, D, generator=g).to(dtype)
        x = qkv.double().requires_grad_(True)
        q, k, v = x.reshape(Bn, N, 3, H, 64).permute(2, 0, 3, 1, 4)
        s = (q[:, :, :1] @ k.transpose(-2, -1)) * 64 ** -0.5
        o0 = (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(Bn, D)
        (o0 * do.double()).sum().backward()
        _ATTN[key] = (qkv, do, o0.detach(), torch.logsumexp(s.detach(), -1).reshape(Bn * H), x.grad.detach(),
                      x.grad.detach().sum(0))
    return _ATTN[key]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("shape", ATTN_CASES, ids=lambda s: "x".join(map(str, s)))
def test_query_limited_attention_forward(shape, dtype):
    """vit_sdpa_fwd_cls: query 0's o and lse against torch fp64 and bit for bit the full kernel's.  bf16 up to 288
    tokens takes query tile 0 of the resident kernel (rows 16.. get o = 0, lse = +inf); f32 and longer
    sequences the full kernels (every row equal).  Bounds from the formats: o passes three bf16 roundings (P,
    the MFMA's bf16 operands are exact, the stored value), each half an ulp = 2^-9 relative, so 2^-7 of its
    scale (f32: 1e-5 of scale, the existing f32 attention tests' bound); lse is f32 arithmetic on exact
    inputs, 1e-4 absolute at |lse| < 10."""
    from vit_amd import _lib, ops
    Bn, H, N = shape
    D = H * 64
    qkv, _, o_ref, lse_ref = _attn_case(shape, dtype)[:4]
    qkv = qkv.to(DEV)
    o_full, lse_full = ops.sdpa_fwd(qkv, Bn, H, N)
    _lib.lib().vit_sdpa_cls_count(1)
    o, lse = ops.sdpa_fwd_cls(qkv, Bn, H, N)
    torch.cuda.synchronize()
    limited = _lib.lib().vit_sdpa_cls_count(1) == 1
    assert limited == (dtype == torch.bfloat16 and N <= 288)
    o3, of3 = o.view(Bn, N, D), o_full.view(Bn, N, D)
    l3, lf3 = lse.view(Bn * H, N), lse_full.view(Bn * H, N)
    rows = min(16, N) if limited else N
    assert torch.equal(o3[:, :rows], of3[:, :rows]) and torch.equal(l3[:, :rows], lf3[:, :rows])
    if limited and N > 16:
        assert not o3[:, 16:].any() and bool((l3[:, 16:] == float("inf")).all())
    e_o = _err(o3[:, 0].double().cpu(), o_ref)
    e_l = (l3[:, 0].double().cpu() - lse_ref).abs().max().item()
    print(f"{shape} {dtype}: o {e_o:.3e} lse {e_l:.3e}")
    assert e_o <= (2.0 ** -7 if dtype == torch.bfloat16 else 1e-5)
    assert e_l <= 1e-4


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("shape", ATTN_CASES, ids=lambda s: "x".join(map(str, s)))
def test_attention_backward_after_the_query_limited_forward(shape, bias, dtype):
    """The tail's attention backward: the full kernel over a dO that is zero outside the class rows, fed the
    query-limited forward's o and lse (zeros and +inf in the rows it skipped).  Bit for bit the same call fed
    the full forward's o and lse (a skipped row has dO = 0: p * 0 and 0 * (0 - 0) either way), with and
    without the qkv-bias partials, and against torch fp64 within the bf16 / f32 attention tests' bounds (bf16:
    dq, dk, dv pass P, dS and the stored value through bf16, 3 * 2^-9 < 2^-6 of scale with the bf16 o in
    delta; f32: 1e-4 of scale)."""
    from vit_amd import ops
    Bn, H, N = shape
    D = H * 64
    qkv, do, _, _, ref, ref_b = _attn_case(shape, dtype)
    qkv = qkv.to(DEV)
    dense = torch.zeros(Bn * N, D, dtype=dtype, device=DEV)
    dense[::N] = do.to(DEV)
    out = []
    for fwd in (ops.sdpa_fwd, ops.sdpa_fwd_cls):
        o, lse = fwd(qkv, Bn, H, N)
        db = torch.empty(3 * D, device=DEV) if bias else None
        out.append((ops.sdpa_bwd(qkv, o, dense, lse, Bn, H, N, dbias=db), db))
    torch.cuda.synchronize()
    (full, db_full), (cls, db_cls) = out
    assert torch.equal(cls, full)
    assert not cls.isnan().any()
    tol = 2.0 ** -6 if dtype == torch.bfloat16 else 1e-4
    e = _err(cls.double().cpu(), ref)
    print(f"{shape} {dtype} dqkv: {e:.3e}")
    assert e <= tol
    if bias:
        assert torch.equal(db_cls, db_full)
        eb = _err(db_cls.double().cpu(), ref_b)
        print(f"{shape} {dtype} dbias: {eb:.3e}")
        assert eb <= tol
