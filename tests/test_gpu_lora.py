"""GPU: the LoRA adapter (csrc/lora.hip, vit_amd/lora.py) -- the weight kernels against float64 and the reference
fixture, LoRALayer.forward, and the CLIP-HBA path (merged weight, full-size step, prefix cache, sweep files).

Bounds.  With u = 2^-23 (twice the f32 unit roundoff) an f32 dot product of length m, summed in any order, is
within m * u / 2 * sum|a||b| of the exact one; the tests allow twice that plus two more roundings (the scaling
and the final add): ``|W - W64| <= (r + 2) u (|W0| + s |B| @ |A|)``, ``|dB - dB64| <= (n + 2) u s |gW| @ |A|^T``,
``|dA - dA64| <= (n + 2) u s |B|^T @ |gW|``.  Against the reference fixture: W to 1e-5 and gradients to 1e-4 of
the tensor's scale (``_close`` of tests/test_gpu_kernels.py, the DoRA test's bounds).
"""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import clip_ref as CR

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -23
CFG = CR.CLIP_TINY
SHAPES = [(1, 1), (63, 3), (64, 8), (65, 1), (96, 4), (200, 33), (768, 32), (1024, 32), (1024, 64)]


@pytest.fixture(scope="module")
def fx(golden_dir):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.load(os.path.join(golden_dir, "lora_golden.pt"), weights_only=True)


@pytest.fixture(scope="module")
def gold(golden_dir):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.load(os.path.join(golden_dir, "clip_golden.pt"), weights_only=True)


def _close(got, ref, rel, what=""):
    got = got.detach().float().cpu()
    ref = ref.detach().float().cpu()
    scale = ref.abs().max().item() + 1e-12
    err = (got - ref).abs().max().item()
    print(f"{what}: max err {err:.3e}, scale {scale:.3e}")
    assert err <= rel * scale, f"{what}: max err {err:.3e} > {rel:.1e} * scale {scale:.3e}"


def _within(got, ref64, bound64, what):
    err = (got.detach().cpu().double() - ref64).abs()
    worst = float((err / bound64.clamp_min(1e-300)).max())
    print(f"{what}: max |err| {float(err.max()):.3e}, worst err / bound {worst:.3f}")
    assert bool((err <= bound64).all()), f"{what}: err / bound up to {worst:.3f}"


def _inputs(n, r):
    g = torch.Generator().manual_seed(1000 * n + r)
    W0 = torch.randn(n, n, generator=g) * 0.05
    A = torch.randn(r, n, generator=g) * 0.3
    Bm = torch.randn(n, r, generator=g) * 0.3
    gW = torch.randn(n, n, generator=g)
    return W0, A, Bm, gW, 16 / r


def _run(W0, A, Bm, gW, s, w0_grad=False):
    import vit_amd
    W0 = W0.to(DEV).requires_grad_(w0_grad)
    A = A.to(DEV).requires_grad_(True)
    Bm = Bm.to(DEV).requires_grad_(True)
    W = vit_amd.lora_weight(W0, A, Bm, s)
    W.backward(gW.to(DEV))
    return W.detach(), A.grad, Bm.grad, W0.grad


@pytest.mark.parametrize("n, r", SHAPES)
def test_lora_weight_against_float64(n, r):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    W0, A, Bm, gW, s = _inputs(n, r)
    W, dA, dB, _ = _run(W0, A, Bm, gW, s)
    assert tuple(W.shape) == (n, n) and tuple(dA.shape) == (r, n) and tuple(dB.shape) == (n, r)
    W0d, Ad, Bd, gd = W0.double(), A.double(), Bm.double(), gW.double()
    _within(W, W0d + s * (Bd @ Ad), (r + 2) * U * (W0d.abs() + s * (Bd.abs() @ Ad.abs())), f"W n={n} r={r}")
    _within(dB, s * (gd @ Ad.T), (n + 2) * U * s * (gd.abs() @ Ad.abs().T), f"dB n={n} r={r}")
    _within(dA, s * (Bd.T @ gd), (n + 2) * U * s * (Bd.abs().T @ gd.abs()), f"dA n={n} r={r}")


@pytest.mark.parametrize("key", ["64x64r8", "96x96r4"])
def test_lora_weight_matches_reference_fixture(fx, key):
    rec = fx[key]
    W, dA, dB, _ = _run(rec["W0"], rec["A"], rec["B"], rec["gW"], rec["scaling"])
    _close(W, rec["W"], 1e-5, "lora W")
    _close(dA, rec["dA"], 1e-4, "dA")
    _close(dB, rec["dB"], 1e-4, "dB")


@pytest.mark.parametrize("key", ["1024x1024r32", "768x768r32"])
def test_lora_layer_matches_reference_summaries(fx, key):
    """Full-size layers: inputs regenerated from the recorded seed (the module's RNG order is the
    reference's), the reference's W and gradients compared through their recorded summaries."""
    import vit_amd
    rec = fx[key]
    torch.manual_seed(rec["seed"])
    base = nn.Linear(rec["n"], rec["n"])
    layer = vit_amd.LoRALayer(base, r=rec["r"], lora_alpha=16, lora_dropout=0.1)
    gW = torch.randn(rec["n"], rec["n"])
    assert abs(layer.lora_A.double().sum().item() - rec["A_sum"]) < 1e-9 * max(1.0, abs(rec["A_sum"]))
    assert abs(layer.lora_B.double().sum().item() - rec["B_sum"]) < 1e-9 * max(1.0, abs(rec["B_sum"]))
    assert layer.scaling == rec["scaling"]
    layer = layer.to(DEV)
    W = layer.weight
    assert abs(W.double().sum().item() - rec["W_sum"]) < 1e-4 * abs(rec["W_abs"])
    assert abs(W.double().abs().sum().item() - rec["W_abs"]) < 1e-5 * abs(rec["W_abs"])
    _close(W[0, :64], rec["W_row0"], 1e-5, "row0")
    W.backward(gW.to(DEV))
    dA, dB = layer.lora_A.grad, layer.lora_B.grad
    assert abs(dA.norm().item() - rec["dA_norm"]) <= 1e-4 * rec["dA_norm"]
    assert abs(dB.norm().item() - rec["dB_norm"]) <= 1e-4 * rec["dB_norm"]
    _close(dA[0, :64], rec["dA_slice"], 1e-4, "dA slice")
    _close(dB[0, :rec["r"]], rec["dB_slice"], 1e-4, "dB slice")
    assert layer.original_layer.weight.grad is not None  # a fresh nn.Linear's weight asks for its gradient
    assert layer.bias is layer.original_layer.bias


def test_rejected_arguments():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import vit_amd
    from vit_amd import _lib as L
    n = 8
    W0 = torch.zeros(n, n, device=DEV)
    for r in (0, 65):
        with pytest.raises(ValueError):
            vit_amd.lora_weight(W0, torch.zeros(r, n, device=DEV), torch.zeros(n, r, device=DEV), 2.0)
    with pytest.raises(ValueError):
        vit_amd.lora_weight(torch.zeros(8, 6, device=DEV), torch.zeros(2, 8, device=DEV),
                            torch.zeros(6, 2, device=DEV), 2.0)
    lib = L.lib()
    invalid = 1  # hipErrorInvalidValue
    buf = torch.zeros(65 * n + n * n, device=DEV)
    ws = torch.zeros(4096, device=DEV)
    p, st = buf.data_ptr(), L.stream_ptr(W0.device)
    for nn_, r in ((n, 0), (n, 65), (0, 4), (-3, 4)):
        assert lib.vit_lora_weight_fwd(nn_, r, p, p, p, 2.0, W0.data_ptr(), st) == invalid
        assert lib.vit_lora_weight_bwd(nn_, r, p, p, p, 2.0, p, p, ws.data_ptr(), st) == invalid
        assert lib.vit_lora_weight_bwd_ws_floats(nn_, r) == 0
    assert lib.vit_lora_weight_bwd_ws_floats(1024, 32) == 2 * 16 * 32 * 1024
    assert lib.vit_lora_weight_bwd_ws_floats(65, 3) == 2 * 2 * 3 * 65
    torch.cuda.synchronize()
    assert float(W0.abs().sum()) == 0.0  # nothing was launched


def test_backward_is_deterministic():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    W0, A, Bm, gW, s = _inputs(1024, 32)
    _, dA1, dB1, _ = _run(W0, A, Bm, gW, s)
    _, dA2, dB2, _ = _run(W0, A, Bm, gW, s)
    assert torch.equal(dA1, dA2) and torch.equal(dB1, dB2)


def test_capture_and_replay_give_the_eager_bits():
    """No allocation, no synchronisation: both entry points record into a graph, and its replay writes the
    bits of the eager calls."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vit_amd import _lib as L
    n, r = 200, 33
    W0, A, Bm, gW, s = (t.to(DEV) if torch.is_tensor(t) else t for t in _inputs(n, r))
    W, dA, dB = torch.empty(n, n, device=DEV), torch.empty(r, n, device=DEV), torch.empty(n, r, device=DEV)
    ws = torch.empty(L.lib().vit_lora_weight_bwd_ws_floats(n, r), device=DEV)
    p = L.ptr

    def both():
        st = L.stream_ptr(W0.device)
        L.call("vit_lora_weight_fwd", n, r, p(W0), p(A), p(Bm), s, p(W), st)
        L.call("vit_lora_weight_bwd", n, r, p(A), p(Bm), p(gW), s, p(dA), p(dB), p(ws), st)

    both()
    torch.cuda.synchronize()
    eager = [t.clone() for t in (W, dA, dB)]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        both()
    for t in (W, dA, dB):
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(eager, (W, dA, dB)))


@pytest.mark.parametrize("n, r", [(96, 4), (65, 3)])
def test_views_give_the_contiguous_bits(n, r):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import vit_amd
    W0, A, Bm, gW, s = _inputs(n, r)
    W, dA, dB, _ = _run(W0, A, Bm, gW, s)
    W0v = W0.t().contiguous().to(DEV).t()                 # a transposed view
    big = torch.zeros(n, n + 5, device=DEV)
    big[:, 3:3 + n] = gW.to(DEV)
    gWv = big[:, 3:3 + n]                                 # a column slice of a wider tensor
    assert not W0v.is_contiguous() and not gWv.is_contiguous()
    flat = torch.zeros(r * n + 1, device=DEV)
    flat[1:] = A.flatten().to(DEV)
    Av = flat[1:].view(r, n).requires_grad_(True)         # contiguous but 4 bytes off 16-byte alignment
    Bv = Bm.to(DEV).requires_grad_(True)
    Wv = vit_amd.lora_weight(W0v, Av, Bv, s)
    Wv.backward(gWv)
    assert torch.equal(Wv.detach(), W) and torch.equal(Av.grad, dA) and torch.equal(Bv.grad, dB)


def test_base_weight_gradient_only_when_asked():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    W0, A, Bm, gW, s = _inputs(96, 4)
    _, _, _, g0 = _run(W0, A, Bm, gW, s, w0_grad=True)
    assert g0 is not None and torch.equal(g0.cpu(), gW)
    _, _, _, g0 = _run(W0, A, Bm, gW, s, w0_grad=False)
    assert g0 is None


# ---------------------------------------------------------------------------- LoRALayer.forward, 96 -> 80

class _Mask(nn.Module):
    """Stands where ``lora_dropout`` stands and multiplies by a recorded dropout multiplier."""

    def __init__(self, mask):
        super().__init__()
        self.mask = mask

    def forward(self, x):
        return x * self.mask


def _fixture_layer(f):
    import vit_amd
    base = nn.Linear(96, 80)
    layer = vit_amd.LoRALayer(base, r=8, lora_alpha=16, lora_dropout=0.1)
    with torch.no_grad():
        base.weight.copy_(f["W0"])
        base.bias.copy_(f["bias"])
        layer.lora_A.copy_(f["A"])
        layer.lora_B.copy_(f["B"])
    return layer.to(DEV)


@pytest.mark.parametrize("mode", ["eval", "train"])
def test_lora_forward_matches_reference_fixture(fx, mode):
    f = fx["forward"]
    layer = _fixture_layer(f)
    layer.train(mode == "train")
    if mode == "train":
        layer.lora_dropout = _Mask(f["train"]["mask"].to(DEV))
    x = f["x"].clone().to(DEV).requires_grad_(True)
    y = layer(x)
    assert tuple(y.shape) == (6, 80)
    y.backward(f["gy"].to(DEV))
    want = f[mode]
    _close(y, want["y"], 1e-5, f"{mode} y")
    _close(x.grad, want["dx"], 1e-4, f"{mode} dx")
    _close(layer.lora_A.grad, want["dA"], 1e-4, f"{mode} dA")
    _close(layer.lora_B.grad, want["dB"], 1e-4, f"{mode} dB")
    # .weight is not the weight forward applies (and does not exist for 96 -> 80)
    with pytest.raises(ValueError):
        layer.weight


def test_lora_forward_draws_torchs_own_mask(fx):
    f = fx["forward"]
    layer = _fixture_layer(f).train()
    x = torch.randn(5, 3, 96, generator=torch.Generator().manual_seed(3)).to(DEV)
    torch.cuda.manual_seed(17)
    y = layer(x)
    torch.cuda.manual_seed(17)
    xd = layer.lora_dropout(x)
    assert (xd == 0).any() and not torch.equal(xd, x)
    with torch.no_grad():
        y2 = (torch.nn.functional.linear(x, layer.original_layer.weight, layer.original_layer.bias)
              + (xd @ layer.lora_B @ layer.lora_A) * layer.scaling)
    assert tuple(y.shape) == (5, 3, 80)
    _close(y, y2, 1e-5, "train-mode forward against its restatement")


# ---------------------------------------------------------------------------- the CLIP-HBA path

def _tiny_clip(gold, dtype=torch.float32):
    from vit_amd import clip
    cm = clip.CLIP(embed_dim=CFG.embed_dim, image_resolution=CFG.image_resolution, vision_layers=CFG.vision_layers,
                   vision_width=CFG.vision_width, vision_patch_size=CFG.vision_patch,
                   context_length=CFG.context_length, vocab_size=CFG.vocab_size, transformer_width=CFG.text_width,
                   transformer_heads=CFG.text_heads, transformer_layers=CFG.text_layers, compute_dtype=dtype)
    cm.load_state_dict(CR.init_params(CFG, seed=gold["seed"]), strict=True)
    return cm


def _tiny_hba(gold, seed=31, lora=True):
    import vit_amd
    m = vit_amd.CLIPHBA([f"c{i}" for i in range(gold["T"])], "ViT-L/14", pos_embedding=True,
                        clip_model=_tiny_clip(gold), tokenized_prompts=gold["prompts"])
    if lora:
        torch.manual_seed(seed)
        vit_amd.apply_lora_to_ViT(m, n_vision_layers=2, n_transformer_layers=1, r=8, lora_dropout=0.1)
        vit_amd.unfreeze_lora_layers(m, freeze_all=True)
    return m


def _lora_modules(m):
    import vit_amd
    return tuple(n for n, mod in m.named_modules() if isinstance(mod, vit_amd.LoRALayer))


def _step(m, target, x=None, prefix=None):
    import vit_amd
    m.train()
    for p in m.parameters():
        p.grad = None
    pred = m(x) if prefix is None else m(visual_prefix=prefix)
    vit_amd.MSELoss()(pred, target).backward()
    return pred.detach(), {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}


def test_clip_path_trains_the_merged_weight(gold):
    ml = _tiny_hba(gold).cuda()
    names = _lora_modules(ml)
    assert len(names) == 3
    mm = _tiny_hba(gold, lora=False).cuda()
    for p in mm.parameters():
        p.requires_grad = False
    mods_l, mods_m = dict(ml.named_modules()), dict(mm.named_modules())
    for n in names:
        with torch.no_grad():
            mods_m[n].weight.copy_(mods_l[n].weight)
            assert torch.equal(mods_m[n].bias, mods_l[n].bias)
        mods_m[n].weight.requires_grad = True
    x, target = gold["image"].cuda(), gold["target"].cuda()
    pred_l, grads_l = _step(ml, target, x)
    pred_m, grads_m = _step(mm, target, x)
    assert torch.equal(pred_l, pred_m)
    assert sorted(grads_l) == sorted(f"{n}.{k}" for n in names for k in ("lora_A", "lora_B"))
    assert sorted(grads_m) == sorted(f"{n}.weight" for n in names)
    for n in names:
        lay = mods_l[n]
        s = lay.scaling
        G = grads_m[f"{n}.weight"].cpu().double()
        Ad, Bd = lay.lora_A.detach().cpu().double(), lay.lora_B.detach().cpu().double()
        k = G.shape[0]
        assert float(G.abs().max()) > 0
        _within(grads_l[f"{n}.lora_A"], s * (Bd.T @ G), (k + 2) * U * s * (Bd.abs().T @ G.abs()), f"{n} dA")
        _within(grads_l[f"{n}.lora_B"], s * (G @ Ad.T), (k + 2) * U * s * (G.abs() @ Ad.abs().T), f"{n} dB")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_clip_l14_lora_step(dtype):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import vit_amd
    m = vit_amd.CLIPHBA(["x%d" % i for i in range(66)], "ViT-L/14", pos_embedding=True, compute_dtype=dtype)
    vit_amd.apply_lora_to_ViT(m, n_vision_layers=2, n_transformer_layers=1, r=32)
    vit_amd.unfreeze_lora_layers(m, freeze_all=True)
    m = m.cuda()
    assert vit_amd.count_trainable_parameters(m) == 180224
    opt = vit_amd.FusedAdamW(m.parameters(), lr=3e-4)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(4, 3, 224, 224, generator=g).cuda()
    y = torch.randn(4, 66, generator=g).cuda()
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    opt.zero_grad()
    pred = m(x)
    loss = vit_amd.mse_loss(pred, y)
    loss.backward()
    assert tuple(pred.shape) == (4, 66) and torch.isfinite(pred).all() and torch.isfinite(loss)
    with_grad = sorted(n for n, p in m.named_parameters() if p.grad is not None)
    want = sorted(f"{n}.{k}" for n in _lora_modules(m) for k in ("lora_A", "lora_B"))
    assert len(want) == 6 and with_grad == want
    for n, p in m.named_parameters():
        if p.grad is not None:
            assert torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0, n
    opt.step()
    torch.cuda.synchronize()
    changed = sorted(n for n, p in m.named_parameters() if not torch.equal(p.detach(), before[n]))
    assert changed == want
    assert all(torch.isfinite(p).all() for p in m.parameters() if p.requires_grad)


def test_prefix_cache_is_exact_with_lora(gold, tmp_path):
    from vit_amd import sweep as S
    from vit_amd.prefix_cache import VisualPrefixCache
    m = _tiny_hba(gold).cuda()
    x, target = gold["image"].cuda(), gold["target"].cuda()
    B = x.shape[0]
    pred, grads = _step(m, target, x)
    cache = VisualPrefixCache.build(m, x, batch_size=B)
    assert cache.first == 1
    pred_c, grads_c = _step(m, target, prefix=cache.take(torch.arange(B)))
    assert torch.equal(pred, pred_c)
    assert sorted(grads) == sorted(grads_c) and len(grads) == 6
    for n in grads:
        assert torch.equal(grads[n], grads_c[n]), n
    # resuming LoRA parameters touches no frozen tensor: the cache stays valid
    names = _lora_modules(m)
    S.save_dora_parameters(m, str(tmp_path / "p"), 0, modules=names)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if p.requires_grad:
                p.mul_(0.5)
    sd = S.load_dora_parameters(m, str(tmp_path / "p"), 1)
    assert sorted(sd) == sorted(f"{n}.{k}" for n in names for k in ("lora_A", "lora_B"))
    for k, v in sd.items():
        assert torch.equal(m.state_dict()[k].cpu(), v)
    assert cache.valid_for(m, x)
    pred_r, _ = _step(m, target, prefix=cache.take(torch.arange(B)))
    assert torch.equal(pred_r, pred)


@pytest.mark.parametrize("cached", [False, True], ids=["uncached", "cache_visual_prefix"])
def test_sweep_condition_on_lora_model(gold, tmp_path, cached):
    """Two baseline epochs on the CLIP_TINY LoRA model, then a perturbed condition resumed from the baseline's
    epoch-1 files: the parameter files carry the LoRA keys under the DoRA file names, and the resumed run
    starts from them."""
    import vit_amd
    from vit_amd import sweep as S
    g = torch.Generator().manual_seed(5)
    T, R = gold["T"], CFG.image_resolution
    mk = lambda n: (torch.randn(n, 3, R, R, generator=g).cuda(), (torch.randn(n, T, generator=g) * 0.5 + 2.0).cuda())
    a = np.random.default_rng(5).random((6, 6))
    ref = (a + a.T) / 2
    np.fill_diagonal(ref, 0)
    data = dict(train=mk(11), test=mk(5), inference=torch.randn(6, 3, R, R, generator=g).cuda(), reference_rdm=ref)
    seeds = iter(range(100, 200))

    def make():
        m = _tiny_hba(gold, seed=next(seeds)).cuda()
        return m, vit_amd.FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=1e-3)

    m, opt = make()
    names = _lora_modules(m)
    keys = sorted(f"{n}.{k}" for n in names for k in ("lora_A", "lora_B"))
    init = {k: m.state_dict()[k].cpu().clone() for k in keys}
    base = tmp_path / "base"
    rows = S.train_condition(m, opt, vit_amd.mse_loss, data, epochs=2, training_run=1, perturb_length=0,
                             perturb_type=None, batch_size=4, training_res_path=str(tmp_path / "b.csv"),
                             dora_parameters_path=str(base / "dora"), random_state_path=str(base / "rs"),
                             dataloader_generator=torch.Generator().manual_seed(0), modules=names,
                             cache_visual_prefix=cached)
    assert len(rows) == 2 and all(np.isfinite(r[1]) and np.isfinite(r[2]) for r in rows)
    sd1 = torch.load(str(base / "dora" / "epoch1_dora_params.pth"), weights_only=True)
    sd2 = torch.load(str(base / "dora" / "epoch2_dora_params.pth"), weights_only=True)
    assert sorted(sd1) == keys and sorted(sd2) == keys
    assert all(not torch.equal(sd1[k], init[k]) and not torch.equal(sd2[k], sd1[k]) for k in keys)  # it trained
    # a differently seeded fresh model takes the file's values
    m2, _ = make()
    assert not torch.equal(m2.state_dict()[keys[0]].cpu(), sd1[keys[0]])
    S.load_dora_parameters(m2, str(base / "dora"), 1)
    assert all(torch.equal(m2.state_dict()[k].cpu(), sd1[k]) for k in keys)
    done = S.run_sweep(make, vit_amd.mse_loss, data, [(2, 1)], perturb_type="label_shuffle",
                       out_dir=str(tmp_path / "sw"), baseline_dora_path=str(base / "dora"),
                       baseline_random_state_path=str(base / "rs"), epochs=2, batch_size=4, modules=names,
                       cache_visual_prefix=cached)
    assert done[0][0] == (2, 1) and done[0][2] == "baseline"
    with open(done[0][1]) as fh:
        out = fh.read().splitlines()
    assert out[0].split(",") == S.CSV_HEADERS and len(out) == 2
    assert out[1].split(",")[0] == "2" and out[1].split(",")[6] == "True"
    sw = torch.load(os.path.join(S.condition_dir(str(tmp_path / "sw"), "label_shuffle", 2, 1), "dora_params_2",
                                 "epoch2_dora_params.pth"), weights_only=True)
    assert sorted(sw) == keys
    # one epoch of lr 1e-3 AdamW from the baseline's epoch-1 values: every element moved by about one step of
    # at most lr, far less than the distance between two seeds' initial draws
    for k in keys:
        assert float((sw[k] - sd1[k]).abs().max()) <= 3 * 3 * 1e-3 + 1e-6, k
