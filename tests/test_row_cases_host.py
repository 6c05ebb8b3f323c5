"""CPU: oracle/row_cases.py -- the float64 references of the row kernels are the operations torch itself
computes, the same formulas in torch float32 stay inside every bound tests/test_gpu_row_kernels.py holds the
kernels to (so the bounds are reachable by plain f32 arithmetic before a GPU is involved), and the case lists
keep the shapes that reach each dispatch branch.

Worst torch-float32 figures against float64 on this file's cases (relative to the reference's largest
magnitude): LayerNorm y 2.5e-7 on ``base`` / ``tiny`` / ``const`` / ``outlier`` and 6.0e-6 on ``offset``, mean 1.0e-6, rstd
1.7e-7, dx 1.9e-7, dgamma 2.4e-7 (3.5e-6 on ``offset``); cross-entropy loss 1.4e-6 (the ``low`` row), lse 5e-8,
dlogits 2.4e-7 -- the 1e-5 bound has a margin of more than six on every kind it is used on unchanged."""
import torch
import torch.nn.functional as F

from oracle import row_cases as RC

BF = torch.bfloat16


def _ln_shapes():
    for D in RC.LN_FWD_VEC_D + RC.LN_FWD_SCALAR_D:
        for rows in RC.LN_FWD_ROWS:
            yield "base", rows, D
    for kind in RC.LN_KINDS:
        for D in RC.LN_KIND_D:
            yield kind, 5, D
    for D in RC.LN_BWD_PIPE_D + RC.LN_BWD_SCALAR_D:
        for rows in RC.LN_BWD_ROWS:
            yield "base", rows, D
    for D in RC.ADD_LN_D:
        for kind in RC.ADD_LN_KINDS:
            yield kind, 5, D


def test_ln_reference_is_torch_layer_norm():
    c = RC.ln_case("base", 37, 200)
    x = c.x.double().requires_grad_(True)
    w, b = c.w.double().requires_grad_(True), c.b.double().requires_grad_(True)
    y = F.layer_norm(x, (c.D,), w, b, c.eps)
    y.backward(c.dy.double())
    torch.testing.assert_close(c.ref["y"], y.detach(), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(c.ref["mean"], c.x.double().mean(1), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(c.ref["rstd"], (c.x.double().var(1, unbiased=False) + c.eps).rsqrt(), rtol=1e-12,
                               atol=1e-12)
    for name, t in (("dx", x), ("dgamma", w), ("dbeta", b)):
        torch.testing.assert_close(c.ref[name], t.grad, rtol=1e-10, atol=1e-12)
    # the written-out backward (what torch_f32 evaluates) is the autograd one
    dx, dg, db = RC.ln_bwd(c.x.double(), c.dy.double(), c.w.double(), c.ref["mean"], c.ref["rstd"])
    for name, t in (("dx", dx), ("dgamma", dg), ("dbeta", db)):
        torch.testing.assert_close(c.ref[name], t, rtol=1e-10, atol=1e-12)
    # rounded inputs: the reference is of what the kernel reads
    cb = RC.ln_case("offset", 5, 768, BF, BF)
    assert cb.x.dtype == BF and cb.dy.dtype == BF and cb.w.dtype == torch.float32
    torch.testing.assert_close(cb.ref["mean"], cb.x.double().mean(1), rtol=1e-12, atol=1e-12)


def test_ln_torch_f32_within_bounds():
    worst = {}
    for kind, rows, D in sorted(set(_ln_shapes())):
        for eps in RC.LN_EPS.get(kind, (1e-6,)):
            for xdt in (torch.float32, BF):
                c = RC.ln_case(kind, rows, D, xdt, xdt, eps)
                for name in ("y", "mean", "rstd", "dx", "dgamma", "dbeta", "dsum"):
                    e = RC.rel_max(c.torch_f32[name], c.ref[name])
                    worst[(kind, name)] = max(worst.get((kind, name), 0.0), e)
                    assert e <= c.bound(name), (kind, rows, D, eps, xdt, name, e, c.bound(name))
                    if kind not in RC.LN_HARD:
                        assert c.bound(name) == RC.F32
                    assert c.bound(name, RC.BF16_LN) >= RC.BF16_LN
    print({k: f"{v:.1e}" for k, v in sorted(worst.items())})


def test_add_ln_torch_f32_within_bounds():
    for D in RC.ADD_LN_D:
        for kind in ("base",) + RC.ADD_LN_KINDS:
            for rows in RC.ADD_LN_ROWS:
                for rdt in (BF, torch.float32):
                    c = RC.add_ln_case(kind, rows, D, rdt)
                    assert c.r.dtype == rdt and torch.equal(c.s, c.x + c.r.float())
                    torch.testing.assert_close(c.ref["y"], F.layer_norm(c.s.double(), (D,), c.w.double(), c.b.double(),
                                                                        c.eps), rtol=1e-12, atol=1e-12)
                    for name in ("y", "mean", "rstd"):
                        e = RC.rel_max(c.torch_f32[name], c.ref[name])
                        assert e <= c.bound(name), (kind, rows, D, rdt, name, e, c.bound(name))
                        assert kind in RC.LN_HARD or c.bound(name) == RC.F32


def test_ln_kinds_keep_their_claims():
    for D in RC.LN_KIND_D:
        x = {k: RC.ln_case(k, 5, D).x.double() for k in RC.LN_KINDS}
        assert (x["offset"].mean(1) - 100).abs().max() < 0.5 and (x["offset"].var(1) - 1).abs().max() < 0.5
        v = x["tiny"].var(1, unbiased=False)
        assert v.min() > 0.5e-6 and v.max() < 2e-6          # about eps = 1e-6, a tenth of eps = 1e-5
        assert (x["const"] == RC.CONST).all()
        assert ((x["outlier"] == 1e4).sum(1) == 1).all() and x["outlier"].abs().median() < 1
        c = RC.ln_case("const", 5, D)
        # exact in f32: the sum of D values of 3.25, in any order
        assert float(torch.tensor(RC.CONST * RC.LN_MAX_D, dtype=torch.float32)) == RC.CONST * RC.LN_MAX_D
        assert torch.equal(c.torch_f32["y"].float(), c.b.expand(5, D))
        assert torch.equal(c.ref["y"], c.b.double().expand(5, D))
        torch.testing.assert_close(c.ref["rstd"], torch.full((5,), c.eps ** -0.5, dtype=torch.float64))
        # a one-pass variance in f32 is wrong on ``offset`` by far more than the bound: the kind bites
        xf = RC.ln_case("offset", 5, D).x
        one_pass = ((xf * xf).mean(1) - xf.mean(1) ** 2 + 1e-6).rsqrt()
        co = RC.ln_case("offset", 5, D)
        assert RC.rel_max(one_pass, co.ref["rstd"]) > 10 * co.bound("rstd")
    t6, t5 = RC.ln_case("tiny", 5, 768, eps=1e-6), RC.ln_case("tiny", 5, 768, eps=1e-5)
    assert RC.rel_max(t5.ref["y"], t6.ref["y"]) > 0.3       # eps matters on this kind


def test_compact_and_spread_rows():
    dx = torch.arange(15.0)[:, None].expand(15, 2)
    assert RC.compact_rows(dx, 4)[:, 0].tolist() == [1, 2, 3, 4, 6, 7, 8, 9, 11, 12, 13, 14]
    assert RC.compact_rows(dx[:13], 4).shape[0] == 10
    c = torch.tensor([[1.0], [2.0], [3.0]])
    assert RC.spread_rows(c, 5, 13)[:, 0].tolist() == [1, 0, 0, 0, 0, 2, 0, 0, 0, 0, 3, 0, 0]


def test_ce_reference_is_torch_cross_entropy_and_f32_within_bounds():
    worst = {}
    for B, C in RC.CE_SHAPES:
        for kind in RC.CE_KINDS:
            c = RC.ce_case(kind, B, C)
            assert c.logits.dtype == torch.float32 and c.target.dtype == torch.int64
            assert c.target[-1] == C - 1 and (B == 1 or c.target[0] == 0)
            l = c.logits.double().requires_grad_(True)
            loss = F.cross_entropy(l, c.target)
            loss.backward()
            torch.testing.assert_close(c.ref["loss"], loss.detach().reshape(1), rtol=1e-12, atol=1e-12)
            torch.testing.assert_close(c.ref["lse"], torch.logsumexp(c.logits.double(), 1), rtol=1e-12, atol=1e-12)
            torch.testing.assert_close(c.ref["d"], l.grad, rtol=1e-10, atol=1e-14)
            for name in ("loss", "lse", "d"):
                e = RC.rel_max(c.torch_f32[name], c.ref[name])
                worst[(kind, name)] = max(worst.get((kind, name), 0.0), e)
                assert e <= c.bound(name), (kind, B, C, name, e, c.bound(name))
                assert kind in RC.CE_HARD or c.bound(name) == RC.F32
    print({k: f"{v:.1e}" for k, v in sorted(worst.items())})
    # the kinds: exp(x) without the max subtraction overflows f32 on ``wide`` and sinks into the denormals
    # (flushed to zero by a GPU's fast exp: log 0) on the ``low`` row
    s, lo, eq = RC.ce_case("spike", 5, 65), RC.ce_case("low", 5, 65), RC.ce_case("equal", 5, 65)
    assert s.logits[0].max() == 80 and (s.logits[0] < -75).sum() == 64
    assert (lo.logits[0] == -90).all() and lo.logits[0].exp().max() < torch.finfo(torch.float32).tiny
    wide = RC.ce_case("wide", 37, 1000).logits
    assert wide.max() > 89 and not torch.isfinite(wide.exp().sum(1).log()).all()
    assert (eq.logits[0] == eq.logits[0, 0]).all()
    torch.testing.assert_close(eq.ref["lse"][0], eq.logits[0, 0].double() + torch.tensor(65.0).double().log())


def test_sgd_reference_is_torch_sgd():
    for n in RC.SGD_N:
        p0, grads = RC.sgd_inputs(n)
        p = torch.nn.Parameter(p0.clone())
        opt = torch.optim.SGD([p], lr=0.1, momentum=0.9, weight_decay=1e-4)
        ref = RC.sgd_steps(p0.double(), grads, 0.1, 0.9, 1e-4)
        f32 = RC.sgd_steps(p0, grads, 0.1, 0.9, 1e-4)
        for gr, r, f in zip(grads, ref, f32):
            p.grad = gr.clone()
            opt.step()
            assert RC.rel_max(p, r) <= RC.OPT and RC.rel_max(f, r) <= RC.OPT, n


def test_mse_rownorm_cast_references():
    for n in RC.MSE_N:
        p, t = RC.mse_inputs(n)
        loss, d = RC.mse(p.double(), t.double())
        pr = p.double().requires_grad_(True)
        lr = F.mse_loss(pr, t.double())
        lr.backward()
        torch.testing.assert_close(loss, lr.detach().reshape(1), rtol=1e-12, atol=1e-14)
        torch.testing.assert_close(d, pr.grad, rtol=1e-12, atol=1e-16)
        lf, df = RC.mse(p, t)
        assert RC.rel_max(lf, loss) <= RC.F32 and RC.rel_max(df, d) <= RC.F32, n
    for D in RC.ROWNORM_D:
        for n in (1, 5):
            for scale in RC.ROWNORM_SCALES:
                for ls in (None, 2.3):
                    x, dy = RC.rownorm_inputs(n, D, scale)
                    y, rn, dx = RC.rownorm(x.double(), dy, ls)
                    k = 1.0 if ls is None else torch.tensor(ls, dtype=torch.float64).exp()
                    torch.testing.assert_close(y, k * F.normalize(x.double(), dim=1, eps=0), rtol=1e-12, atol=0)
                    yf, rf, dxf = RC.rownorm(x, dy, ls)
                    assert RC.rel_max(yf, y) <= RC.F32 and RC.row_rel_max(rf[:, None], rn[:, None]) <= RC.F32
                    assert RC.row_rel_max(dxf, dx, RC.rownorm_dx_scale(rn, dy, ls)) <= RC.F32, (D, n, scale, ls)
    x = RC.cast_input(4099)
    assert torch.equal(x[:RC.CAST_SPECIALS.numel()].view(torch.int32), RC.CAST_SPECIALS.view(torch.int32))
    y = x.to(BF).view(torch.int16).to(torch.int32) & 0xFFFF
    assert y[:4].tolist() == [0x3F80, 0x3F82, 0xBF80, 0xBF82]      # ties to even, both directions and signs
    assert y[4:8].tolist() == [0x3F81, 0x3F81, 0x0000, 0x8000]
    assert y[8:12].tolist() == [0x0000, 0x8080, 0x0000, 0x0002]    # denormals; 0x8000 ties to 0, 0x18000 to 2
    assert y[12:18].tolist() == [0x7F7F, 0x7F80, 0x7F80, 0xFF80, 0x7F80, 0xFF80]
    assert torch.isnan(x[18:22]).all() and torch.isnan(x.to(BF)[18:22]).all()
    assert torch.isfinite(x[22:]).all()


def test_case_lists_hold_the_branch_shapes():
    """Each listed size is the smallest that reaches a branch: a later edit that drops one fails here."""
    assert set(RC.LN_FWD_VEC_D) == {256, 512, 768, 1024, 1536, 2048}     # ln_fwd_kernel NV 1, 2, 3, 4, 6, 8
    assert {1280, 1792, 8, 33, 64, 200, 1000} <= set(RC.LN_FWD_SCALAR_D)  # NV 5, 7 missing: scalar; ragged D
    assert {1, 3, 4, 5, 37} <= set(RC.LN_FWD_ROWS)
    assert RC.LN_FWD_LAST_SLOT == (2048, 2050) and RC.LN_FWD_LAST_SLOT[1] % 4 != 0 and RC.LN_MAX_D == 2048
    assert RC.LN_KINDS == ("base", "offset", "tiny", "const", "outlier") and set(RC.LN_KIND_D) == {768, 200}
    assert RC.LN_EPS["tiny"] == (1e-6, 1e-5)
    assert RC.ADD_LN_D == (256, 512, 768, 1024, 1280, 1536, 1792, 2048) and {1, 5, 37} <= set(RC.ADD_LN_ROWS)
    assert set(RC.ADD_LN_KINDS) == {"offset", "tiny"}
    assert set(RC.LN_BWD_PIPE_D) == {768, 1024} and {256, 1280, 2048, 200, 33} <= set(RC.LN_BWD_SCALAR_D)
    assert {1, 4, 5, 8, 9, 12, 13, 32, 33, 37, 130} <= set(RC.LN_BWD_ROWS)
    assert RC.LN_BWD_RES_EVERY == (5, (13, 37)) and all(r % 5 for r in RC.LN_BWD_RES_EVERY[1])
    assert RC.LN_BWD_COMPACT_NP == (4, (15, 35)) and RC.LN_BWD_ODD_LD % 4 != 0
    assert set(RC.CE_SHAPES) == {(1, 1), (1, 10), (3, 63), (4, 64), (5, 65), (9, 1001), (37, 1000)}
    assert RC.CE_KINDS == ("base", "wide", "spike", "equal", "low") and RC.CE_LD_PAD == 3
    assert set(RC.CAST_N) == {1, 3, 4, 5, 1023, 1024, 1025, 4099}
    assert set(RC.POS_B) == {1, 7, 8, 9, 31, 32, 33, 40}
    assert set(RC.POS_SD) == {(5, 64), (17, 192), (3, 6), (2, 1)}
    assert [(S * D) % 4 == 0 and D % 4 == 0 for S, D in RC.POS_SD] == [True, True, False, False]
    assert set(RC.UNFOLD_PS) == {16, 14, 8, 6}
    assert set(RC.SGD_N) == {1, 3, 4, 5, 4095, 4096, 4097, 8193}
    assert set(RC.EMBED_D) == {4, 128, 260, 768} and set(RC.ROWS_D) == {1, 63, 64, 65, 200}
    assert set(RC.ROWNORM_D) == {1, 63, 64, 65, 66, 768} and set(RC.ROWNORM_SCALES) == {1.0, 1e-6, 1e6}
    assert set(RC.MSE_N) == {1, 63, 1023, 1024, 1025, 4224, 70001}
