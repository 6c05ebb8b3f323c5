"""CPU: oracle/dora_cases.py -- the end-to-end reference is float64 autograd of the oracle's DoRA weight, the stage
references composed in float64 reproduce it, the same stages in torch float32 stay inside every stage bound
tests/test_gpu_dora.py holds the kernels to (so the bounds are reachable by plain f32 arithmetic before a GPU is
involved), each planted error breaks the bound of the stage it is planted in, and ``vit_amd.dora_weight`` refuses
operands that do not fit.

Worst torch-float32 err / bound per stage over every case of this file (``test_torch_f32_within_every_stage_bound``
prints the table; profiles/r23/dora_host_bounds.txt keeps it): DnT 0.42, nu 0.07, W 0.34, dm 0.05, sdDnT 0.29,
dB 0.06, dA 0.16."""
import math

import pytest
import torch

from oracle import dora_cases as DC
from oracle import vit_ref as R

CLOSE = dict(rtol=1e-11, atol=0)


def _unmasked():
    return [c for c in DC.cases() if c[3] not in ("masked", "zero_delta_noise0")]


def test_reference_is_float64_autograd_of_the_oracle():
    for fin, fout, r, kind in _unmasked():
        c = DC.case(fin, fout, r, kind)
        m, A, Bm = (t.double().clone().requires_grad_(True) for t in (c.m, c.A, c.B))
        W = R.dora_weight(m, A, Bm, c.D.double(), c.s)
        W.backward(c.gW.double())
        torch.testing.assert_close(c.ref["W"], W.detach(), **CLOSE)
        for name, t in (("dm", m), ("dA", A), ("dB", Bm)):
            torch.testing.assert_close(c.ref[name], t.grad, rtol=1e-11, atol=1e-300)
        assert all(bool(torch.isfinite(v).all()) for v in c.ref.values())
    # with a noise: the oracle's formula on the dropped-out delta, and sdDnT is what the factor gradients are made of
    for fin, fout, r, kind in DC.cases():
        c = DC.case(fin, fout, r, kind)
        if c.noise is not None:
            m, A, Bm = (t.double().clone().requires_grad_(True) for t in (c.m, c.A, c.B))
            Dn = c.D.double() + (Bm @ A) * c.s * c.noise.double()
            W = ((Dn / (torch.norm(Dn, dim=0, keepdim=True) + 1e-8)) * m).T
            W.backward(c.gW.double())
            torch.testing.assert_close(c.ref["W"], W.detach(), **CLOSE)
            for name, t in (("dm", m), ("dA", A), ("dB", Bm)):
                torch.testing.assert_close(c.ref[name], t.grad, rtol=1e-11, atol=1e-300)
        sd = c.ref["sdDnT"]
        scale = lambda t: float(t.abs().max()) * 1e-12 + 1e-300
        torch.testing.assert_close(sd.T @ c.A.double().T, c.ref["dB"], rtol=0, atol=scale(c.ref["dB"]))
        torch.testing.assert_close(c.B.double().T @ sd.T, c.ref["dA"], rtol=0, atol=scale(c.ref["dA"]))


def test_stage_references_compose_to_the_end_to_end_reference():
    for fin, fout, r, kind in DC.cases():
        c = DC.case(fin, fout, r, kind)
        d = lambda t: None if t is None else t.double()
        m, A, Bm, D, gW, nz = d(c.m), d(c.A), d(c.B), d(c.D), d(c.gW), d(c.noise)
        DnT = DC.ref_DnT(A, Bm, D, c.s, nz)[0]
        nu = DC.ref_nu(DnT)[0]
        sd = DC.ref_sdDnT(gW, DnT, nu, m, c.s, nz)[0]
        got = dict(DnT=DnT, nu=nu, W=DC.ref_W(DnT, nu, m)[0], dm=DC.ref_dm(gW, DnT, nu)[0], sdDnT=sd,
                   dB=DC.ref_dB(sd, A)[0], dA=DC.ref_dA(sd, Bm)[0])
        for name in DC.STAGES:
            # per column where columns differ in scale by 1e8; dB against its own largest magnitude
            if name == "dB":
                e = float((got[name] - c.ref[name]).abs().max() / c.ref[name].abs().max().clamp_min(1e-300))
            else:
                e = float(DC.col_rel(name, got[name], c.ref[name]).max())
            # at in = 1 the gradient with respect to Dn is the 1e-8 residue of a complete cancellation
            assert e <= (1e-6 if fin == 1 and name in ("sdDnT", "dA", "dB") else 1e-10), (fin, fout, r, kind, name, e)


def test_torch_f32_within_every_stage_bound():
    worst = {}
    for fin, fout, r, kind in DC.cases():
        c = DC.case(fin, fout, r, kind)
        fr = DC.stage_fractions(c, c.torch_f32)
        assert set(fr) == set(DC.STAGES)
        for name, f in fr.items():
            assert f <= 1.0, (fin, fout, r, kind, name, f)
            if f > worst.get(name, (0.0,))[0]:
                worst[name] = (f, f"{fin}x{fout} r{r} {kind}")
        for name, base in DC.E2E.items():
            assert c.e2e_bound(name) >= base
            assert c.e2e_fraction(name, c.torch_f32[name]) <= 1.0, (fin, fout, r, kind, name)
            assert c.e2e_fraction(name, c.ref[name]) == 0.0
        # the forward never needs the hard rule: no forward stage cancels
        assert all(c.e2e_bound(name) == DC.FWD for name in ("W", "DnT", "nu")), (fin, fout, r, kind)
    print("worst torch f32 err / bound per stage:")
    for name in DC.STAGES:
        print(f"  {name:6s} {worst.get(name, (0.0, '-'))[0]:.3f}  {worst.get(name, (0.0, '-'))[1]}")


def test_fraction_counts_non_finite_and_zero_bounds():
    ref, bound = torch.tensor([1.0, 0.0], dtype=torch.float64), torch.tensor([0.5, 0.0], dtype=torch.float64)
    assert DC.fraction(torch.tensor([1.25, 0.0]), ref, bound) == 0.5
    assert DC.fraction(torch.tensor([1.25, 1e-30]), ref, bound) == math.inf
    assert DC.fraction(torch.tensor([float("nan"), 0.0]), ref, bound) == math.inf
    assert DC.fraction(torch.tensor([float("inf"), 0.0]), ref, bound) == math.inf


def test_kinds_keep_their_claims():
    for fin, fout, r in DC.KIND_SHAPES:
        base = DC.case(fin, fout, r, "base")
        torch.testing.assert_close(base.D.double().norm(dim=0), torch.ones(fout, dtype=torch.float64), rtol=1e-6,
                                   atol=0)
        assert base.noise is None and base.s == 16 / r
        mk = DC.case(fin, fout, r, "masked")
        assert sorted(mk.noise.unique().tolist()) == [0.0, 2.0] and 0.4 < float((mk.noise == 0).float().mean()) < 0.6
        assert not torch.equal(mk.noise, mk.noise.flatten().view(fout, fin).T)
        for kind in ("zero_delta", "zero_delta_noise0"):
            z = DC.case(fin, fout, r, kind)
            assert not z.B.any() and (z.noise is None) == (kind == "zero_delta")
            assert z.noise is None or not z.noise.any()
            assert torch.equal(z.torch_f32["DnT"], z.D.T) and not z.torch_f32["dA"].any() and not z.ref["dA"].any()
        zc = DC.case(fin, fout, r, "zero_col")
        cols = DC.zero_cols(fout)
        assert cols == [1, fout - 1] and not zc.D[:, cols].any() and not zc.A[:, cols].any() and zc.m[cols].all()
        for src in (zc.ref, zc.torch_f32):
            assert not src["nu"][cols].any() and not src["W"][cols].any() and not src["dm"][cols].any()
            assert all(bool(torch.isfinite(v).all()) for v in src.values())
        want = zc.s * zc.m.double()[cols, None] / 1e-8 * zc.gW.double()[cols]
        torch.testing.assert_close(zc.ref["sdDnT"][cols], want, rtol=1e-12, atol=0)
        torch.testing.assert_close(zc.torch_f32["sdDnT"][cols].double(), want, rtol=1e-6, atol=0)
        tc = DC.case(fin, fout, r, "tiny_col")
        nu = tc.ref["nu"][DC.tiny_cols(fout)]
        assert len(DC.tiny_cols(fout)) == 2 and bool(((nu > 2.9e-8) & (nu < 3.1e-8)).all())   # 1e-8 is a quarter of n
        # what DoRALayer.__init__ makes, in its RNG order
        import vit_amd
        ic = DC.case(fin, fout, r, "init")
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(131 + fin + fout + r)
            layer = vit_amd.DoRALayer(torch.nn.Linear(fin, fout), r=r, dora_alpha=16)
        for got, want in ((ic.m, layer.m), (ic.A, layer.delta_D_A), (ic.B, layer.delta_D_B), (ic.D, layer.D)):
            assert torch.equal(got, want.detach())
        assert ic.s == layer.scaling and ic.B.any()


def test_index_kind_is_exact():
    for fin, fout, r, kind in DC.cases():
        if kind != "index":
            continue
        c = DC.case(fin, fout, r, kind)
        want = DC.index_expected(c)
        assert not c.B.any() and math.log2(c.s) == int(math.log2(c.s))
        assert set(want) == set(DC.STAGES)
        for name in DC.STAGES:
            w32 = want[name].float()
            assert torch.equal(w32.double(), want[name]), (name, "not an f32 value")
            got = c.torch_f32[name]
            assert torch.equal((got + 0.0).view(torch.int32), (w32.reshape(got.shape) + 0.0).view(torch.int32)), (
                fin, fout, r, name)
            if name == "dB":
                e = float((want[name] - c.ref[name]).abs().max() / c.ref[name].abs().max().clamp_min(1e-300))
            else:
                e = float(DC.col_rel(name, want[name], c.ref[name]).max())
            assert e <= 1e-7, (fin, fout, r, name, e)      # the float64 autograd carries the 1e-8
        assert bool((2 * want["dB"] == (2 * want["dB"]).round()).all())   # halves of integers: an exact sum
        assert want["dB"].any() and want["sdDnT"].any() and not want["dA"].any()


# (plant, kind, (in, out, r), the stages whose bound breaks): every other stage stays inside its bound, because it
# is held against float64 of what the planted stage stored
PLANTED = [
    ("no_eps", "tiny_col", (96, 80, 8), {"W", "dm", "sdDnT"}),
    ("no_eps", "zero_col", (96, 80, 8), {"W", "dm", "sdDnT", "dB", "dA"}),   # 0 / 0: nothing finite downstream
    ("n_for_nu", "tiny_col", (96, 80, 8), {"sdDnT"}),
    ("no_guard", "zero_col", (130, 257, 33), {"sdDnT", "dB", "dA"}),         # NaN rows reach both factor products
    ("skip_rank_term", "base", (96, 80, 8), {"DnT"}),
    ("skip_rank_term", "base", (65, 63, 1), {"DnT"}),
    ("norm_skips_last_row", "base", (96, 80, 8), {"nu"}),
    ("norm_skips_last_row", "base", (1024, 1024, 32), {"nu"}),               # one row of 1024: the bound does not grow with in
    ("noise_as_out_in", "masked", (96, 80, 8), {"DnT"}),
    ("bwd_unmasked", "masked", (130, 257, 33), {"sdDnT"}),
    ("W_untransposed", "base", (96, 80, 8), {"W"}),
    ("W_untransposed", "base", (64, 64, 64), {"W"}),
]


@pytest.mark.parametrize("plant, kind, shape, breaks", PLANTED, ids=[f"{p[0]}-{p[1]}-{p[2][0]}x{p[2][1]}" for p in PLANTED])
def test_planted_errors_break_their_stage(plant, kind, shape, breaks):
    c = DC.case(*shape, kind)
    fr = DC.stage_fractions(c, DC.f32_stages(c, plant))
    broken = {name for name, f in fr.items() if not f <= 1.0}
    print(plant, kind, shape, {k: f"{v:.3g}" for k, v in fr.items()})
    assert broken == breaks, (plant, kind, shape, fr)


def test_every_planted_error_is_listed():
    assert {p[0] for p in PLANTED} == set(DC.PLANTS)
    # the planted errors that only special columns see are invisible on ``base``: the kinds are needed
    c = DC.case(96, 80, 8, "base")
    for plant in ("no_eps", "n_for_nu", "no_guard"):
        assert all(f <= 1.0 for f in DC.stage_fractions(c, DC.f32_stages(c, plant)).values()), plant


def test_case_list_holds_the_edge_shapes():
    """Each listed size is the smallest that reaches its edge: a later edit that drops one fails here."""
    assert set(DC.SHAPES) == {(1, 1, 1), (3, 5, 2), (63, 65, 8), (65, 63, 1), (64, 64, 64), (96, 80, 8), (130, 257, 33),
                              (257, 130, 5), (256, 320, 8), (260, 333, 5), (768, 768, 32), (1024, 1024, 32)}
    assert DC.KIND_SHAPES == ((96, 80, 8), (130, 257, 33)) and DC.SPLIT_SHAPES == ((256, 320, 8), (260, 333, 5))
    assert DC.KINDS == ("base", "init", "masked", "zero_delta", "zero_delta_noise0", "zero_col", "tiny_col", "index")
    listed = DC.cases()
    assert len(listed) == len(set(listed)) == 12 + 2 * 7 + 2
    assert all((i, o, r, "base") in listed for i, o, r in DC.SHAPES)
    assert all((i, o, r, k) in listed for i, o, r in DC.KIND_SHAPES for k in DC.KINDS)
    # vit_gemm_splitk splits a factor GEMM [M, N] over R when R >= 256 and M * N % 4 == 0: dB is [in, r] over out,
    # dA is [r, out] over in
    (i0, o0, r0), (i1, o1, r1) = DC.SPLIT_SHAPES
    assert o0 // 128 == 2 and i0 // 128 == 2 and (i0 * r0) % 4 == 0 and (r0 * o0) % 4 == 0
    assert o1 // 128 == 2 and i1 // 128 == 2 and (i1 * r1) % 4 == 0 and (r1 * o1) % 4 != 0
    assert all(i < 256 and o < 256 or (i, o, r) in DC.SPLIT_SHAPES or i == o for i, o, r in DC.SHAPES if i != 257 and o != 257)
    assert DC.nu_depth(1) == DC.nu_depth(1024) == 26 and DC.c_depth(64) == 8 and DC.c_depth(65) == 9


def test_dora_weight_refuses_operands_that_do_not_fit():
    """The checks come before the GPU is asked for: CPU tensors reach them."""
    import vit_amd
    from vit_amd import _lib as L
    fin, fout, r = 6, 8, 2
    z = torch.zeros
    good = dict(m=z(fout), A=z(r, fout), Bm=z(fin, r), D=z(fin, fout), noise=None)

    def call(**kw):
        a = {**good, **kw}
        return vit_amd.dora_weight(a["m"], a["A"], a["Bm"], a["D"], 2.0, a["noise"])

    with pytest.raises(L.HipError):          # everything fits: only the device is wrong
        call()
    with pytest.raises(L.HipError):
        call(noise=z(fin, fout))
    bad = [dict(A=z(r, fin)), dict(A=z(r, fout + 1)), dict(Bm=z(fout, r)), dict(Bm=z(fin, r + 1)), dict(m=z(fin)),
           dict(m=z(1, fout)), dict(noise=z(fout, fin)), dict(noise=z(fin * fout)), dict(D=z(fout, fin)),
           dict(D=z(fin * fout)), dict(A=z(fout)), dict(A=z(0, fout), Bm=z(fin, 0)),
           dict(A=z(65, fout), Bm=z(fin, 65)), dict(D=z(0, fout), Bm=z(0, r)),
           dict(D=z(fin, 0), A=z(r, 0), m=z(0))]
    for kw in bad:
        with pytest.raises(ValueError):
            call(**kw)
    with pytest.raises(L.HipError):          # r = 64 and r = 1 are inside the range
        call(A=z(64, fout), Bm=z(fin, 64))
    with pytest.raises(L.HipError):
        call(A=z(1, fout), Bm=z(fin, 1))
