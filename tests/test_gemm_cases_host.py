"""Host: the premises of oracle/gemm_cases.py, without a GPU.

For every case the GPU tests run (tests/test_gpu_gemm_exact.py): the operands round-trip their storage dtype and
every accumulated value stays in the range where f32 holds it exactly, so one float64 reference serves every
kernel bit for bit; torch's own f32 matmul reproduces that reference bitwise; the activation bound admits the two
f32 restatements of the activations; and every dispatch branch the GPU file names keeps a listed shape under the
host's rules as the header documents them.
"""
import pytest
import torch

from oracle import gemm_cases as G

F32, BF = G.F32, G.BF


def _exact_in(t, dtype):
    return torch.equal(t.to(dtype).double(), t.double())


def _mm_cases():
    out = [(s, BF, "int") for s in G.G4_SHAPES + (G.V1_FWD, G.V3_DGRAD, G.RESID_SHAPE, G.MISALIGNED, G.N_MOD8_4)]
    out += [(s, BF, "quarter") for s in G.PAIR_SHAPES]
    out += [(s, BF, "int") for s in G.ACT_BWD_SHAPES]
    out += [(G.F32_MFMA, F32, "int"), (G.F32_MFMA, F32, "quarter"), (G.F32_STREAMK, F32, "int")]
    out += [(s, dt, "int") for s in G.GEN_SHAPES for dt in (BF, F32)]
    out += [(G.SPLITK, F32, "int"), (G.G4_SHAPES[1], F32, "int")]
    return sorted(set(out), key=str)


@pytest.mark.parametrize("shape,dtype,kind", _mm_cases(), ids=str)
def test_mm_case_is_exact(shape, dtype, kind):
    c = G.mm_case(*shape, dtype, kind)
    for t in (c.p, c.q, c.qT):
        assert t.dtype == dtype and _exact_in(t, dtype)
    assert torch.equal(c.qT.double(), c.q.double().T)
    assert torch.equal(c.acc, c.p.double() @ c.q.double().T) and torch.equal(c.pre, c.acc + c.bias.double())
    # every partial sum is a multiple of 1/16 bounded by sum |p| |q| < 2^24 / 16: exact in f32 in any order
    assert (c.p.double().abs() @ c.q.double().abs().T).max().item() * 16 < 2 ** 24
    step = 4 if kind == "quarter" else 1
    assert torch.equal((c.pre * step).round(), c.pre * step)
    if kind == "quarter":
        assert c.pre.abs().max().item() < 64
        if dtype == BF:  # spread over both tails and the middle of GELU
            assert c.pre.min().item() <= -6 and c.pre.max().item() >= 6 and (c.pre.abs() < 1).float().mean() > 0.1
    else:
        assert c.pre.abs().max().item() <= 256 and c.acc.abs().max().item() <= 256
    if dtype == BF:
        assert _exact_in(c.pre, BF) and _exact_in(c.acc, BF)
    # torch's f32 matmul: the same bits as the float64 reference
    got = c.p.float() @ c.q.float().T
    assert torch.equal(got.double(), c.acc)
    assert torch.equal((got + c.bias).double(), c.pre)


@pytest.mark.parametrize("shape", G.ACT_BWD_SHAPES + (G.F32_MFMA,), ids=str)
def test_act_bwd_sums_are_exact_and_tell_the_two_readings_apart(shape):
    M, N, R = shape
    dtype = F32 if shape == G.F32_MFMA else BF
    c = G.mm_case(M, N, R, dtype)
    aux = G.sixteenths(M, N, dtype)
    assert _exact_in(aux, dtype) and aux.min().item() >= 0 and aux.max().item() <= 1.25
    assert torch.equal((aux.double() * 16).round(), aux.double() * 16)
    stored, s_stored, s_prod = G.act_bwd_ref(c.acc, aux, dtype)
    assert torch.equal((stored.double() * 16).round(), stored.double() * 16)
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(5))
    for vals, ref in ((stored.float(), s_stored), ((c.acc * aux.double()).float(), s_prod)):
        assert vals.abs().sum(0).max().item() * 16 < 2 ** 24
        for v in (vals, vals[perm], vals.flip(0)):   # any order: the same f32 bits, and the float64 sum
            assert torch.equal(v.sum(0).double(), ref)
            assert torch.equal(v.cumsum(0)[-1].double(), ref)
    if dtype == BF:
        differ = (s_stored != s_prod).float().mean().item()
        print(f"{shape}: stored and unrounded column sums differ in {differ:.0%} of the columns")
        assert differ > 0.5
    else:
        assert torch.equal(s_stored, s_prod)  # an f32 output stores the product itself


@pytest.mark.parametrize("N,K", G.WGRAD_NK)
@pytest.mark.parametrize("M,split", G.WGRAD_ROWS)
def test_wgrad_case_is_exact(M, split, N, K):
    c = G.wg_case(M, N, K)
    assert _exact_in(c.dy, BF) and _exact_in(c.x, BF)
    assert torch.equal((c.dy.float().T @ c.x.float()).double(), c.dW) and c.dW.abs().max().item() < 2 ** 24
    # the host's slab count: at most `split`, and each slab at least one k-step
    nz = G.wgrad_nslabs(M, split)
    assert 1 <= nz <= split
    if (M, split) == (160, 3):
        assert nz == 3
    assert G.bf16_branch("wgrad", N, K, M - M % 32) == ("pp" if M >= 32 else "gen")


@pytest.mark.parametrize("M,N,K,split", G.WGRAD_F32)
def test_wgrad_f32_case_is_exact(M, N, K, split):
    c = G.wg_case(M, N, K, F32)
    assert torch.equal((c.dy.T @ c.x).double(), c.dW)


@pytest.mark.parametrize("B,np_,D,K", G.PATCH)
def test_patch_case_is_exact(B, np_, D, K):
    c = G.patch_case(B, np_, D, K)
    got = (c.U.float() @ c.W.float().T + c.bias).view(B, np_, D) + c.pos[1:]
    assert torch.equal(got.double(), c.rows) and _exact_in(c.pos, F32)
    assert torch.equal((c.rows * 8).round(), c.rows * 8)


@pytest.mark.parametrize("shape,dtype", [(s, BF) for s in G.PAIR_SHAPES] + [(G.F32_MFMA, F32)], ids=str)
@pytest.mark.parametrize("act", ["gelu", "qgelu"])
def test_activation_bound_admits_the_f32_restatements(act, shape, dtype):
    """The bound is derived from the code's approximation; here the f32 restatement of the fast form and torch's
    f32 erf GELU are held to it on the exact pre of every listed case, rounded to the output type as the kernels
    round.  (The restatements are not the kernel: a kernel that misses the bound is a finding.)"""
    c = G.mm_case(*shape, dtype, "quarter")
    ref64, fast32 = G.ACTS[act]
    ra, rd = ref64(c.pre)
    forms = {"restated": fast32(c.pre)}
    if act == "gelu":
        x = c.pre.float()
        forms["torch erf"] = (torch.nn.functional.gelu(x), G.gelu_both(x)[1])
    for name, (a, d) in forms.items():
        for which, got, ref in (("act", a, ra), ("act'", d, rd)):
            f = G.act_fraction(got.to(dtype), ref, c.pre, dtype)
            f32only = ((got.double() - ref).abs() / (G.ACT_ABS * c.pre.abs().clamp_min(1.0))).max().item()
            print(f"{act} {which} {name} {shape}: {f:.3f} of the bound; f32 error {f32only:.3f} of its second term")
            assert f <= 1.0 and f32only <= 1.0


def test_every_named_branch_keeps_a_shape():
    B = G.bf16_branch
    for M, N, R in G.G4_SHAPES + (G.MISALIGNED,):
        assert B("fwd", M, N, R) == "g4" and B("dgrad", M, N, R) == "g4"
    M, N, R = G.G4_SHAPES[1]
    assert -(-M // 256) == 2 and M % 256 == 1 and N % 256 == 136 and (R // 64) % 2 == 1
    assert G.G4_SHAPES[2][1] % 256 == 8 and -(-G.G4_SHAPES[3][0] // 256) == 3
    for M, N, R in G.PAIR_SHAPES:
        assert B("fwd", M, N, R, "pair", g4_gelu=1) == "v5" and B("fwd", M, N, R, "pair", g4_gelu=3) == "g4"
    assert B("fwd", *G.V1_FWD) == "v1"
    assert B("fwd", *G.N_MOD8_4) == "v5" and B("dgrad", *G.N_MOD8_4) == "gen" and G.N_MOD8_4[1] % 8 == 4
    for M, N, R in G.ACT_BWD_SHAPES:
        assert B("dgrad", M, N, R, "act_bwd", csum=True, g4_gelu=0) == "v1"
        assert B("dgrad", M, N, R, "act_bwd", csum=True, g4_gelu=3) == "g4" and R == 128
    assert [-(-s[0] // 64) for s in G.ACT_BWD_SHAPES] == [2, 5] and all(s[0] % 64 for s in G.ACT_BWD_SHAPES)
    assert B("dgrad", *G.V3_DGRAD, csum=True) == "v3" and B("dgrad", *G.V3_DGRAD) == "g4"
    assert B("fwd", *G.RESID_SHAPE, "resid") == "v5"
    # weight gradient: MFMA rows + generic tail
    assert [(m - m % 32, m % 32) for m, _ in G.WGRAD_ROWS] == [(32, 0), (96, 0), (160, 0), (32, 18), (0, 19)]
    (M, N, K, s), small, odd = G.WGRAD_F32
    assert G.f32_branch(G.CR, G.CR, N, K, M, s) == "mfma" and G.f32_tiles(N, K) * s == 64
    assert G.f32_branch(G.CR, G.CR, small[1], small[2], small[0], small[3]) == "gen"
    assert G.f32_branch(G.CR, G.CR, odd[1], odd[2], odd[0], odd[3]) == "gen" and (odd[1] * odd[2]) % 4 and odd[3] > 1
    # f32 MFMA: exactly the 64-tile rule, ragged both ways; stream-K only with a workspace
    M, N, R = G.F32_MFMA
    assert G.f32_tiles(M, N) == 64 and M % 128 and N % 128
    for pl, ql, m, n in ((G.RC, G.RC, M, N), (G.RC, G.CR, M, N), (G.CR, G.CR, M, N), (G.CR, G.RC, M, N)):
        assert G.f32_branch(pl, ql, m, n, R) == "mfma"
    assert G.f32_branch(G.RC, G.RC, *G.F32_STREAMK, streamk_ws=True) == "streamk"
    assert G.f32_branch(G.RC, G.RC, *G.F32_STREAMK) == "mfma" and G.f32_tiles(*G.F32_STREAMK[:2]) == 520
    for M, N, R in G.GEN_SHAPES:
        for pl in (G.RC, G.CR):
            for ql in (G.RC, G.CR):
                assert not G.bf16_mfma_ok(pl, ql, M, N, R) and G.f32_branch(pl, ql, M, N, R) == "gen"
        assert G.gen_tile(M, N) == 32
    assert G.GEN_SHAPES[2][2] == 1
    (B_, np_, D, K), (_, _, _, K2) = G.PATCH
    assert B("fwd", B_ * np_, D, K, "patch") == "v5" and B("fwd", B_ * np_, D, K2, "patch") == "gen"
    M, N, R = G.SPLITK
    assert min(256 // (-(-N // 32) * -(-M // 32)), R // 128) == 4 and (M * N) % 4 == 0
