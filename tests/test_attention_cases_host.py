"""CPU: oracle/attn_cases.py -- the attention test kinds do what they claim, and the float64 restatement of a
correct bf16 kernel's own roundings (``emulate_bf16``) stays inside every bf16 bound that
tests/test_gpu_attention_conformance.py holds the kernels to, so those bounds ask nothing of a kernel that
the number format forbids.

Bounds (relative to the reference's largest magnitude, as ``_close`` uses them everywhere): o 1.5e-2, lse 2e-3
and 2e-2 absolute, dq / dk / dv and the qkv-bias gradient 3e-2; per (b, h) item (its dq, dk and dv together) 3e-2;
per row 1.5e-2 for o and dv.  Worst emulation figures over all kinds at N = 33 and N = 289 (B = H = 2), CPU
numbers from the reference alone: o 3.3e-3, dq / dk / dv 1.3e-2 (``falling`` dq), qkv-bias gradient 1.8e-2
(``outlier``), per item 1.6e-2 (``offset``), per-row o 4.1e-3, per-row dv 4.4e-3 -- at least a 1.6x margin under each
bound."""
import pytest
import torch

from oracle import attn_cases as AC

BF16 = torch.bfloat16
B, H = 2, 2
_CASES = {}


def _case(kind, N, causal=False):
    key = (kind, N, causal)
    if key not in _CASES:
        _CASES[key] = AC.make_case(kind, B, H, N, BF16, causal=causal)
    return _CASES[key]


@pytest.mark.parametrize("N", [33, 289])
@pytest.mark.parametrize("kind", AC.KINDS)
def test_bf16_emulation_within_bounds(kind, N):
    c = _case(kind, N)
    D = c.D
    o, lse, g, colsum = AC.emulate_bf16(c)
    fig = {"o": AC.rel_max(o, c.o), "lse": AC.rel_max(lse, c.lse), "lse abs": AC.abs_max(lse, c.lse),
           "row o": AC.row_rel(o, c.o, B, H, N), "colsum": AC.rel_max(colsum, c.colsum)}
    for i, name in enumerate(("dq", "dk", "dv")):
        gi, ri = g[:, i * D:(i + 1) * D], c.grads[:, i * D:(i + 1) * D]
        fig[name] = AC.rel_max(gi, ri)
    fig["item"] = AC.item_rel(g, c.grads, B, H, N)
    fig["row dv"] = AC.row_rel(g[:, 2 * D:], c.grads[:, 2 * D:], B, H, N)
    print(kind, N, " ".join(f"{k}={v:.2e}" for k, v in fig.items()))
    assert fig["o"] <= AC.BF16_O and fig["row o"] <= AC.BF16_ROW
    assert fig["lse"] <= AC.BF16_LSE and fig["lse abs"] <= AC.BF16_LSE_ABS
    for name in ("dq", "dk", "dv", "colsum", "item"):
        assert fig[name] <= AC.BF16_GRAD, (name, fig[name])
    assert fig["row dv"] <= AC.BF16_ROW


def test_bf16_emulation_causal_within_bounds():
    c = _case("outlier", 33, causal=True)
    D = c.D
    o, lse, g, colsum = AC.emulate_bf16(c)
    assert AC.rel_max(o, c.o) <= AC.BF16_O and AC.row_rel(o, c.o, B, H, 33) <= AC.BF16_ROW
    assert AC.abs_max(lse, c.lse) <= AC.BF16_LSE_ABS
    for i in range(3):
        assert AC.rel_max(g[:, i * D:(i + 1) * D], c.grads[:, i * D:(i + 1) * D]) <= AC.BF16_GRAD
    assert AC.row_rel(g[:, 2 * D:], c.grads[:, 2 * D:], B, H, 33) <= AC.BF16_ROW
    # only the last query sees the outlier key
    p = AC.probabilities(c)
    assert (p[..., :-1, -1] == 0).all() and (p[..., -1, -1] > 0).all()


def test_reference_is_the_plain_formula():
    """The float64 reference against a loop over heads written without the module's helpers, and the layouts."""
    N, scale = 19, 0.3
    c = AC.make_case("base", B, H, N, torch.float32, causal=True, seed=3, scale=scale)
    D = c.D
    assert c.qkv.shape == (B * N, 3 * D) and c.do.shape == (B * N, D) and c.qkv.dtype == torch.float32
    assert c.o.dtype == c.lse.dtype == c.grads.dtype == c.colsum.dtype == torch.float64
    x, do = c.qkv.double(), c.do.double()
    for b in range(B):
        for h in range(H):
            rows, cols = slice(b * N, (b + 1) * N), slice(h * 64, (h + 1) * 64)
            q, k, v = (x[rows, i * D + h * 64:i * D + (h + 1) * 64].clone().requires_grad_(True) for i in range(3))
            s = (q @ k.T) * scale + torch.full((N, N), float("-inf"), dtype=torch.float64).triu(1)
            o = torch.softmax(s, -1) @ v
            o.backward(do[rows, cols])
            torch.testing.assert_close(c.o[rows, cols], o.detach(), rtol=1e-12, atol=1e-12)
            torch.testing.assert_close(c.lse[(b * H + h) * N:(b * H + h + 1) * N], torch.logsumexp(s, -1).detach(),
                                       rtol=1e-12, atol=1e-12)
            for i, t in enumerate((q, k, v)):
                torch.testing.assert_close(c.grads[rows, i * D + h * 64:i * D + (h + 1) * 64], t.grad, rtol=1e-10,
                                           atol=1e-12)
    torch.testing.assert_close(c.colsum, c.grads.sum(0))
    # rounded inputs: the reference is of what the kernel reads
    cb = AC.make_case("peaked", B, H, N, BF16)
    assert cb.qkv.dtype == BF16 and cb.do.dtype == BF16


@pytest.mark.parametrize("N", [33, 289])
def test_kinds_keep_their_claims(N):
    base = AC.probabilities(_case("base", N)).amax(-1).median().item()
    peaked = AC.probabilities(_case("peaked", N)).amax(-1).median().item()
    print(f"median row max: base {base:.3f} peaked {peaked:.3f}")
    assert base < 0.5 and peaked > 0.9
    assert _case("offset", N).lse.min().item() > 200
    assert _case(AC.MILDER["offset"], N).lse.min().item() > 100
    assert _case("peaked", N).lse.max().item() > 40 > _case("base", N).lse.max().item()
    last = (AC.probabilities(_case("outlier", N)).argmax(-1) == N - 1).double().mean().item()
    print(f"outlier: rows with their maximum at the last key {last:.3f}")
    assert last > 0.25
    # the ramp lifts the scores by 40 over the keys, 4 over the last tenth, under a spread of about 5 from
    # the random parts: most rows peak in the last (first) tenth, every row in the last (first) third
    for kind in ("rising", "falling"):
        arg = AC.probabilities(_case(kind, N)).argmax(-1)
        arg = arg if kind == "rising" else N - 1 - arg
        tenth = (arg >= N - 1 - N // 10).double().mean().item()
        print(f"{kind}: rows with their maximum in the last tenth {tenth:.3f}, earliest {arg.min().item()}")
        assert tenth > 0.75 and arg.min().item() >= N - 1 - N // 3
    z = _case("zerorows", N)
    q, k, v = AC.split_qkv(z.qkv.float(), B, H, N)
    assert (q[:, :, ::3] == 0).all() and (k[:, :, 1::5] == 0).all() and (v[:, :, 2::7] == 0).all()
    pz = AC.probabilities(z)
    assert torch.allclose(pz[:, :, ::3], torch.full_like(pz[:, :, ::3], 1.0 / N))
    # no kind is another under a different name
    seen = [_case(kind, N).qkv for kind in AC.KINDS + tuple(AC.MILDER.values())]
    for i in range(len(seen)):
        for j in range(i):
            assert not torch.equal(seen[i], seen[j])
