"""GPU: the DoRA weight build and its backward (csrc/dora.hip, vit_amd/dora.py) stage by stage against float64.

Every case of oracle/dora_cases.py runs through ``vit_dora_weight_fwd`` and ``vit_dora_weight_bwd_ws`` with raw
pointers.  Each stored tensor (DnT, nu, W, dm, sdDnT, dB, dA) is held to the per-element bound of its stage,
against float64 of what the stage before it stored (the bounds and their derivations: oracle/dora_cases.py), and
end to end against float64 autograd per column of Dn at the project's 1e-5 / 1e-4.  Outputs and workspaces start
as NaN inside a sentinel-filled buffer, inputs sit inside NaN: a value a kernel reads before it wrote it, a store
outside an output and a load outside an input all show.  Then the split-K settings of the factor gradients,
capture and replay, views and a shared workspace through ``vit_amd.dora_weight``, and the refusals.
"""
import functools

import pytest
import torch

from oracle import dora_cases as DC
from vit_amd import _lib as L

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
SENT = 640.0          # outside every value the cases produce
OFF = 64              # floats in front of a view: 256 bytes, so every view keeps the allocation's 16-byte alignment
GUARD = 4096          # floats behind a view
ROOM = 2 * 256 * 1024  # the slab room vit_amd/dora.py passes
INVALID = 1           # hipErrorInvalidValue
OUTS = ("W", "nu", "DnT", "colsq", "dm", "dA", "dB", "sdDnT")
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    L.load()


class Buf:
    """``n`` floats ``OFF`` into a buffer with ``GUARD`` floats behind them.  An input (``src`` given) lies in NaN
    and keeps a snapshot; an output starts as NaN and lies in the sentinel."""

    def __init__(self, n, src=None, fill=NAN):
        self.n = n
        self.buf = torch.full((OFF + n + GUARD,), NAN if src is not None else SENT, dtype=torch.float32, device=DEV)
        self.v = self.buf[OFF:OFF + n]
        if src is not None:
            self.v.copy_(src.reshape(-1))
            self.snap = self.buf.clone()
        else:
            self.v.fill_(fill)

    @property
    def ptr(self):
        return self.v.data_ptr()

    def unchanged(self, what):
        assert torch.equal(self.buf.view(torch.int32), self.snap.view(torch.int32)), f"{what}: an input changed"

    def outside_untouched(self, what):
        out = torch.cat([self.buf[:OFF], self.buf[OFF + self.n:]])
        assert bool((out == SENT).all()), f"{what}: wrote outside its {self.n} floats"

    def all_untouched(self, what):
        assert bool((self.buf == SENT).all()), f"{what}: wrote into a buffer of a refused call"


def _bits(t):
    """The int32 image of an f32 tensor with -0 folded onto +0 (the sign of a zero is no part of any claim)."""
    return (t.detach().float().cpu().contiguous() + 0.0).view(torch.int32)


def _same_bits(a, b):
    return a.keys() == b.keys() and all(torch.equal(_bits(a[k]), _bits(b[k])) for k in a)


def _sizes(c):
    fin, fout, r = c.fin, c.fout, c.r
    return dict(W=fout * fin, nu=fout, DnT=fout * fin, colsq=((fin + 63) // 64) * fout, dm=fout, dA=r * fout,
                dB=fin * r, sdDnT=fout * fin)


def _shape(c, name):
    fin, fout, r = c.fin, c.fout, c.r
    return dict(W=(fout, fin), DnT=(fout, fin), sdDnT=(fout, fin), dA=(r, fout), dB=(fin, r)).get(name, (-1,))


def _launch(c, ins, outs, slabs, room, entry, st=None):
    st = L.stream_ptr(DEV) if st is None else st
    p = lambda b: None if b is None else b.ptr
    nz = p(ins.get("noise"))
    L.call("vit_dora_weight_fwd", c.fin, c.fout, c.r, p(ins["m"]), p(ins["A"]), p(ins["B"]), p(ins["D"]), c.s, nz,
           p(outs["W"]), p(outs["nu"]), p(outs["DnT"]), p(outs["colsq"]), st)
    head = (c.fin, c.fout, c.r, p(ins["m"]), p(ins["A"]), p(ins["B"]), p(ins["gW"]), p(outs["DnT"]), c.s,
            p(outs["nu"]), p(outs["dm"]), p(outs["dA"]), p(outs["dB"]), p(outs["sdDnT"]))
    if entry == "ws":
        L.call("vit_dora_weight_bwd_ws", *head, p(slabs), room, nz, st)
    else:
        L.call("vit_dora_weight_bwd", *head, nz, st)


def _buffers(c, room):
    ins = {k: Buf(t.numel(), t) for k, t in (("m", c.m), ("A", c.A), ("B", c.B), ("D", c.D), ("gW", c.gW))}
    if c.noise is not None:
        ins["noise"] = Buf(c.noise.numel(), c.noise)
    outs = {k: Buf(n) for k, n in _sizes(c).items()}
    return ins, outs, Buf(room)


def _settle(c, ins, outs, slabs, what):
    torch.cuda.synchronize()
    for k, b in ins.items():
        b.unchanged(f"{what} {k}")
    for k, b in outs.items():
        b.outside_untouched(f"{what} {k}")
    slabs.outside_untouched(f"{what} slabs")
    got = {k: outs[k].v.cpu().clone().reshape(_shape(c, k)) for k in OUTS}
    assert bool(torch.isfinite(got.pop("colsq")).all()), f"{what}: colsq holds a value the kernel did not write"
    return got


def run(c, room=ROOM, entry="ws", null_slabs=False):
    """Forward and backward of one case in fresh poisoned buffers; the guards are checked, the stored tensors come
    back on the CPU with the slab buffer."""
    what = f"{c.fin}x{c.fout} r{c.r} {c.kind} room {room} {entry}"
    ins, outs, slabs = _buffers(c, room)
    _launch(c, ins, outs, None if null_slabs else slabs, room, entry)
    return _settle(c, ins, outs, slabs, what), slabs


@functools.lru_cache(maxsize=None)
def stored(fin, fout, r, kind):
    return run(DC.case(fin, fout, r, kind))[0]


def _note(stage, f, what):
    if not f <= WORST.get(stage, (-1.0,))[0]:
        WORST[stage] = (f, what)


def _hold_stages(c, got, what):
    fr = DC.stage_fractions(c, got)
    assert set(fr) == set(DC.STAGES)
    print(f"{what}: err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in fr.items()))
    for k, v in fr.items():
        _note(k, v, what)
    bad = {k: v for k, v in fr.items() if not v <= 1.0}
    assert not bad, f"{what}: outside the stage bound: {bad}"


IDS = [f"{i}x{o}r{r}-{k}" for i, o, r, k in DC.cases()]


@pytest.mark.parametrize("fin, fout, r, kind", DC.cases(), ids=IDS)
def test_every_stage_within_its_float64_bound(fin, fout, r, kind):
    c = DC.case(fin, fout, r, kind)
    got = stored(fin, fout, r, kind)
    what = f"{fin}x{fout} r{r} {kind}"
    _hold_stages(c, got, what)
    if kind == "index":
        want = DC.index_expected(c)
        for name in DC.STAGES:
            nbad = int((_bits(got[name]) != _bits(want[name].reshape(got[name].shape))).sum())
            assert nbad == 0, f"{what} {name}: {nbad} elements differ from the exact result"
    if kind in ("zero_delta", "zero_delta_noise0"):
        assert torch.equal(_bits(got["DnT"]), _bits(c.D.T)), f"{what}: DnT is not D^T bit for bit"
        assert not got["dA"].any(), f"{what}: dA is not exactly zero"
    if kind == "zero_delta_noise0":
        assert not got["sdDnT"].any() and not got["dB"].any()
    if kind == "zero_col":
        cols = DC.zero_cols(fout)
        assert not got["nu"][cols].any() and not got["W"][cols].any() and not got["dm"][cols].any()
        assert not got["DnT"][cols].any() and got["sdDnT"][cols].any()
    assert all(bool(torch.isfinite(v).all()) for v in got.values()), f"{what}: a non-finite output"


@pytest.mark.parametrize("fin, fout, r, kind", DC.cases(), ids=IDS)
def test_end_to_end_against_float64_autograd_per_column(fin, fout, r, kind):
    """W, DnT, nu at 1e-5 and dm, sdDnT, dA at 1e-4 of each column's own largest magnitude (four times torch
    float32's own figure where that is larger: ``DoraCase.e2e_bound``); dB mixes the columns and is held by its
    stage bound above."""
    c = DC.case(fin, fout, r, kind)
    got = stored(fin, fout, r, kind)
    fr = {name: c.e2e_fraction(name, got[name]) for name in DC.E2E}
    print(f"{fin}x{fout} r{r} {kind}: end to end, err / bound "
          + ", ".join(f"{k} {v:.3f} (of {c.e2e_bound(k):.1e})" for k, v in fr.items()))
    for k, v in fr.items():
        _note("e2e " + k, v, f"{fin}x{fout} r{r} {kind}")
    bad = {k: v for k, v in fr.items() if not v <= 1.0}
    assert not bad, f"outside the end-to-end bound: {bad}"


def _rooms(c):
    return (0, 2 * c.fin * c.r, 2 * max(c.fin, c.fout) * c.r)


def _slab_floats_written(c, room):
    """What vit_gemm_splitk's contract (include/vit_hip.h) says the two factor GEMMs put into the slabs: dB [in, r]
    over out, then dA [r, out] over in, each split in two when R >= 256, M * N % 4 == 0 and two slabs fit."""
    n = 0
    for mn, R in ((c.fin * c.r, c.fout), (c.r * c.fout, c.fin)):
        if R // 128 >= 2 and mn % 4 == 0 and 2 * mn <= room:
            n = max(n, 2 * mn)
    return n


@pytest.mark.parametrize("kind", ["base", "index"])
@pytest.mark.parametrize("fin, fout, r", DC.SPLIT_SHAPES, ids=[f"{i}x{o}r{r}" for i, o, r in DC.SPLIT_SHAPES])
def test_split_k_settings(fin, fout, r, kind):
    c = DC.case(fin, fout, r, kind)
    assert _rooms(c)[1] < _rooms(c)[2]
    plain = run(c, 0, "plain")[0]
    by_room = {}
    for room in _rooms(c):
        what = f"{fin}x{fout} r{r} {kind} room {room}"
        got, slabs = run(c, room)
        again, _ = run(c, room)
        assert _same_bits(got, again), f"{what}: two runs differ"
        _hold_stages(c, got, what)
        written = int((~torch.isnan(slabs.v)).sum())
        assert written == _slab_floats_written(c, room), f"{what}: {written} slab floats written"
        by_room[room] = got
    assert _same_bits(by_room[0], plain), "room 0 is not vit_dora_weight_bwd"
    assert _same_bits(run(c, _rooms(c)[2], null_slabs=True)[0], plain), "null slabs are not vit_dora_weight_bwd"
    # the split is taken where the contract says: dB at both shapes, dA only where r * out % 4 == 0
    assert _slab_floats_written(c, _rooms(c)[1]) == 2 * fin * r
    assert _slab_floats_written(c, _rooms(c)[2]) == (2 * fout * r if (r * fout) % 4 == 0 else 2 * fin * r)
    if kind == "index":      # exact data does not see the summation order
        assert all(_same_bits(g, plain) for g in by_room.values())


def test_forward_without_nu_gives_the_same_weight():
    c = DC.case(63, 65, 8, "base")
    ins, outs, slabs = _buffers(c, 0)
    p = lambda b: b.ptr
    L.call("vit_dora_weight_fwd", c.fin, c.fout, c.r, p(ins["m"]), p(ins["A"]), p(ins["B"]), p(ins["D"]), c.s, None,
           p(outs["W"]), None, p(outs["DnT"]), p(outs["colsq"]), L.stream_ptr(DEV))
    torch.cuda.synchronize()
    for b in outs.values():
        b.outside_untouched("forward without nu")
    assert bool(torch.isnan(outs["nu"].v).all())
    want = stored(63, 65, 8, "base")
    assert torch.equal(_bits(outs["W"].v), _bits(want["W"].reshape(-1)))
    assert torch.equal(_bits(outs["DnT"].v), _bits(want["DnT"].reshape(-1)))


def test_capture_and_replay_give_the_eager_bits():
    """Forward plus backward record into a graph on one stream (no allocation, no synchronisation), and its replay
    writes the bits of the eager calls into re-poisoned buffers."""
    fin, fout, r = 130, 257, 33
    c = DC.case(fin, fout, r, "masked")
    ins, outs, slabs = _buffers(c, ROOM)

    def both():
        _launch(c, ins, outs, slabs, ROOM, "ws", L.stream_ptr(DEV))

    both()
    eager = _settle(c, ins, outs, slabs, "eager")
    assert _same_bits(eager, run(c)[0])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        both()
    for b in list(outs.values()) + [slabs]:
        b.v.fill_(NAN)
    graph.replay()
    replayed = _settle(c, ins, outs, slabs, "replay")
    assert _same_bits(eager, replayed)
    _hold_stages(c, replayed, f"{fin}x{fout} r{r} masked, replayed")


# ---------------------------------------------------------------------------- through vit_amd.dora_weight

def _through(c, m, A, Bm, D, noise, gW):
    import vit_amd
    W = vit_amd.dora_weight(m, A, Bm, D, c.s, noise)
    W.backward(gW)
    return dict(W=W.detach(), dm=m.grad, dA=A.grad, dB=Bm.grad)


def _leaves(c):
    return [t.to(DEV).requires_grad_(True) for t in (c.m, c.A, c.B)]


@pytest.mark.parametrize("fin, fout, r", [(96, 80, 8), (65, 63, 1)])
def test_views_give_the_contiguous_bits(fin, fout, r):
    c = DC.case(fin, fout, r, "masked")
    m, A, Bm = _leaves(c)
    plain = _through(c, m, A, Bm, c.D.to(DEV), c.noise.to(DEV), c.gW.to(DEV))
    raw = stored(fin, fout, r, "masked")
    assert all(torch.equal(_bits(plain[k]), _bits(raw[k])) for k in plain)     # the module path is the raw call
    long = torch.zeros(2 * fout + 3, device=DEV)
    long[3::2] = c.m.to(DEV)
    mv = long[3::2].requires_grad_(True)                          # every second element, 12 bytes in
    flat = torch.zeros(r * fout + 1, device=DEV)
    flat[1:] = c.A.flatten().to(DEV)
    Av = flat[1:].view(r, fout).requires_grad_(True)              # contiguous but 4 bytes off 16-byte alignment
    Bv = c.B.t().contiguous().to(DEV).t().requires_grad_(True)    # a transposed view
    Dv = c.D.t().contiguous().to(DEV).t()
    wide = torch.zeros(fin, fout + 5, device=DEV)
    wide[:, 2:2 + fout] = c.noise.to(DEV)
    nzv = wide[:, 2:2 + fout]                                     # a column slice of a wider tensor
    wide2 = torch.zeros(fout, fin + 7, device=DEV)
    wide2[:, 3:3 + fin] = c.gW.to(DEV)
    gWv = wide2[:, 3:3 + fin]
    assert not any(t.is_contiguous() for t in (mv, Dv, nzv, gWv)) and (r == 1 or not Bv.is_contiguous())
    assert Av.data_ptr() % 16 == 4
    viewed = _through(c, mv, Av, Bv, Dv, nzv, gWv)
    assert _same_bits(plain, viewed)


def test_adapters_of_one_graph_share_the_workspace():
    """Three adapters of different shapes in one autograd graph use the one ``dora_sdDnT`` workspace in turn, the
    smallest first, so that it grows between their backward calls: each gives the gradients it gives alone."""
    from vit_amd import ops
    cs = [DC.case(3, 5, 2, "base"), DC.case(96, 80, 8, "masked"), DC.case(130, 257, 33, "base")]
    dev = lambda t: None if t is None else t.to(DEV)
    alone = [_through(c, *_leaves(c), dev(c.D), dev(c.noise), dev(c.gW)) for c in cs]
    for order in ((2, 1, 0), (0, 1, 2)):       # autograd runs the last-built node first: (2, 1, 0) is smallest first
        for key in [k for k in ops._WS if k[0] == "dora_sdDnT"]:
            del ops._WS[key]
        import vit_amd
        leaves = {i: _leaves(cs[i]) for i in order}
        Ws = {i: vit_amd.dora_weight(*leaves[i], dev(cs[i].D), cs[i].s, dev(cs[i].noise)) for i in order}
        loss = sum((Ws[i] * dev(cs[i].gW)).sum() for i in order)
        loss.backward()
        torch.cuda.synchronize()
        for i in order:
            got = dict(W=Ws[i].detach(), dm=leaves[i][0].grad, dA=leaves[i][1].grad, dB=leaves[i][2].grad)
            assert _same_bits(alone[i], got), f"order {order}: adapter {i} differs from its run alone"


# ---------------------------------------------------------------------------- refusals

def test_refused_calls_return_invalid_value_and_launch_nothing():
    c = DC.case(3, 5, 2, "base")
    ins, outs, slabs = _buffers(c, 64)
    lib, st = L.lib(), L.stream_ptr(DEV)
    for b in list(outs.values()) + [slabs]:
        b.v.fill_(SENT)
    p = lambda b: b.ptr
    fwd_ops = [p(ins["m"]), p(ins["A"]), p(ins["B"]), p(ins["D"])]
    fwd_outs = [p(outs["W"]), p(outs["nu"]), p(outs["DnT"]), p(outs["colsq"])]
    bwd_ops = [p(ins["m"]), p(ins["A"]), p(ins["B"]), p(ins["gW"]), p(outs["DnT"])]
    bwd_outs = [p(outs["nu"]), p(outs["dm"]), p(outs["dA"]), p(outs["dB"]), p(outs["sdDnT"])]

    def fwd(fin, fout, r, ops=fwd_ops, res=fwd_outs, nz=None):
        return lib.vit_dora_weight_fwd(fin, fout, r, *ops, c.s, nz, *res, st)

    def bwd(fin, fout, r, ops=bwd_ops, res=bwd_outs):
        return (lib.vit_dora_weight_bwd_ws(fin, fout, r, *ops, c.s, *res, p(slabs), 64, None, st),
                lib.vit_dora_weight_bwd_ws(fin, fout, r, *ops, c.s, *res, None, 0, None, st),
                lib.vit_dora_weight_bwd(fin, fout, r, *ops, c.s, *res, None, st))

    for fin, fout, r in ((0, 5, 2), (-3, 5, 2), (3, 0, 2), (3, -1, 2), (3, 5, 0), (3, 5, -1), (3, 5, 65)):
        assert fwd(fin, fout, r) == INVALID, (fin, fout, r)
        assert bwd(fin, fout, r) == (INVALID,) * 3, (fin, fout, r)
    for k in range(4):       # a null m, A, B, D
        assert fwd(3, 5, 2, ops=[None if j == k else v for j, v in enumerate(fwd_ops)]) == INVALID, k
    for k in (0, 2, 3):      # a null W, DnT_ws, colsq_ws (nu may be null)
        assert fwd(3, 5, 2, res=[None if j == k else v for j, v in enumerate(fwd_outs)]) == INVALID, k
    for k in range(5):       # a null m, A, B, gW, DnT
        assert bwd(3, 5, 2, ops=[None if j == k else v for j, v in enumerate(bwd_ops)]) == (INVALID,) * 3, k
    for k in range(5):       # a null nu, dm, dA, dB, sdDnT_ws
        assert bwd(3, 5, 2, res=[None if j == k else v for j, v in enumerate(bwd_outs)]) == (INVALID,) * 3, k
    torch.cuda.synchronize()
    for k, b in outs.items():
        b.all_untouched(k)
    slabs.all_untouched("slabs")
    for k, b in ins.items():
        b.unchanged(k)
    # the same buffers, accepted: the refusals left nothing behind
    for b in outs.values():
        b.v.fill_(NAN)
    _launch(c, ins, outs, slabs, 64, "ws")
    got = _settle(c, ins, outs, slabs, "after the refusals")
    assert _same_bits(got, stored(3, 5, 2, "base"))


def test_dora_weight_refuses_before_it_launches():
    import vit_amd
    z = lambda *s: torch.zeros(*s, device=DEV)
    fin, fout, r = 6, 8, 2
    with pytest.raises(ValueError):
        vit_amd.dora_weight(z(fout), z(r, fin), z(fin, r), z(fin, fout), 2.0)          # A [r, in]: read out of bounds
    with pytest.raises(ValueError):
        vit_amd.dora_weight(z(fout), z(65, fout), z(fin, 65), z(fin, fout), 2.0)
    with pytest.raises(ValueError):
        vit_amd.dora_weight(z(fout), z(r, fout), z(fin, r), z(fin, fout), 2.0, z(fout, fin))
    m = torch.ones(fout, device=DEV, requires_grad=True)
    D = torch.eye(fin, fout, device=DEV) + 0.5
    W = vit_amd.dora_weight(m, z(r, fout).requires_grad_(True), z(fin, r).requires_grad_(True), D, 2.0)
    with pytest.raises(ValueError):
        vit_amd.dora._DoraWeightFn.backward(W.grad_fn, z(fin, fout))                    # gW [in, out]
    W.backward(torch.ones(fout, fin, device=DEV))
    assert bool(torch.isfinite(m.grad).all())


def test_worst_fractions_of_this_run():
    """Prints the worst err / bound per stage over the tests of this file that ran before it (``-s`` shows it)."""
    print("worst err / bound per stage on the GPU:")
    for k in list(DC.STAGES) + ["e2e " + n for n in DC.E2E]:
        if k in WORST:
            print(f"  {k:10s} {WORST[k][0]:.3f}  {WORST[k][1]}")
    assert all(v[0] <= 1.0 for v in WORST.values())
