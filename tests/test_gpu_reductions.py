"""GPU: the column-reduction kernels (colsum_partial, splitk_reduce, colreduce one- and two-stage, the batched
colreduce with its short, tall and ticketed paths) held to equality on every dispatch branch, with the cases of
oracle/reduce_cases.py.

No tolerance anywhere.  Measure (a), ``ints``: the result is the float64 column sum bit for bit (integer partials,
exact in any order).  Measure (b), ``normals``: the result is bit for bit the torch-float32 restatement of the
order the kernel source states.  Partials sit in NaN-filled buffers with NaN rows behind row S - 1, scratch and
partial workspaces are NaN before every call, outputs are views inside sentinel buffers: a row past S, a scratch
word read before it is written or a store outside the N floats shows.  tests/test_reduce_cases_host.py holds the
restatements and the shape lists themselves.
"""
import ctypes
from dataclasses import replace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import reduce_cases as RD  # noqa: E402
from vit_amd import _lib as L  # noqa: E402
from vit_amd import ops  # noqa: E402
from vit_amd._lib import call  # noqa: E402

DEV = "cuda"
F32, BF = torch.float32, torch.bfloat16
SENT = 640.0     # exact in f32 and bf16
NAN = float("nan")
PRE = 4          # floats in front of every view (16 bytes: the view keeps the buffer's alignment)
PAD = 5          # elements behind the last row
GUARD_ROWS = 3   # NaN rows behind row S - 1 of every partial matrix
INVALID = 1      # hipErrorInvalidValue
KINDS = ("ints", "normals")


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    L.load()


class Buf:
    """A [rows, cols] view with row stride ``ld`` that starts PRE + ``off`` elements into a buffer filled with
    ``fill`` (the sentinel, or NaN for partials and scratch)."""

    def __init__(self, rows, cols, ld=None, off=0, dtype=F32, src=None, fill=SENT, extra=0):
        self.rows, self.cols, self.ld, self.off = rows, cols, cols if ld is None else ld, PRE + off
        assert self.ld >= cols
        self.buf = torch.full((self.off + rows * self.ld + extra + PAD,), fill, dtype=dtype, device=DEV)
        self.v = self.buf[self.off:self.off + rows * self.ld].view(rows, self.ld)[:, :cols]
        if src is not None:
            self.v.copy_(src.reshape(rows, cols))
        self.before = None

    @property
    def ptr(self):
        return self.v.data_ptr()

    @property
    def flat(self):
        assert self.rows == 1 or self.ld == self.cols
        return self.buf[self.off:self.off + self.rows * self.cols]

    def set(self, src):
        self.v.copy_(src.reshape(self.rows, self.cols))

    def freeze(self):
        self.before = self.buf.clone()
        return self

    def unchanged(self, what):
        assert torch.equal(_bits(self.buf), _bits(self.before)), f"{what}: an input changed"

    def outside_untouched(self, what):
        m = torch.ones(self.buf.numel(), dtype=torch.bool, device=DEV)
        m[self.off:self.off + self.rows * self.ld].view(self.rows, self.ld)[:, :self.cols] = False
        assert bool((self.buf[m] == SENT).all()), f"{what}: wrote outside its [{self.rows}, {self.cols}] view"

    def is_sentinel(self):
        return bool((self.buf == SENT).all())


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def _same_bits(got, want, what=""):
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if not torch.equal(_bits(got), _bits(want)):
        bad = (_bits(got) != _bits(want)).reshape(-1).nonzero().reshape(-1)
        j = int(bad[0])
        raise AssertionError(f"{what}: not bitwise equal in {bad.numel()} of {got.numel()} columns; column {j}: "
                             f"got {got.reshape(-1)[j].item()!r}, want {want.reshape(-1)[j].item()!r}")


def _stream():
    return L.stream_ptr(DEV)


def _parts(c, off=0, nq=1):
    """The partials of nq stacked cases in one NaN buffer, GUARD_ROWS NaN rows behind the last row."""
    S, N = c[0].S, c[0].N
    b = Buf(nq * S, N, off=off, src=torch.cat([x.part for x in c]), fill=NAN, extra=GUARD_ROWS * N)
    return b.freeze()


def _nan_vec(n):
    """n NaN floats on 16 bytes with PAD more behind them."""
    return torch.full((n + PAD,), NAN, device=DEV)


def _want(kind, c, total, acc):
    """The bits the kernel must produce: the float64 sum (a) or the restated f32 sum (b), plus ``out`` if asked."""
    if kind == "ints":
        return (c.ref + (c.out0.double() if acc else 0)).float()
    return RD.finish(total, c.out0, acc)


# ---------------------------------------------------------------------------- vit_colreduce_batch

class _Batch:
    """One job list on the GPU: partials, outputs, the int64 job table and the restated plan."""

    def __init__(self, jobs, kind, seed0=0):
        self.jobs, self.kind, self.seed0 = jobs, kind, seed0
        self.plans, self.launches, self.sf, self.nc = RD.batch_plan(jobs)
        self.cases = [RD.case(kind, j.S, j.N, F32, seed0 + i) for i, j in enumerate(jobs)]
        self.parts = [_parts([c], j.part_off) for j, c in zip(jobs, self.cases)]
        self.outs = [Buf(1, j.N, off=j.out_off, src=c.out0) for j, c in zip(jobs, self.cases)]
        for j, p, o in zip(jobs, self.parts, self.outs):
            assert (p.ptr % 16 == 0) == (j.part_off % 4 == 0) and (o.ptr % 16 == 0) == (j.out_off % 4 == 0)
        self.table = np.array([(p.ptr, o.ptr, j.S, j.N, j.accumulate)
                               for j, p, o in zip(jobs, self.parts, self.outs)], dtype=np.int64).reshape(-1)

    @property
    def jp(self):
        return self.table.ctypes.data_as(ctypes.c_void_p)

    def sizes(self):
        sf, nc = ctypes.c_int64(-1), ctypes.c_int(-1)
        assert L.lib().vit_colreduce_batch_sizes(self.jp, len(self.jobs), ctypes.byref(sf), ctypes.byref(nc)) == 0
        return sf.value, nc.value

    def reset(self):
        for o, c in zip(self.outs, self.cases):
            o.set(c.out0)

    def want(self, i):
        j, p, c = self.jobs[i], self.plans[i], self.cases[i]
        total = None if self.kind == "ints" else RD.batch_case_sum(self.kind, j.S, j.N, p.path, self.seed0 + i)
        return _want(self.kind, c, total, j.accumulate)

    def check(self, what, quiet=False):
        torch.cuda.synchronize()
        for i, (j, p) in enumerate(zip(self.jobs, self.plans)):
            w = f"{what} job {i} S {j.S} N {j.N} acc {j.accumulate} part+{j.part_off} out+{j.out_off}: {p.path}"
            if not quiet:
                print(f"{w} strips {p.strips} chunks {p.chunks} launch {p.launch} wg0 {p.wg0} cnt0 {p.cnt0} scr0 {p.scr0}")
            _same_bits(self.outs[i].flat, self.want(i), w)
            self.outs[i].outside_untouched(w)
            self.parts[i].unchanged(w)
        return [o.flat.clone() for o in self.outs]


def _flip(jobs, flip):
    return [replace(j, accumulate=j.accumulate ^ flip) for j in jobs]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(RD.CB_MIXES))
def test_batch_every_path_bit_for_bit(name, kind):
    """Every job of every mix, accumulate as listed and flipped, through the C ABI with exactly the scratch and the
    counters vit_colreduce_batch_sizes asks for, NaN in the scratch before each call: the restated bits, twice the
    same, nothing written outside the outputs or behind the scratch, the counters left zero."""
    for flip in (0, 1):
        b = _Batch(_flip(RD.CB_MIXES[name], flip), kind)
        assert b.sizes() == (b.sf, b.nc), "the library's sizes are not the restated plan's"
        cnt = torch.zeros(b.nc + PAD, dtype=torch.int32, device=DEV)
        cnt[b.nc:] = 7
        runs = []
        for rep in range(2):
            scratch = _nan_vec(b.sf)
            assert scratch.data_ptr() % 16 == 0
            b.reset()
            call("vit_colreduce_batch", b.jp, len(b.jobs), scratch.data_ptr(), b.sf, cnt.data_ptr(), b.nc, _stream())
            runs.append(b.check(f"batch {name} {kind} flip {flip}", quiet=rep > 0))
            assert bool(torch.isnan(scratch[b.sf:]).all()), "wrote behind the scratch it asked for"
            assert bool((cnt[:b.nc] == 0).all()), "a ticket counter was left non-zero"
            assert bool((cnt[b.nc:] == 7).all()), "touched a counter past those it asked for"
        for i, (r0, r1) in enumerate(zip(*runs)):
            _same_bits(r0, r1, f"batch {name} job {i}: second run")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", RD.CB_OPS_MIXES)
def test_colbatch_launch_over_a_stale_workspace(name, kind):
    """ops.ColBatch with the shared "colbatch" workspace full of NaN bytes: the kernel writes its scratch before it
    reads it, and leaves the counters zero."""
    b = _Batch(RD.CB_MIXES[name], kind)
    runs = []
    for rep in range(2):
        ops.workspace("colbatch", max(16, b.sf * 4), DEV).fill_(255)
        b.reset()
        cb = ops.ColBatch()
        for j, p, o in zip(b.jobs, b.parts, b.outs):
            cb.add(p.v, j.S, j.N, o.flat, accumulate=bool(j.accumulate))
        assert [tuple(int(x) for x in b.table[5 * i:5 * i + 5]) for i in range(len(b.jobs))] == cb.jobs
        cb.launch()
        runs.append(b.check(f"ColBatch {name} {kind}", quiet=rep > 0))
        assert int(ops._counters("colbatch", 1, DEV).abs().sum()) == 0, "a ticket counter was left non-zero"
    for i, (r0, r1) in enumerate(zip(*runs)):
        _same_bits(r0, r1, f"ColBatch {name} job {i}: second run")


def test_colbatch_graph_replay():
    """One captured ColBatch launch of a ticketed mix, replayed three times over different partials: the restated
    bits each time, the counters zero after each."""
    jobs = RD.CB_MIXES[RD.CB_GRAPH_MIX]

    def launch(b):
        cb = ops.ColBatch()
        for j, p, o in zip(b.jobs, b.parts, b.outs):
            cb.add(p.v, j.S, j.N, o.flat, accumulate=bool(j.accumulate))
        cb.launch()

    b = _Batch(jobs, "normals")
    launch(b)                       # eager: the workspace and the counters exist before the capture
    b.check("graph warm-up", quiet=True)
    b.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch(b)
    cnt = ops._counters("colbatch", 1, DEV)
    for r in range(3):
        fresh = [RD.case("normals", j.S, j.N, F32, 1000 * (r + 1) + i) for i, j in enumerate(jobs)]
        for p, o, c in zip(b.parts, b.outs, fresh):
            p.set(c.part)
            p.freeze()
            o.set(c.out0)
        graph.replay()
        torch.cuda.synchronize()
        for i, (j, p, c) in enumerate(zip(jobs, b.plans, fresh)):
            w = f"replay {r} job {i} S {j.S} N {j.N} acc {j.accumulate}: {p.path}"
            _same_bits(b.outs[i].flat, RD.finish(RD.batch_sum(j, p, c.part), c.out0, j.accumulate), w)
            b.outs[i].outside_untouched(w)
            b.parts[i].unchanged(w)
        print(f"replay {r}: {len(jobs)} jobs, {len(b.launches)} launches, counters {int(cnt.abs().sum())}")
        assert int(cnt.abs().sum()) == 0, f"replay {r}: a ticket counter was left non-zero"


def test_batch_refuses_too_little_scratch_or_too_few_counters():
    b = _Batch(RD.CB_MIXES["fix"], "ints")
    for o in b.outs:
        o.buf.fill_(SENT)
    scratch = _nan_vec(b.sf)
    cnt = torch.zeros(b.nc + PAD, dtype=torch.int32, device=DEV)
    lib, n = L.lib(), len(b.jobs)
    assert b.sf > 0 and b.nc > 0
    assert lib.vit_colreduce_batch(b.jp, n, scratch.data_ptr(), b.sf - 1, cnt.data_ptr(), b.nc, _stream()) == INVALID
    assert lib.vit_colreduce_batch(b.jp, n, scratch.data_ptr(), b.sf, cnt.data_ptr(), b.nc - 1, _stream()) == INVALID
    assert lib.vit_colreduce_batch(b.jp, n, None, b.sf, cnt.data_ptr(), b.nc, _stream()) == INVALID
    assert lib.vit_colreduce_batch(b.jp, n, scratch.data_ptr(), b.sf, None, b.nc, _stream()) == INVALID
    assert lib.vit_colreduce_batch(b.jp, n, scratch.data_ptr() + 4, b.sf, cnt.data_ptr(), b.nc, _stream()) == INVALID
    torch.cuda.synchronize()
    assert all(o.is_sentinel() for o in b.outs), "a refused call wrote an output"
    assert bool(torch.isnan(scratch).all()) and int(cnt.abs().sum()) == 0


# ---------------------------------------------------------------------------- vit_colreduce, vit_colreduce_multi

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("scratch", [False, True], ids=["one-stage", "scratch"])
@pytest.mark.parametrize("nq", RD.CR_NQ)
def test_colreduce_multi_bit_for_bit(nq, scratch, kind):
    """nq stacked matrices (the rows behind matrix q are matrix q + 1's, behind the last NaN) into separate
    sentinel buffers; an output past nq keeps its sentinel; nq = 1 through vit_colreduce as well."""
    for S in RD.CR_S:
        for N in RD.CR_N:
            cs = [RD.case(kind, S, N, F32, q) for q in range(nq)]
            part = _parts(cs, nq=nq)
            sfl = nq * RD.colreduce_scratch_floats(S, N)
            two = RD.colreduce_two_stage(S, scratch)
            print(f"colreduce nq {nq} S {S} N {N} {kind}: {'two stages' if two else 'one stage'}, scratch {sfl if scratch else None}")
            for acc in (0, 1):
                for entry in ("vit_colreduce_multi",) + (("vit_colreduce",) if nq == 1 else ()):
                    outs = [Buf(1, N, src=cs[q].out0 if q < nq else None) for q in range(3)]
                    sc = _nan_vec(sfl) if scratch else None
                    scp = sc.data_ptr() if scratch else None
                    if entry == "vit_colreduce":
                        call(entry, part.ptr, S, N, outs[0].ptr, acc, scp, _stream())
                    else:
                        call(entry, part.ptr, nq, S, N, outs[0].ptr, outs[1].ptr, outs[2].ptr, acc, scp, _stream())
                    torch.cuda.synchronize()
                    w = f"{entry} nq {nq} S {S} N {N} acc {acc} scratch {scratch} {kind}"
                    for q in range(nq):
                        total = None if kind == "ints" else RD.colreduce_case_sum(kind, S, N, scratch, q)
                        _same_bits(outs[q].flat, _want(kind, cs[q], total, acc), f"{w} out{q}")
                        outs[q].outside_untouched(f"{w} out{q}")
                    assert all(outs[q].is_sentinel() for q in range(nq, 3)), f"{w}: wrote an unused output"
                    part.unchanged(w)
                    if scratch:
                        assert bool(torch.isnan(sc[sfl:]).all()), f"{w}: wrote behind its scratch"


def test_colreduce_multi_refuses_four_matrices():
    c = RD.ints(5, 8)
    part = _parts([c] * 4, nq=4)
    outs = [Buf(1, 8) for _ in range(3)]
    lib = L.lib()
    assert lib.vit_colreduce_multi(part.ptr, 4, 5, 8, outs[0].ptr, outs[1].ptr, outs[2].ptr, 0, None, _stream()) == INVALID
    assert lib.vit_colreduce_multi(part.ptr, -1, 5, 8, outs[0].ptr, outs[1].ptr, outs[2].ptr, 0, None, _stream()) == INVALID
    assert lib.vit_colreduce_multi(part.ptr, 0, 5, 8, outs[0].ptr, outs[1].ptr, outs[2].ptr, 0, None, _stream()) == 0
    torch.cuda.synchronize()
    assert all(o.is_sentinel() for o in outs)
    part.unchanged("refused colreduce_multi")


# ---------------------------------------------------------------------------- vit_colsum, ops.colsum

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M", RD.CS_M)
@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_colsum_bit_for_bit(dtype, M, kind):
    """x [M][N] with a row stride of N + 3 inside a sentinel buffer; a NaN partial buffer of exactly the floats
    passed, NaN behind it still after the call."""
    for N in RD.CS_N:
        c = RD.case(kind, M, N, dtype)
        x = Buf(M, N, ld=N + RD.CS_LD_PAD, dtype=dtype, src=c.part).freeze()
        seen = set()
        for sreq in RD.CS_SREQ:
            pf = RD.colsum_floats(M, N, sreq)
            plan = RD.colsum_plan(M, N, pf)
            if plan in seen:   # the same S, rows_per and stages as a size already run
                continue
            seen.add(plan)
            S, rows_per, two = plan
            print(f"colsum {kind} {dtype} M {M} N {N} partial_floats {pf} ({sreq}): S {S} rows_per {rows_per} "
                  f"{'two stages' if two else 'one stage'}")
            total = None if kind == "ints" else RD.colsum_case_sum(kind, M, N, dtype, S, rows_per, two)
            for acc in (0, 1):
                out, part = Buf(1, N, src=c.out0), _nan_vec(pf)
                call("vit_colsum", L.dt(c.part), M, N, x.ptr, x.ld, out.ptr, part.data_ptr(), pf, acc, _stream())
                torch.cuda.synchronize()
                w = f"colsum {kind} {dtype} M {M} N {N} pf {pf} acc {acc}"
                _same_bits(out.flat, _want(kind, c, total, acc), w)
                out.outside_untouched(w)
                x.unchanged(w)
                assert bool(torch.isnan(part[pf:]).all()), f"{w}: wrote behind its partial buffer"


@pytest.mark.parametrize("kind", KINDS)
def test_ops_colsum_over_a_stale_workspace(kind):
    """ops.colsum sizes its own partial buffer (restated in ops_colsum_floats); the workspace holds NaN bytes."""
    for dtype in (F32, BF):
        for M in (64, 300, 1000):
            for N in (255, 256):
                c = RD.case(kind, M, N, dtype)
                pf = RD.ops_colsum_floats(M, N)
                S, rows_per, two = RD.colsum_plan(M, N, pf)
                total = None if kind == "ints" else RD.colsum_case_sum(kind, M, N, dtype, S, rows_per, two)
                x = c.part.to(DEV)
                for acc in (0, 1):
                    ops.workspace("colsum", pf * 4, DEV).fill_(255)
                    out = Buf(1, N, src=c.out0)
                    ops.colsum(x, out=out.flat, accumulate=bool(acc))
                    torch.cuda.synchronize()
                    w = f"ops.colsum {kind} {dtype} M {M} N {N} acc {acc}: S {S} rows_per {rows_per}"
                    print(w)
                    _same_bits(out.flat, _want(kind, c, total, acc), w)
                    out.outside_untouched(w)


# ---------------------------------------------------------------------------- split-K slab sums

@pytest.mark.parametrize("M,N,K,split,dtype", RD.WGRAD_SLABS, ids=["bf16", "f32", "bf16-ragged"])
def test_wgrad_slab_sum_through_colbatch_is_the_immediate_path_bit_for_bit(M, N, K, split, dtype):
    """At most 8 slabs: the batch's short path adds the slabs in the order of splitk_reduce_kernel, so the weight
    gradient reduced by a ColBatch job equals vit_linear_wgrad's own reduction bit for bit (both fold a ragged
    M % 32 tail into the last slab first); for bf16 both are the restated slab sum of the slabs
    vit_linear_wgrad_partials writes."""
    g = torch.Generator().manual_seed(77)
    dy = torch.randn(M, N, generator=g).to(dtype).to(DEV)
    x = torch.randn(M, K, generator=g).to(dtype).to(DEV)
    imm = ops.linear_wgrad(dy, x, split=split)
    cb = ops.ColBatch()
    out = Buf(N, K)
    ops.workspace("colbatch", 16, DEV).fill_(255)
    ops.linear_wgrad(dy, x, out=out.v, split=split, reduce_on=cb)
    nz = L.lib().vit_linear_wgrad_nslabs(L.dt(dy), M, N, K, split)
    print(f"wgrad {dtype} M {M} N {N} K {K} split {split}: {nz} slabs, {len(cb.jobs)} batch job(s)")
    assert nz == split
    if dtype == BF:
        assert len(cb.jobs) == 1 and cb.jobs[0][2] == nz and RD.batch_plan([RD.Job(nz, N * K)])[0][0].path == "short"
    cb.launch()
    torch.cuda.synchronize()
    _same_bits(out.v, imm, "ColBatch slab sum vs the immediate reduction")
    out.outside_untouched("wgrad via ColBatch")
    ref = dy.double().T @ x.double()
    assert float((imm.double() - ref).abs().max()) <= 2e-5 * float(ref.abs().max())
    if dtype == BF:
        slabs = torch.full((nz * N * K + PAD,), NAN, device=DEV)
        call("vit_linear_wgrad_partials", L.dt(dy), M, N, K, dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0),
             split, slabs.data_ptr(), nz * N * K * 4, _stream())
        torch.cuda.synchronize()
        assert bool(torch.isnan(slabs[nz * N * K:]).all())
        sl = slabs[:nz * N * K].view(nz, N * K).cpu()
        _same_bits(imm.reshape(-1), RD.splitk_reduce(sl), "immediate reduction vs restated splitk_reduce")
        _same_bits(imm.reshape(-1), RD.colbatch_short(sl), "immediate reduction vs restated short path")
