"""CPU: the column-reduction cases of oracle/reduce_cases.py are what tests/test_gpu_reductions.py takes them for.

Every order restatement gives the float64 sum bit for bit on ``ints`` (so measure (a) can be held on every path)
and stays inside the textbook bound of S f32 adds on ``normals`` (so each is a sum of exactly the rows, once
each); every shape list reaches the branch its comment names, by the restated dispatch rules; and the library's
host-only vit_colreduce_batch_sizes agrees with the restated plan on every job list the GPU tests run.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import reduce_cases as RD

F32, BF = torch.float32, torch.bfloat16


def _bits(t):
    return t.contiguous().view(torch.int32)


def _restatements(S, N):
    """(name, function of the [S][N] partials) for every restatement that takes S rows."""
    r = [("colreduce one stage", lambda p: RD.colreduce(p, False)),
         ("colreduce with scratch", lambda p: RD.colreduce(p, True)),
         ("splitk_reduce", RD.splitk_reduce)]
    r.append(("colbatch short", RD.colbatch_short) if S <= RD.CB_SHORT else ("colbatch tall", RD.colbatch_tall))
    for rows_per in sorted({1, 3, 4, 7, max(1, S // 3), S}):
        r.append((f"colsum_partial rows_per {rows_per} + colreduce",
                  lambda p, rp=rows_per: RD.colreduce(RD.colsum_partial(p, rp), True)))
    return r


HOST_SN = [(1, 5), (2, 4), (7, 30), (8, 9), (9, 4), (17, 33), (63, 7), (64, 65), (65, 12), (129, 6), (300, 10),
           (577, 5), (1089, 3)]


@pytest.mark.parametrize("S,N", HOST_SN)
def test_every_restatement_is_exact_on_ints(S, N):
    c = RD.ints(S, N)
    assert bool((c.part != 0).all()) and float(c.part.abs().max()) <= 4
    for name, f in _restatements(S, N):
        got = f(c.part)
        assert got.dtype == F32 and torch.equal(got.double(), c.ref), name
        assert torch.equal(_bits(got), _bits(c.ref.float())), name
        assert torch.equal(RD.finish(got, c.out0, 1).double(), c.ref + c.out0.double()), name


@pytest.mark.parametrize("S,N", HOST_SN)
def test_every_restatement_is_within_the_textbook_bound_on_normals(S, N):
    c = RD.normals(S, N)
    assert bool((c.part.abs() >= 2.0 ** -10).all())
    bound = RD.textbook_bound(c.part)
    for name, f in _restatements(S, N):
        err = (f(c.part).double() - c.ref).abs()
        assert bool((err <= bound).all()), (name, float((err / bound).max()))


def test_bf16_ints_are_exact_and_the_orders_differ_on_normals():
    c = RD.ints(300, 17, BF)
    assert c.part.dtype == BF and torch.equal(c.part.double().sum(0), c.ref)
    s, part = RD.colsum(c.part, 5 * 17)
    assert torch.equal(s.double(), c.ref) and part.shape == (5, 17)
    # measure (b) can tell the orders apart: on normals the restatements do not all give the same bits
    n = RD.normals(577, 64)
    tall, two, one = RD.colbatch_tall(n.part), RD.colreduce(n.part, True), RD.colreduce(n.part, False)
    assert not torch.equal(tall, two) and not torch.equal(two, one) and not torch.equal(tall, one)
    # ... while at most 8 slabs the batch's short path is the slab reduce's order
    for nslab in range(1, 9):
        p = RD.normals(nslab, 64).part
        assert torch.equal(_bits(RD.colbatch_short(p)), _bits(RD.splitk_reduce(p)))
    p = RD.normals(9, 64).part
    assert not torch.equal(RD.colbatch_tall(p), RD.splitk_reduce(p))


# ---------------------------------------------------------------------------- the batch's shape lists
def _paths(jobs):
    return [p.path for p in RD.batch_plan(jobs)[0]]


def test_batch_shape_lists_reach_their_branches():
    J = RD.Job
    for S in RD.CB_SHORT_S:
        for N in RD.CB_SHORT_N:
            (p,), launches, sf, nc = RD.batch_plan([J(S, N)])
            assert p.path == "short" and p.chunks == 1 and sf == 0 and nc == 0 and launches == [p.strips]
    assert max(RD.CB_SHORT_S) == RD.CB_SHORT and min(RD.CB_TALL1_S) == RD.CB_SHORT + 1
    halves = {(min(N, 2048) > 1024, N > 2048) for N in RD.CB_SHORT_N}   # (second half used, second workgroup)
    assert halves == {(False, False), (True, False), (True, True)}
    assert {1024, 1028, 2044, 2048, 2052} <= set(RD.CB_SHORT_N)
    for S in RD.CB_TALL1_S:
        for N in RD.CB_TALL1_N:
            (p,), launches, sf, nc = RD.batch_plan([J(S, N)])
            assert p.path == "tall1" and p.chunks == 1 and sf == 0 and nc == 0
            assert p.strips == (1 if N <= 256 else 2)
    assert max(RD.CB_TALL1_S) == RD.CB_ROWS and min(RD.CB_TICKET_S) == RD.CB_ROWS + 1
    assert {252, 256, 260} <= set(RD.CB_TALL1_N)
    for S, chunks in zip(RD.CB_TICKET_S, RD.CB_TICKET_CHUNKS):
        for N in RD.CB_TICKET_N:
            (p,), launches, sf, nc = RD.batch_plan([J(S, N)])
            assert p.path == "ticket" and p.chunks == chunks and nc == p.strips == -(-N // 256)
            assert sf == chunks * N and launches == [chunks * p.strips]
    # the combine loop: q = 1, batches of eight while q + 8 <= chunks, then one by one
    shapes = {((c - 1) // 8, (c - 1) % 8) for c in RD.CB_TICKET_CHUNKS}
    assert {(0, 1), (0, 2), (0, 7), (1, 0), (1, 1), (2, 1)} == shapes
    assert _paths([J(S, N) for S, N in RD.CB_FALLBACK_SN]) == ["fallback1", "fallback1", "fallback2", "fallback2"]
    assert all(N % 4 for _, N in RD.CB_FALLBACK_SN)
    off = [J(S, N, part_off=1) for S, N in RD.CB_FALLBACK_OFF_SN]
    assert all(N % 4 == 0 for _, N in RD.CB_FALLBACK_OFF_SN) and set(_paths(off)) == {"fallback1", "fallback2"}
    assert _paths([J(S, N) for S, N in RD.CB_FALLBACK_OFF_SN]) == ["short", "tall1", "ticket"]
    assert _paths([J(S, N, out_off=1) for S, N in RD.CB_OUT_OFF_SN]) == ["short", "ticket"]
    assert all(N % 4 == 0 for _, N in RD.CB_OUT_OFF_SN)


def test_batch_mixes_reach_their_branches():
    M = RD.CB_MIXES
    for name, jobs in M.items():
        plans, launches, sf, nc = RD.batch_plan(jobs)
        by_path = {}
        for j, p in zip(jobs, plans):
            by_path.setdefault(p.path, set()).add(j.accumulate)
            assert p.scr0 % RD.SCR_ALIGN == 0 and p.scratch_floats % RD.SCR_ALIGN == 0, (name, j)
            assert max(j.S, 1) * j.N <= 1089 * 772
        assert all(a == {0, 1} for a in by_path.values()), (name, by_path)   # accumulate 0 and 1 on every path
    assert set(_paths(M["short"])) == {"short"} and len(RD.batch_plan(M["short"])[1]) == 2
    assert set(_paths(M["tall1"])) == {"tall1"}
    assert set(_paths(M["ticket"])) == {"ticket"} and len(RD.batch_plan(M["ticket"])[1]) == 2
    assert set(_paths(M["fallback"])) == {"fallback1", "fallback2"}
    assert all(j.out_off == 1 for j in M["out_off"]) and set(_paths(M["out_off"])) == {"short", "ticket"}
    for name, n in (("batch16", 16), ("batch17", 17), ("batch33", 33)):
        jobs = M[name]
        plans, launches, sf, nc = RD.batch_plan(jobs)
        vec = [p for p in plans if p.launch >= 0]
        assert len(vec) == n and len(launches) == (n + 15) // 16
        for k in range(1, len(launches)):       # ticketed jobs on both sides of every flush
            before, after = vec[16 * k - 1], vec[16 * k]
            assert before.path == "ticket" and after.path == "ticket" and before.launch == k - 1 and after.launch == k
            assert after.wg0 == 0                                           # the workgroup base starts again
            assert after.cnt0 == before.cnt0 + before.counters > 0          # the offsets carry over
            assert after.scr0 == before.scr0 + before.scratch_floats > 0
        if n == 16:
            assert vec[-1].path == "ticket"
    assert any(p.path == "fallback2" for p in RD.batch_plan(M["batch33"])[0])
    # the mix of the scratch-slice rounding: without it the ticketed slices would start at 90 and 393 floats
    plans = RD.batch_plan(M["fix"])[0]
    assert [p.path for p in plans[:3]] == ["fallback2", "fallback2", "ticket"]
    assert RD.colreduce_scratch_floats(130, 30) == 90 and RD.colreduce_scratch_floats(130, 101) == 303
    assert (plans[0].scr0, plans[1].scr0, plans[2].scr0) == (0, 92, 396)
    later = [p for p in plans[3:] if p.path == "ticket"]
    assert len(later) >= 2 and any(p.path == "fallback2" for p in plans[3:])
    for name in RD.CB_OPS_MIXES + (RD.CB_GRAPH_MIX,):
        assert "ticket" in _paths(M[name])
    assert all(j.part_off == 0 and j.out_off == 0 for j in M[RD.CB_GRAPH_MIX])


def _lib_sizes(jobs):
    """vit_colreduce_batch_sizes (host only) on jobs whose pointers carry nothing but their alignment."""
    from vit_amd import _lib
    rows = [(4096 + 4 * j.part_off, 8192 + 4 * j.out_off, j.S, j.N, j.accumulate) for j in jobs]
    arr = np.array(rows, dtype=np.int64).reshape(-1)
    sf, nc = ctypes.c_int64(-1), ctypes.c_int(-1)
    rc = _lib.load().vit_colreduce_batch_sizes(arr.ctypes.data_as(ctypes.c_void_p), len(jobs), ctypes.byref(sf),
                                               ctypes.byref(nc))
    assert rc == 0
    return sf.value, nc.value


@pytest.mark.parametrize("name", list(RD.CB_MIXES))
def test_library_batch_sizes_are_the_restated_plan(name):
    jobs = RD.CB_MIXES[name]
    plans, launches, sf, nc = RD.batch_plan(jobs)
    assert _lib_sizes(jobs) == (sf, nc)
    assert sf % RD.SCR_ALIGN == 0 and sf == sum(p.scratch_floats for p in plans)
    assert nc == sum(p.counters for p in plans)
    for k in range(1, len(jobs) + 1):   # every prefix: the running offset of job k is the size of jobs [0, k)
        want = (plans[k].scr0, plans[k].cnt0) if k < len(jobs) else (sf, nc)
        assert _lib_sizes(jobs[:k]) == want, (name, k)


def test_library_batch_sizes_round_every_slice():
    J = RD.Job
    assert _lib_sizes([J(130, 30)]) == (92, 0)
    assert _lib_sizes([J(130, 30), J(130, 101)]) == (396, 0)
    assert _lib_sizes([J(130, 30), J(130, 260)]) == (92 + 3 * 260, 2)
    assert _lib_sizes([J(65, 256, part_off=1)]) == (512, 0)       # N % 4 == 0, misaligned: fallback, 2 * 256
    assert _lib_sizes([J(7, 30), J(64, 30), J(8, 2052), J(64, 260)]) == (0, 0)


# ---------------------------------------------------------------------------- colreduce and colsum lists
def test_colreduce_shape_list_reaches_its_branches():
    def slice_shape(z0, z1, sl):   # (four-wide steps, tail steps) of slice sl
        z, four, tail = z0 + sl, 0, 0
        while z + 48 < z1:
            four, z = four + 1, z + 64
        while z < z1:
            tail, z = tail + 1, z + 16
        return four, tail
    seen = {S: {slice_shape(0, S, sl) for sl in range(16)} for S in RD.CR_S}
    assert seen[1] == {(0, 1), (0, 0)} and seen[15] == {(0, 1), (0, 0)} and seen[16] == {(0, 1)}
    assert seen[17] == {(0, 2), (0, 1)} and seen[63] == {(0, 3), (1, 0)} and seen[64] == {(1, 0)}
    assert seen[65] == {(1, 1), (1, 0)} and (2, 0) in seen[128] and (2, 1) in seen[129]
    assert seen[300] == {(4, 3), (4, 2)}
    two = [S for S in RD.CR_S if RD.colreduce_two_stage(S, True)]
    assert two == [65, 128, 129, 300] and not any(RD.colreduce_two_stage(S, False) for S in RD.CR_S)
    assert {-(-S // 64) for S in two} == {2, 3, 5}
    assert {(-(-N // 64), N % 64) for N in RD.CR_N} == {(1, 1), (1, 63), (1, 0), (2, 1), (3, 8)}
    assert RD.CR_NQ == (1, 2, 3)


def test_colsum_shape_list_reaches_its_branches():
    plans = {}
    for M in RD.CS_M:
        for N in RD.CS_N:
            for sreq in RD.CS_SREQ:
                pf = RD.colsum_floats(M, N, sreq)
                plan = RD.colsum_plan(M, N, pf)
                assert plan is not None
                S, rows_per, two = plan
                assert 1 <= S <= min(M, 256) and (S - 1) * rows_per < M <= S * rows_per
                assert pf >= S * N + (RD.colreduce_scratch_floats(S, N) if two else 0)   # what the call may touch
                plans[M, N, sreq] = plan
    N = 257
    assert all(plans[M, N, 1][0] == 1 for M in RD.CS_M)                                   # S = 1
    assert plans[1000, N, 5] == (5, 200, False) and plans[300, N, 5] == (5, 60, False)
    assert plans[1000, N, 300] == (250, 4, True)                                          # 300 -> 256 -> 250 rows of 4
    assert plans[5, N, 5] == (5, 1, False) and plans[3, N, 5] == (3, 1, False)            # S capped by M
    assert plans[300, N, 300] == (150, 2, True)                                           # capped at 256, then 150 x 2
    assert plans[300, N, 100] == (100, 3, False) and plans[300, N, 102] == (100, 3, True)  # second stage: room or not
    assert plans[1000, N, 100] == (100, 10, False) and plans[1000, N, 102] == (100, 10, True)
    assert plans[1000, N, 5000] == (250, 4, True)                                         # far too large: capped at 256
    # ops.colsum asks for 15 rows and a group row: vit_colsum makes 16 partial rows of the 16 * N floats, ragged
    assert RD.ops_colsum_floats(1000, N) == 16 * N and plans[1000, N, "ops"] == (16, 63, False) and 1000 % 63 != 0
    assert plans[64, N, "ops"] == (2, 32, False) and plans[5, N, "ops"] == (2, 3, False)
    ragged = [k for k, (S, rp, _) in plans.items() if k[0] % rp]
    assert any(k[0] == 1000 for k in ragged) and any(k[0] == 300 for k in ragged) and any(k[0] == 5 for k in ragged)
    # the four-row steps of a chunk: tail only, one step, a step and a tail
    assert {(rp // 4, rp % 4) for (M, _, s), (S, rp, _) in plans.items() if s == 1 and M <= 5} == {(0, 1), (0, 3), (1, 0), (1, 1)}
    assert {(-(-n // 256), n % 256) for n in RD.CS_N} == {(1, 1), (1, 255), (1, 0), (2, 1)}
    assert RD.CS_LD_PAD % 4 != 0
    assert RD.colsum_plan(5, 4, 3) is None   # no room for one partial row: refused


def test_wgrad_slab_shapes_keep_their_slab_counts():
    """448 rows in 7 chunks of 64, 512 rows in 4 of 128, 192 + 19 rows in 3 of 64: the slab counts of the 6336-,
    4096- and 6323-row cases, the last with their ragged M % 32 = 19 rows."""
    for M, N, K, split, dtype in RD.WGRAD_SLABS:
        R0 = M - M % 32
        assert M <= 512 and 2 <= split <= RD.CB_SHORT and (N * K) % 4 == 0
        assert R0 % split == 0 and (R0 // split) % 64 == 0   # r_chunk = R0 / split for a BK of 32 or 64 alike
    assert [M % 32 for M, *_ in RD.WGRAD_SLABS] == [0, 0, 19]
