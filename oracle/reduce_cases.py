"""Cases for the column-reduction kernels (colsum_partial_kernel and splitk_reduce_kernel of csrc/gemm.hip,
colreduce_kernel of csrc/reduce.hpp, colreduce_batch_kernel of csrc/colbatch.hip) that hold them to equality
(test infrastructure only: imported by tests/).

These kernels only add, in IEEE f32 without fast-math, so a stated order fixes every bit.  Two measures, neither
with a tolerance:

  (a) exact    ``ints``: non-zero integers in [-4, 4].  Every partial sum of up to 4096 rows is an integer below
               2^24, so the f32 result is the float64 column sum bit for bit in ANY order.  A dropped, doubled or
               foreign row or column changes the sum (no row contributes zero anywhere).
  (b) ordered  ``normals``: f32 standard normals.  The result is bit for bit a torch float32 restatement, on the
               CPU, of the order the kernel source states.  A silent change of order changes low bits.

The restatements below are written from the kernel source, one vector add over the columns per add of the kernel
(torch's CPU float32 add is the IEEE add).  They return the SUM; with ``accumulate`` every path stores
``out + sum`` (one more add, :func:`finish`).  tests/test_reduce_cases_host.py holds each restatement to (a)
and to the textbook bound S * 2^-24 * sum |x| on ``normals``, and each shape list below to the branch its comment
names, by the host's dispatch rules as restated in :func:`batch_plan` and :func:`colsum_plan`.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import torch

F32, BF = torch.float32, torch.bfloat16

# ---------------------------------------------------------------------------- constants of the kernels
CB_MAXJ, CB_ROWS, CB_COLS = 16, 64, 256        # colbatch.hip: jobs per launch, rows x columns of a tall workgroup
CB_SHORT, CB_SHORT_COLS = 8, 2048              # short jobs: most rows, columns per workgroup
CR_GROUP, CR_SLICES, CR_COLS = 64, 16, 64      # reduce.hpp: rows per stage-1 group, row slices, columns per block
SCR_ALIGN = 4                                  # floats: every scratch slice of a batch starts on 16 bytes
COLSUM_MAX_S = 256                             # vit_colsum: most partial rows
MAX_EXACT_ROWS = 4096                          # 4 * 4096 = 2^14 per column, far below 2^24


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------- case builders
@dataclass(frozen=True)
class Case:
    kind: str            # "ints" | "normals"
    part: torch.Tensor   # [S][N] f32 (or bf16 for vit_colsum)
    out0: torch.Tensor   # [N] f32: what ``out`` holds before an accumulating call
    ref: torch.Tensor    # [N] float64: the column sum of ``part``

    @property
    def S(self):
        return self.part.shape[0]

    @property
    def N(self):
        return self.part.shape[1]


@functools.lru_cache(maxsize=None)
def ints(S, N, dtype=F32, seed=0):
    """Non-zero integers in [-4, 4] (bf16 holds them too) and an integer-valued ``out0`` in [-8, 8]."""
    assert S <= MAX_EXACT_ROWS
    g = _gen(7001 + 131 * S + N + 17 * seed)
    mag = torch.randint(1, 5, (S, N), generator=g)
    sign = torch.randint(0, 2, (S, N), generator=g) * 2 - 1
    part = (mag * sign).to(dtype)
    out0 = torch.randint(-8, 9, (N,), generator=g).to(F32)
    return Case("ints", part, out0, part.double().sum(0))


@functools.lru_cache(maxsize=None)
def normals(S, N, dtype=F32, seed=0):
    """Standard normals; anything below 2^-10 in magnitude is replaced by 1 (no zeros, no denormals)."""
    g = _gen(9001 + 131 * S + N + 17 * seed)
    part = torch.randn(S, N, generator=g)
    part = torch.where(part.abs() < 2.0 ** -10, torch.ones_like(part), part).to(dtype)
    out0 = torch.randn(N, generator=g)
    out0 = torch.where(out0.abs() < 2.0 ** -10, torch.ones_like(out0), out0)
    return Case("normals", part, out0, part.double().sum(0))


def case(kind, S, N, dtype=F32, seed=0):
    return {"ints": ints, "normals": normals}[kind](S, N, dtype, seed)


def finish(total, out0, accumulate):
    """What every path stores: ``out + s`` with accumulate, else ``s``."""
    return out0 + total if accumulate else total.clone()


def textbook_bound(part):
    """Per column, the bound on |f32 sum in any order - exact sum| of S adds: S * 2^-24 * sum_r |x_r| (float64)."""
    S = part.shape[0]
    return S * 2.0 ** -24 * part.double().abs().sum(0)


# ---------------------------------------------------------------------------- order restatements (torch f32, CPU)
def _zeros(N):
    return torch.zeros(N, dtype=F32)


def colsum_partial(x, rows_per):
    """colsum_partial_kernel: [S][N] f32 partial rows of x [M][N] (f32 or bf16, converted element by element).
    Chunk y takes rows [y * rows_per, min(M, (y + 1) * rows_per)); four accumulators take rows i, i+1, i+2, i+3
    while four are left, the tail goes into the first; the chunk value is (s0 + s1) + (s2 + s3)."""
    M, N = x.shape
    x = x.to(F32)
    S = (M + rows_per - 1) // rows_per
    part = torch.empty(S, N, dtype=F32)
    for y in range(S):
        r0, r1 = y * rows_per, min(M, (y + 1) * rows_per)
        s = [_zeros(N) for _ in range(4)]
        i = r0
        while i + 4 <= r1:
            for t in range(4):
                s[t] = s[t] + x[i + t]
            i += 4
        while i < r1:
            s[0] = s[0] + x[i]
            i += 1
        part[y] = (s[0] + s[1]) + (s[2] + s[3])
    return part


def _colreduce_stage(part, z0, z1):
    """One colreduce_kernel block row: rows [z0, z1) of part.  Slice sl (of 16) starts at z0 + sl and steps by 64
    with a0..a3 taking z, z+16, z+32, z+48 while z + 48 < z1; the rest goes into a0 in steps of 16; the slice
    value is (a0 + a1) + (a2 + a3); the slices are summed 0..15 starting from 0."""
    N = part.shape[1]
    slices = []
    for sl in range(CR_SLICES):
        a = [_zeros(N) for _ in range(4)]
        z = z0 + sl
        while z + 48 < z1:
            for t in range(4):
                a[t] = a[t] + part[z + 16 * t]
            z += 64
        while z < z1:
            a[0] = a[0] + part[z]
            z += 16
        slices.append((a[0] + a[1]) + (a[2] + a[3]))
    s = _zeros(N)
    for k in range(CR_SLICES):
        s = s + slices[k]
    return s


def colreduce_two_stage(S, scratch):
    """launch_colreduce_multi: two stages with scratch and S > 64, one otherwise."""
    return bool(scratch) and S > CR_GROUP


def colreduce(part, scratch):
    """launch_colreduce on [S][N]: one stage over all S rows, or (scratch, S > 64) stage 1 per 64-row group and
    stage 2 over the group sums."""
    S, N = part.shape
    part = part.to(F32)
    if not colreduce_two_stage(S, scratch):
        return _colreduce_stage(part, 0, S)
    G = (S + CR_GROUP - 1) // CR_GROUP
    groups = torch.stack([_colreduce_stage(part, g * CR_GROUP, min(S, (g + 1) * CR_GROUP)) for g in range(G)])
    return _colreduce_stage(groups, 0, G)


def colreduce_scratch_floats(S, N):
    return (S + CR_GROUP - 1) // CR_GROUP * N if S > CR_GROUP else 0


def colbatch_short(part):
    """colreduce_batch_kernel, S <= 8: a = row 0, then a += row r in row order."""
    S = part.shape[0]
    assert 1 <= S <= CB_SHORT
    a = part[0].to(F32).clone()
    for r in range(1, S):
        a = a + part[r]
    return a


def _colbatch_chunk(part, r0):
    """One 64-row chunk: wave w sums rows r0 + w + 4 i for i = 0..15 starting from 0 (+0 for rows past S), then
    (w0 + w1) + (w2 + w3)."""
    S, N = part.shape
    w = []
    for wave in range(4):
        s = _zeros(N)
        for i in range(16):
            r = r0 + wave + 4 * i
            s = s + (part[r] if r < S else _zeros(N))
        w.append(s)
    return (w[0] + w[1]) + (w[2] + w[3])


def colbatch_tall(part):
    """colreduce_batch_kernel, S > 8: the 64-row chunks in chunk order, starting from chunk 0's value."""
    S = part.shape[0]
    assert S > CB_SHORT
    part = part.to(F32)
    chunks = (S + CB_ROWS - 1) // CB_ROWS
    a = _colbatch_chunk(part, 0)
    for q in range(1, chunks):
        a = a + _colbatch_chunk(part, q * CB_ROWS)
    return a


def splitk_reduce(slabs):
    """splitk_reduce_kernel on [nslab][n]: slab 0, then += slab z in order (the last n % 4 elements start from
    0 and add slab 0 too: the same bits unless slab 0 holds -0)."""
    nslab, n = slabs.shape
    s = slabs[0].to(F32).clone()
    nv = n - n % 4
    s[nv:] = _zeros(n - nv) + slabs[0, nv:]
    for z in range(1, nslab):
        s = s + slabs[z]
    return s


# ---------------------------------------------------------------------------- vit_colsum and ops.colsum
def colsum_plan(M, N, partial_floats):
    """(S, rows_per, two_stage) as vit_colsum derives them from the partial buffer's size; None where it refuses."""
    S = partial_floats // max(N, 1)
    S = min(S, COLSUM_MAX_S)
    if S > M:
        S = M if M > 0 else 1
    if S < 1:
        return None
    rows_per = (M + S - 1) // S
    S = max(1, (M + rows_per - 1) // rows_per)
    return S, rows_per, colreduce_two_stage(S, partial_floats >= S * N + colreduce_scratch_floats(S, N))


def ops_colsum_floats(M, N):
    """The partial buffer ops.colsum passes: S = M // 64 rows (1..256) and the second stage's group sums."""
    S = max(1, min(COLSUM_MAX_S, M // 64))
    return (S + (S + 63) // 64) * N


def colsum(x, partial_floats):
    """vit_colsum on x [M][N] with a partial buffer of that many floats: (sum [N], partial rows [S][N])."""
    M, N = x.shape
    S, rows_per, two = colsum_plan(M, N, partial_floats)
    part = colsum_partial(x, rows_per)
    assert part.shape[0] == S
    return colreduce(part, two), part


@functools.lru_cache(maxsize=None)
def colsum_case_sum(kind, M, N, dtype, S, rows_per, two_stage):
    """:func:`colsum` of ``case(kind, M, N, dtype)`` under a plan, computed once per distinct plan."""
    part = colsum_partial(case(kind, M, N, dtype).part, rows_per)
    assert part.shape[0] == S
    return colreduce(part, two_stage)


@functools.lru_cache(maxsize=None)
def colreduce_case_sum(kind, S, N, scratch, seed=0):
    return colreduce(case(kind, S, N, F32, seed).part, scratch)


@functools.lru_cache(maxsize=None)
def batch_case_sum(kind, S, N, path, seed=0):
    part = case(kind, S, N, F32, seed).part
    return batch_sum(None, JobPlan(path, 0, 0, 0, 0, 0, 0, 0, 0, 0), part)


# ---------------------------------------------------------------------------- vit_colreduce_batch: dispatch
@dataclass(frozen=True)
class Job:
    S: int
    N: int
    accumulate: int = 0
    part_off: int = 0   # floats the partials start past a 16-byte boundary (1: not vector loadable)
    out_off: int = 0    # floats ``out`` starts past a 16-byte boundary (1: store_out's scalar branch)


@dataclass(frozen=True)
class JobPlan:
    path: str           # "short" | "tall1" | "ticket" | "fallback1" | "fallback2"
    strips: int
    chunks: int
    wgs: int            # workgroups of the batch kernel (0 on the fallback path)
    counters: int
    scratch_floats: int  # as handed out: rounded up to SCR_ALIGN
    scr0: int
    cnt0: int
    wg0: int            # first workgroup within its launch
    launch: int         # index of the batch-kernel launch (-1 on the fallback path)


def job_vec_ok(job):
    return job.N % 4 == 0 and job.part_off % 4 == 0


def scr_round(floats):
    return (floats + SCR_ALIGN - 1) // SCR_ALIGN * SCR_ALIGN


def batch_plan(jobs):
    """The host side of vit_colreduce_batch / vit_colreduce_batch_sizes restated: per job its JobPlan, then the
    workgroups of every batch-kernel launch (16 jobs each), the scratch floats and the counters."""
    plans, launches = [], []
    wg = cnt0 = scr = nb = 0
    for j in jobs:
        assert j.S > 0 and j.N > 0
        if not job_vec_ok(j):
            sf = colreduce_scratch_floats(j.S, j.N)
            plans.append(JobPlan("fallback2" if j.S > CR_GROUP else "fallback1", (j.N + CR_COLS - 1) // CR_COLS,
                                 (j.S + CR_GROUP - 1) // CR_GROUP if j.S > CR_GROUP else 1, 0, 0,
                                 scr_round(scr + sf) - scr, scr, cnt0, 0, -1))
            scr = scr_round(scr + sf)
            continue
        short = j.S <= CB_SHORT
        strips = (j.N + CB_SHORT_COLS - 1) // CB_SHORT_COLS if short else (j.N + CB_COLS - 1) // CB_COLS
        chunks = 1 if short else (j.S + CB_ROWS - 1) // CB_ROWS
        ticket = chunks > 1
        sf = scr_round(scr + chunks * j.N) - scr if ticket else 0
        plans.append(JobPlan("short" if short else "ticket" if ticket else "tall1", strips, chunks, strips * chunks,
                             strips if ticket else 0, sf, scr, cnt0, wg, len(launches)))
        wg += strips * chunks
        if ticket:
            cnt0 += strips
            scr += sf
        nb += 1
        if nb == CB_MAXJ:
            launches.append(wg)
            wg = nb = 0
    if nb:
        launches.append(wg)
    return plans, launches, scr, cnt0


def batch_sum(job, plan, part):
    """The restated sum of one batch job on the path the plan names."""
    if plan.path == "short":
        return colbatch_short(part)
    if plan.path in ("tall1", "ticket"):
        return colbatch_tall(part)
    return colreduce(part, True)   # the batch always hands launch_colreduce a scratch slice


# ---------------------------------------------------------------------------- the shapes the GPU tests run
# -- vit_colreduce_batch
# short path: 1 row, 2 rows, one below the limit, the limit (8 / 9 is the short / tall boundary)
CB_SHORT_S = (1, 2, 7, 8)
# one lane; the first 1024-column half full, one f32x4 into the second half; the workgroup's last f32x4 empty,
# the workgroup full; one f32x4 into a second workgroup
CB_SHORT_N = (4, 1024, 1028, 2044, 2048, 2052)
# tall path, one chunk: first tall row count, a ragged chunk one row short, the full chunk (64 / 65 is the
# one-chunk / ticketed boundary)
CB_TALL1_S = (9, 63, 64)
# one lane; the strip's last lane empty, the strip full, one lane into a second strip
CB_TALL1_N = (4, 252, 256, 260)
# ticketed path: chunks -> (S): 2 with one row in the last (65), 2 full (128), 3 (129): tail loop only;
# 8 (512): tail loop of 7; 9 (576): one batch of eight loads; 10 (577): a batch plus one; 18 (1089): two batches plus one
CB_TICKET_S = (65, 128, 129, 512, 576, 577, 1089)
CB_TICKET_CHUNKS = (2, 2, 3, 8, 9, 10, 18)
# one full strip, a second strip of one lane, four strips with the last ragged
CB_TICKET_N = (256, 260, 772)
# fallback (two-stage colreduce): N % 4 != 0 with S <= 8, one stage of 64, two stages with 3 * 30 = 90 and
# 3 * 101 = 303 scratch floats (no multiples of 4: the slice rounding)
CB_FALLBACK_SN = ((7, 30), (64, 30), (130, 30), (130, 101))
# N % 4 == 0 but the partials one float off 16 bytes: a short, a one-chunk and a many-row shape fall back
CB_FALLBACK_OFF_SN = ((7, 32), (64, 256), (130, 260))
# an aligned vector job whose ``out`` starts one float off: store_out's scalar branch on the short and the
# ticketed path
CB_OUT_OFF_SN = ((5, 1028), (130, 260))


def _alt(sn, acc0=0, **kw):
    return [Job(S, N, (acc0 + i) % 2, **kw) for i, (S, N) in enumerate(sn)]


def _filler(n, acc0=0):
    """n cheap vector jobs (short and one-chunk tall in turn) to fill a launch."""
    return [Job((3, 20)[i % 2], (1028, 260)[i % 2], (acc0 + i // 2) % 2) for i in range(n)]


def _mixes():
    m = {}
    m["short"] = _alt([(S, N) for S in CB_SHORT_S for N in CB_SHORT_N])            # 24 jobs: two launches
    m["tall1"] = _alt([(S, N) for S in CB_TALL1_S for N in CB_TALL1_N])
    m["ticket"] = _alt([(S, N) for S in CB_TICKET_S for N in CB_TICKET_N])         # 21 jobs: counters carry over
    m["fallback"] = _alt(CB_FALLBACK_SN) + _alt(CB_FALLBACK_OFF_SN, part_off=1)
    m["out_off"] = _alt(CB_OUT_OFF_SN, out_off=1) + _alt(CB_OUT_OFF_SN, 1, out_off=1)
    # exactly 16 jobs, the last one ticketed: the flush inside the loop and nothing left for the one after it
    m["batch16"] = [Job(129, 260, 1)] + _filler(14) + [Job(65, 772, 0)]
    # 17: ticketed jobs 15 and 16 stand on both sides of the flush (counter and scratch offsets carry over,
    # the workgroup base starts again)
    m["batch17"] = _filler(7) + [Job(130, 256, 0)] + _filler(7, 1) + [Job(577, 260, 1), Job(129, 772, 0)]
    # 33: the same at both flushes, with a fallback job (not counted among the 16) in the first two launches' spans
    m["batch33"] = (_filler(6) + [Job(130, 30, 1)] + _filler(9, 1) + [Job(128, 260, 0), Job(65, 256, 1)]
                    + _filler(7) + [Job(130, 101, 0)] + _filler(7, 1) + [Job(576, 260, 1), Job(129, 256, 0)])
    # the scratch-slice rounding: two two-stage fallback jobs (90 and 303 scratch floats) in front of ticketed
    # jobs, whose slices start at 92 and 396 floats rather than 90 and 393
    m["fix"] = [Job(130, 30, 0), Job(130, 101, 1), Job(130, 260, 0), Job(3, 1028, 1), Job(65, 256, 1),
                Job(20, 260, 0), Job(130, 30, 1), Job(129, 772, 0), Job(5, 2052, 0), Job(9, 4, 1)]
    return m


CB_MIXES = _mixes()
# the mixes ops.ColBatch runs over a NaN-filled workspace, and the one the graph replay captures
CB_OPS_MIXES = ("ticket", "batch33", "fix")
CB_GRAPH_MIX = "batch17"

# -- vit_colreduce, vit_colreduce_multi
# S: one slice; 15 / 16 / 17: the last slice empty, every slice one row, slice 0 a second row (the a0 tail);
# 63 / 64 / 65: slice 15 short of a four-wide step (15 + 48 < 63 fails: three tail rows), every slice exactly one
# four-wide step, slice 0 a tail row after it -- and with scratch the second stage's first two group rows;
# 128 / 129: two full groups, a third of one row; 300: five groups, ragged
CR_S = (1, 15, 16, 17, 63, 64, 65, 128, 129, 300)
# N: one column; a block one short, full, one over; three blocks with the last ragged
CR_N = (1, 63, 64, 65, 136)
CR_NQ = (1, 2, 3)

# -- vit_colsum
# M: one row; 3 / 4 / 5: tail only, one four-row step, a step and a tail; 64: sixteen steps and no tail; 300 and 1000:
# many chunks
CS_M = (1, 3, 4, 5, 64, 300, 1000)
# N: one column; a 256-column block one short, full, one over
CS_N = (1, 255, 256, 257)
CS_LD_PAD = 3   # the row stride is N + 3: wider than N and no multiple of 4
# partial rows the buffer has room for, S_req (partial_floats = S_req * N unless said otherwise):
#   1, 5, 300: the sizes test_colsum_with_a_partial_buffer_of_exactly_the_documented_size checks at 300 x 136
#              (S = 1; five chunks; capped by M below 300, at 256 from there on: the rows the cap frees
#              leave room for the second stage)
#   7:         a ragged last chunk at M = 300 (43 rows, then 42) and M = 1000 (143, then 142)
#   100, 102:  S = 100 > 64 at M >= 300 without and with room for the second stage's two group rows
#   5000:      capped at 256 (M = 1000: 250 rows of 4), with room
#   "ops":     what ops.colsum passes: M // 64 rows (1..256) and a row per 64 of them for the second stage, which
#              vit_colsum then spends on partial rows too (M = 1000: 16 rows of 63, not 15 of 67)
CS_SREQ = (1, 5, 300, 7, 100, 102, 5000, "ops")


def colsum_floats(M, N, sreq):
    return ops_colsum_floats(M, N) if sreq == "ops" else sreq * N


# -- split-K slab sums: (M, N, K, split, dtype) of test_linear_wgrad_partials_sum_to_dw shrunk to a few hundred
# rows with the same number of slabs (7 of 64 rows; 4 of 128 rows), and its ragged case (6323 = 3 slabs and
# M % 32 = 19 rows folded into the last) as 3 slabs of 64 rows and 19 more
WGRAD_SLABS = ((448, 256, 128, 7, BF), (512, 512, 256, 4, F32), (211, 256, 384, 3, BF))
