"""Tensor-level wrappers over the C-ABI kernels (no compute happens in Python).

Every function takes torch tensors that live on the ROCm device, launches the
HIP kernel on the current stream and returns.  These mirror the torch ops the
reference's hot path reaches through timm:

  linear_fwd / linear_dgrad / linear_wgrad   F.linear fwd / bwd  (timm Attention.qkv/proj, Mlp.fc1/fc2, head)
  layer_norm_fwd / layer_norm_bwd            F.layer_norm         (timm Block.norm1/norm2, final norm)
  sdpa_fwd / sdpa_bwd                        F.scaled_dot_product_attention
  patch_unfold + patch_embed_fwd             Conv2d(k16, s16) + cat(cls) + pos_embed (timm PatchEmbed/_pos_embed)
  cross_entropy_fwd / _bwd                   F.cross_entropy (VIT:140)
  sgd_step                                   torch.optim.SGD.step (VIT:294-299)
"""
from __future__ import annotations

import os

import torch

from . import _lib as L
from ._lib import call, ptr

_WS = {}


def workspace(name: str, nbytes: int, device) -> torch.Tensor:
    """Grow-only scratch buffer, reused across calls on the same stream."""
    key = (name, torch.device(device))
    t = _WS.get(key)
    if t is None or t.numel() < nbytes:
        t = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=device)
        _WS[key] = t
    return t


def _s(t: torch.Tensor) -> int:
    return L.stream_ptr(t.device)


def _keep(t: torch.Tensor):
    """t is read by work queued on the current stream after its producer's stream moves on:
    the caching allocator must not hand its memory out again before that work ran."""
    if t.is_cuda:
        t.record_stream(torch.cuda.current_stream(t.device))


# ----------------------------------------------------------------------------
# GEMMs
# ----------------------------------------------------------------------------

_SK = {}  # (device index, stream handle) -> (part, counters) registered with vit_gemm_streamk_workspace


def _streamk(device, stream=None):
    """Register (once per (device, stream)) the stream-K workspace the f32 MFMA GEMMs use on the
    current stream (or ``stream``).  Keyed by device too: the null stream has handle 0 on every device.
    Under graph capture an unregistered stream stays unregistered (the workspace's zero-fill would be
    captured, not run, and its memory would come from the graph's pool): the plain launch runs there.
    The two forms sum k in different orders, so an f32 GEMM that ran stream-K eagerly and as the plain
    launch in a replayed graph agree to rounding, not bit for bit -- unless the capture
    stream was registered before capture: ``register_capture_stream``."""
    st = L.stream_ptr(device) if stream is None else stream.cuda_stream
    key = (torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device(), st)
    if key in _SK or torch.cuda.is_current_stream_capturing():
        return
    g = 2 * torch.cuda.get_device_properties(device).multi_processor_count
    part = torch.empty(g * 2 * 128 * 128, dtype=torch.float32, device=device)
    cnt = torch.zeros(g, dtype=torch.int32, device=device)
    with torch.cuda.device(key[0]):
        call("vit_gemm_streamk_workspace", st, ptr(part), part.numel() * 4, ptr(cnt), g)
    _SK[key] = (part, cnt)


def register_capture_stream(stream, device=None):
    """Give ``stream`` (e.g. the side stream a ``torch.cuda.graph`` captures on) its stream-K workspace
    before capture, so the f32 GEMMs captured on it take the same form -- and the same bits -- as the
    eager launches on a registered stream."""
    _streamk(stream.device if device is None else device, stream)


def linear_fwd(x2d, w, bias=None, epi=L.EPI_STORE, out=None, out_dtype=None, resid=None, act_out=None, wimg=None,
               x_image=False, out_image=False):
    """y = epi(x @ w^T + bias).  x2d [M,K] (row stride x2d.stride(0)), w [N,K] contiguous.
    EPI_BIAS_GELU / EPI_BIAS_QGELU return (act'(pre), act(pre)) with pre = x @ w^T + bias;
    EPI_BIAS_GELU_FWD / EPI_BIAS_QGELU_FWD (no backward follows) return act(pre) alone, the same bits.
    ``wimg``: the pre-split image of ``w`` (:func:`weight_image`), read in its place by the fp32 "high" MFMA
    kernels -- the same bits.
    ``x_image`` / ``out_image`` (fp32 "high" with ``wimg`` only): ``x2d`` holds / ``out`` receives the
    pre-split image of the f32 matrix instead of its values (:func:`linear_fwd_takes_image`); a call the pre-split
    MFMA kernels cannot run raises."""
    L.require_gpu(x2d)
    M, K = x2d.shape
    N = w.shape[0]
    assert w.shape[1] == K and w.is_contiguous() and x2d.stride(1) == 1
    assert w.dtype == x2d.dtype
    if out is None:
        if epi == L.EPI_RESID:
            od = torch.float32
        else:
            od = out_dtype or x2d.dtype
        out = torch.empty(M, N, dtype=od, device=x2d.device)
    if epi in (L.EPI_BIAS_GELU, L.EPI_BIAS_QGELU):
        if act_out is None:
            act_out = torch.empty_like(out)
    if epi == L.EPI_RESID:
        assert resid is not None and resid.dtype == torch.float32 and out.dtype == torch.float32
        assert resid.stride(0) == out.stride(0)
    if x2d.dtype == torch.float32:
        _streamk(x2d.device)
    if x_image or out_image:
        assert wimg is not None and x2d.dtype == torch.float32 and out.dtype == torch.float32
    args = (L.F32_SPLIT if x_image else L.dt(x2d), L.F32_SPLIT if out_image else L.dt(out), epi, M, N, K, ptr(x2d),
            x2d.stride(0), ptr(w), ptr(bias), ptr(out), out.stride(0), ptr(resid), ptr(act_out))
    if wimg is not None:
        assert wimg.numel() == N * K and wimg.dtype == torch.float32 and wimg.device == w.device
        call("vit_linear_fwd_wimg", *args, ptr(wimg), _s(x2d))
    else:
        call("vit_linear_fwd", *args, _s(x2d))
    return (out, act_out) if epi in (L.EPI_BIAS_GELU, L.EPI_BIAS_QGELU) else out


# rows per column-sum partial of the input-gradient epilogues (gemm.hip / gemm_g4.hip: one partial row per
# 64-row group, vit_linear_dgrad_partial_floats) and rows per k-tile of the weight-gradient kernels (big::PP::BK)
DGRAD_SUM_ROWS = 64
WGRAD_KTILE_ROWS = 32
_LN_ROWS = []
_PART_ROWS = {}


def ln_bwd_rows_per() -> int:
    """Rows per partial block of the LayerNorm backward (VIT_LN_BWD_ROWS, read by the library), recovered from
    vit_layer_norm_bwd_blocks: the largest row count that is still one block."""
    if not _LN_ROWS:
        blocks = L.lib().vit_layer_norm_bwd_blocks
        r = 1
        while r < (1 << 16) and blocks(r + 1) == 1:
            r += 1
        _LN_ROWS.append(r)
    return _LN_ROWS[0]


class PartRows:
    """Where the partial rows of a row-padded launch go in the dense launch's [S][N] partial matrix: the
    launch has n * every partial rows, of which row every * i (image i's, the others are zero rows' sums)
    becomes row rows[i].  Checked on the host: rows distinct and inside the matrix."""

    def __init__(self, rows, S, every, device):
        rows = [int(r) for r in rows]
        if not rows or min(rows) < 0 or max(rows) >= S or len(set(rows)) != len(rows) or every < 1:
            raise ValueError(f"partial rows {rows[:4]}.. do not fit a dense partial matrix of {S} rows one to one")
        self.n, self.S, self.every = len(rows), int(S), int(every)
        self.idx = torch.tensor(rows, dtype=torch.int64, device=device)


def dense_part_rows(B, N, unit, every, device):
    """PartRows of a launch over B images padded to ``every * unit`` rows each, against the dense launch over
    B * N rows: image b's class row b * N lies in the dense launch's partial row b * N // unit.  Cached: it
    depends on the shapes alone."""
    key = (B, N, unit, every, torch.device(device))
    if key not in _PART_ROWS:
        _PART_ROWS[key] = PartRows([b * N // unit for b in range(B)], (B * N + unit - 1) // unit, every, device)
    return _PART_ROWS[key]


def spread_partials(part2d, pr):
    """[S][N] f32, zero but for row pr.idx[i] = row pr.every * i of part2d ([n * every][N]): partial sums of a
    row-padded launch laid out as the dense launch's partial rows, so that a ColBatch job reduces them in the
    dense launch's order."""
    rows, N = part2d.shape
    assert part2d.is_contiguous() and part2d.dtype == torch.float32
    assert rows == pr.n * pr.every and pr.idx.numel() == pr.n and pr.idx.device == part2d.device, (rows, pr.n, pr.every)
    out = zero_(torch.empty(pr.S * N, dtype=torch.float32, device=part2d.device))
    scatter_rows(part2d.view(pr.n, pr.every * N)[:, :N], pr.idx, out.view(pr.S, N))
    return out


def linear_dgrad(dy2d, w, out_dtype=torch.float32, epi=L.EPI_STORE, pre=None, out=None, dbias=None, reduce_on=None,
                 part_rows=None, wimg=None):
    """dx = dy @ w  (dy [M,N], w [N,K]); with EPI_GELU_BWD / EPI_QGELU_BWD times ``pre`` [M,K] =
    the act'(pre) the forward's BIAS_GELU epilogue saved;
    dbias [K] (optional) receives the column sums of dx (fused into the GEMM epilogue).
    ``reduce_on`` (an object with ``.run(fn)``, e.g. the model's side stream): the final
    reduction of those column sums is issued through it instead of inline.
    ``part_rows`` (a PartRows, with a ColBatch): the partial rows are laid out as a dense launch's before
    they are reduced (:func:`spread_partials`).
    ``wimg``: the pre-split image of ``w^T`` (:func:`weight_image` with ``transposed=True``), read in place of
    ``w`` by the fp32 "high" MFMA kernels -- the same bits."""
    M, N = dy2d.shape
    K = w.shape[1]
    assert w.shape[0] == N and w.dtype == dy2d.dtype and dy2d.stride(1) == 1
    if out is None:
        out = torch.empty(M, K, dtype=out_dtype, device=dy2d.device)
    if pre is not None:
        assert pre.stride(0) == out.stride(0)
    part, nfl = None, 0
    defer = dbias is not None and reduce_on is not None
    if dbias is not None:
        assert dbias.dtype == torch.float32 and dbias.is_contiguous() and dbias.numel() == K
        nfl = L.lib().vit_linear_dgrad_partial_floats(M, K)
        # a deferred reduction reads the partials later on another stream: own buffer
        part = (torch.empty(nfl, dtype=torch.float32, device=dy2d.device) if defer
                else workspace("dgrad_bias", nfl * 4, dy2d.device))
    if dy2d.dtype == torch.float32:
        _streamk(dy2d.device)
    args = (L.dt(dy2d), L.dt(out), epi, M, N, K, ptr(dy2d), dy2d.stride(0), ptr(w), ptr(out), out.stride(0), ptr(pre),
            ptr(dbias), ptr(part), nfl, int(defer))
    if wimg is not None:
        assert wimg.numel() == N * K and wimg.dtype == torch.float32 and wimg.device == w.device
        call("vit_linear_dgrad_wimg", *args, ptr(wimg), _s(dy2d))
    else:
        call("vit_linear_dgrad", *args, _s(dy2d))
    if defer:
        rows = (M + DGRAD_SUM_ROWS - 1) // DGRAD_SUM_ROWS
        if isinstance(reduce_on, ColBatch):
            if part_rows is not None:
                part, rows = spread_partials(part[:rows * K].view(rows, K), part_rows), part_rows.S
            reduce_on.add(part, rows, K, dbias)
            return out

        def finish():
            _keep(part)
            colreduce(part, rows, K, dbias, scratch=part[rows * K:])
        reduce_on.run(finish)
    return out


def colreduce(part, S, N, out, accumulate=False, scratch=None):
    """out[N] (+)= part[:S].sum(0) (partials from a fused epilogue)."""
    call("vit_colreduce", ptr(part), S, N, ptr(out), int(accumulate), ptr(scratch), _s(out))
    return out


class ColBatch:
    """Collects the deferred column reductions of one block's backward (bias and LayerNorm-affine
    gradients from their producers' partial sums) and issues them as ONE vit_colreduce_batch launch
    (``launch``, on whatever stream is current then -- the model's side stream).  The partial
    buffers stay referenced until ``launch`` has been enqueued; the caller guards them for the
    stream (``tensors``)."""

    def __init__(self):
        self.jobs = []
        self.parts = []  # the partial buffers (guard them for the stream the launch runs on)
        self.device = None

    def add(self, part, S, N, out, accumulate=False):
        """out[N] (+)= sum of the S rows of part ([S][N] f32, contiguous rows).  Only the output's
        address is kept (gradient views must stay stealable by AccumulateGrad)."""
        if out is None or S <= 0:
            return
        assert part.dtype == torch.float32 and out.dtype == torch.float32 and part.is_contiguous()
        self.jobs.append((part.data_ptr(), out.data_ptr(), int(S), int(N), int(accumulate)))
        self.parts.append(part)
        self.device = part.device

    def launch(self):
        if not self.jobs:
            return
        import ctypes
        import numpy as np
        dev = self.device
        arr = np.array(self.jobs, dtype=np.int64).reshape(-1)
        jp = arr.ctypes.data_as(ctypes.c_void_p)
        sf, nc = ctypes.c_int64(0), ctypes.c_int(0)
        L.lib().vit_colreduce_batch_sizes(jp, len(self.jobs), ctypes.byref(sf), ctypes.byref(nc))
        scratch = workspace("colbatch", max(16, sf.value * 4), dev)
        cnt = _counters("colbatch", nc.value, dev)
        call("vit_colreduce_batch", jp, len(self.jobs), ptr(scratch), sf.value, ptr(cnt), nc.value, L.stream_ptr(dev))
        self.jobs = []


_CNT = {}


def _counters(name, n, device):
    """Grow-only int32 ticket counters, zero-filled when allocated (the kernels that use them leave
    them zero)."""
    key = (name, torch.device(device))
    t = _CNT.get(key)
    if t is None or t.numel() < n:
        t = torch.zeros(max(n, 64), dtype=torch.int32, device=device)
        _CNT[key] = t
    return t


_WGRAD_WGS = [int(os.environ.get("VIT_WGRAD_WGS", "128"))]


# the backward's tail (block 0's last weight gradients, the patch embedding's): nothing else is
# left to run beside them, so they split for the whole GPU
_WGRAD_TAIL_WGS = [int(os.environ.get("VIT_WGRAD_TAIL_WGS", "256"))]


def _wgrad_split(M, N, K, wgs=None):
    """Split of the M reduction so (256x256 output tiles) x split ~ _WGRAD_WGS workgroups
    (default 128: half the CUs, so the side-stream weight gradients leave CUs to the
    input-gradient chain on the main stream -- +1.3 % step rate vs 256): fp32 slab traffic split*N*K*8 bytes stays ~10% of the
    GEMM time."""
    tiles = max(1, ((N + 255) // 256) * ((K + 255) // 256))
    want = max(1, round((wgs or _WGRAD_WGS[0]) / tiles))
    return max(1, min(want, M // 1024))


def linear_wgrad(dy2d, x2d, out=None, split=None, tail=False, reduce_on=None):
    """dW [N,K] (f32) = dy^T @ x,  dy [M,N], x [M,K].  tail: split for _WGRAD_TAIL_WGS workgroups.
    ``reduce_on`` (a ColBatch): the split-K slabs go to a buffer of their own and their sum into
    ``out`` becomes a job of that batch (no separate slab-reduce launch)."""
    M, N = dy2d.shape
    K = x2d.shape[1]
    assert x2d.shape[0] == M and x2d.dtype == dy2d.dtype
    if out is None:
        out = torch.empty(N, K, dtype=torch.float32, device=dy2d.device)
    if split is None:
        split = _wgrad_split(M, N, K, _WGRAD_TAIL_WGS[0] if tail else None)
    defer = isinstance(reduce_on, ColBatch) and split > 1 and dy2d.dtype == torch.bfloat16
    probe = WGRAD_PROBE[0]
    if probe is not None:  # bench.py: HIP events around this launch, on the stream it runs on
        e0 = torch.cuda.Event(enable_timing=True)
        e0.record()
    if defer:
        nz = L.lib().vit_linear_wgrad_nslabs(L.dt(dy2d), M, N, K, split)
        slabs = torch.empty(nz * N * K, dtype=torch.float32, device=dy2d.device)
        call("vit_linear_wgrad_partials", L.dt(dy2d), M, N, K, ptr(dy2d), dy2d.stride(0), ptr(x2d), x2d.stride(0),
             split, ptr(slabs), slabs.numel() * 4, _s(dy2d))
        reduce_on.add(slabs.view(nz, N * K), nz, N * K, out)
    else:
        ws = workspace("wgrad", split * N * K * 4, dy2d.device) if split > 1 else None
        call("vit_linear_wgrad", L.dt(dy2d), M, N, K, ptr(dy2d), dy2d.stride(0), ptr(x2d), x2d.stride(0), ptr(out),
             split, ptr(ws), 0 if ws is None else ws.numel(), _s(dy2d))
    if probe is not None:
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        probe.append((e0, e1, 2.0 * M * N * K, L.dt(dy2d) == L.BF16 and M % 32 == 0))
    return out


def pair_split(M, Na, Ka, Nb, Kb, tail=False):
    """The split-K factor :func:`linear_wgrad_pair` chooses for a pair over M rows."""
    tiles = ((Na + 255) // 256) * ((Ka + 255) // 256) + ((Nb + 255) // 256) * ((Kb + 255) // 256)
    wgs = _WGRAD_TAIL_WGS[0] if tail else _WGRAD_WGS[0]
    return max(1, min(max(1, round(wgs / tiles)), M // 1024))


def linear_wgrad_pair(a, b, reduce_on, tail=False, split=None):
    asked = split  # (the fallback launches choose their own split unless the caller fixed one)
    """Two weight gradients of a block over the same token rows, a = (dy, x, out), b likewise, as
    ONE grouped launch of split-K partials whose slab sums become two jobs of ``reduce_on`` (a
    ColBatch).  The split is chosen for the pair's tiles together (half the slabs of two separate
    launches).  Falls back to two linear_wgrad calls when the pair does not meet the grouped
    kernel's rules (bf16, M % 32 == 0, MFMA operand alignment)."""
    (dya, xa, outa), (dyb, xb, outb) = a, b
    M, Na = dya.shape
    Ka, Nb, Kb = xa.shape[1], dyb.shape[1], xb.shape[1]
    ok = (isinstance(reduce_on, ColBatch) and dya.dtype == torch.bfloat16 and dyb.dtype == torch.bfloat16
          and xa.dtype == dya.dtype and xb.dtype == dyb.dtype and dyb.shape[0] == M and M % 32 == 0)
    if ok:
        if split is None:
            split = pair_split(M, Na, Ka, Nb, Kb, tail)
        nz = L.lib().vit_linear_wgrad_nslabs(L.BF16, M, Na, Ka, split)
        sa = torch.empty(nz * Na * Ka, dtype=torch.float32, device=dya.device)
        sb = torch.empty(nz * Nb * Kb, dtype=torch.float32, device=dya.device)
        probe = WGRAD_PROBE[0]
        if probe is not None:
            e0 = torch.cuda.Event(enable_timing=True)
            e0.record()
        rc = L.lib().vit_linear_wgrad_partials2(M, split, Na, Ka, ptr(dya), dya.stride(0), ptr(xa), xa.stride(0),
                                                ptr(sa), sa.numel() * 4, Nb, Kb, ptr(dyb), dyb.stride(0), ptr(xb),
                                                xb.stride(0), ptr(sb), sb.numel() * 4, _s(dya))
        if rc not in (0, 1):  # 1 = hipErrorInvalidValue: the pair does not fit the grouped kernel
            L.check(rc, "vit_linear_wgrad_partials2")
        if rc == 0:
            if probe is not None:
                e1 = torch.cuda.Event(enable_timing=True)
                e1.record()
                probe.append((e0, e1, 2.0 * M * (Na * Ka + Nb * Kb), True))
            reduce_on.add(sa.view(nz, Na * Ka), nz, Na * Ka, outa)
            reduce_on.add(sb.view(nz, Nb * Kb), nz, Nb * Kb, outb)
            return outa, outb
    linear_wgrad(dya, xa, out=outa, split=asked, tail=tail, reduce_on=reduce_on)
    linear_wgrad(dyb, xb, out=outb, split=asked, tail=tail, reduce_on=reduce_on)
    return outa, outb


# bench.py's live roofline of the weight-gradient GEMMs: a list to collect
# (start event, end event, flop, on the MFMA path) per vit_linear_wgrad launch, or None
WGRAD_PROBE = [None]


def colsum(x2d, out=None, accumulate=False):
    """out[N] (f32) = x.sum(0)."""
    M, N = x2d.shape
    if out is None:
        out = torch.empty(N, dtype=torch.float32, device=x2d.device)
    S = max(1, min(256, M // 64))
    nfl = (S + (S + 63) // 64) * N
    part = workspace("colsum", nfl * 4, x2d.device)
    call("vit_colsum", L.dt(x2d), M, N, ptr(x2d), x2d.stride(0), ptr(out), ptr(part), nfl, int(accumulate),
         _s(x2d))
    return out


# ----------------------------------------------------------------------------
# LayerNorm
# ----------------------------------------------------------------------------

def layer_norm_fwd(x2d, w, b, eps, out_dtype, rows=None, ldx=None, out=None, need_stats=True, mean=None, rstd=None,
                   out_image=False):
    """``out_image``: ``out`` (f32) receives the pre-split image of the f32 result (D % 256 == 0)."""
    rows = x2d.shape[0] if rows is None else rows
    D = w.numel()
    ldx = x2d.stride(0) if ldx is None else ldx
    if out is None:
        out = torch.empty(rows, D, dtype=out_dtype, device=x2d.device)
    if need_stats and mean is None:
        mean = torch.empty(rows, dtype=torch.float32, device=x2d.device)
        rstd = torch.empty(rows, dtype=torch.float32, device=x2d.device)
    assert not out_image or out.dtype == torch.float32
    call("vit_layer_norm_fwd", L.dt(x2d), L.F32_SPLIT if out_image else L.dt(out), rows, D, ptr(x2d), ldx, ptr(out), out.stride(0), ptr(w),
         ptr(b), ptr(mean), ptr(rstd), float(eps), _s(x2d))
    return out, mean, rstd


def add_layer_norm_supported(D: int) -> bool:
    """Widths ``vit_add_layer_norm_fwd`` takes: D a multiple of 256 up to 2048 (ViT-B 768, ViT-L
    1024, ViT-H 1280, ...); other widths keep the residual add in the GEMM epilogue."""
    return D % 256 == 0 and 256 <= D <= 2048


def add_layer_norm_fwd(x2d, r2d, xs, w=None, b=None, eps=1e-6, out=None, mean=None, rstd=None, out_image=False):
    """xs = x2d + r2d (f32 + bf16 / f32 -> f32; xs may be x2d) and, with ``out`` given, out =
    LayerNorm(xs) (bf16 / f32) with its row mean / rstd: a Linear's residual add fused into the
    LayerNorm after it.  ``out_image``: ``out`` (f32) receives the pre-split image of the f32 LayerNorm result."""
    assert x2d.dtype == torch.float32 and xs.dtype == torch.float32
    rows, D = xs.shape
    if out is not None:
        assert mean is not None and rstd is not None
    ydt = L.dt(r2d) if out is None else L.dt(out)
    if out_image:
        assert out is not None and out.dtype == torch.float32
        ydt = L.F32_SPLIT
    call("vit_add_layer_norm_fwd", L.dt(r2d), ydt, rows, D, ptr(x2d),
         x2d.stride(0), ptr(r2d), r2d.stride(0), ptr(xs), xs.stride(0),
         ptr(out), out.stride(0) if out is not None else 0, ptr(w), ptr(b), ptr(mean), ptr(rstd), float(eps), _s(xs))
    return xs


def layer_norm_bwd(x, ldx, dy, w, mean, rstd, dx, lddx, rows, dres=None, ldres=0, dx_copy=None, ld_copy=0,
                   compact_np=0, dgamma=None, dbeta=None, dsum=None, ws="ln_partial", reduce_on=None, res_every=0,
                   part_rows=None):
    """dsum [D] (optional) receives the column sums of dx (a Linear bias gradient).
    ``res_every`` > 0: ``dres`` is compact, one row per ``res_every`` rows of dx, added to rows 0, res_every,
    ... alone (the class-token rows' gradient; vit_layer_norm_bwd_cls).
    ``reduce_on`` (an object with ``.run(fn)``): the dgamma / dbeta / dsum reductions of the
    per-64-row partials are issued through it (e.g. on the side stream) instead of inline."""
    D = w.numel()
    part = None
    nfl = 0
    want = dgamma is not None or dsum is not None
    defer = want and reduce_on is not None
    if want:
        nfl = L.lib().vit_layer_norm_bwd_partial_floats(rows, D)
        part = (torch.empty(nfl, dtype=torch.float32, device=x.device) if defer
                else workspace(ws, nfl * 4, x.device))
    tail = (ptr(dx), lddx, ptr(dx_copy), ld_copy, L.dt(dx_copy) if dx_copy is not None else L.BF16, compact_np,
            ptr(dgamma), ptr(dbeta), ptr(dsum), ptr(part), nfl, int(defer), _s(x))
    head = (L.dt(x), L.dt(dy), rows, D, ptr(x), ldx, ptr(dy), dy.stride(0), ptr(w), ptr(mean), ptr(rstd), ptr(dres),
            ldres)
    if res_every:
        assert dres is not None and dres.dtype == torch.float32 and dres.shape[0] * res_every >= rows
        call("vit_layer_norm_bwd_cls", *head, int(res_every), *tail)
    else:
        call("vit_layer_norm_bwd", *head, *tail)
    if defer:
        nb = L.lib().vit_layer_norm_bwd_blocks(rows)
        if isinstance(reduce_on, ColBatch):
            for q, o in enumerate((dgamma, dbeta, dsum)):
                if o is None:
                    continue
                pq = part[q * nb * D:(q + 1) * nb * D]
                if part_rows is not None:  # a PartRows: laid out as the dense launch's partial blocks
                    reduce_on.add(spread_partials(pq.view(nb, D), part_rows), part_rows.S, D, o)
                else:
                    reduce_on.add(pq, nb, D, o)
            return
        sc = part[3 * nb * D:]

        def finish():
            _keep(part)
            # the [dgamma | dbeta | dsum] partials are stacked: one launch per reduction stage
            if dgamma is not None:
                call("vit_colreduce_multi", ptr(part), 3 if dsum is not None else 2, nb, D, ptr(dgamma),
                     ptr(dbeta), ptr(dsum), 0, ptr(sc), _s(dgamma))
            else:
                call("vit_colreduce_multi", ptr(part[2 * nb * D:]), 1, nb, D, ptr(dsum), None, None, 0,
                     ptr(sc), _s(dsum))
        reduce_on.run(finish)


# ----------------------------------------------------------------------------
# attention
# ----------------------------------------------------------------------------

FP8_ATTN_MAX_TOKENS = 320  # vit_sdpa_fwd_fp8 holds the head's quantised K and V in LDS


def check_fp8_tokens(N, long=False):
    """The resident fp8 attention kernel holds at most 320 tokens; past that the streamed fp8 kernel runs only
    when asked for (``long``): otherwise refuse, never fall back to another precision."""
    if N > FP8_ATTN_MAX_TOKENS and not long:
        raise ValueError(f"fp8 attention (vit_sdpa_fwd_fp8) supports at most {FP8_ATTN_MAX_TOKENS} tokens, got "
                         f"{N}: switch it off (set_attention_fp8(False)) for this model, or ask for the streamed "
                         f"fp8 kernel (set_attention_fp8(True, long_sequences=True))")


def fp8_switches(enable, long_sequences=False, prequantize=False):
    """The three stored switches of ``set_attention_fp8`` (fp8, streamed past 320 tokens, pre-quantised K / V):
    the pre-quantised kernel is a form of the streamed one, so asking for it without ``long_sequences`` would
    be a silent no-op and raises instead."""
    if enable and prequantize and not long_sequences:
        raise ValueError("set_attention_fp8(prequantize=True) needs long_sequences=True: up to 320 tokens the "
                         "resident fp8 kernel already quantises K and V once per head")
    on = bool(enable)
    return on, on and bool(long_sequences), on and bool(long_sequences) and bool(prequantize)


def sdpa_fwd(qkv2d, B, H, N, o=None, scale=None, lse=None, causal=False, fp8=False, fp8_long=False, fp8_pre=False,
             image=False):
    """softmax(q k^T * scale) v per (b, h) from the fused qkv [B*N, 3D], any N (past 288 tokens the
    streamed bf16 or f32 kernels, or the generic ones for causal / misaligned rows); fp8: the block-scaled e4m3
    MFMA kernels (forward only: their lse is not the bf16 backward's) -- the resident one up to 320 tokens,
    past that the streamed one if ``fp8_long``, else ValueError.  ``fp8_pre`` (with ``fp8`` and ``fp8_long``,
    past 320 tokens only): K and V are quantised once into a workspace that lives for this call and the
    pre-quantised kernel streams it -- the streamed kernel's bits.  ``image`` (fp32 ``"high"`` only):
    ``qkv2d`` holds and ``o`` receives the pre-split image of the f32 tensor (vit_sdpa_fwd_image;
    :func:`sdpa_fwd_takes_image`); a call the image kernels cannot run raises."""
    if fp8:
        check_fp8_tokens(N, long=fp8_long)
    D = H * 64
    if o is None:
        o = torch.empty(B * N, D, dtype=qkv2d.dtype, device=qkv2d.device)
    if lse is None:
        lse = torch.empty(B * H * N, dtype=torch.float32, device=qkv2d.device)
    scale = 64 ** -0.5 if scale is None else scale
    if image:
        L.require_gpu(qkv2d)
        assert not fp8 and qkv2d.dtype == torch.float32 and o.dtype == torch.float32
        assert qkv2d.stride(1) == 1 and o.stride(1) == 1
        call("vit_sdpa_fwd_image", B, H, N, 64, ptr(qkv2d), qkv2d.stride(0), ptr(o), o.stride(0), ptr(lse),
             float(scale), int(causal), _s(qkv2d))
        return o, lse
    if fp8 and fp8_long and fp8_pre and N > FP8_ATTN_MAX_TOKENS:
        ws = sdpa_fp8_quant_kv(qkv2d, B, H, N)  # from the caching allocator, on this stream; not kept
        return sdpa_fwd_fp8_pre(qkv2d, ws, B, H, N, o=o, scale=scale, lse=lse, causal=causal)
    name = "vit_sdpa_fwd"
    if fp8:
        name = "vit_sdpa_fwd_fp8" if N <= FP8_ATTN_MAX_TOKENS else "vit_sdpa_fwd_fp8_stream"
    call(name, L.dt(qkv2d), B, H, N, 64, ptr(qkv2d), qkv2d.stride(0), ptr(o), o.stride(0), ptr(lse),
         float(scale), int(causal), _s(qkv2d))
    return o, lse


def sdpa_fwd_fp8_stream(qkv2d, B, H, N, o=None, scale=None, lse=None, causal=False):
    """The streamed fp8 forward (vit_sdpa_fwd_fp8_stream) at any N, for tests and tools: up to 320 tokens its o
    and lse are bit for bit the resident fp8 kernel's."""
    D = H * 64
    if o is None:
        o = torch.empty(B * N, D, dtype=qkv2d.dtype, device=qkv2d.device)
    if lse is None:
        lse = torch.empty(B * H * N, dtype=torch.float32, device=qkv2d.device)
    scale = 64 ** -0.5 if scale is None else scale
    call("vit_sdpa_fwd_fp8_stream", L.dt(qkv2d), B, H, N, 64, ptr(qkv2d), qkv2d.stride(0), ptr(o), o.stride(0),
         ptr(lse), float(scale), int(causal), _s(qkv2d))
    return o, lse


def sdpa_fp8_kv_bytes(B, H, N):
    """Bytes of the quantised K / V workspace of :func:`sdpa_fp8_quant_kv` (vit_sdpa_fp8_kv_bytes)."""
    n = L.i64(0)
    call("vit_sdpa_fp8_kv_bytes", B, H, N, L.C.addressof(n))
    return int(n.value)


def sdpa_fp8_quant_kv(qkv2d, B, H, N, ws=None):
    """The pre-pass of the pre-quantised fp8 forward (vit_sdpa_fp8_quant_kv) at any N: K and V of qkv2d as
    block-scaled e4m3 in ``ws`` (a uint8 tensor of at least sdpa_fp8_kv_bytes bytes; allocated if None).
    Returns ``ws``."""
    if ws is None:
        ws = torch.empty(sdpa_fp8_kv_bytes(B, H, N), dtype=torch.uint8, device=qkv2d.device)
    call("vit_sdpa_fp8_quant_kv", L.dt(qkv2d), B, H, N, 64, ptr(qkv2d), qkv2d.stride(0), ptr(ws),
         ws.numel() * ws.element_size(), _s(qkv2d))
    return ws


def sdpa_fwd_fp8_pre(qkv2d, ws, B, H, N, o=None, scale=None, lse=None, causal=False):
    """The pre-quantised fp8 forward (vit_sdpa_fwd_fp8_pre) at any N, for tests and tools: Q from qkv2d, K and
    V from ``ws`` (sdpa_fp8_quant_kv); o and lse are bit for bit sdpa_fwd_fp8_stream's."""
    D = H * 64
    if o is None:
        o = torch.empty(B * N, D, dtype=qkv2d.dtype, device=qkv2d.device)
    if lse is None:
        lse = torch.empty(B * H * N, dtype=torch.float32, device=qkv2d.device)
    scale = 64 ** -0.5 if scale is None else scale
    call("vit_sdpa_fwd_fp8_pre", L.dt(qkv2d), B, H, N, 64, ptr(qkv2d), qkv2d.stride(0), ptr(ws),
         ws.numel() * ws.element_size(), ptr(o), o.stride(0), ptr(lse), float(scale), int(causal), _s(qkv2d))
    return o, lse


def sdpa_fwd_cls(qkv2d, B, H, N, o=None, scale=None, lse=None):
    """:func:`sdpa_fwd` for a caller that reads query 0 of every (b, h) alone (the class-token tail): bf16 up to
    288 tokens runs query tile 0 of the resident kernel -- rows 0..15 of each image bit for bit sdpa_fwd's, the
    other rows o = 0 and lse = +inf; anything else runs sdpa_fwd (all rows)."""
    D = H * 64
    if o is None:
        o = torch.empty(B * N, D, dtype=qkv2d.dtype, device=qkv2d.device)
    if lse is None:
        lse = torch.empty(B * H * N, dtype=torch.float32, device=qkv2d.device)
    scale = 64 ** -0.5 if scale is None else scale
    call("vit_sdpa_fwd_cls", L.dt(qkv2d), B, H, N, 64, ptr(qkv2d), qkv2d.stride(0), ptr(o), o.stride(0), ptr(lse),
         float(scale), _s(qkv2d))
    return o, lse


CLS1_MAX_TOKENS = 2048  # vit_sdpa_cls1_fwd / vit_sdpa_cls1_bwd refuse more


def sdpa_cls1_fwd(qkv2d, B, H, N, o=None, scale=None, lse=None):
    """One-query attention forward (vit_sdpa_cls1_fwd): query row 0 of every image against all N keys and
    values, bf16 or f32, N up to 2048.  Returns (o [B, D] in the qkv dtype, lse [B * H] f32); ``o`` may be any
    [B, D] view with 16-byte-aligned rows (e.g. the class rows of a dense o, row stride N * D).  Agrees with
    sdpa_fwd's row 0 to rounding, not in bits."""
    D = H * 64
    if o is None:
        o = torch.empty(B, D, dtype=qkv2d.dtype, device=qkv2d.device)
    if lse is None:
        lse = torch.empty(B * H, dtype=torch.float32, device=qkv2d.device)
    assert o.shape == (B, D) and o.stride(1) == 1 and o.dtype == qkv2d.dtype and lse.numel() == B * H
    scale = 64 ** -0.5 if scale is None else scale
    call("vit_sdpa_cls1_fwd", L.dt(qkv2d), B, H, N, 64, ptr(qkv2d), qkv2d.stride(0), ptr(o), o.stride(0), ptr(lse),
         float(scale), _s(qkv2d))
    return o, lse


def sdpa_row1_fwd(qkv2d, qrow, B, H, N, causal=False, o=None, scale=None, lse=None):
    """One-query attention forward at a row per sequence (vit_sdpa_row1_fwd): query row ``qrow[b]`` (int64 [B] on
    the device, clamped to [0, N - 1] by the kernel) against keys ``0 .. qrow[b]`` (``causal``) or all N; bf16 or
    f32, N up to 2048.  Returns (o [B, D] in the qkv dtype, lse [B * H] f32); ``o`` may be any [B, D] view with
    16-byte-aligned rows.  ``qrow = 0`` without the mask is :func:`sdpa_cls1_fwd` bit for bit; against sdpa_fwd's
    row ``qrow[b]`` it agrees to rounding.  Forward only: there is no matching backward."""
    D = H * 64
    if o is None:
        o = torch.empty(B, D, dtype=qkv2d.dtype, device=qkv2d.device)
    if lse is None:
        lse = torch.empty(B * H, dtype=torch.float32, device=qkv2d.device)
    assert o.shape == (B, D) and o.stride(1) == 1 and o.dtype == qkv2d.dtype and lse.numel() == B * H
    assert qrow.dtype == torch.int64 and qrow.shape == (B,) and qrow.stride(0) == 1 and qrow.device == qkv2d.device
    scale = 64 ** -0.5 if scale is None else scale
    call("vit_sdpa_row1_fwd", L.dt(qkv2d), B, H, N, 64, ptr(qkv2d), qkv2d.stride(0), ptr(qrow), int(bool(causal)),
         ptr(o), o.stride(0), ptr(lse), float(scale), _s(qkv2d))
    return o, lse


def sdpa_cls1_bwd(qkv2d, o, do, lse, B, H, N, dqkv=None, scale=None):
    """One-query attention backward (vit_sdpa_cls1_bwd) from the class rows' dO: ``o`` / ``do`` [B, D] (any row
    stride), ``lse`` [B * H] of sdpa_cls1_fwd.  Writes every element of dqkv [B*N, 3D] (dq rows 1 .. N-1 of each
    image exact zeros); no workspace and no qkv bias partials."""
    D = H * 64
    if dqkv is None:
        dqkv = torch.empty(B * N, 3 * D, dtype=qkv2d.dtype, device=qkv2d.device)
    assert o.shape == (B, D) and do.shape == (B, D) and o.stride(1) == 1 and do.stride(1) == 1
    assert o.dtype == qkv2d.dtype and do.dtype == qkv2d.dtype and dqkv.dtype == qkv2d.dtype
    assert dqkv.shape == (B * N, 3 * D) and dqkv.stride(1) == 1 and lse.numel() == B * H
    scale = 64 ** -0.5 if scale is None else scale
    call("vit_sdpa_cls1_bwd", L.dt(qkv2d), B, H, N, 64, ptr(qkv2d), qkv2d.stride(0), ptr(o), o.stride(0), ptr(do),
         do.stride(0), ptr(lse), ptr(dqkv), dqkv.stride(0), float(scale), _s(qkv2d))
    return dqkv


def sdpa_bwd(qkv2d, o, do, lse, B, H, N, dqkv=None, scale=None, dbias=None, causal=False, ws="", reduce_on=None):
    """dbias [3*H*64] (optional) receives the column sums of dqkv (the qkv bias gradient).
    ``ws``: workspace-name suffix (calls running concurrently on different streams need their own).
    ``reduce_on`` (a ColBatch, bf16): the per-image bias partials are left for that batch to reduce.
    Past 288 tokens: the streamed kernels of the dtype (bf16 or f32; generic for causal / misaligned rows);
    in f32 dbias is a column sum over dqkv after the two kernels."""
    if dqkv is None:
        dqkv = torch.empty_like(qkv2d)
    scale = 64 ** -0.5 if scale is None else scale
    delta = workspace("sdpa_delta" + ws, B * H * N * 4, qkv2d.device)
    part, nfl = None, 0
    defer = dbias is not None and isinstance(reduce_on, ColBatch) and qkv2d.dtype == torch.bfloat16
    if dbias is not None:
        nfl = L.lib().vit_sdpa_bwd_partial_floats(B, N, H * 64)
        part = (torch.empty(nfl, dtype=torch.float32, device=qkv2d.device) if defer
                else workspace("sdpa_bias" + ws, nfl * 4, qkv2d.device))
    call("vit_sdpa_bwd", L.dt(qkv2d), B, H, N, 64, ptr(qkv2d), qkv2d.stride(0), ptr(o), o.stride(0), ptr(do),
         do.stride(0), ptr(lse), ptr(dqkv), dqkv.stride(0), ptr(delta), float(scale), int(causal),
         None if defer else ptr(dbias), ptr(part), nfl, _s(qkv2d))
    if defer:
        reduce_on.add(part, B, 3 * H * 64, dbias)
    return dqkv


# ----------------------------------------------------------------------------
# patch embed, CE, casts
# ----------------------------------------------------------------------------

def patch_unfold(img, ps, dtype, ld=None):
    """U [B*np, C*ps*ps]; with ``ld`` > C*ps*ps the rows are ``ld`` wide and the extra columns zero (a
    reduction padded to the GEMM tile depth, for padded weights from :func:`pad_cols`)."""
    B, C, Hi, Wi = img.shape
    assert img.dtype == torch.float32 and img.is_contiguous()
    npatch = (Hi // ps) * (Wi // ps)
    K = C * ps * ps
    U = torch.empty(B * npatch, max(K, ld or K), dtype=dtype, device=img.device)
    call("vit_patch_unfold_ld", L.dt(U), B, C, Hi, Wi, ps, U.shape[1], ptr(img), ptr(U), _s(img))
    return U


def pad_cols(w2d, ld, out=None):
    """[rows, cols] -> [rows, ld] with columns [cols, ld) zero (vit_copy_rows_padded); rows of any stride
    (ld == cols gathers strided rows, e.g. each image's class-token row, into a compact tensor)."""
    rows, cols = w2d.shape
    assert w2d.stride(1) == 1 and ld >= cols
    if out is None:
        out = torch.empty(rows, ld, dtype=w2d.dtype, device=w2d.device)
    assert out.shape == (rows, ld) and out.is_contiguous() and out.dtype == w2d.dtype
    call("vit_copy_rows_padded", L.dt(w2d), rows, cols, ptr(w2d), w2d.stride(0), ptr(out), ld, _s(w2d))
    return out


def patch_embed_fwd(U, w2d, bias, pos, cls, B, npatch):
    """x[b, 1 + p] = U[b*np + p] . w2d + bias + pos[1 + p]; U and w2d may both carry zero padding
    columns (same width)."""
    D, K = w2d.shape
    assert U.shape[1] == K and U.stride(1) == 1 and w2d.stride(1) == 1
    x = torch.empty(B, npatch + 1, D, dtype=torch.float32, device=U.device)
    call("vit_patch_embed_fwd_ld", L.dt(U), B, npatch, D, K, ptr(U), U.stride(0), ptr(w2d), w2d.stride(0),
         ptr(bias), ptr(pos), ptr(x), _s(U))
    call("vit_cls_pos_fill", B, npatch + 1, D, ptr(x), ptr(cls), ptr(pos), _s(U))
    return x


def pos_grad(dx, B, S, D, dpos, dcls):
    call("vit_pos_grad", B, S, D, ptr(dx), ptr(dpos), ptr(dcls), _s(dx))


def cross_entropy_fwd(logits, target):
    B, C = logits.shape
    assert logits.dtype == torch.float32 and target.dtype == torch.int64
    row_lse = torch.empty(B, dtype=torch.float32, device=logits.device)
    row_loss = torch.empty(B, dtype=torch.float32, device=logits.device)
    loss = torch.empty((), dtype=torch.float32, device=logits.device)
    call("vit_cross_entropy_fwd", B, C, ptr(logits), logits.stride(0), ptr(target), ptr(row_lse), ptr(row_loss),
         ptr(loss), _s(logits))
    return loss, row_lse


def cross_entropy_bwd(logits, target, row_lse, grad_loss, out_dtype=torch.float32):
    B, C = logits.shape
    d = torch.empty(B, C, dtype=out_dtype, device=logits.device)
    g = grad_loss.to(torch.float32).contiguous() if grad_loss is not None else None
    call("vit_cross_entropy_bwd", L.dt(d), B, C, ptr(logits), logits.stride(0), ptr(target), ptr(row_lse), ptr(g),
         ptr(d), d.stride(0), _s(logits))
    return d


def eval_metrics(logits, target, acc, topk=5, row_ws=None):
    """Add one batch's validation metrics into ``acc`` (f64 [6] on the device: mean loss, loss sum,
    top-1 hits, top-k hits, rows, batches); nothing is synchronised.  ``row_ws``: f32 scratch of
    >= 2 * B elements (taken from the allocator when absent)."""
    L.require_gpu(logits)
    B, C = logits.shape
    assert logits.dtype == torch.float32 and logits.stride(1) == 1 and target.dtype == torch.int64
    assert target.is_contiguous() and target.numel() == B and target.device == logits.device
    assert acc.dtype == torch.float64 and acc.numel() >= 6 and acc.is_contiguous() and acc.device == logits.device
    if row_ws is None:
        row_ws = torch.empty(2 * B, dtype=torch.float32, device=logits.device)
    assert row_ws.dtype == torch.float32 and row_ws.numel() >= 2 * B
    call("vit_eval_metrics", B, C, ptr(logits), logits.stride(0), ptr(target), int(topk), ptr(row_ws), ptr(acc),
         _s(logits))
    return acc


def cast_bf16(src: torch.Tensor, dst: torch.Tensor):
    assert src.dtype == torch.float32 and dst.dtype == torch.bfloat16 and src.numel() == dst.numel()
    call("vit_cast_f32_bf16", ptr(src), ptr(dst), src.numel(), _s(src))


def zero_(t: torch.Tensor):
    call("vit_zero", ptr(t), t.numel() * t.element_size(), _s(t))
    return t


# ----------------------------------------------------------------------------
# CLIP-HBA pieces (csrc/clip.hip)
# ----------------------------------------------------------------------------

def token_embed(tokens, table, pos):
    """x [S*L, D] f32 = table[tokens] + pos[t]  (tokens int64 [S, L])."""
    S, Lq = tokens.shape
    D = table.shape[1]
    x = torch.empty(S * Lq, D, dtype=torch.float32, device=table.device)
    call("vit_token_embed", S * Lq, Lq, D, table.shape[0], ptr(tokens.contiguous()), ptr(table), ptr(pos), ptr(x),
         _s(table))
    return x


def gather_rows(src2d, idx, out=None):
    n = idx.numel()
    D = src2d.shape[1]
    if out is None:
        out = torch.empty(n, D, dtype=torch.float32, device=src2d.device)
    call("vit_gather_rows", n, D, ptr(src2d), src2d.stride(0), ptr(idx), ptr(out), out.stride(0), _s(src2d))
    return out


def scatter_rows(src2d, idx, dst2d):
    n = idx.numel()
    call("vit_scatter_rows", n, src2d.shape[1], ptr(src2d), src2d.stride(0), ptr(idx), ptr(dst2d), dst2d.stride(0),
         _s(src2d))
    return dst2d


def check_block_indices(idx, rows: int):
    """The host-side guard of :func:`gather_blocks`: int64, one-dimensional, every entry in [0, rows)."""
    if idx.dtype != torch.int64 or idx.dim() != 1:
        raise TypeError(f"gather_blocks: idx must be a 1-D int64 tensor, got {idx.dtype} {tuple(idx.shape)}")
    if idx.numel():
        lo, hi = int(idx.min()), int(idx.max())
        if lo < 0 or hi >= rows:
            raise IndexError(f"gather_blocks: index {lo if lo < 0 else hi} is out of range for {rows} rows")


def gather_blocks(src3d, idx, out=None):
    """out[i] = src3d[idx[i]] for whole [N, W] token blocks (f32, contiguous, N * W a multiple of 4):
    ``torch.index_select(src3d, 0, idx)`` with the grid spread over each block, not one wave per row.

    ``idx`` is checked on the host before anything is queued (``IndexError``, nothing launched).  Pass
    the batch order as the CPU tensor it already is: the check then costs no synchronisation; a device
    ``idx`` is read back for it."""
    L.require_gpu(src3d)
    if src3d.dim() != 3 or src3d.dtype != torch.float32 or not src3d.is_contiguous():
        raise ValueError(f"gather_blocks: src must be a contiguous f32 [n, N, W] tensor, got {src3d.dtype} "
                         f"{tuple(src3d.shape)} strides {src3d.stride()}")
    rows, N, W = src3d.shape
    if (N * W) % 4 or src3d.data_ptr() % 16:
        raise ValueError(f"gather_blocks: blocks of {N * W} floats at {src3d.data_ptr():#x} are not 16-byte vectors")
    check_block_indices(idx, rows)
    n = idx.numel()
    if out is None:
        out = torch.empty(n, N, W, dtype=torch.float32, device=src3d.device)
    elif (out.shape != (n, N, W) or out.dtype != torch.float32 or out.device != src3d.device
          or not out.is_contiguous() or out.data_ptr() % 16):
        raise ValueError(f"gather_blocks: out must be a contiguous, 16-byte aligned f32 {(n, N, W)} tensor on "
                         f"{src3d.device}")
    if n == 0:
        return out
    didx = idx.to(src3d.device).contiguous()
    call("vit_gather_blocks", n, N * W, ptr(src3d), ptr(didx), ptr(out), _s(src3d))
    return out


def rownorm_fwd(x2d, log_scale=None):
    n, D = x2d.shape
    y = torch.empty_like(x2d)
    rn = torch.empty(n, dtype=torch.float32, device=x2d.device)
    call("vit_rownorm_fwd", n, D, ptr(x2d), ptr(log_scale), ptr(y), ptr(rn), _s(x2d))
    return y, rn


def rownorm_bwd(x2d, dy, rn, log_scale=None):
    n, D = x2d.shape
    dx = torch.empty_like(x2d)
    call("vit_rownorm_bwd", n, D, ptr(x2d), ptr(dy.contiguous()), ptr(rn), ptr(log_scale), ptr(dx), _s(x2d))
    return dx


def mse_fwd(pred, target):
    loss = torch.empty((), dtype=torch.float32, device=pred.device)
    call("vit_mse_fwd", pred.numel(), ptr(pred), ptr(target), ptr(loss), _s(pred))
    return loss


def mse_bwd(pred, target, grad_loss=None):
    d = torch.empty_like(pred)
    g = grad_loss.to(torch.float32).contiguous() if grad_loss is not None else None
    call("vit_mse_bwd", pred.numel(), ptr(pred), ptr(target), ptr(g), ptr(d), _s(pred))
    return d


_F32_MATMUL = ("highest", "high")  # vit_gemm_f32_precision 0 / 1


def set_float32_matmul_precision(precision, presplit_weights=False, presplit_activations=False):
    """The arithmetic of the fp32 MFMA GEMMs (``compute_dtype=torch.float32``), after
    ``torch.set_float32_matmul_precision``:

    - ``"highest"`` (the default): ``v_mfma_f32_16x16x4_f32``, exact f32 products;
    - ``"high"``: each f32 operand as the sum of two bfloat16 (``hi = bf16(x)``, ``lo = bf16(x - hi)``) and
      three bf16 MFMA products with f32 accumulation: about 4.4e-6 rms relative error on random data, tested to
      ``|C - C64| <= (3 * 2^-18 + (R + 3) * 2^-24) |P||Q|^T``; exact when both operands hold bf16 values.
      At most bf16x3: GEMMs too small or misaligned for the MFMA path stay exact f32.  An infinite operand
      gives NaN where ``"highest"`` gives an infinity.

    ``"medium"`` is refused: operands rounded to one bfloat16 are ``compute_dtype=torch.bfloat16``.  The
    setting is process-wide and read when a GEMM is launched, so a backward pass runs in the mode current
    when it runs, not the one its forward ran in; cached frozen-prefix tensors carry the mode in their keys and
    are rebuilt after a switch.  The environment variable ``VIT_F32_MATMUL=high`` sets the initial value when
    the library loads (spawned workers inherit it).  bf16 models, attention, LayerNorm and everything else
    are untouched.  Host-only: works without a GPU.

    ``presplit_weights=True`` (with ``"high"`` only; with ``"highest"`` it raises ``ValueError`` and changes
    nothing) keeps, for every registered fp32 GEMM weight parameter, a pre-split ``hi`` / ``lo``
    image in the layout the kernels' fragment reads expect (:func:`weight_image`), built on first use and rebuilt
    when the parameter's version, address, shape or device changes.  The forward and input-gradient GEMMs then
    read the image and split only their activation operand: the same MFMAs on the same bits, so results, and
    every cache key, are those of ``"high"``.  It costs 4 bytes per covered weight element, twice that for
    weights whose input gradient runs (about 1.2 GB for the ViT-L/14 visual tower): :func:`weight_image_bytes`.
    Computed weights (DoRA / LoRA ``out_proj.weight``), weight gradients and the patch embedding keep the
    in-loop split.  Both switches are set on every call, so a call without the keyword switches pre-splitting
    off (the images are freed at the model's next forward); :func:`get_float32_matmul_presplit` reads it and
    ``VIT_F32_MATMUL_PRESPLIT=1`` beside ``VIT_F32_MATMUL=high`` sets the initial value.

    ``presplit_activations=True`` (with ``"high"`` and ``presplit_weights=True`` only; anything else raises
    ``ValueError`` and changes nothing): in forward-only fp32 blocks on the dense chain, the
    LayerNorms write ``h1`` / ``h2`` and fc1's epilogue writes ``act`` as pre-split images, byte for byte in place of
    the f32 tensors, and the qkv / fc1 / fc2 GEMMs read both operands as images: no split is left in their k-steps.
    The same MFMAs on the same bits again, so results and cache keys stay those of ``"high"``.  Training blocks,
    the class-token / EOT tails, proj, computed weights and GEMMs off the MFMA path run as without the switch.
    All three switches are set on every call; :func:`get_float32_matmul_presplit_activations` reads this one and
    ``VIT_F32_MATMUL_PRESPLIT_ACT=1`` beside the other two variables sets its initial value."""
    if precision == "medium":
        raise ValueError('float32 matmul precision "medium" (operands rounded to one bfloat16) is not a mode of '
                         'the fp32 path: build the model with compute_dtype=torch.bfloat16')
    if precision not in _F32_MATMUL:
        raise ValueError(f'float32 matmul precision must be "highest" or "high", got {precision!r}')
    if presplit_weights and precision != "high":
        raise ValueError('presplit_weights=True keeps hi / lo images of the weights for the three bf16 products: it '
                         'needs precision "high"')
    if presplit_activations and not presplit_weights:
        raise ValueError('presplit_activations=True runs the GEMMs whose two operands are both pre-split images: it '
                         'needs precision "high" and presplit_weights=True')
    L.lib().vit_gemm_f32_precision(_F32_MATMUL.index(precision))
    _F32_PRESPLIT[0] = bool(presplit_weights)
    _F32_PRESPLIT_ACT[0] = bool(presplit_activations)


def get_float32_matmul_precision() -> str:
    """``"highest"`` or ``"high"``: see :func:`set_float32_matmul_precision`."""
    return _F32_MATMUL[L.lib().vit_gemm_f32_precision(-1)]


_F32_PRESPLIT = [os.environ.get("VIT_F32_MATMUL_PRESPLIT", "") == "1"]


def get_float32_matmul_presplit() -> bool:
    """Whether the fp32 "high" GEMMs read pre-split weight images: both switches of
    :func:`set_float32_matmul_precision` are on.  (``VIT_F32_MATMUL_PRESPLIT=1`` without ``VIT_F32_MATMUL=high``
    leaves this ``False``.)"""
    return bool(_F32_PRESPLIT[0] and L.lib().vit_gemm_f32_precision(-1) == 1)


_F32_PRESPLIT_ACT = [os.environ.get("VIT_F32_MATMUL_PRESPLIT_ACT", "") == "1"]


def get_float32_matmul_presplit_activations() -> bool:
    """Whether forward-only fp32 blocks hand pre-split activation images from producer to GEMM: all three switches
    of :func:`set_float32_matmul_precision` are on.  (``VIT_F32_MATMUL_PRESPLIT_ACT=1`` without the other two
    variables leaves this ``False``.)"""
    return bool(_F32_PRESPLIT_ACT[0] and get_float32_matmul_presplit())


def linear_fwd_takes_image(x2d, w, wimg) -> bool:
    """Whether ``linear_fwd(x2d, w, .., wimg=wimg)`` may be given ``x2d`` as a pre-split activation image: the switch
    is on, the weight has an image and the library says an f32 forward of this geometry takes the MFMA path
    (vit_linear_fwd_f32_mfma, host-only).  Ask before asking a producer for an image: the library refuses an image
    it has no kernel for."""
    if wimg is None or x2d.dtype != torch.float32 or not get_float32_matmul_presplit_activations():
        return False
    M, K = x2d.shape
    return bool(L.lib().vit_linear_fwd_f32_mfma(M, w.shape[0], K, ptr(x2d), x2d.stride(0), ptr(w)))


def layer_norm_writes_image(out, *others, add=False) -> bool:
    """Whether ``layer_norm_fwd`` (``add=False``) / ``add_layer_norm_fwd`` (``add=True``) can write ``out`` as a
    pre-split image, given every other 2-D tensor and vector of the call (vit_layer_norm_fwd_image_ok, host-only): f32
    throughout, D a multiple of 256 up to 2048 that the entry runs on its vector kernels, strides and addresses
    aligned.  Ask before asking the producer: the library refuses what it cannot write."""
    ts = [t for t in (out, *others) if t is not None]
    if not get_float32_matmul_presplit_activations() or any(t.dtype != torch.float32 for t in ts):
        return False
    strides = ptrs = 0
    for t in ts:
        ptrs |= t.data_ptr()
        if t.dim() == 2:
            if t.stride(1) != 1:
                return False
            strides |= t.stride(0)
    return bool(L.lib().vit_layer_norm_fwd_image_ok(int(add), out.shape[1], strides, ptrs))


def weight_image_raw(w, transposed=False, out=None):
    """The pre-split image of an f32 matrix ``w`` [N, K] (row stride ``w.stride(0)``) for the fp32 "high" GEMMs
    (vit_gemm_f32_weight_image): a contiguous f32-typed tensor of ``w``'s size holding, per 128-byte block of 32
    reduction values, four 16-byte ``hi`` chunks then four ``lo`` chunks of bf16.  ``transposed``: the image of
    ``w^T`` ([K, N] cells), the input gradient's operand."""
    L.require_gpu(w)
    N, K = w.shape
    assert w.dtype == torch.float32 and w.stride(1) == 1
    if out is None:
        out = torch.empty((K, N) if transposed else (N, K), dtype=torch.float32, device=w.device)
    call("vit_gemm_f32_weight_image", N, K, ptr(w), w.stride(0), int(transposed), ptr(out), _s(w))
    return out


def register_weight_image(p):
    """Mark a parameter as an fp32 GEMM weight that may hold pre-split images (the models' ``_ensure_shadows``)."""
    p._vit_wimg_ok = True


def drop_weight_images(params):
    for p in params:
        for name in ("_vit_wimg", "_vit_wimg_t"):
            if getattr(p, name, None) is not None:
                setattr(p, name, None)
                setattr(p, name + "_version", None)


def weight_image(p, dtype=torch.float32, transposed=False):
    """The current pre-split image of a registered fp32 weight parameter (``p._vit_wimg`` / ``p._vit_wimg_t`` with
    the version it was built from in ``..._version``), or None when pre-splitting is off, ``p`` is not a registered
    parameter (computed weights: the in-loop split), or its shape does not qualify.  Built on first use, rebuilt
    when ``p._version``, its address, shape or device changed.  Under graph capture a stale image is not rebuilt:
    the GEMM takes the in-loop split, the same bits."""
    if not _F32_PRESPLIT[0] or dtype != torch.float32 or not getattr(p, "_vit_wimg_ok", False):
        return None
    if not get_float32_matmul_presplit() or not p.is_cuda or p.dtype != torch.float32 or p.dim() != 2:
        return None
    name = "_vit_wimg_t" if transposed else "_vit_wimg"
    N, K = p.shape
    if (N if transposed else K) % 32 or not p.is_contiguous() or p.data_ptr() % 16:
        return None
    ver = (p._version, p.data_ptr(), tuple(p.shape), p.device)
    img = getattr(p, name, None)
    if img is not None and getattr(p, name + "_version", None) == ver:
        return img
    if torch.cuda.is_current_stream_capturing():
        return None
    # a fresh tensor, not the old image rewritten: the old one goes back to the allocator, which hands it out
    # again only behind the GEMMs already queued on this stream
    img = weight_image_raw(p.detach(), transposed)
    setattr(p, name, img)
    setattr(p, name + "_version", ver)
    return img


def weight_image_bytes(module_or_params) -> int:
    """Bytes held by the pre-split weight images of a module's (or an iterable of) parameters."""
    ps = module_or_params.parameters() if hasattr(module_or_params, "parameters") else module_or_params
    return sum(img.numel() * 4 for p in ps for img in (getattr(p, "_vit_wimg", None), getattr(p, "_vit_wimg_t", None))
               if img is not None)


_F32_ATTENTION = ("highest", "high")  # vit_sdpa_f32_precision 0 / 1


def set_float32_attention_precision(precision, long_sequences=False, presplit=False):
    """The arithmetic of the fp32 attention kernels (f32 operands, head_dim 64, aligned rows): the resident ones
    (up to 288 tokens, causal or not) and, with ``long_sequences=True``, the streamed ones past 288
    tokens (not causal):

    - ``"highest"`` (the default): ``v_mfma_f32_16x16x4_f32``, exact f32 products;
    - ``"high"``: every matrix product of the forward (``QK^T``, ``PV``) and the backward (``S``, ``dP``, ``dQ``,
      ``dK``, ``dV``) as three bf16 MFMA products of ``hi + lo`` operands with f32 accumulation, the rule of
      :func:`set_float32_matmul_precision`.  The softmax, ``delta``, ``lse``, the scale factors and the stores
      stay f32.  At most bf16x3: the generic and the one-query kernels and the class-token-only forward stay exact
      f32, and so do the streamed f32 kernels past 288 tokens unless ``long_sequences=True``.  An infinite operand
      gives NaN.

    ``long_sequences=True`` (with ``"high"`` only; with ``"highest"`` it raises ``ValueError`` and changes
    nothing) also runs streamed f32 attention -- 577 tokens for CLIP ViT-L/14@336px -- as three bf16 products, after
    ``set_attention_fp8(True, long_sequences=True)``.  All three switches are set on every call, so a call without a
    keyword switches that form off; :func:`get_float32_attention_long` reads this one.

    ``presplit=True`` (with ``"high"`` only; with ``"highest"`` it raises ``ValueError`` and changes nothing; DESIGN
    §4.27) carries pre-split images through attention in forward-only fp32 blocks on the dense chain, where the
    pre-split activation chain of :func:`set_float32_matmul_precision` runs: the qkv GEMM writes ``qkv`` as an image,
    the ``"high"`` forward kernels read K, V and Q from it and write ``o`` as one, and proj reads that -- no operand
    split is left in attention but P's, and none in proj.  The same MFMAs on the same bits, so results and cache keys
    stay those of ``"high"``.  Both ends or neither: a block whose qkv GEMM cannot write an image, whose attention
    geometry the image kernels do not cover (:func:`sdpa_fwd_takes_image`) or whose proj cannot read one runs the
    f32 calls.  Without ``set_float32_matmul_precision("high", presplit_weights=True, presplit_activations=True)``
    this switch has no effect: the image GEMM forms at both ends exist only on that path.
    :func:`get_float32_attention_presplit` reads it and ``VIT_F32_ATTENTION_PRESPLIT=1`` beside
    ``VIT_F32_ATTENTION=high`` sets its initial value.

    Independent of the GEMM switch: ``set_float32_matmul_precision("high")`` leaves attention exact, and this
    leaves the GEMMs exact.  Process-wide and read when a kernel is launched; cached frozen-prefix tensors carry the
    mode in their keys when it is ``"high"``.  ``VIT_F32_ATTENTION=high`` sets the initial value when the library
    loads and ``VIT_F32_ATTENTION_LONG=1`` that of the long form (spawned workers inherit them).  Host-only: works
    without a GPU."""
    if precision not in _F32_ATTENTION:
        raise ValueError(f'float32 attention precision must be "highest" or "high", got {precision!r}')
    if long_sequences and precision != "high":
        raise ValueError('long_sequences=True runs streamed fp32 attention as three bf16 products: it needs '
                         'precision "high"')
    if presplit and precision != "high":
        raise ValueError('presplit=True carries hi / lo images through the three-bf16-product attention kernels: it '
                         'needs precision "high"')
    L.lib().vit_sdpa_f32_precision(_F32_ATTENTION.index(precision))
    L.lib().vit_sdpa_f32_long_precision(1 if long_sequences else 0)
    _F32_ATTENTION_PRESPLIT[0] = bool(presplit)


def get_float32_attention_precision() -> str:
    """``"highest"`` or ``"high"``: see :func:`set_float32_attention_precision`."""
    return _F32_ATTENTION[L.lib().vit_sdpa_f32_precision(-1)]


def get_float32_attention_long() -> bool:
    """Whether streamed fp32 attention past 288 tokens runs as three bf16 products: both switches of
    :func:`set_float32_attention_precision` are on.  (``VIT_F32_ATTENTION_LONG=1`` without ``VIT_F32_ATTENTION=high``
    leaves the C switch set and this ``False``: the kernels stay exact.)"""
    lib = L.lib()
    return bool(lib.vit_sdpa_f32_precision(-1) == 1 and lib.vit_sdpa_f32_long_precision(-1) == 1)


_F32_ATTENTION_PRESPLIT = [os.environ.get("VIT_F32_ATTENTION_PRESPLIT", "") == "1"]


def get_float32_attention_presplit() -> bool:
    """Whether forward-only fp32 blocks carry pre-split images through attention: ``presplit=True`` of
    :func:`set_float32_attention_precision` while the mode is ``"high"``.  (``VIT_F32_ATTENTION_PRESPLIT=1`` without
    ``VIT_F32_ATTENTION=high`` leaves this ``False``.)"""
    return bool(_F32_ATTENTION_PRESPLIT[0] and L.lib().vit_sdpa_f32_precision(-1) == 1)


def sdpa_fwd_takes_image(qkv2d, B, H, N, o, lse=None, causal=False) -> bool:
    """Whether ``sdpa_fwd(qkv2d, B, H, N, o=o, lse=lse, causal=causal, image=True)`` has a kernel
    (vit_sdpa_fwd_takes_image, host-only): f32 tensors whose call would take the fp32 ``"high"`` kernels -- the mode,
    head_dim 64, row pitches that are multiples of 4 floats, 16-byte aligned ``qkv2d`` and ``o`` (``lse`` may sit
    anywhere), up to 288 tokens or, not causal, past them with ``long_sequences=True``.  Ask before asking the qkv GEMM for an image: the library refuses
    an image it has no kernel for."""
    if qkv2d.dtype != torch.float32 or o.dtype != torch.float32 or qkv2d.stride(1) != 1 or o.stride(1) != 1:
        return False
    ptrs = qkv2d.data_ptr() | o.data_ptr()
    return bool(L.lib().vit_sdpa_fwd_takes_image(B, H, N, 64, int(causal), qkv2d.stride(0) | o.stride(0), ptrs))


def gemm(P, p_layout, Q, q_layout, M, N, R, out=None, out_dtype=torch.float32, bias=None):
    """Raw C[i][j] = sum_r P(i,r) Q(j,r) (+bias[j]); layouts L.LAY_RC (r contiguous) / L.LAY_CR."""
    assert P.dtype == Q.dtype and P.stride(-1) == 1 and Q.stride(-1) == 1
    if (out is None and bias is None and P.dtype == torch.float32 and out_dtype == torch.float32
            and R >= 256 and ((M + 31) // 32) * ((N + 31) // 32) < 128):
        # few output tiles over a long reduction: split it (vit_gemm_splitk, slab sum in a fixed order)
        out = torch.empty(M, N, dtype=torch.float32, device=P.device)
        ws = workspace(f"gemm_splitk:{_s(P)}", 2 * 256 * 1024 * 4, P.device).view(torch.float32)
        call("vit_gemm_splitk", p_layout, q_layout, M, N, R, ptr(P), P.stride(0), ptr(Q), Q.stride(0), ptr(out),
             ptr(ws), ws.numel(), _s(P))
        return out
    if out is None:
        out = torch.empty(M, N, dtype=out_dtype, device=P.device)
    if P.dtype == torch.float32:
        _streamk(P.device)
    call("vit_gemm", L.dt(P), L.dt(out), p_layout, q_layout, L.EPI_STORE, M, N, R, ptr(P), P.stride(0), ptr(Q),
         Q.stride(0), ptr(out), out.stride(0), ptr(bias), None, 0, None, 1, _s(P))
    return out
