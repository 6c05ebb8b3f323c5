"""Validation on the device: the reference's ``validate`` (VIT:167-204, duplicated at MEAS:262-296).

The reference reads ``loss.item()`` and ``predicted.eq(targets).sum().item()`` for every batch: one
host synchronisation per batch.  Here each batch's forward is the forward-only block chain
(``torch.no_grad()``: no act'(pre) tensor, act-only fc1 epilogue) and its loss / top-1 / top-k counts
are added into six f64 accumulators by ``vit_eval_metrics``; the host synchronises once, in
:meth:`EvalMeter.result`.
"""
from __future__ import annotations

import torch

from . import ops


class EvalMeter:
    """Accumulates cross-entropy loss and top-1 / top-k accuracy over batches without synchronising.

    ``update(logits, targets)`` only enqueues work on the current stream; ``result()`` performs the one
    synchronisation (the copy of six numbers to the host)."""

    def __init__(self, device, topk: int = 5):
        self.device = torch.device(device)
        self.topk = int(topk)
        self.acc = torch.empty(6, dtype=torch.float64, device=self.device)
        self._ws = None
        self.reset()

    def reset(self):
        ops.zero_(self.acc)
        return self

    def update(self, logits: torch.Tensor, targets: torch.Tensor):
        """logits [B, C] (f32, rows may be strided), targets [B] int64 in [0, C), both on the device."""
        if logits.dtype != torch.float32:
            logits = logits.float()
        if logits.dim() != 2 or logits.stride(1) != 1:
            logits = logits.reshape(logits.shape[0], -1).contiguous()
        targets = targets.to(device=logits.device, dtype=torch.int64).contiguous()
        B = logits.shape[0]
        # the scratch rows are reused by the next update: same stream, so the launches are ordered
        if self._ws is None or self._ws.numel() < 2 * B:
            self._ws = torch.empty(2 * B, dtype=torch.float32, device=logits.device)
        ops.eval_metrics(logits, targets, self.acc, self.topk, self._ws)
        return self

    def result(self) -> dict:
        """loss = mean of the batch means (VIT:191), acc1 / acc5 in percent (acc5: the meter's top-k),
        total, correct, batches.  The one host synchronisation."""
        mean_sum, _, c1, ck, total, batches = self.acc.tolist()
        total, batches = int(total), int(batches)
        return {
            "loss": mean_sum / batches if batches else float("nan"),
            "acc1": 100.0 * c1 / total if total else float("nan"),
            "acc5": 100.0 * ck / total if total else float("nan"),
            "total": total,
            "correct": int(c1),
            "batches": batches,
        }


def reduce_metrics(metrics: torch.Tensor, world_size: int = 1, group=None):
    """VIT:193-199 over ``metrics = [avg_loss, accuracy, total, correct]``: SUM-all-reduce across the
    ranks (in place) when ``world_size > 1``, then global_loss = metrics[0] -- the sum of the ranks'
    average losses, not divided, as the reference reports it -- and global_acc = 100 * correct / total
    from the summed counts.  Returns (global_loss, global_acc)."""
    if world_size > 1:
        import torch.distributed as dist
        dist.all_reduce(metrics, op=dist.ReduceOp.SUM, group=group)
    m = metrics.tolist()
    global_total, global_correct = int(m[2]), int(m[3])
    return m[0], 100.0 * global_correct / global_total


def validate(model, loader, local_rank=None, world_size: int = 1, group=None):
    """The reference's ``validate(model, val_loader, local_rank, world_size)`` -> (global_loss,
    global_acc): ``model.eval()`` (left in eval mode, as there), a no-grad forward per batch, the
    metrics on the device, one synchronisation at the end, then :func:`reduce_metrics`.  The metrics
    tensor is f64 (the reference's is f32: counts past 2^24 stay exact here)."""
    model.eval()
    dev = next(model.parameters()).device if local_rank is None else torch.device("cuda", local_rank)
    meter = EvalMeter(dev)
    with torch.no_grad():
        for images, targets in loader:
            images = images.to(dev, non_blocking=True)
            targets = targets.to(dev, non_blocking=True)
            meter.update(model(images), targets)
    r = meter.result()
    metrics = torch.tensor([r["loss"], r["acc1"], r["total"], r["correct"]], dtype=torch.float64, device=dev)
    return reduce_metrics(metrics, world_size, group)
