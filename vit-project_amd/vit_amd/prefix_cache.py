"""The frozen visual blocks' output, kept across the steps of a CLIP-HBA sweep.

The reference's datasets apply ``Resize``, ``ToTensor`` and ``Normalize`` and nothing random, and
``switch_dora_layers`` freezes everything in front of the DoRA blocks: the visual stem and the frozen
blocks map an image to the same tokens in every step, epoch and condition.  ``VisualPrefixCache`` runs
``CLIP.visual_prefix`` once over a fixed image set, keeps the f32 residual stream ``[n, N, W]`` on the
device, and hands a batch's rows to ``CLIPHBA.forward(visual_prefix=...)`` through one HIP gather
(``ops.gather_blocks``).  Opt-in: nothing here runs unless a caller builds a cache.

The key follows ``CLIP._text_prefix``: ``(data_ptr, _version)`` of the stem's and the frozen blocks'
parameters, the cut, the compute dtype, the fp8-attention switch, ``pos_embedding``, the images'
``(data_ptr, _version, shape)`` and the streamed-fp8 switch (``long_sequences``).  Under
``set_float32_matmul_precision("high")`` the compute-dtype element is the pair ``(compute_dtype, "high")``: rows
built in one fp32 GEMM mode are rebuilt in the other, never read, and the key's length, its last element and
its default-mode value stay what they were; under ``set_float32_attention_precision("high")`` it is the triple
``(compute_dtype, gemm mode, "attention-high")``, for the same reason, and with ``long_sequences=True``
(streamed fp32 attention as three bf16 products) ``(compute_dtype, gemm mode, "attention-high-long")``.  The cache holds references to those tensors, so an address in the key
cannot come back as another tensor while the cache lives.  ``valid_for`` recomputes the key; a stale
cache is rebuilt by ``ensure`` (the sweep calls it before every condition), never read.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib as L
from . import ops


def _hba(model):
    """The CLIPHBA behind ``model`` (a DataParallel wrapper is looked through), or ValueError."""
    from .clip import CLIP, CLIPHBA
    m = model.module if isinstance(model, nn.DataParallel) else model
    if not isinstance(m, CLIPHBA) or not isinstance(m.clip_model, CLIP):
        raise ValueError(f"the visual prefix cache needs a vit_amd.CLIPHBA model, got {type(m).__name__}")
    return m


def frozen_visual_blocks(model) -> int:
    """The number of frozen blocks in front of the first trainable visual block; ValueError when there
    is none (or ``model`` is no CLIPHBA): such a model has nothing to cache."""
    from .clip import _first_trainable
    first = _first_trainable(list(_hba(model).clip_model.visual.transformer.resblocks))
    if first == 0:
        raise ValueError("the visual prefix cache needs at least one frozen visual block in front of the "
                         "trainable ones; this model's first visual block is trainable")
    return first


def _frozen_tensors(cm, first):
    v = cm.visual
    stem = [v.conv1.weight, v.class_embedding, v.positional_embedding, v.ln_pre.weight, v.ln_pre.bias]
    return stem + [p for b in list(v.transformer.resblocks)[:first] for p in b.parameters()]


def compute_key(cm):
    """The arithmetic the cached rows were computed in: the compute dtype, paired with the fp32 GEMM mode when
    that is not the default ``"highest"`` (``ops.set_float32_matmul_precision``), and with both modes when the
    fp32 attention mode is not (``ops.set_float32_attention_precision``): ``(dtype, gemm mode, "attention-high")``,
    or ``"attention-high-long"`` when its ``long_sequences`` switch is on as well."""
    mode = ops.get_float32_matmul_precision()
    attn = ops.get_float32_attention_precision()
    if attn != "highest":
        return (cm.compute_dtype, mode, "attention-" + attn + ("-long" if ops.get_float32_attention_long() else ""))
    return cm.compute_dtype if mode == "highest" else (cm.compute_dtype, mode)


def prefix_key(model, images):
    """What the cached tokens depend on, as a hashable tuple (see the module docstring)."""
    m = _hba(model)
    cm = m.clip_model
    first = frozen_visual_blocks(m)
    return (tuple((p.data_ptr(), p._version) for p in _frozen_tensors(cm, first)), first, compute_key(cm),
            bool(cm.attention_fp8), bool(m.pos_embedding), (images.data_ptr(), images._version, tuple(images.shape)),
            bool(cm.attention_fp8_long))


class VisualPrefixCache:
    """``visual_prefix`` of a fixed image set, row ``i`` for image ``i``.

    ``hits``: batches served by :meth:`take`; ``bypassed``: batches a caller sent down the uncached path
    although a cache existed (perturbed images, :meth:`bypass`); ``builds``: times the rows were computed."""

    def __init__(self):
        self.x = None
        self.key = None
        self.first = 0
        self._held = ()
        self.hits = self.bypassed = self.builds = 0

    @classmethod
    def build(cls, model, images, batch_size=64, max_bytes=None):
        """Run ``visual_prefix`` over ``images`` in order, ``batch_size`` at a time, into one
        ``[n, N, W]`` f32 tensor on the model's device.  ``MemoryError`` before anything is allocated
        when that tensor exceeds ``max_bytes`` (default: a quarter of the device's memory)."""
        self = cls()
        self._fill(model, images, batch_size, max_bytes)
        return self

    def _fill(self, model, images, batch_size, max_bytes):
        m = _hba(model)
        cm = m.clip_model
        first = frozen_visual_blocks(m)
        v = cm.visual
        n, N, W = images.shape[0], (v.input_resolution // v.patch_size) ** 2 + 1, v.conv1.out_channels
        dev = cm.logit_scale.device
        nbytes = n * N * W * 4
        if max_bytes is None:
            L.require_gpu(cm.logit_scale)
            max_bytes = torch.cuda.get_device_properties(dev).total_memory // 4
        if nbytes > max_bytes:
            raise MemoryError(f"visual prefix cache: {n} x [{N}, {W}] f32 rows are {nbytes} bytes, over max_bytes = "
                              f"{max_bytes}")
        if batch_size < 1:
            raise ValueError(f"batch_size {batch_size}")
        L.require_gpu(cm.logit_scale)
        L.require_gpu(images)
        self.x = self.key = None  # release the old rows (and what they were made from) before the new ones
        self._held = ()
        # (the frozen blocks have no train-mode behaviour: the modules' modes are left as they are)
        x = torch.empty(n, N, W, dtype=torch.float32, device=dev)
        for i in range(0, n, batch_size):
            xi, k = cm.visual_prefix(images[i:i + batch_size], m.pos_embedding)
            assert k == first
            x[i:i + xi.shape[0]].copy_(xi)
        self.x, self.first = x, first
        self.key = prefix_key(m, images)
        self._held = (tuple(_frozen_tensors(cm, first)), images)
        self.builds += 1

    def valid_for(self, model, images) -> bool:
        return self.key is not None and self.key == prefix_key(model, images)

    def ensure(self, model, images, batch_size=64, max_bytes=None) -> bool:
        """Rebuild if the key no longer matches ``model`` and ``images``; True when it did rebuild."""
        if self.valid_for(model, images):
            return False
        self._fill(model, images, batch_size, max_bytes)
        return True

    def take(self, idx):
        """Rows ``idx`` (1-D int64, the batch order as the CPU tensor it is) as a new ``[len(idx), N, W]``
        tensor: the ``visual_prefix`` argument of ``CLIPHBA.forward``."""
        if self.x is None:
            raise RuntimeError("the visual prefix cache has not been built")
        out = ops.gather_blocks(self.x, idx)
        self.hits += 1
        return out

    def bypass(self):
        """Count a batch that took the uncached path (its images were perturbed)."""
        self.bypassed += 1

    @property
    def nbytes(self) -> int:
        return 0 if self.x is None else self.x.numel() * 4
