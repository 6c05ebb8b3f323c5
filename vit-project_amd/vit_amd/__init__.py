"""vit_amd: MI355X-native (gfx950) ViT training step behind the timm / DoRA surface.

Compute runs only in ``lib/libvit_hip.so`` (C-ABI, include/vit_hip.h); this
package is the host-side mirror of the reference's module/optimizer interface.
"""
from . import _lib
from .model import (VisionTransformer, create_model, cross_entropy, set_wgrad_overlap, set_forward_only,
                    set_cls_tail, block_forward_only)
from .pos_embed import resample_abs_pos_embed, adapt_state_dict
from .optim import FusedSGD, FusedAdamW, CosineAnnealingLRWithWarmup
from .dora import DoRALayer, dora_weight
from .lora import LoRALayer, lora_weight
from .ops import set_float32_matmul_precision, get_float32_matmul_precision
from .ops import get_float32_matmul_presplit, get_float32_matmul_presplit_activations, weight_image_bytes
from .ops import set_float32_attention_precision, get_float32_attention_precision, get_float32_attention_long
from .ops import get_float32_attention_presplit
from . import rsa
from . import clip
from . import prefix_cache
from .prefix_cache import VisualPrefixCache
from . import sweep
from . import data
from . import evaluate
from .evaluate import EvalMeter, validate
from .clip import CLIPHBA, MSELoss, mse_loss, apply_dora_to_ViT, switch_dora_layers, count_trainable_parameters
from .clip import apply_lora_to_ViT, unfreeze_lora_layers

__all__ = ["VisionTransformer", "create_model", "cross_entropy", "set_wgrad_overlap", "FusedSGD", "FusedAdamW",
           "CosineAnnealingLRWithWarmup", "DoRALayer", "dora_weight", "rsa", "clip", "data", "CLIPHBA", "MSELoss",
           "mse_loss", "apply_dora_to_ViT", "switch_dora_layers", "count_trainable_parameters", "set_forward_only",
           "set_cls_tail", "block_forward_only", "evaluate", "EvalMeter", "validate", "resample_abs_pos_embed", "adapt_state_dict",
           "prefix_cache", "VisualPrefixCache", "LoRALayer", "lora_weight", "apply_lora_to_ViT", "unfreeze_lora_layers",
           "set_float32_matmul_precision", "get_float32_matmul_precision", "set_float32_attention_precision",
           "get_float32_attention_precision", "get_float32_attention_long", "get_float32_matmul_presplit",
           "get_float32_matmul_presplit_activations", "weight_image_bytes", "get_float32_attention_presplit"]


def load_library(path=None):
    return _lib.load(path)
