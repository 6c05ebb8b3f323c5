"""Generate tests/golden/lora_golden.pt from the reference's own ``LoRALayer`` (NEWP:307-336).

Run where the reference tree is present (not on the GPU box):

    python tests/golden/make_lora_golden.py

The reference module is imported with the stub modules ``make_golden.py`` uses for the absent third-party
packages; only input / output vectors are stored, none of the reference's text.  Records:

  * ``"{n}x{n}r{r}"`` for (64, 8) and (96, 4): full tensors -- seed, W0, bias, A, B, scaling, gW, and the
    reference's ``.weight`` W with the autograd gradients dA, dB of ``(W * gW).sum()``;
  * the same keys for (1024, 32) and (768, 32) with the seed and summaries only (W_sum, W_abs, W_row0,
    gradient norms and slices): the inputs are regenerated from the seed, which also pins the RNG order
    (``randn`` for A, kaiming A, kaiming B, then ``randn`` for gW);
  * ``"forward"``: ``LoRALayer.forward`` on 96 -> 80, r = 8, in eval mode (x, gy, y, dx, dA, dB) and in train
    mode with the x-shaped dropout multiplier it drew (recovered by re-seeding; the generator asserts that the
    reference's output equals the multiplier restatement);
  * ``"state_dict_keys"`` of a reference layer and ``"clip_trainable"`` for ViT-L/14 with r = 32.
"""
from __future__ import annotations

import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import _stub_reference_imports  # noqa: E402

SEED0 = 4321


def weight_records(NEWP):
    out = {}
    for n, r in [(64, 8), (96, 4), (1024, 32), (768, 32)]:
        seed = SEED0 + n
        torch.manual_seed(seed)
        base = torch.nn.Linear(n, n)
        layer = NEWP.LoRALayer(base, r=r, lora_alpha=16, lora_dropout=0.1)
        W = layer.weight
        gW = torch.randn_like(W)
        (W * gW).sum().backward()
        dA, dB = layer.lora_A.grad, layer.lora_B.grad
        rec = {"n": n, "r": r, "scaling": layer.scaling, "seed": seed}
        if n <= 100:
            rec.update({"W0": base.weight.detach().clone(), "bias": base.bias.detach().clone(),
                        "A": layer.lora_A.detach().clone(), "B": layer.lora_B.detach().clone(), "gW": gW,
                        "W": W.detach().clone(), "dA": dA.clone(), "dB": dB.clone()})
        else:
            rec.update({"W_sum": float(W.double().sum()), "W_abs": float(W.double().abs().sum()),
                        "W_row0": W[0, :64].detach().clone(), "dA_norm": float(dA.norm()),
                        "dB_norm": float(dB.norm()), "dA_slice": dA[0, :64].clone(), "dB_slice": dB[0, :r].clone(),
                        "A_sum": float(layer.lora_A.double().sum()), "B_sum": float(layer.lora_B.double().sum())})
        out[f"{n}x{n}r{r}"] = rec
    return out


def forward_record(NEWP):
    torch.manual_seed(SEED0 + 7)
    base = torch.nn.Linear(96, 80)
    layer = NEWP.LoRALayer(base, r=8, lora_alpha=16, lora_dropout=0.1)
    try:
        layer.weight
        raise AssertionError("the reference's .weight is expected to fail for in != out")
    except RuntimeError:
        pass
    x0 = torch.randn(6, 96)
    gy = torch.randn(6, 80)
    rec = {"W0": base.weight.detach().clone(), "bias": base.bias.detach().clone(),
           "A": layer.lora_A.detach().clone(), "B": layer.lora_B.detach().clone(), "scaling": layer.scaling,
           "x": x0, "gy": gy, "state_dict_keys": list(layer.state_dict().keys())}
    for mode in ("eval", "train"):
        layer.train(mode == "train")
        layer.zero_grad()
        x = x0.clone().requires_grad_(True)
        torch.manual_seed(SEED0 + 8)
        y = layer(x)
        (y * gy).sum().backward()
        rec[mode] = {"y": y.detach().clone(), "dx": x.grad.clone(), "dA": layer.lora_A.grad.clone(),
                     "dB": layer.lora_B.grad.clone()}
        if mode == "train":
            torch.manual_seed(SEED0 + 8)
            mask = layer.lora_dropout(torch.ones_like(x0))
            with torch.no_grad():
                y2 = base(x0) + ((x0 * mask) @ layer.lora_B @ layer.lora_A) * layer.scaling
            assert torch.equal(y2, y.detach()), (y2 - y).abs().max()
            assert (mask == 0).any() and ((mask == 0) | (mask == mask.max())).all()
            rec[mode]["mask"] = mask
    return rec


def main():
    _stub_reference_imports()
    import functions.new_cvpr_train_behavior_things_pipeline as NEWP
    out = weight_records(NEWP)
    out["forward"] = forward_record(NEWP)
    out["clip_trainable"] = 2 * (2 * 32 * 1024) + 2 * 32 * 768
    path = os.path.join(HERE, "lora_golden.pt")
    torch.save(out, path)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
