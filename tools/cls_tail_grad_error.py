"""Per-parameter gradient error of the class-token tail and of the dense last block against the fp64 oracle.

    python tools/cls_tail_grad_error.py [out.json]

The models and inputs of tests/test_gpu_cls_tail.py (depth 2, D = 128, 2 heads, B = 3; N = 17 and 197; bf16
and f32).  At these shapes bitwise equality with the dense block is not promised (N = 17 keeps the dense
layout; at N = 197 the dense weight gradients take their ragged-row path, M % 32 != 0, and the tail's padded
ones do not), so the contract is the error bound: per parameter, max |got - ref| / max |ref| of the tail at most
2 x the dense block's + 2^-22, logits bit for bit equal.  (Measured, the two errors agree to the printed digits:
the reordered sums move less than the error both paths share.)  tools/cls_tail_first_step.py checks the
benchmark's shape, where every gradient is bitwise equal.  Needs the GPU."""
import json
import os
import sys
from collections import OrderedDict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vit-project_amd")]

import torch  # noqa: E402

import vit_amd  # noqa: E402
from oracle import vit_ref as R  # noqa: E402

B = 3


def run(cfg, p, x, y, dtype, tail):
    prev = vit_amd.set_cls_tail(tail)
    try:
        m = vit_amd.VisionTransformer(img_size=cfg.img_size, patch_size=cfg.patch_size, num_classes=cfg.num_classes,
                                      embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.num_heads,
                                      compute_dtype=dtype)
        m.load_state_dict(p)
        m = m.cuda()
        logits = m(x.cuda())
        vit_amd.cross_entropy(logits, y.cuda()).backward()
        torch.cuda.synchronize()
        return logits.detach().cpu(), OrderedDict((k, q.grad.double().cpu()) for k, q in m.named_parameters())
    finally:
        vit_amd.set_cls_tail(prev)


def main():
    out = {"error": "max|got - ref| / max|ref| per parameter, ref = oracle/vit_ref.py in fp64", "cases": []}
    for n, img in ((17, 64), (197, 224)):
        cfg = R.ViTConfig(img_size=img, patch_size=16, embed_dim=128, depth=2, num_heads=2, num_classes=10)
        p = R.init_params(cfg, seed=31 + n, random_affine=True)
        g = torch.Generator().manual_seed(32 + n)
        x = torch.randn(B, 3, img, img, generator=g)
        y = torch.randint(0, 10, (B,), generator=g)
        leaf = OrderedDict((k, v.double().requires_grad_(True)) for k, v in p.items())
        R.cross_entropy(R.forward(leaf, x.double(), cfg), y).backward()
        for dtype in (torch.bfloat16, torch.float32):
            l0, g0 = run(cfg, p, x, y, dtype, False)
            l1, g1 = run(cfg, p, x, y, dtype, True)
            params, worst = {}, 0.0
            for k, v in leaf.items():
                ref = v.grad
                s = ref.abs().max().item() + 1e-300
                e0, e1 = (g0[k] - ref).abs().max().item() / s, (g1[k] - ref).abs().max().item() / s
                params[k] = {"dense": e0, "tail": e1}
                worst = max(worst, e1 / (2 * e0 + 2.0 ** -22))
            out["cases"].append({"tokens": n, "batch": B, "dtype": str(dtype).replace("torch.", ""),
                                 "logits_equal": bool(torch.equal(l0, l1)),
                                 "worst_tail_over_bound": worst, "params": params})
            print(n, dtype, "logits equal", torch.equal(l0, l1), "worst tail / (2 dense + 2^-22)", round(worst, 4))
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r11", "cls_tail_grad_error.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
