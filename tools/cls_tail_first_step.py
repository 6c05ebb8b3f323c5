"""bench.py's model and batch (same seeds, ViT-B/16, bs 256, bf16): the first step with the class-token tail off and on.

    python tools/cls_tail_first_step.py out.json

Prints and writes whether logits and loss are bitwise equal, and the largest gradient difference between the two
paths per parameter (relative to the parameter's largest gradient).  Needs the GPU."""
import os, sys, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vit-project_amd")]
import torch, vit_amd
dev = torch.device("cuda", 0)
torch.manual_seed(1234)
model = vit_amd.create_model("vit_base_patch16_224", num_classes=1000, compute_dtype=torch.bfloat16).to(dev)
x = torch.randn(256, 3, 224, 224, device=dev)
y = torch.randint(0, 1000, (256,), device=dev)
res = {}
for on in (False, True):
    vit_amd.set_cls_tail(on)
    for p in model.parameters():
        p.grad = None
    logits = model(x)
    loss = vit_amd.cross_entropy(logits, y)
    loss.backward()
    torch.cuda.synchronize()
    res[on] = (logits.detach().clone(), loss.detach().clone(), {k: p.grad.detach().clone() for k, p in model.named_parameters()})
out = {"logits_equal": bool(torch.equal(res[0][0], res[1][0])), "loss_equal": bool(torch.equal(res[0][1], res[1][1])),
       "loss": float(res[1][1])}
worst = {}
for k in res[0][2]:
    a, b = res[0][2][k].double(), res[1][2][k].double()
    worst[k] = float((a - b).abs().max() / (a.abs().max() + 1e-300))
unequal = [k for k in res[0][2] if not torch.equal(res[0][2][k], res[1][2][k])]
out["grads_bitwise_equal"] = not unequal
out["grads_not_equal"] = unequal
out["grad_max_rel_diff_tail_vs_dense"] = {"max": max(worst.values()), "argmax": max(worst, key=worst.get),
                                          "last_block_fc1_weight": worst["blocks.11.mlp.fc1.weight"],
                                          "block0_qkv_weight": worst["blocks.0.attn.qkv.weight"]}
print(json.dumps(out, indent=1))
json.dump(out, open(sys.argv[1], "w"), indent=1)
