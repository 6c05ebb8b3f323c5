"""GPU: on-device validation metrics (vit_eval_metrics, EvalMeter, validate) against a float64 CPU
reference.  Counts must match exactly; losses within the 1e-5 relative bound test_cross_entropy applies
to vit_cross_entropy_fwd (fp32 exp / log of O(1) row sums)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from vit_amd import _lib as L  # noqa: E402
from vit_amd import ops  # noqa: E402

DEV = "cuda"
PAD = 1e30  # in the row padding: a read past C would swamp the log-sum-exp and outrank every class


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    L.load()


def _ref(logits, target, topk):
    """float64: row losses and the rank rule (larger logit, or equal logit at a smaller index)."""
    x = logits.astype(np.float64)
    B, C = x.shape
    m = x.max(axis=1, keepdims=True)
    lse = (m + np.log(np.exp(x - m).sum(axis=1, keepdims=True)))[:, 0]
    xt = x[np.arange(B), target]
    idx = np.arange(C)[None, :]
    rank = ((x > xt[:, None]) | ((x == xt[:, None]) & (idx < target[:, None]))).sum(axis=1)
    assert np.array_equal(rank == 0, np.argmax(x, axis=1) == target)  # np.argmax: the first maximum
    return lse - xt, int((rank == 0).sum()), int((rank < topk).sum())


def _strided(logits_np):
    """The logits in a device buffer with ld = C + 8, padding set to PAD."""
    B, C = logits_np.shape
    buf = torch.full((B, C + 8), PAD, dtype=torch.float32, device=DEV)
    buf[:, :C] = torch.from_numpy(logits_np).to(DEV)
    return buf[:, :C]


def _data(B, C, seed):
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((B, C)) * 3.0).astype(np.float32)
    target = rng.integers(0, C, size=B).astype(np.int64)
    # make about a third of the rows top-1 hits so the counts are not trivially small
    for r in range(0, B, 3):
        target[r] = int(np.argmax(logits[r]))
    return logits, target


def _run(logits_np, target_np, topk=5):
    acc = ops.zero_(torch.empty(6, dtype=torch.float64, device=DEV))
    ops.eval_metrics(_strided(logits_np), torch.from_numpy(target_np).to(DEV), acc, topk)
    return acc.cpu()


@pytest.mark.parametrize("B,C", [(37, 1000), (130, 1000), (1, 10), (5, 3)])
def test_eval_metrics_match_float64_reference(B, C):
    logits, target = _data(B, C, seed=B * 7 + C)
    rows, top1, top5 = _ref(logits, target, 5)
    if C < 5:
        assert top5 == B  # topk > C: every row counts
    acc = _run(logits, target)
    print(f"B={B} C={C}: mean {acc[0].item():.9f} ref {rows.mean():.9f}; sum {acc[1].item():.9f} "
          f"ref {rows.sum():.9f}; top1 {acc[2].item()} ref {top1}; top5 {acc[3].item()} ref {top5}")
    assert acc[2].item() == top1 and acc[3].item() == top5
    assert acc[4].item() == B and acc[5].item() == 1
    assert abs(acc[0].item() - rows.mean()) <= 1e-5 * abs(rows.mean())
    assert abs(acc[1].item() - rows.sum()) <= 1e-5 * abs(rows.sum())


def test_eval_metrics_ties_take_the_first_maximum():
    rng = np.random.default_rng(0)
    logits = rng.standard_normal((2, 10)).astype(np.float32)
    logits[:, 3] = logits[:, 7] = 9.0  # the row maximum, twice
    target = np.array([3, 7], dtype=np.int64)
    rows, top1, top5 = _ref(logits, target, 5)
    assert (top1, top5) == (1, 2)
    acc = _run(logits, target)
    assert acc[2].item() == 1 and acc[3].item() == 2  # target 3: top-1; target 7: rank 1, top-5 only
    only7 = _run(logits[1:], target[1:])
    assert only7[2].item() == 0 and only7[3].item() == 1


def test_eval_meter_accumulates_and_is_bitwise_reproducible():
    import vit_amd
    C = 1000
    batches = [_data(b, C, seed=40 + i) for i, b in enumerate((4, 4, 3))]
    refs = [_ref(lg, tg, 5) for lg, tg in batches]

    def run():
        meter = vit_amd.EvalMeter(DEV, topk=5)
        for lg, tg in batches:
            meter.update(_strided(lg), torch.from_numpy(tg).to(DEV))
        return meter.acc.clone().cpu(), meter.result()

    acc_a, res = run()
    acc_b, _ = run()
    assert torch.equal(acc_a, acc_b)  # fixed-order sums: the same bits on every run
    assert res["batches"] == 3 and res["total"] == 11
    assert res["correct"] == sum(r[1] for r in refs)
    mean_of_means = float(np.mean([r[0].mean() for r in refs]))
    assert abs(res["loss"] - mean_of_means) <= 1e-5 * abs(mean_of_means)
    assert res["acc1"] == 100.0 * sum(r[1] for r in refs) / 11
    assert res["acc5"] == 100.0 * sum(r[2] for r in refs) / 11
    meter = vit_amd.EvalMeter(DEV)
    meter.update(_strided(batches[0][0]), torch.from_numpy(batches[0][1]).to(DEV))
    assert meter.reset().result()["batches"] == 0


def test_validate_matches_reference_loop():
    """vit_amd.validate against VIT:167-204 restated with model(x), F.cross_entropy and max(1)."""
    import vit_amd
    torch.manual_seed(11)
    model = vit_amd.VisionTransformer(img_size=64, patch_size=16, embed_dim=256, depth=2, num_heads=4, num_classes=10,
                                      compute_dtype=torch.bfloat16).cuda()
    g = torch.Generator().manual_seed(12)
    loader = [(torch.randn(b, 3, 64, 64, generator=g), torch.randint(0, 10, (b,), generator=g)) for b in (4, 4, 3)]
    model.train()
    loss, acc = vit_amd.validate(model, loader)
    assert not model.training  # left in eval mode, as the reference leaves it

    correct = total = num_batches = 0
    val_loss = 0.0
    with torch.no_grad():
        for images, targets in loader:
            images, targets = images.cuda(), targets.cuda()
            outputs = model(images)
            val_loss += torch.nn.functional.cross_entropy(outputs, targets).item()
            num_batches += 1
            _, predicted = outputs.max(1)
            total += targets.size(0)
            correct += predicted.eq(targets).sum().item()
    ref_loss, ref_acc = val_loss / num_batches, 100.0 * correct / total
    assert acc == ref_acc
    assert abs(loss - ref_loss) <= 1e-5 * abs(ref_loss), (loss, ref_loss)
