"""CPU: host logic of the forward-only path and of validate() -- the routing rule, its switch, the
metrics all-reduce (gloo, world_size 2) and the header declarations."""
import os
import re
import socket
import subprocess
import sys

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_routing_predicate_truth_table():
    from vit_amd.model import wants_forward_only as w
    for x_rg in (False, True):
        for p_rg in (False, True):
            # autograd off: always forward-only; switch off: never
            assert w(True, False, x_rg, p_rg) is True
            assert w(False, False, x_rg, p_rg) is False
            assert w(False, True, x_rg, p_rg) is False
    # autograd on: only when neither the input nor a parameter wants a gradient
    assert w(True, True, False, False) is True
    assert w(True, True, True, False) is False   # frozen block behind a trainable one
    assert w(True, True, False, True) is False   # trainable block on a constant input
    assert w(True, True, True, True) is False


def test_set_forward_only_round_trip():
    import vit_amd
    from vit_amd import model
    start = model.forward_only_enabled()
    try:
        assert vit_amd.set_forward_only(False) is start
        assert model.forward_only_enabled() is False
        assert vit_amd.set_forward_only(True) is False
        assert model.forward_only_enabled() is True
        assert vit_amd.set_forward_only(True) is True
    finally:
        vit_amd.set_forward_only(start)
    assert model.forward_only_enabled() is start


def test_env_switch_sets_the_default():
    code = "from vit_amd import model; print(int(model.forward_only_enabled()))"
    path = os.pathsep.join([os.path.join(ROOT, "vit-project_amd")] + [p for p in sys.path if p])
    for val, want in ((None, "1"), ("1", "1"), ("0", "0")):
        env = {k: v for k, v in os.environ.items() if k != "VIT_FWD_ONLY"}
        env["PYTHONPATH"] = path
        if val is not None:
            env["VIT_FWD_ONLY"] = val
        out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True)
        assert out.stdout.strip() == want, (val, out.stdout, out.stderr)


def test_reduce_metrics_single_rank():
    from vit_amd.evaluate import reduce_metrics
    loss, acc = reduce_metrics(torch.tensor([0.75, 12.5, 8.0, 1.0], dtype=torch.float64))
    assert loss == 0.75 and acc == 12.5


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


# per rank: (avg_loss, total, correct); accuracy is what that rank alone would report
_RANKS = ((1.25, 40, 10), (0.5, 24, 18))


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    from vit_amd import parallel
    from vit_amd.evaluate import reduce_metrics
    parallel.init_from_env(backend="gloo")
    avg_loss, total, correct = _RANKS[rank]
    metrics = torch.tensor([avg_loss, 100.0 * correct / total, total, correct], dtype=torch.float64)
    q.put((rank,) + tuple(reduce_metrics(metrics, world)))
    dist.barrier()
    dist.destroy_process_group()


def test_reduce_metrics_world2():
    """VIT:193-199: the loss is the SUM of the ranks' average losses (not divided) and the accuracy comes
    from the summed counts, not from the ranks' accuracies."""
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want_loss = sum(r[0] for r in _RANKS)
    want_acc = 100.0 * sum(r[2] for r in _RANKS) / sum(r[1] for r in _RANKS)
    assert want_acc != sum(100.0 * r[2] / r[1] for r in _RANKS) / world  # not the mean of the rank accuracies
    for rank, loss, acc in res:
        assert loss == want_loss, (rank, loss)
        assert acc == want_acc, (rank, acc)


def test_act_only_gemm_instantiations_have_no_spills():
    """Every GEMM kernel instantiated for the act-only codes (template EPI 8 / 9, forward layout): no VGPR
    spill and no scratch, as their pair forms (tools/kres.sh on the built object)."""
    import pytest
    obj = os.path.join(ROOT, "vit-project_amd", "csrc", "build", "gemm.o")
    if not os.path.exists(obj) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("gemm.o not built / no ROCm LLVM tools")
    pat = r"Li0ELi0ELi[89]E|kernelILi(32|64)E(DF16b|f)Li[89]E"  # <PL, QL, EPI> = <RC, RC, 8|9>; gen: <TILE, T, EPI>
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kres.sh"), obj, pat], capture_output=True, text=True,
                         check=True).stdout.splitlines()
    assert len(out) >= 40, len(out)  # 2 codes x (10 bf16 configurations + 2 f32 MFMA + 8 generic)
    bad = [l for l in out if " spill 0 " not in l or " priv 0 " not in l]
    assert not bad, bad[:5]


def test_header_declares_the_new_surface():
    txt = open(os.path.join(ROOT, "include", "vit_hip.h")).read()
    assert re.search(r"\bVIT_EPI_BIAS_GELU_FWD\s*=\s*8\b", txt)
    assert re.search(r"\bVIT_EPI_BIAS_QGELU_FWD\s*=\s*9\b", txt)
    assert re.search(r"\bint\s+vit_eval_metrics\s*\(", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))
    from vit_amd import _lib
    assert (_lib.EPI_BIAS_GELU_FWD, _lib.EPI_BIAS_QGELU_FWD) == (8, 9)
    assert "vit_eval_metrics" in _lib.SIGNATURES
    # the library's own selector: 7 stays the internal accumulate code, 8 / 9 are the act-only forms
    epi = open(os.path.join(ROOT, "vit-project_amd", "csrc", "gemm_epi.hpp")).read()
    assert re.search(r"EPI_ACC\s*=\s*7\b", epi) and re.search(r"EPI_BIAS_GELU_FWD\s*=\s*8\b", epi)
    assert re.search(r"EPI_BIAS_QGELU_FWD\s*=\s*9\b", epi)
