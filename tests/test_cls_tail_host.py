"""CPU: host logic of the class-token tail -- the routing rule, its switch, and, with the launch layer
stubbed, the shapes each block's launches are issued at."""
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_routing_rule_truth_table():
    from vit_amd.model import wants_cls_tail as w
    assert w(True, True, "token") is True
    assert w(False, True, "token") is False       # switched off
    assert w(True, False, "token") is False       # forward_features(): every row is read
    assert w(True, True, "avg") is False          # another pooling reads every row
    assert w(True, True, "token", True) is False  # fp8 attention passes keep the dense block


def test_set_cls_tail_round_trip():
    import vit_amd
    from vit_amd import model
    start = model.cls_tail_enabled()
    try:
        assert vit_amd.set_cls_tail(False) is start
        assert model.cls_tail_enabled() is False
        assert vit_amd.set_cls_tail(True) is False
        assert model.cls_tail_enabled() is True
    finally:
        vit_amd.set_cls_tail(start)


def test_env_switch_sets_the_default():
    code = "from vit_amd import model; print(int(model.cls_tail_enabled()))"
    path = os.pathsep.join([os.path.join(ROOT, "vit-project_amd")] + [p for p in sys.path if p])
    for val, want in ((None, "1"), ("1", "1"), ("0", "0")):
        env = {k: v for k, v in os.environ.items() if k != "VIT_CLS_TAIL"}
        env["PYTHONPATH"] = path
        if val is not None:
            env["VIT_CLS_TAIL"] = val
        out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True)
        assert out.stdout.strip() == want, (val, out.stdout, out.stderr)


def test_header_declares_the_new_entry_points():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vit_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+vit_layer_norm_bwd_cls\s*\(", txt)
    assert re.search(r"\bint\s+vit_sdpa_fwd_cls\s*\(", txt) and re.search(r"\bint\s+vit_sdpa_cls_count\s*\(", txt)
    from vit_amd import _lib
    # the dense entry point's arguments with res_every after ldres
    dense, cls = _lib.SIGNATURES["vit_layer_norm_bwd"], _lib.SIGNATURES["vit_layer_norm_bwd_cls"]
    assert cls == dense[:13] + [_lib.i32] + dense[13:]
    assert _lib.load().vit_abi_version() == 10


class _NoSide:
    """The model's two-stream helper with no second stream (what it is on a device without one)."""
    on = False

    def __init__(self, dev):
        pass

    def run(self, fn):
        return fn()

    def join(self):
        pass

    def guard(self, *ts):
        pass


@pytest.fixture
def launches(monkeypatch):
    """Every kernel launch recorded as (entry point, arguments) instead of run; tensors live on the CPU."""
    from vit_amd import _lib, model, ops
    rec = []
    monkeypatch.setattr(ops, "call", lambda name, *a: rec.append((name, a)))
    monkeypatch.setattr(_lib, "call", lambda name, *a: rec.append((name, a)))
    monkeypatch.setattr(ops, "_streamk", lambda device, stream=None: None)  # (the f32 head's stream-K workspace)
    monkeypatch.setattr(_lib, "require_gpu", lambda t: None)
    monkeypatch.setattr(_lib, "stream_ptr", lambda device=None: 0)
    monkeypatch.setattr(model, "_Side", _NoSide)
    real = _lib.load()

    class Lib:  # the host-only queries answer; the one launch made through the handle is recorded
        def __getattr__(self, name):
            return getattr(real, name)

        def vit_linear_wgrad_partials2(self, *a):
            rec.append(("vit_linear_wgrad_partials2", a))
            return 0

    monkeypatch.setattr(_lib, "lib", lambda: Lib())
    return rec


B, N, D, F, DEPTH = 4, 65, 128, 512, 3  # 65 tokens: past the 64 rows per image of the tail's backward
P = 64


def _tiny():
    import vit_amd
    return vit_amd.VisionTransformer(img_size=128, patch_size=16, embed_dim=D, depth=DEPTH, num_heads=2, num_classes=10)


def _gemm_rows(rec, name, n_at, k_at, m_at=3):
    """(M, N, K) of every launch of a GEMM entry point, in issue order."""
    return [(a[m_at], a[n_at], a[k_at]) for nm, a in rec if nm == name]


def test_last_block_forward_launches_run_at_batch_rows(launches):
    import vit_amd
    m = _tiny()
    prev = vit_amd.set_cls_tail(True)
    try:
        with torch.no_grad():
            out = m(torch.zeros(B, 3, 128, 128))
    finally:
        vit_amd.set_cls_tail(prev)
    assert out.shape == (B, 10)
    fwd = _gemm_rows(launches, "vit_linear_fwd", 4, 5)
    per_block = {"qkv": (3 * D, D), "proj": (D, D), "fc1": (F, D), "fc2": (D, F)}
    for name, (n, k) in per_block.items():
        rows = [mm for mm, nn, kk in fwd if (nn, kk) == (n, k)]
        if name == "proj":  # the head is a [10, D] GEMM, not a proj
            assert len(rows) == DEPTH
        want_last = B * N if name == "qkv" else B
        assert rows == [B * N] * (DEPTH - 1) + [want_last], (name, rows)
    # the last block's attention forward is the query-limited one, the others' the full kernel
    assert [a[1:4] for nm, a in launches if nm == "vit_sdpa_fwd"] == [(B, 2, N)] * (DEPTH - 1)
    assert [a[1:4] for nm, a in launches if nm == "vit_sdpa_fwd_cls"] == [(B, 2, N)]


def test_last_block_backward_launches_run_on_padded_class_rows(launches):
    import vit_amd
    m = _tiny()
    prev = vit_amd.set_cls_tail(True)
    try:
        logits = m(torch.zeros(B, 3, 128, 128))
        del launches[:]
        logits.sum().backward()
    finally:
        vit_amd.set_cls_tail(prev)
    # input gradients: (M, K) of dX = dY W per launch; the last block runs first, its MLP / proj part on
    # P rows per image (the class row and zero rows)
    dg = [(a[3], a[4], a[5]) for nm, a in launches if nm == "vit_linear_dgrad"]
    blocks = [x for x in dg if (x[1], x[2]) != (10, D)]  # (the head's)
    assert len(blocks) == 4 * DEPTH
    last, rest = blocks[:4], blocks[4:]
    assert [x[0] for x in last] == [B * P, B * P, B * P, B * N]  # fc2, fc1, proj padded; qkv dense
    assert all(x[0] == B * N for x in rest)
    # the last block's MLP weight gradients: one grouped launch over B * P rows with the dense pair's split
    from vit_amd import ops
    pair = [a for nm, a in launches if nm == "vit_linear_wgrad_partials2"]
    assert [(a[0], a[1]) for a in pair] == [(B * P, ops.pair_split(B * N, D, F, F, D))]
    # its proj gradient over B * P rows; every other single launch over B * N
    wg = [(a[1], a[2], a[3]) for nm, a in launches if nm in ("vit_linear_wgrad", "vit_linear_wgrad_partials")]
    assert [x[0] for x in wg if (x[1], x[2]) == (D, D)] == [B * P] + [B * N] * (DEPTH - 1)
    assert all(x[0] == B * N for x in wg if (x[1], x[2]) in ((D, F), (F, D), (3 * D, D)))
    # the head allocates no dense zero tensors; the zero fills are the dense-layout partial matrices of the
    # fc1 bias (64-row groups) and of norm2's three column sums
    nb = _lib_blocks(B * N)
    zeros = sorted(a[1] for nm, a in launches if nm == "vit_zero")
    assert zeros == sorted([((B * N + 63) // 64) * F * 4] + [nb * D * 4] * 3), zeros
    # attention backward stays the full kernel in every block
    assert [a[1:4] for nm, a in launches if nm == "vit_sdpa_bwd"] == [(B, 2, N)] * DEPTH
    # norm1's backward of the last block takes the class rows' residual gradient, every N-th row
    cls = [a for nm, a in launches if nm == "vit_layer_norm_bwd_cls"]
    assert len(cls) == 1 and cls[0][2] == B * N and cls[0][13] == N and cls[0][12] == P * D


def _lib_blocks(rows):
    from vit_amd import _lib
    return _lib.load().vit_layer_norm_bwd_blocks(rows)


def test_padded_layout_only_where_the_reduction_units_line_up():
    """64 rows per image only past 64 tokens and when the LayerNorm backward's rows per partial block
    (VIT_LN_BWD_ROWS) divide 64; any other setting keeps N rows per image (the dense layout)."""
    from vit_amd.model import tail_pad
    assert tail_pad(197) == 64 and tail_pad(65) == 64 and tail_pad(64) == 64 and tail_pad(17) == 17
    for rp in (8, 16, 32, 64):
        assert tail_pad(197, rp) == 64
    for rp in (24, 48, 128, 256, 0):
        assert tail_pad(197, rp) == 197


def test_ln_rows_per_block_is_read_from_the_library():
    from vit_amd import _lib, ops
    rp = ops.ln_bwd_rows_per()
    blocks = _lib.load().vit_layer_norm_bwd_blocks
    assert blocks(rp) == 1 and blocks(rp + 1) == 2 and blocks(5 * rp) == 5


def test_partial_row_maps_are_checked_on_the_host():
    """The scatter kernel has no bounds check: the map is validated where it is built."""
    from vit_amd import ops
    pr = ops.dense_part_rows(4, 197, 64, 1, "cpu")
    assert pr.idx.tolist() == [0, 3, 6, 9] and pr.S == 13 and pr.n == 4 and pr.every == 1
    assert ops.dense_part_rows(4, 197, 64, 1, "cpu") is pr  # cached: it depends on the shapes alone
    pr = ops.dense_part_rows(4, 197, 32, 2, "cpu")
    assert pr.idx.tolist() == [0, 6, 12, 18] and pr.S == 25 and pr.every == 2
    with pytest.raises(ValueError):  # two class rows in one dense partial row
        ops.PartRows([0, 0, 1], 4, 1, "cpu")
    with pytest.raises(ValueError):  # past the dense matrix
        ops.PartRows([0, 4], 4, 1, "cpu")
    with pytest.raises(ValueError):  # 17 tokens: rows 0, 17, 34 share 64-row groups
        ops.dense_part_rows(3, 17, 64, 1, "cpu")


def test_spread_partials_refuses_a_launch_that_does_not_match_its_map(launches):
    from vit_amd import ops
    pr = ops.PartRows([0, 3, 6, 9], 13, 2, "cpu")
    out = ops.spread_partials(torch.zeros(8, 128), pr)  # 4 images x 2 partial rows each
    assert out.numel() == 13 * 128
    sc = [a for nm, a in launches if nm == "vit_scatter_rows"]
    assert len(sc) == 1 and sc[0][0] == 4 and sc[0][1] == 128 and sc[0][3] == 256  # rows 0, 2, 4, 6 of the source
    with pytest.raises(AssertionError):
        ops.spread_partials(torch.zeros(4, 128), pr)  # the launch has half the rows the map was built for
    with pytest.raises(AssertionError):
        ops.spread_partials(torch.zeros(16, 128), pr)


def test_pair_fallback_launches_choose_their_own_split(launches, monkeypatch):
    """A pair that does not fit the grouped kernel falls back to two single launches: each chooses its own
    split, as before, unless the caller fixed one."""
    from vit_amd import ops
    M = 4100  # M % 32 != 0: no grouped launch
    dya, xa = torch.zeros(M, 128, dtype=torch.bfloat16), torch.zeros(M, 128, dtype=torch.bfloat16)
    dyb, xb = torch.zeros(M, 3072, dtype=torch.bfloat16), torch.zeros(M, 768, dtype=torch.bfloat16)
    oa, ob = torch.zeros(128, 128), torch.zeros(3072, 768)
    for asked in (None, 3):
        del launches[:]
        ops.linear_wgrad_pair((dya, xa, oa), (dyb, xb, ob), ops.ColBatch(), split=asked)
        got = [a[8] for nm, a in launches if nm == "vit_linear_wgrad_partials"]
        got += [a[9] for nm, a in launches if nm == "vit_linear_wgrad"]
        want = [3, 3] if asked else [ops._wgrad_split(M, 128, 128), ops._wgrad_split(M, 3072, 768)]
        assert sorted(got) == sorted(want), (asked, got, want)


def test_forward_features_and_switch_off_never_take_the_tail(launches):
    import vit_amd
    m = _tiny()
    prev = vit_amd.set_cls_tail(True)
    try:
        with torch.no_grad():
            f = m.forward_features(torch.zeros(B, 3, 128, 128))
        assert f.shape == (B, N, D)
        vit_amd.set_cls_tail(False)
        with torch.no_grad():
            m(torch.zeros(B, 3, 128, 128))
    finally:
        vit_amd.set_cls_tail(prev)
    fwd = _gemm_rows(launches, "vit_linear_fwd", 4, 5)
    assert all(mm == B * N for mm, nn, kk in fwd if (nn, kk) != (10, D))
    assert not [1 for nm, a in launches if nm == "vit_layer_norm_bwd_cls"]
