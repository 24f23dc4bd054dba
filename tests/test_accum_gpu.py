"""Gradient accumulation on the MI355X: the accumulating gather kernels (reduce.hip multi_add_ / multi_reduce_add_)
bitwise against the copying ones, the hip backend's accumulated flat gradient, the micro-step graph against the eager
micro-step, the graph-DP rehearsal, and the untouched k = 1 path."""
from unittest import mock

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ext():
    from pytorch_rt1_for_distributed_training_amd import ops
    return ops.load()


# ------------------------------------------------------------------------------------------------ 1. multi_add_
def test_multi_add_is_bitwise_old_plus_src(ext):
    """The 70 odd-sized entries of test_multi_copy_gathers_into_flat_views, destinations one float apart so that some
    are not 16-B aligned (scalar path); then 130 distinct entries, more than one launch takes (MC_MAX = 128)."""
    torch.manual_seed(0)
    sizes = [1, 3, 4, 5, 17, 64, 1000, 4097, 65537, 300_001] * 7
    srcs = [torch.randn(n, device="cuda") for n in sizes]
    flat = torch.randn(sum(sizes) + len(sizes), device="cuda")
    old = flat.clone()
    dsts, olds, off = [], [], 0
    inside = torch.zeros_like(flat, dtype=torch.bool)
    for n in sizes:
        dsts.append(flat[off:off + n])
        olds.append(old[off:off + n])
        inside[off:off + n] = True
        off += n + 1                      # odd offsets: some views are not 16-B aligned
    assert any(d.data_ptr() % 16 for d in dsts) and any(d.data_ptr() % 16 == 0 for d in dsts)
    ext.multi_add_(dsts, srcs)
    for d, o, s in zip(dsts, olds, srcs):
        assert torch.equal(d, o + s)
    assert torch.equal(flat[~inside], old[~inside])   # the gaps stay untouched
    # more than MC_MAX entries: split over launches, every entry added exactly once
    sizes = [5, 64, 1000, 7, 129] * 26
    srcs = [torch.randn(n, device="cuda") for n in sizes]
    flat = torch.randn(sum(sizes), device="cuda")
    want = flat + torch.cat(srcs)
    ext.multi_add_(list(flat.split(sizes)), srcs)
    assert torch.equal(flat, want)


# ------------------------------------------------------------------------------------------------ 2. multi_reduce_add_
# (splits, shape): the entries of test_multi_reduce_copy_matches_fixed_order_sum, then G = 4, 8, 16 split groups per
# workgroup, then the n % 4 tail
REDUCE_ENTRIES = ((1, (7,)), (3, (64, 40)), (16, (512, 512)), (5, (3072, 512)), (2, (33,)),
                  (32, (40, 24)), (64, (16, 24)), (256, (16, 24)), (3, (33,)))
ROW_SLICE = 3          # entry whose source is a row slice of the first split
MISALIGNED = 1         # entry whose destination starts one float off a 16-B boundary (scalar path)


def _reduce_case():
    torch.manual_seed(5)
    parts = [torch.randn(s, *shape, device="cuda") for s, shape in REDUCE_ENTRIES]
    srcs = [p[0] for p in parts]
    srcs[ROW_SLICE] = parts[ROW_SLICE][0][1024:2048]
    splits = [p.shape[0] for p in parts]
    strides = [p[0].numel() for p in parts]
    return parts, srcs, splits, strides


def _layout(srcs):
    """(start, numel) of each destination in one flat buffer and its length: 16-B aligned starts with a gap of at
    least 4 floats after each, MISALIGNED one float on."""
    out, off = [], 0
    for i, s in enumerate(srcs):
        n = s.numel()
        out.append((off + (1 if i == MISALIGNED else 0), n))
        off += (n + 1 + 3) // 4 * 4 + 4
    return out, off


def _views(flat, srcs):
    return [flat[o:o + n].view_as(s) for (o, n), s in zip(_layout(srcs)[0], srcs)]


def test_multi_reduce_add_is_bitwise_old_plus_multi_reduce_copy(ext):
    parts, srcs, splits, strides = _reduce_case()
    _, total = _layout(srcs)
    # the copying kernel's result, in the same layout (same alignment -> same vector / scalar path per entry)
    ref_flat = torch.zeros(total, device="cuda")
    ref = _views(ref_flat, srcs)
    assert ref[MISALIGNED].data_ptr() % 16 == 4 and all(r.data_ptr() % 16 == 0 for i, r in enumerate(ref)
                                                        if i != MISALIGNED)
    ext.multi_reduce_copy_(ref, srcs, splits, strides)
    inside = torch.zeros(total, dtype=torch.bool, device="cuda")
    for v in _views(inside, srcs):
        v.fill_(True)
    for i, (r, p) in enumerate(zip(ref, parts)):       # the reference itself is the fixed-order sum
        want = p.double().sum(0).float()
        torch.testing.assert_close(r, want[1024:2048] if i == ROW_SLICE else want, rtol=1e-5, atol=1e-5)
    for fill in ("random", "zeros"):
        flat = torch.randn(total, device="cuda") if fill == "random" else torch.zeros(total, device="cuda")
        old = flat.clone()
        dsts, olds = _views(flat, srcs), _views(old, srcs)
        ext.multi_reduce_add_(dsts, srcs, splits, strides)
        for i, (d, o, r) in enumerate(zip(dsts, olds, ref)):
            assert torch.equal(d, o + r), (fill, i, REDUCE_ENTRIES[i])
            if fill == "zeros":
                assert torch.equal(d, r), (i, REDUCE_ENTRIES[i])
        assert torch.equal(flat[~inside], old[~inside]), fill      # neighbours of every view untouched


# ------------------------------------------------------------------------------------------------ engines
def _cfg(**kw):
    from pytorch_rt1_for_distributed_training_amd.config import RT1Config
    base = dict(height=96, width=96, seq_len=2, num_layers=2, backend="hip", dropout_rate=0.0, drop_connect_rate=0.0,
                crop_ratio=0.0)
    base.update(kw)
    return RT1Config(**base)


def _engine(cfg, graph=False, **kw):
    from pytorch_rt1_for_distributed_training_amd.engine.step import TrainEngine
    from pytorch_rt1_for_distributed_training_amd.models import build_rt1
    from pytorch_rt1_for_distributed_training_amd.ops import rng
    rng._COUNTERS.clear()
    torch.manual_seed(0)
    kw.setdefault("order_probe", False)
    return TrainEngine(build_rt1(cfg), cfg, graph=graph, **kw)


def _batches(cfg, n, b=4):
    from pytorch_rt1_for_distributed_training_amd.data.synthetic import make_batch
    torch.manual_seed(123)
    return [make_batch(b, cfg.seq_len, cfg.height, cfg.width, device="cuda") for _ in range(n)]


def _fwd_bwd(eng, batch):
    from pytorch_rt1_for_distributed_training_amd.parallel.flat import deferred_sums
    eng.model.train()
    loss, _ = eng.forward_loss(batch)
    with deferred_sums(eng._defer_sums):
        loss.backward()


# ------------------------------------------------------------------------------------------------ 3. gradient sum
@pytest.mark.parametrize("hw", [96, 128, 256])
def test_hip_accumulated_gradient_is_the_sum_of_the_micro_batch_gradients(ext, hw):
    """flat.grad after two accumulating gathers == G_A + G_B bitwise, G from a non-accumulating engine in the same
    state (backward + gather on A, then on B, no optimizer step).  128 x 128 is the size
    test_deferred_split_sums_match_immediate_sums runs at, but at T = 2, b = 4 no weight-gradient site leaves a
    deferred split-K partial set there, nor at 96, 160, 192 or 224 (every such gradient comes out of one split);
    256 x 256 is the smallest size, in steps of 32 pixels, at which one does (2 splits of a [96, 288] project
    weight), so that is where multi_reduce_add_ must run."""
    from pytorch_rt1_for_distributed_training_amd.parallel import flat as flat_mod
    cfg = _cfg(height=hw, width=hw)
    a, b = _batches(cfg, 2)
    plain = _engine(cfg)
    grads = []
    for batch in (a, b):
        plain.optimizer.zero_grad()
        _fwd_bwd(plain, batch)
        plain.flat.gather_grads()
        grads.append(plain.flat.grad.clone())
    eng = _engine(cfg, accumulate_grad_batches=2)
    eng.flat.grad.zero_()
    with mock.patch.object(ext, "multi_reduce_add_", wraps=ext.multi_reduce_add_) as red, \
            mock.patch.object(ext, "multi_add_", wraps=ext.multi_add_) as add:
        for batch in (a, b):
            eng.flat.release_grads()
            _fwd_bwd(eng, batch)
            eng.flat.gather_grads(accumulate=True)
    torch.cuda.synchronize()
    assert not flat_mod._PENDING
    assert add.call_count >= 2
    if hw == 256:
        assert red.call_count >= 1, "no split-K partial set was deferred at 256 x 256"
    assert float(grads[0].abs().max()) > 0 and not torch.equal(grads[0], grads[1])
    assert torch.equal(eng.flat.grad, grads[0] + grads[1])


# ------------------------------------------------------------------------------------------------ 4. graph vs eager
def test_micro_step_graph_matches_eager_micro_steps():
    """k = 3 over 7 batches: two full windows and a flushed window of one.  Losses, the flat gradient at each window
    end, parameters and second moments are bitwise equal between the replayed micro-step graph and eager micro-steps."""
    cfg = _cfg()
    batches = _batches(cfg, 7)

    def run(graph):
        eng = _engine(cfg, graph=graph, accumulate_grad_batches=3)
        losses, ends = [], []
        for i, b in enumerate(batches):
            losses.append(float(eng.train_step(b)))
            assert eng.stepped == (i % 3 == 2) and eng.micro_step == (i + 1) % 3
            if eng.stepped:
                ends.append(eng.flat.grad.clone())
        assert eng.flush_window() is True and eng.micro_step == 0
        ends.append(eng.flat.grad.clone())
        torch.cuda.synchronize()
        return eng, losses, ends

    eager, le, ge = run(False)
    graphed, lg, gg = run(True)
    assert graphed.graph and graphed._graph is not None, "capture did not happen"
    assert eager._graph is None
    assert graphed.optimizer.step_count == graphed.global_step == 3
    assert eager.optimizer.step_count == eager.global_step == 3
    assert le == lg, (le, lg)
    assert len(ge) == len(gg) == 3
    for w, (x, y) in enumerate(zip(ge, gg)):
        assert float(x.abs().max()) > 0
        assert torch.equal(x, y), f"window {w}: flat gradients differ"
    assert torch.equal(graphed.flat.data, eager.flat.data)
    assert torch.equal(graphed.optimizer.exp_avg_sq, eager.optimizer.exp_avg_sq)


# ------------------------------------------------------------------------------------------------ 5. self-check
def test_graph_eager_check_of_a_micro_step_with_dropout():
    from pytorch_rt1_for_distributed_training_amd.config import RT1Config
    cfg = RT1Config(height=96, width=96, seq_len=2, num_layers=2, backend="hip")     # dropout / drop-path / shift on
    eng = _engine(cfg, graph=True, accumulate_grad_batches=2)
    bs = _batches(cfg, 5)
    for b in bs[:3]:                       # eager + capture, one replayed window end, one replay into a new window
        eng.train_step(b)
    torch.cuda.synchronize()
    assert eng._graph is not None and eng.micro_step == 1 and eng.global_step == 1
    for position in (1, 0):                # the check's micro-step ends the window, then opens one
        assert eng.micro_step == position
        data, grad, gstep = eng.flat.data.clone(), eng.flat.grad.clone(), eng.global_step
        res = eng.graph_eager_check(bs[3])
        assert res is not None and res["equal"], (position, res)
        assert torch.equal(data, eng.flat.data) and torch.equal(grad, eng.flat.grad)
        assert eng.micro_step == position and eng.global_step == gstep
        eng.train_step(bs[3 + (1 - position)])
    torch.cuda.synchronize()
    assert eng.global_step == 2 and eng.micro_step == 1


# ------------------------------------------------------------------------------------------------ 6. graph-DP, world 1
def test_graph_dp_rehearsal_matches_the_one_graph_engine():
    """comm='native' at world 1 with k = 2: the segments hold no memset, a non-final micro-batch replays them without
    launching a bucket, the final one all-reduces every bucket; parameters after two windows equal the one-graph
    engine's bitwise."""
    cfg = _cfg(height=128, width=128)
    en = _engine(cfg, graph=True, order_probe=True, bucket_cap_mb=4.0, comm="native", accumulate_grad_batches=2)
    et = _engine(cfg, graph=True, order_probe=True, accumulate_grad_batches=2)    # same flat layout
    assert en.ddp.enabled and len(en.ddp.buckets) > 1 and not et.ddp.enabled
    launched = []
    launch = en.ddp.launch_bucket
    en.ddp.launch_bucket = lambda i: (launched.append(i), launch(i))[1]
    try:
        for i, b in enumerate(_batches(cfg, 4)):
            launched.clear()
            ln, lt = float(en.train_step(b)), float(et.train_step(b))
            torch.cuda.synchronize()
            assert ln == lt, (i, ln, lt)
            assert en.stepped == et.stepped == (i % 2 == 1)
            if i >= 1:                     # replayed segments (micro-batch 0 ran the eager hook-driven step)
                assert sorted(launched) == (list(range(len(en.ddp.buckets))) if i % 2 == 1 else []), (i, launched)
            if en.stepped:
                assert torch.equal(en.flat.grad, et.flat.grad), i
                assert torch.equal(en.flat.data, et.flat.data), i
        assert en._segments is not None and en._segments.num_segments > 1 and et._graph is not None
        assert en.global_step == et.global_step == 2
        assert not en.ddp.comm.timed_out
    finally:
        en.ddp.comm.destroy()


def test_eager_final_micro_step_in_the_capture_window_all_reduces_every_bucket():
    """comm='native' at world 1, k = 2.  The segmented capture after micro-batch 0 leaves every bucket marked launched;
    an EAGER final micro-step in that same window (the eager half of graph_eager_check at micro_step == 1, and the
    next train_step once the graph is dropped) must still launch every bucket's all-reduce from its hooks."""
    cfg = _cfg(height=128, width=128)
    en = _engine(cfg, graph=True, order_probe=True, bucket_cap_mb=4.0, comm="native", accumulate_grad_batches=2)
    ee = _engine(cfg, graph=False, order_probe=True, accumulate_grad_batches=2)   # same flat layout, no DP
    every = list(range(len(en.ddp.buckets)))
    assert en.ddp.enabled and len(every) > 1
    b0, b1 = _batches(cfg, 2)
    try:
        en.train_step(b0)
        ee.train_step(b0)
        assert en._segments is not None and en._segments.num_segments > 1 and en.micro_step == 1
        assert all(b.launched for b in en.ddp.buckets)             # what the capture leaves behind
        en.ddp.launch_log = []
        res = en.graph_eager_check(b1)                             # replayed, then eager: both end the window
        assert res is not None and res["equal"], res
        assert sorted(en.ddp.launch_log) == every, en.ddp.launch_log       # the eager side (replays do not log)
        assert en.micro_step == 1 and en.global_step == 0
        en.drop_graph()
        en.ddp.launch_log = []
        le, lg = float(ee.train_step(b1)), float(en.train_step(b1))       # eager final micro-step, hooks launch
        torch.cuda.synchronize()
        assert en.stepped and en.global_step == 1 and en._segments is None
        assert sorted(en.ddp.launch_log) == every, en.ddp.launch_log
        assert lg == le and torch.equal(en.flat.grad, ee.flat.grad) and torch.equal(en.flat.data, ee.flat.data)
        assert not en.ddp.comm.timed_out
    finally:
        en.ddp.comm.destroy()


# ------------------------------------------------------------------------------------------------ 7. k = 1
def test_default_graph_step_never_calls_the_accumulating_kernels(ext):
    cfg = _cfg()
    eng = _engine(cfg, graph=True)
    new = ["multi_add_", "multi_reduce_add_"]
    with mock.patch.object(ext, "multi_copy_", wraps=ext.multi_copy_) as old:
        spies = [mock.patch.object(ext, n, wraps=getattr(ext, n)) for n in new]
        mocks = [s.start() for s in spies]
        try:
            for b in _batches(cfg, 3):
                eng.train_step(b)
                assert eng.stepped is True and eng.micro_step == 0
            torch.cuda.synchronize()
        finally:
            for s in spies:
                s.stop()
    assert eng._graph is not None, "capture did not happen"
    assert eng.global_step == 3 and eng.optimizer.step_count == 3
    assert old.call_count > 0
    assert [m.call_count for m in mocks] == [0, 0]
