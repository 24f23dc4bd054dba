"""Global-norm gradient clipping and the non-finite step skip on the GPU: the gradnorm.hip kernels against fp64
oracles, the clip variant of the fused Adam, the BN-buffer guard, and the engine's eager / one-graph / graph-DP steps."""
import math
from unittest import mock

import pytest
import torch

pytestmark = pytest.mark.gpu

GS = 0.25
CAP = 2048
PER_BLOCK = 256 * 4 * 4          # floats one workgroup covers per trip: 256 lanes x 4 loads x 4 floats
# the cap is reached at (CAP - 1) * PER_BLOCK + 1; at 2 * CAP * PER_BLOCK every lane of every workgroup makes a second
# full trip, and the extra 192 floats send 48 lanes of workgroup 0 through the remainder loop as well
N_BIG = 2 * CAP * PER_BLOCK + 192
SIZES = [64, 4096 * 3, 1_000_003, N_BIG]
ADAM = dict(beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0)


def _ops():
    from pytorch_rt1_for_distributed_training_amd.ops import adam
    return adam


_BASE = {}


def _base(n):
    """Seeded randn of n floats whose storage starts 16 bytes into an allocation for the odd size (a slice on a
    16-byte boundary, so the vector path and the scalar tail both run).  Computed once per size, never modified."""
    if n not in _BASE:
        g = torch.Generator(device="cuda").manual_seed(1234 + n % 1000)
        full = torch.randn(n + 4, device="cuda", generator=g)
        _BASE[n] = full[4:4 + n]
        assert _BASE[n].data_ptr() % 16 == 0
    return _BASE[n]


def _data(n, kind):
    if kind == "zeros":
        return torch.zeros(n + 4, device="cuda")[4:]
    return _base(n) * {"1e-3": 1e-3, "1": 1.0, "1e6": 1e6}[kind]


def _norm_call(g, max_norm, skip=False, clip_state=None, partials=None):
    ops = _ops()
    P = ops.gradnorm_partials(g.numel())
    cs = torch.zeros(8, device="cuda") if clip_state is None else clip_state
    pt = torch.zeros(P, dtype=torch.float64, device="cuda") if partials is None else partials
    ops.grad_norm_clip_(g, cs, pt, max_norm=max_norm, grad_scale=GS, skip_nonfinite=skip)
    return cs, pt


def test_partials_are_a_function_of_n():
    ops = _ops()
    assert ops.gradnorm_partials(0) == 0 and ops.gradnorm_partials(-5) == 0
    assert ops.gradnorm_partials(1) == 1 and ops.gradnorm_partials(PER_BLOCK) == 1
    assert ops.gradnorm_partials(PER_BLOCK + 1) == 2
    assert ops.gradnorm_partials((CAP - 1) * PER_BLOCK) == CAP - 1
    assert ops.gradnorm_partials((CAP - 1) * PER_BLOCK + 1) == CAP
    assert ops.gradnorm_partials(N_BIG) == CAP and ops.gradnorm_partials(2 ** 31 + 5) == CAP


# ---------------------------------------------------------------------------------------------- 7. norm vs fp64
@pytest.mark.parametrize("kind", ["1e-3", "1", "1e6", "zeros"])
@pytest.mark.parametrize("n", SIZES)
def test_norm_and_coef_match_fp64_oracle(n, kind):
    """rtol 1e-5 on the norm: the only fp32 rounding is in the per-lane chains of L non-negative terms, which bounds
    the sum's relative error by (L+1) * 2^-24 and the norm's by half of that; L <= 32 at these sizes (two trips of four
    float4 loads over four accumulators is 8 terms each), i.e. below 1e-6."""
    ops = _ops()
    g = _data(n, kind)
    want = float(g.double().pow(2).sum().sqrt()) * GS
    cs, pt = _norm_call(g, 0.0)
    got = cs.tolist()
    print(f"n={n} kind={kind} norm {got[0]!r} oracle {want!r} rel {abs(got[0] - want) / max(want, 1e-300):.3e}")
    if kind == "zeros":
        assert got[0] == 0.0 and got[1] == 1.0 and got[2] == 1.0
    else:
        assert got[0] == pytest.approx(want, rel=1e-5, abs=0)
        assert got[1] == 1.0 and got[2] == 1.0
    assert got[3:] == [0.0] * 5
    # clip coefficient at half and at twice the true norm
    for factor in (0.5, 2.0):
        max_norm = factor * want if want > 0 else factor
        cs2, pt2 = _norm_call(g, max_norm)
        ref = ops.reference_clip_coef(g, max_norm, GS)
        coef = float(cs2[1])
        print(f"  max_norm {max_norm!r}: coef {coef!r} oracle {ref!r}")
        if factor == 2.0 or want == 0:
            assert coef == 1.0 and ref == 1.0
            assert float(cs2[4]) == 0.0
        else:
            assert coef == pytest.approx(ref, rel=1e-6, abs=0) and coef < 1.0
            assert float(cs2[4]) == 1.0
        # determinism: the same input gives the same bits
        assert torch.equal(pt2, pt)
        assert torch.equal(cs2[0:1], cs[0:1]) and float(cs2[2]) == 1.0
    a, pa = _norm_call(g, 0.5 * want if want > 0 else 0.5)
    b, pb = _norm_call(g, 0.5 * want if want > 0 else 0.5)
    assert torch.equal(pa, pb) and torch.equal(a[0:3], b[0:3])


# ---------------------------------------------------------------------------------------------- 8. non-finite inputs
@pytest.mark.parametrize("bad", ["nan_last", "inf_first", "neg_inf_middle"])
@pytest.mark.parametrize("n", SIZES)
def test_nonfinite_inputs_reach_the_verdict(n, bad):
    g = _base(n).clone()
    assert g.data_ptr() % 16 == 0
    if bad == "nan_last":
        g[-1] = float("nan")            # in the scalar tail (n % 4 != 0) or the last lane's last float
    elif bad == "inf_first":
        g[0] = float("inf")
    else:
        g[n // 2] = float("-inf")
    cs, pt = _norm_call(g, 1.0, skip=True)
    got = cs.tolist()
    assert not math.isfinite(got[0])
    assert got[1] == 1.0 and got[2] == 0.0 and got[3] == 1.0 and got[4] == 0.0 and got[5] == 1.0
    _norm_call(g, 1.0, skip=True, clip_state=cs, partials=pt)
    assert cs.tolist()[2:6] == [0.0, 2.0, 0.0, 2.0]
    # a finite call resets the streak and keeps the total
    _norm_call(_base(n), 1e30, skip=True, clip_state=cs, partials=pt)
    got = cs.tolist()
    assert math.isfinite(got[0]) and got[1:6] == [1.0, 1.0, 2.0, 0.0, 0.0]
    # without the skip the step is not stopped and nothing is clipped
    cs0, _ = _norm_call(g, 1.0, skip=False)
    got = cs0.tolist()
    assert not math.isfinite(got[0]) and got[1:6] == [1.0, 1.0, 0.0, 0.0, 0.0]


# ---------------------------------------------------------------------------------------------- 9. clip Adam
def _adam_buffers(n, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    p = torch.randn(n + 4, device="cuda", generator=g)[4:]
    m = (torch.randn(n + 4, device="cuda", generator=g) * 0.1)[4:]
    v = (torch.rand(n + 4, device="cuda", generator=g) * 0.1)[4:]
    return p, m, v


def _clone4(t):
    """A copy with the same 16-byte-aligned, 16-bytes-in placement."""
    c = torch.empty(t.numel() + 4, device=t.device, dtype=t.dtype)[4:]
    c.copy_(t)
    return c


@pytest.mark.parametrize("n", SIZES)
def test_clip_adam_with_inactive_clip_is_bitwise_flat_adam_dev(n):
    ops = _ops()
    p, m, v = _adam_buffers(n)
    ref = [_clone4(t) for t in (p, m, v)]
    grad = _base(n)
    state = torch.tensor([0.0, 5e-4], device="cuda")
    cs = torch.zeros(8, device="cuda")
    pt = torch.zeros(ops.gradnorm_partials(n), dtype=torch.float64, device="cuda")
    for _ in range(3):
        state[0:1].add_(1.0)
        ops.grad_norm_clip_(grad, cs, pt, max_norm=1e30, grad_scale=GS, skip_nonfinite=True)
        ops.flat_adam_clip_dev_step(p, grad, m, v, state, cs, grad_scale=GS, **ADAM)
        ops.flat_adam_dev_step(ref[0], grad, ref[1], ref[2], state, grad_scale=GS, **ADAM)
    assert cs.tolist()[1:6] == [1.0, 1.0, 0.0, 0.0, 0.0]
    assert torch.equal(p, ref[0]) and torch.equal(m, ref[1]) and torch.equal(v, ref[2])


@pytest.mark.parametrize("n", SIZES)
def test_clip_adam_with_active_clip_matches_reference(n):
    ops = _ops()
    p, m, v = _adam_buffers(n, seed=1)
    ref = [t.clone() for t in (p, m, v)]
    grad = _base(n)
    true_norm = float(grad.double().pow(2).sum().sqrt()) * GS
    max_norm = 0.5 * true_norm
    coef = ops.reference_clip_coef(grad, max_norm, GS)
    assert 0.49 < coef < 0.51
    state = torch.tensor([0.0, 5e-4], device="cuda")
    cs = torch.zeros(8, device="cuda")
    pt = torch.zeros(ops.gradnorm_partials(n), dtype=torch.float64, device="cuda")
    for step in (1, 2, 3):
        state[0:1].add_(1.0)
        ops.grad_norm_clip_(grad, cs, pt, max_norm=max_norm, grad_scale=GS, skip_nonfinite=False)
        ops.flat_adam_clip_dev_step(p, grad, m, v, state, cs, grad_scale=GS, **ADAM)
        ops.reference_adam_step(ref[0], grad * GS * coef, ref[1], ref[2], lr=5e-4, step=step, **ADAM)
    assert float(cs[4]) == 3.0
    torch.testing.assert_close(p, ref[0], rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(m, ref[1], rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(v, ref[2], rtol=1e-5, atol=1e-8)


@pytest.mark.parametrize("n", SIZES)
def test_skipped_call_touches_nothing_and_does_not_advance_the_bias_correction(n):
    ops = _ops()
    p, m, v = _adam_buffers(n, seed=2)
    before = [t.clone() for t in (p, m, v)]
    ref = [t.clone() for t in (p, m, v)]
    grad = _base(n)
    bad = grad.clone()
    bad[n // 3] = float("nan")
    state = torch.tensor([0.0, 5e-4], device="cuda")      # lr 5e-4: step sizes at t=1 and t=2 differ by 1.9x
    cs = torch.zeros(8, device="cuda")
    pt = torch.zeros(ops.gradnorm_partials(n), dtype=torch.float64, device="cuda")
    state[0:1].add_(1.0)
    ops.grad_norm_clip_(bad, cs, pt, max_norm=0.0, grad_scale=GS, skip_nonfinite=True)
    ops.flat_adam_clip_dev_step(p, bad, m, v, state, cs, grad_scale=GS, **ADAM)
    assert float(cs[2]) == 0.0
    assert all(torch.equal(a, b) for a, b in zip((p, m, v), before))
    state[0:1].add_(1.0)
    ops.grad_norm_clip_(grad, cs, pt, max_norm=0.0, grad_scale=GS, skip_nonfinite=True)
    ops.flat_adam_clip_dev_step(p, grad, m, v, state, cs, grad_scale=GS, **ADAM)
    ops.reference_adam_step(ref[0], grad * GS, ref[1], ref[2], lr=5e-4, step=1, **ADAM)
    torch.testing.assert_close(p, ref[0], rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(m, ref[1], rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(v, ref[2], rtol=1e-5, atol=1e-8)


# ---------------------------------------------------------------------------------------------- 10. buffer guard
@pytest.mark.parametrize("n", [87_296, 67])
def test_buffer_guard_follows_or_rolls_back(n):
    ops = _ops()
    torch.manual_seed(3)
    buf, shadow = torch.randn(n, device="cuda"), torch.randn(n, device="cuda")
    buf0, shadow0 = buf.clone(), shadow.clone()
    cs = torch.zeros(8, device="cuda")
    cs[2] = 1.0
    ops.buffer_guard_(buf, shadow, cs)
    assert torch.equal(shadow, buf0) and torch.equal(buf, buf0)
    shadow.copy_(shadow0)
    buf[n // 2] = float("nan")
    cs[2] = 0.0
    ops.buffer_guard_(buf, shadow, cs)
    assert torch.equal(buf, shadow0) and torch.equal(shadow, shadow0)


# ---------------------------------------------------------------------------------------------- engine
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
    return TrainEngine(build_rt1(cfg), cfg, order_probe=False, graph=graph, **kw)


def _batches(cfg, n, b=4):
    from pytorch_rt1_for_distributed_training_amd.data.synthetic import make_batch
    torch.manual_seed(123)
    return [make_batch(b, cfg.seq_len, cfg.height, cfg.width, device="cuda") for _ in range(n)]


@pytest.fixture(scope="module")
def plain_step():
    """One step of an engine without the feature: initial parameters, flat gradient, its fp64 norm."""
    cfg = _cfg()
    eng = _engine(cfg)
    p0 = eng.flat.data.clone()
    eng.train_step(_batches(cfg, 1)[0])
    torch.cuda.synchronize()
    grad = eng.flat.grad.clone()
    return dict(p0=p0, grad=grad, norm=float(grad.double().pow(2).sum().sqrt()))


def test_engine_eager_clip_matches_reference(plain_step):
    ops = _ops()
    cfg = _cfg()
    G, N0 = plain_step["grad"], plain_step["norm"]
    assert math.isfinite(N0) and N0 > 0
    eng = _engine(cfg, max_grad_norm=N0 / 4)
    eng.train_step(_batches(cfg, 1)[0])
    torch.cuda.synchronize()
    assert torch.equal(eng.flat.grad, G)
    assert float(eng.optimizer.last_grad_norm) == pytest.approx(N0, rel=1e-5, abs=0)
    assert eng.optimizer.clipped_steps == 1 and eng.optimizer.skipped_steps == 0
    coef = ops.reference_clip_coef(G, N0 / 4, 1.0)
    p, m, v = plain_step["p0"].clone(), torch.zeros_like(G), torch.zeros_like(G)
    ops.reference_adam_step(p, G * coef, m, v, lr=5e-4, step=1, **ADAM)
    torch.testing.assert_close(eng.flat.data, p, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(eng.optimizer.exp_avg, m, rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(eng.optimizer.exp_avg_sq, v, rtol=1e-5, atol=1e-8)


def test_graph_and_eager_agree_with_clipping_active(plain_step):
    cfg = _cfg()
    batches = _batches(cfg, 4)
    out = []
    for graph in (False, True):
        eng = _engine(cfg, graph=graph, max_grad_norm=plain_step["norm"] / 4, skip_nonfinite=True)
        grads = []
        for b in batches:
            eng.train_step(b)
            grads.append(eng.flat.grad.clone())
        torch.cuda.synchronize()
        out.append((eng, grads))
    (eager, ge), (graphed, gg) = out
    assert graphed._graph is not None, "capture did not happen"
    for step, (a, b) in enumerate(zip(ge, gg)):
        assert torch.equal(a, b), f"step {step + 1}: gradients differ"
    assert torch.equal(graphed.flat.data, eager.flat.data)
    assert torch.equal(graphed.optimizer.exp_avg_sq, eager.optimizer.exp_avg_sq)
    assert torch.equal(graphed.optimizer.clip_state, eager.optimizer.clip_state)
    assert graphed.optimizer.clipped_steps == 4 and eager.optimizer.clipped_steps == 4
    assert graphed.optimizer.skipped_steps == 0


def test_graph_eager_check_with_both_options_and_dropout(plain_step):
    from pytorch_rt1_for_distributed_training_amd.config import RT1Config
    cfg = RT1Config(height=96, width=96, seq_len=2, num_layers=2, backend="hip")     # dropout / drop-path / shift on
    eng = _engine(cfg, graph=True, max_grad_norm=plain_step["norm"] / 4, skip_nonfinite=True)
    bs = _batches(cfg, 3)
    eng.train_step(bs[0])
    eng.train_step(bs[1])
    torch.cuda.synchronize()
    before, clip_before = eng.flat.data.clone(), eng.optimizer.clip_state.clone()
    shadow_before = eng._bn_shadow.clone()
    res = eng.graph_eager_check(bs[2])
    assert res is not None and res["equal"], res
    assert torch.equal(before, eng.flat.data) and torch.equal(clip_before, eng.optimizer.clip_state)
    assert torch.equal(shadow_before, eng._bn_shadow)


def _bn_stats(model):
    return [b.detach().clone() for n, b in model.named_buffers()
            if n.endswith("running_mean") or n.endswith("running_var")]


def _full_state(eng):
    return [eng.flat.data.clone(), eng.optimizer.exp_avg.clone(), eng.optimizer.exp_avg_sq.clone()] + \
        _bn_stats(eng.model)


def test_skipped_step_leaves_no_trace_in_the_captured_graph():
    """A batch with a NaN context (what a bad shard produces) in step 3 of 5: nothing of it remains, eagerly and in
    the replayed graph, and both equal an engine without the feature that never saw the batch."""
    cfg = _cfg()
    batches = _batches(cfg, 5)
    batches[2]["train_observation"]["natural_language_embedding"].fill_(float("nan"))
    final = {}
    for graph in (False, True):
        eng = _engine(cfg, graph=graph, skip_nonfinite=True)
        after2 = None
        for i, b in enumerate(batches):
            eng.train_step(b)
            if i == 1:
                torch.cuda.synchronize()
                after2 = _full_state(eng)
            if i == 2:
                torch.cuda.synchronize()
                now = _full_state(eng)
                assert len(now) == len(after2) and len(now) > 3
                for k, (a, c) in enumerate(zip(after2, now)):
                    assert torch.isfinite(c).all(), (graph, k)
                    assert torch.equal(a, c), (graph, k)
                assert eng.optimizer.skipped_steps == 1
        torch.cuda.synchronize()
        if graph:
            assert eng._graph is not None, "capture did not happen"
        assert eng.optimizer.skipped_steps == 1 and eng.optimizer.step_count == 5
        final[graph] = _full_state(eng)
    clean = _engine(cfg, graph=False)
    for i in (0, 1, 3, 4):
        clean.train_step(batches[i])
    torch.cuda.synchronize()
    want = _full_state(clean)
    for k, (e, g, w) in enumerate(zip(final[False], final[True], want)):
        assert torch.equal(e, g), f"graph != eager at {k}"
        assert torch.equal(e, w), f"feature != clean engine at {k}"


def test_graph_dp_path_world1_with_both_options():
    """comm='native' at world 1: the segmented graph-DP step (norm, clip Adam and guard run eagerly after wait_all)
    equals the eager bucketed step bitwise."""
    import pytorch_rt1_for_distributed_training_amd as rt1
    from pytorch_rt1_for_distributed_training_amd.data.synthetic import make_batch
    from pytorch_rt1_for_distributed_training_amd.engine.step import TrainEngine
    from pytorch_rt1_for_distributed_training_amd.models import build_rt1
    cfg = rt1.RT1Config(height=128, width=128, seq_len=6, backend="hip", dropout_rate=0.0, drop_connect_rate=0.0,
                        crop_ratio=0.0)
    engines = []
    for graph in (True, False):
        torch.manual_seed(0)
        engines.append(TrainEngine(build_rt1(cfg), cfg, order_probe=True, bucket_cap_mb=4.0, comm="native",
                                   graph=graph, max_grad_norm=1e-3, skip_nonfinite=True))
    eg, ee = engines
    assert eg.ddp.enabled and len(eg.ddp.buckets) > 1 and eg._bn_flat is eg.ddp.buffers
    g = torch.Generator().manual_seed(7)
    try:
        for step in range(3):
            batch = make_batch(4, cfg.seq_len, 128, 128, device="cuda", generator=g)
            lg, le = float(eg.train_step(batch)), float(ee.train_step(batch))
            torch.cuda.synchronize()
            assert lg == le, (step, lg, le)
            assert torch.equal(eg.flat.grad, ee.flat.grad), step
            assert torch.equal(eg.flat.data, ee.flat.data), step
            assert torch.equal(eg.optimizer.clip_state, ee.optimizer.clip_state), step
            assert torch.equal(eg._bn_flat, ee._bn_flat) and torch.equal(eg._bn_shadow, eg._bn_flat), step
        assert eg._segments is not None and eg._segments.num_segments > 1
        assert eg.optimizer.clipped_steps == 3 and eg.optimizer.skipped_steps == 0
    finally:
        eg.ddp.comm.destroy()
        ee.ddp.comm.destroy()


def test_defaults_stay_on_the_old_path():
    from pytorch_rt1_for_distributed_training_amd.ops import adam
    ext = adam.load()
    new = ["grad_sumsq", "grad_clip_finalize", "buffer_guard_"]
    cfg = _cfg()
    eng = _engine(cfg)
    assert eng.optimizer.clip_state is None and eng._bn_flat is None
    with mock.patch.object(ext, "flat_adam_dev", wraps=ext.flat_adam_dev) as old:
        spies = [mock.patch.object(ext, n, wraps=getattr(ext, n)) for n in new]
        mocks = [s.start() for s in spies]
        try:
            for b in _batches(cfg, 2):
                eng.train_step(b)
            torch.cuda.synchronize()
        finally:
            for s in spies:
                s.stop()
    assert old.call_count == 2
    # the one binding carries every form: the old path is the call whose optional tensors (ema, ema_state, clip_state,
    # group_state, chunk_group: positions 5 to 9) are all absent, which launches the plain kernel
    assert all(len(c.args) == 17 and all(a is None for a in c.args[5:10]) for c in old.call_args_list)
    assert [m.call_count for m in mocks] == [0, 0, 0]
