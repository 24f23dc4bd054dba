"""Exponential moving average of the weights inside the fused Adam launch, on the GPU: the EMA variant of the
device-state Adam kernels against the existing kernels (bitwise) and an fp64 oracle (element-wise), its ema_state, the
skipped step, the binding checks, and the engine's eager / one-graph / accumulating / graph-DP steps and ema_weights().

The element-wise bound: the kernel forms ema' = fma(omd_t, fl(p - ema), ema), i.e. one rounding in the subtraction
(at most 2^-24 |p - ema|, scaled by omd_t) and one in the fma (at most 2^-24 |ema'|); the bound is twice their sum,
2^-23 * (|want| + omd_t * |p - ema|), with want formed in fp64 from the same fp32 inputs and the omd_t the kernel
recorded."""
from unittest import mock

import pytest
import torch

pytestmark = pytest.mark.gpu

GS = 0.25
# 2 * 2048 * 1024 + 192 + 3: every lane makes two full trips past the 2048-workgroup cap, 48 lanes of workgroup 0 a
# third, and 3 floats are left to the scalar tail
N_BIG = 2 * 2048 * 1024 + 192 + 3
SIZES = [64, 12288, 1_000_003, N_BIG]
ADAM = dict(beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0)
LR = 5e-4
EPS23 = 2.0 ** -23


def _ops():
    from pytorch_rt1_for_distributed_training_amd.ops import adam
    return adam


def _off4(n, fill=None):
    """n floats whose storage starts 16 bytes into an allocation: for the odd sizes the vector body and the scalar
    tail both run."""
    t = torch.empty(n + 4, device="cuda")[4:]
    assert t.data_ptr() % 16 == 0
    if fill is not None:
        t.copy_(fill)
    return t


_BASE = {}


def _base(n):
    """Seeded gradient of n floats, computed once per size and never modified."""
    if n not in _BASE:
        g = torch.Generator(device="cuda").manual_seed(1234 + n % 1000)
        _BASE[n] = _off4(n, torch.randn(n, device="cuda", generator=g))
    return _BASE[n]


def _buffers(n, seed=0):
    """p, m, v and an ema that differs from p by up to ~1e-2 relative (magnitudes from ~1e-3 to ~1e3 across p)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    scale = torch.pow(10.0, torch.rand(n, device="cuda", generator=g) * 6 - 3)
    p = _off4(n, torch.randn(n, device="cuda", generator=g) * scale)
    m = _off4(n, torch.randn(n, device="cuda", generator=g) * 0.1)
    v = _off4(n, torch.rand(n, device="cuda", generator=g) * 0.1)
    ema = _off4(n, p * (1 + 1e-2 * torch.randn(n, device="cuda", generator=g)))
    return p, m, v, ema


def _clones(ts):
    return [_off4(t.numel(), t) for t in ts]


def _omd32(decay):
    return float(torch.tensor(1.0 - decay, dtype=torch.float32))


def _assert_ema(got, e_prev, p_new, omd_t, what=""):
    want = _ops().reference_ema_step(e_prev, p_new, omd_t)
    assert want.dtype == torch.float64
    bound = EPS23 * (want.abs() + omd_t * (p_new.double() - e_prev.double()).abs())
    err = (got.double() - want).abs()
    worst = float((err - bound).max())
    print(f"{what} omd_t {omd_t!r}: max err {float(err.max()):.3e}, max (err - bound) {worst:.3e}")
    assert torch.isfinite(got).all()
    assert bool((err <= bound).all()), f"{what}: {int((err > bound).sum())} elements beyond the bound"


# ---------------------------------------------------------------------------------------------- 1. Adam unchanged
@pytest.mark.parametrize("mode", ["plain", "clip_inactive", "clip_active"])
@pytest.mark.parametrize("n", SIZES)
def test_adam_part_is_bitwise_the_existing_kernel(n, mode):
    ops = _ops()
    p, m, v, ema = _buffers(n)
    ref = _clones((p, m, v))
    grad = _base(n)
    state = torch.tensor([0.0, LR], device="cuda")
    es = torch.zeros(4, device="cuda")
    cs = pt = None
    if mode != "plain":
        cs = torch.zeros(8, device="cuda")
        pt = torch.zeros(ops.gradnorm_partials(n), dtype=torch.float64, device="cuda")
        true_norm = float(grad.double().pow(2).sum().sqrt()) * GS
        max_norm = 1e30 if mode == "clip_inactive" else 0.5 * true_norm
    for _ in range(3):
        state[0:1].add_(1.0)
        if cs is not None:
            ops.grad_norm_clip_(grad, cs, pt, max_norm=max_norm, grad_scale=GS, skip_nonfinite=True)
            ops.flat_adam_clip_dev_step(ref[0], grad, ref[1], ref[2], state, cs, grad_scale=GS, **ADAM)
        else:
            ops.flat_adam_dev_step(ref[0], grad, ref[1], ref[2], state, grad_scale=GS, **ADAM)
        ops.flat_adam_ema_dev_step(p, grad, m, v, ema, state, es, cs, grad_scale=GS, one_minus_decay=1e-3,
                                   warmup=True, **ADAM)
    if mode == "clip_active":
        assert 0.49 < float(cs[1]) < 0.51 and float(cs[4]) == 3.0
    elif mode == "clip_inactive":
        assert cs.tolist()[1:6] == [1.0, 1.0, 0.0, 0.0, 0.0]
    assert torch.equal(p, ref[0]) and torch.equal(m, ref[1]) and torch.equal(v, ref[2])
    assert float(es[1]) == 3.0


# ---------------------------------------------------------------------------------------------- 2. EMA vs fp64
SCHEDULES = [("warm", 0.999, True, 0), ("warm", 0.999, True, 7), ("warm", 0.999, True, 10_000),
             ("fixed", 0.9999, False, 0), ("fixed", 0.5, False, 0)]


@pytest.mark.parametrize("kind,decay,warmup,t0", SCHEDULES)
@pytest.mark.parametrize("n", SIZES)
def test_ema_matches_fp64_oracle_elementwise(n, kind, decay, warmup, t0):
    ops = _ops()
    p, m, v, ema = _buffers(n, seed=1)
    grad = _base(n)
    state = torch.tensor([float(t0), LR], device="cuda")
    es = torch.zeros(4, device="cuda")
    omd = 1.0 - decay
    seen = []
    for k in range(3):
        t = t0 + k + 1
        e_prev = ema.clone()
        state[0:1].add_(1.0)
        ops.flat_adam_ema_dev_step(p, grad, m, v, ema, state, es, None, grad_scale=GS, one_minus_decay=omd,
                                   warmup=warmup, **ADAM)
        omd_t, t_seen = float(es[0]), float(es[1])
        assert t_seen == t and es.tolist()[2:] == [0.0, 0.0]
        if warmup:
            assert omd_t == pytest.approx(max(omd, 9.0 / (10.0 + t)), rel=1e-6, abs=0)
        else:
            assert omd_t == _omd32(decay)
        seen.append(omd_t)
        _assert_ema(ema, e_prev, p, omd_t, f"n={n} {kind} decay={decay} t={t}")
        assert not torch.equal(ema, e_prev)
    if warmup and t0 < 100:
        assert len(set(seen)) == 3              # the schedule moved on every call
    if warmup and t0 == 10_000:
        assert seen == [_omd32(decay)] * 3      # past the warm-up the configured decay governs


# ---------------------------------------------------------------------------------------------- 3. ema_state
@pytest.mark.parametrize("warmup", [True, False])
@pytest.mark.parametrize("n", SIZES)
def test_ema_state_and_determinism(n, warmup):
    ops = _ops()
    start = _buffers(n, seed=2)
    grad = _base(n)
    outs = []
    for _ in range(2):
        p, m, v, ema = _clones(start)
        state = torch.tensor([4.0, LR], device="cuda")
        es = torch.zeros(4, device="cuda")
        ops.flat_adam_ema_dev_step(p, grad, m, v, ema, state, es, None, grad_scale=GS, one_minus_decay=1.0 - 0.9999,
                                   warmup=warmup, **ADAM)
        outs.append((p, m, v, ema, es))
    es = outs[0][4].tolist()
    if warmup:
        assert es[0] == pytest.approx(9.0 / 14.0, rel=1e-6, abs=0)
    else:
        assert es[0] == _omd32(0.9999)
    assert es[1:] == [4.0, 0.0, 0.0]
    for a, b in zip(*outs):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------- 4. skipped call
@pytest.mark.parametrize("n", SIZES)
def test_skipped_call_touches_nothing_and_the_next_uses_the_effective_step(n):
    ops = _ops()
    p, m, v, ema = _buffers(n, seed=3)
    grad = _base(n)
    bad = _off4(n, grad)
    bad[n - 1] = float("nan")
    state = torch.tensor([0.0, LR], device="cuda")
    es = torch.tensor([0.25, 17.0, 0.0, 0.0], device="cuda")       # a recognisable "before"
    cs = torch.zeros(8, device="cuda")
    pt = torch.zeros(ops.gradnorm_partials(n), dtype=torch.float64, device="cuda")
    before = [t.clone() for t in (p, m, v, ema, es)]
    kw = dict(grad_scale=GS, one_minus_decay=1e-3, warmup=True, **ADAM)
    state[0:1].add_(1.0)
    ops.grad_norm_clip_(bad, cs, pt, max_norm=0.0, grad_scale=GS, skip_nonfinite=True)
    ops.flat_adam_ema_dev_step(p, bad, m, v, ema, state, es, cs, **kw)
    assert float(cs[2]) == 0.0 and float(cs[3]) == 1.0
    for a, b in zip((p, m, v, ema, es), before):
        assert torch.equal(a, b)
    ref = _clones((p, m, v))
    state[0:1].add_(1.0)
    ops.grad_norm_clip_(grad, cs, pt, max_norm=0.0, grad_scale=GS, skip_nonfinite=True)
    ops.flat_adam_ema_dev_step(p, grad, m, v, ema, state, es, cs, **kw)
    ops.flat_adam_clip_dev_step(ref[0], grad, ref[1], ref[2], state, cs, grad_scale=GS, **ADAM)
    assert float(state[0]) == 2.0 and float(es[1]) == 1.0           # t = step - skipped steps
    assert float(es[0]) == pytest.approx(9.0 / 11.0, rel=1e-6, abs=0)
    assert torch.equal(p, ref[0]) and torch.equal(m, ref[1]) and torch.equal(v, ref[2])
    _assert_ema(ema, before[3], p, float(es[0]), f"n={n} after a skipped call")


# ---------------------------------------------------------------------------------------------- 5. binding checks
def test_binding_rejects_bad_buffers():
    ops = _ops()
    n = 4096
    p, m, v, ema = _buffers(n, seed=4)
    grad = _base(12288)[:n]
    state = torch.tensor([1.0, LR], device="cuda")
    es = torch.zeros(4, device="cuda")
    kw = dict(grad_scale=GS, one_minus_decay=1e-3, warmup=True, **ADAM)
    before = [t.clone() for t in (p, m, v, ema)]
    misaligned = torch.zeros(n + 1, device="cuda")[1:]
    assert misaligned.data_ptr() % 16 != 0
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        ops.flat_adam_ema_dev_step(p, grad, m, v, misaligned, state, es, None, **kw)
    with pytest.raises(RuntimeError, match="sizes"):
        ops.flat_adam_ema_dev_step(p, grad, m, v, torch.zeros(n - 4, device="cuda"), state, es, None, **kw)
    with pytest.raises(RuntimeError, match="ema_state"):
        ops.flat_adam_ema_dev_step(p, grad, m, v, ema, state, torch.zeros(3, device="cuda"), None, **kw)
    with pytest.raises(RuntimeError, match="alias"):
        ops.flat_adam_ema_dev_step(p, grad, m, v, p, state, es, None, **kw)
    with pytest.raises(RuntimeError, match="clip_state"):
        ops.flat_adam_ema_dev_step(p, grad, m, v, ema, state, es, torch.zeros(4, device="cuda"), **kw)
    torch.cuda.synchronize()
    for a, b in zip((p, m, v, ema), before):
        assert torch.equal(a, b)


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


def test_eager_engine_follows_the_recurrence():
    cfg = _cfg()
    eng = _engine(cfg, ema_decay=0.999)
    opt = eng.optimizer
    assert opt.ema is not None and torch.equal(opt.ema, eng.flat.data)
    assert opt.ema.data_ptr() != eng.flat.data.data_ptr()
    assert opt.ema_state.tolist() == [0.0] * 4
    for step, b in enumerate(_batches(cfg, 3), 1):
        e_prev = opt.ema.clone()
        eng.train_step(b)
        torch.cuda.synchronize()
        omd_t = float(opt.ema_state[0])
        assert float(opt.ema_state[1]) == step
        assert omd_t == pytest.approx(9.0 / (10.0 + step), rel=1e-6, abs=0)
        assert float(opt.ema_decay_now) == pytest.approx(1.0 - omd_t, rel=1e-6)
        _assert_ema(opt.ema, e_prev, eng.flat.data, omd_t, f"engine step {step}")
        if step == 1:
            assert not torch.equal(opt.ema, eng.flat.data)


def test_graph_and_eager_agree_while_the_decay_moves_every_step():
    """A decay computed on the host and baked into the capture would replay step 2's value for ever: the schedule
    gives another omd_t on each of these steps."""
    cfg = _cfg()
    batches = _batches(cfg, 4)
    out = []
    for graph in (False, True):
        eng = _engine(cfg, graph=graph, ema_decay=0.999)
        omds = []
        for b in batches:
            eng.train_step(b)
            omds.append(float(eng.optimizer.ema_state[0]))
        torch.cuda.synchronize()
        out.append((eng, omds))
    (eager, oe), (graphed, og) = out
    assert graphed._graph is not None, "capture did not happen"
    assert oe == og and len(set(og)) == 4
    assert torch.equal(graphed.optimizer.ema, eager.optimizer.ema)
    assert torch.equal(graphed.optimizer.ema_state, eager.optimizer.ema_state)
    assert torch.equal(graphed.flat.data, eager.flat.data)
    assert torch.equal(graphed.optimizer.exp_avg_sq, eager.optimizer.exp_avg_sq)
    assert not torch.equal(graphed.optimizer.ema, graphed.flat.data)


def test_graph_eager_check_with_ema_clipping_skip_and_dropout():
    from pytorch_rt1_for_distributed_training_amd.config import RT1Config
    cfg = RT1Config(height=96, width=96, seq_len=2, num_layers=2, backend="hip")     # dropout / drop-path / shift on
    eng = _engine(cfg, graph=True, max_grad_norm=1e-3, skip_nonfinite=True, ema_decay=0.999)
    bs = _batches(cfg, 3)
    eng.train_step(bs[0])
    eng.train_step(bs[1])
    torch.cuda.synchronize()
    assert eng.optimizer.clipped_steps == 2
    before = [t.clone() for t in (eng.flat.data, eng.optimizer.ema, eng.optimizer.ema_state)]
    res = eng.graph_eager_check(bs[2])
    assert res is not None and res["equal"] and res["ema"], res
    for a, b in zip(before, (eng.flat.data, eng.optimizer.ema, eng.optimizer.ema_state)):
        assert torch.equal(a, b)


def test_skipped_step_leaves_the_average_alone():
    """A NaN context in batch 3 of 5: the average does not move on it, and ends, eagerly and in the replayed graph,
    where an EMA engine without the skip option that never saw the batch ends."""
    cfg = _cfg()
    batches = _batches(cfg, 5)
    batches[2]["train_observation"]["natural_language_embedding"].fill_(float("nan"))
    final = {}
    for graph in (False, True):
        eng = _engine(cfg, graph=graph, skip_nonfinite=True, ema_decay=0.999)
        opt = eng.optimizer
        after2 = None
        for i, b in enumerate(batches):
            eng.train_step(b)
            if i == 1:
                torch.cuda.synchronize()
                after2 = (opt.ema.clone(), opt.ema_state.clone())
            if i == 2:
                torch.cuda.synchronize()
                assert opt.skipped_steps == 1
                assert torch.equal(opt.ema, after2[0]) and torch.equal(opt.ema_state, after2[1])
                assert torch.isfinite(opt.ema).all()
        torch.cuda.synchronize()
        if graph:
            assert eng._graph is not None, "capture did not happen"
        assert float(opt.ema_state[1]) == 4.0 and opt.step_count == 5
        final[graph] = (opt.ema.clone(), opt.ema_state.clone(), eng.flat.data.clone())
    clean = _engine(cfg, graph=False, ema_decay=0.999)
    for i in (0, 1, 3, 4):
        clean.train_step(batches[i])
    torch.cuda.synchronize()
    want = (clean.optimizer.ema, clean.optimizer.ema_state, clean.flat.data)
    for k, (e, g, w) in enumerate(zip(final[False], final[True], want)):
        assert torch.equal(e, g), f"graph != eager at {k}"
        assert torch.equal(e, w), f"skip engine != clean engine at {k}"


def test_accumulation_updates_the_average_once_per_window():
    cfg = _cfg()
    batches = _batches(cfg, 6)
    out = []
    for graph in (False, True):
        eng = _engine(cfg, graph=graph, accumulate_grad_batches=2, ema_decay=0.999)
        opt = eng.optimizer
        for i, b in enumerate(batches):
            before = (opt.ema.clone(), opt.ema_state.clone())
            eng.train_step(b)
            torch.cuda.synchronize()
            if i % 2 == 0:                      # a non-final micro-step
                assert not eng.stepped
                assert torch.equal(opt.ema, before[0]) and torch.equal(opt.ema_state, before[1])
                with pytest.raises(RuntimeError, match="accumulation window"):
                    with eng.ema_weights():
                        pass
            else:
                assert eng.stepped and not torch.equal(opt.ema, before[0])
        assert float(opt.ema_state[1]) == 3.0 and eng.global_step == 3
        out.append(eng)
    eager, graphed = out
    assert graphed._graph is not None, "capture did not happen"
    assert torch.equal(graphed.optimizer.ema, eager.optimizer.ema)
    assert torch.equal(graphed.optimizer.ema_state, eager.optimizer.ema_state)
    assert torch.equal(graphed.flat.data, eager.flat.data)


def test_graph_dp_path_world1_with_ema():
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
                                   graph=graph, ema_decay=0.999))
    eg, ee = engines
    assert eg.ddp.enabled and len(eg.ddp.buckets) > 1
    g = torch.Generator().manual_seed(7)
    try:
        for step in range(3):
            batch = make_batch(4, cfg.seq_len, 128, 128, device="cuda", generator=g)
            lg, le = float(eg.train_step(batch)), float(ee.train_step(batch))
            torch.cuda.synchronize()
            assert lg == le, (step, lg, le)
            assert torch.equal(eg.flat.data, ee.flat.data), step
            assert torch.equal(eg.optimizer.ema, ee.optimizer.ema), step
            assert torch.equal(eg.optimizer.ema_state, ee.optimizer.ema_state), step
        assert eg._segments is not None and eg._segments.num_segments > 1
        assert float(eg.optimizer.ema_state[1]) == 3.0
        assert not torch.equal(eg.optimizer.ema, eg.flat.data)
    finally:
        eg.ddp.comm.destroy()
        ee.ddp.comm.destroy()


def test_ema_weights_context():
    cfg = _cfg()
    batches = _batches(cfg, 5)
    graphed = _engine(cfg, graph=True, ema_decay=0.999)
    eager = _engine(cfg, graph=False, ema_decay=0.999)
    other = _engine(cfg, graph=False)           # built before any step: _engine() resets the dropout counters
    for b in batches[:3]:
        graphed.train_step(b)
        eager.train_step(b)
    torch.cuda.synchronize()
    assert graphed._graph is not None, "capture did not happen"
    fixed = batches[3]
    live = graphed.flat.data.clone()
    loss_live = graphed.eval_step(fixed).clone()
    with graphed.ema_weights() as e:
        assert e is graphed and torch.equal(graphed.flat.data, graphed.optimizer.ema)
        loss_ema = graphed.eval_step(fixed).clone()
    torch.cuda.synchronize()
    assert torch.equal(graphed.flat.data, live)
    assert not torch.equal(loss_ema, loss_live)
    # a second engine that simply has the averaged weights and the same (live) BN buffers
    with torch.no_grad():
        other.flat.data.copy_(graphed.optimizer.ema)
        for dst, src in zip(other.model.buffers(), graphed.model.buffers()):
            dst.copy_(src)
    assert torch.equal(other.eval_step(fixed), loss_ema)
    assert torch.equal(graphed.eval_step(fixed), loss_live)
    # the captured graph and the weight shadow survived the round trip
    lg, le = graphed.train_step(batches[4]), eager.train_step(batches[4])
    torch.cuda.synchronize()
    assert torch.equal(lg, le)
    assert torch.equal(graphed.flat.data, eager.flat.data)
    assert torch.equal(graphed.optimizer.ema, eager.optimizer.ema)
    with pytest.raises(RuntimeError, match="EMA is off"):
        with other.ema_weights():
            pass


def test_defaults_stay_on_the_old_path():
    from pytorch_rt1_for_distributed_training_amd.ops import adam
    from pytorch_rt1_for_distributed_training_amd.utils.checkpoint import build_checkpoint, ema_entry
    ext = adam.load()
    cfg = _cfg()
    eng = _engine(cfg)
    assert eng.optimizer.ema is None and eng.optimizer.ema_state is None and eng.optimizer.ema_decay_now is None
    # the one binding carries every form: its optional tensors (ema, ema_state, clip_state, group_state, chunk_group:
    # positions 5 to 9) select the kernel, and the old path is the call in which all of them are absent
    with mock.patch.object(ext, "flat_adam_dev", wraps=ext.flat_adam_dev) as adam_dev:
        for b in _batches(cfg, 2):
            eng.train_step(b)
        torch.cuda.synchronize()
    assert adam_dev.call_count == 2
    assert all(len(c.args) == 17 and all(a is None for a in c.args[5:10]) for c in adam_dev.call_args_list)
    ck = build_checkpoint(eng.model, eng.optimizer, eng.scheduler, ema=ema_entry(eng.optimizer))
    assert "ema" not in ck
    # and with the option on the EMA form is the only Adam launch
    on = _engine(cfg, ema_decay=0.999)
    with mock.patch.object(ext, "flat_adam_dev", wraps=ext.flat_adam_dev) as adam_dev:
        on.train_step(_batches(cfg, 1)[0])
        torch.cuda.synchronize()
    assert adam_dev.call_count == 1
    args = adam_dev.call_args.args
    assert args[5] is on.optimizer.ema and args[6] is on.optimizer.ema_state and all(a is None for a in args[7:10])
