"""The per-step learning-rate schedule on the GPU: lr_schedule_kernel alone against engine.optim.lr_factor (the factor
within one fp32 ulp -- both sides are fp64 evaluations rounded once --, the products bitwise, nothing else touched, the
skipped verdict, the effective step), in front of every Adam form (bitwise the same Adam op with the lr written from the
host), the binding's refusals, and the engine: eager against the one-graph step across a MultiStepLR step, with
accumulation and with a skipped step, graph_eager_check, the default engine, and resume."""
from unittest import mock

import numpy as np
import pytest
import torch

from pytorch_rt1_for_distributed_training_amd.engine.optim import LR_SCHEDULE_KINDS, lr_factor
from test_param_groups_gpu import BETAS, GS, LR, _batches, _cfg, _engine

pytestmark = pytest.mark.gpu

W, N = 4, 20
# warm-up, its end, the decay, its end and beyond, and the last step fp32 counts exactly
STEPS = [1, 3, 4, 5, 19, 20, 21, 16777215]
MAX_ULP = {"factor": 0}


def _ops():
    from pytorch_rt1_for_distributed_training_amd.ops import adam
    return adam


def _ulps(a, b) -> int:
    """Distance in fp32 representable values between two non-negative fp32 numbers."""
    ia, ib = (int(np.float32(x).view(np.int32)) for x in (a, b))
    return abs(ia - ib)


def _base_lrs(G):
    """Distinct base learning rates; with more than one group the last one is 0."""
    lrs = [LR * (1 + g) / 2 for g in range(G)]
    if G > 1:
        lrs[-1] = 0.0
    return lrs


def _group_state(G):
    """A sentinel in every slot: the kernel may write column 0 only."""
    return (torch.arange(4 * G, dtype=torch.float32).reshape(G, 4) + 100.0).cuda()


def _clip_state(ok, skipped):
    return torch.tensor([1.5, 1.0, float(ok), float(skipped), 0.0, 0.0 if ok else 1.0, 0.0, 0.0], device="cuda")


def _run(t, G, with_gs, kind, r, clip=None):
    state = torch.tensor([float(t), 123.0], device="cuda")
    lr_base = torch.tensor(_base_lrs(G), dtype=torch.float32, device="cuda")
    gs = _group_state(G) if with_gs else None
    ss = torch.full((4,), 7.0, device="cuda")
    _ops().lr_schedule_dev(state, lr_base, ss, group_state=gs, clip_state=clip, kind=kind, warmup_steps=W,
                           decay_steps=N, min_lr_ratio=r)
    return state.cpu().numpy(), (gs.cpu().numpy() if with_gs else None), ss.cpu().numpy()


def _check(t_eff, G, with_gs, kind, r, state, gs, ss, t_raw):
    want = np.float32(lr_factor(kind, t_eff, W, N, r))
    d = _ulps(ss[0], want)
    MAX_ULP["factor"] = max(MAX_ULP["factor"], d)
    what = f"{kind} r={r} t={t_eff} G={G}"
    assert d <= 1, f"{what}: factor {ss[0]!r} is {d} ulp from {want!r}"
    assert ss[1] == np.float32(t_eff) and ss[2] == 0.0 and ss[3] == 0.0, (what, ss)
    base = np.array(_base_lrs(G), dtype=np.float32)
    assert state[0] == np.float32(t_raw), what
    assert state[1].tobytes() == (base[0] * ss[0]).tobytes(), (what, state[1], base[0] * ss[0])
    if with_gs:
        assert gs[:, 0].tobytes() == (base * ss[0]).tobytes(), (what, gs[:, 0], base * ss[0])
        assert np.array_equal(gs[:, 1:], _group_state(G).cpu().numpy()[:, 1:]), what


# ---------------------------------------------------------------------------------------- 1. the kernel alone
@pytest.mark.parametrize("G,with_gs", [(1, False), (1, True), (2, True), (16, True)])
def test_factor_and_products_against_the_host_formula(G, with_gs):
    for kind in LR_SCHEDULE_KINDS:
        for r in (0.0, 0.1):
            for t in STEPS:
                state, gs, ss = _run(t, G, with_gs, kind, r)
                _check(t, G, with_gs, kind, r, state, gs, ss, t)
    print(f"G={G}: largest distance of the device factor from np.float32(lr_factor) so far: {MAX_ULP['factor']} ulp")
    # the values are the schedule's: exact ones where the formula is exact
    for kind in LR_SCHEDULE_KINDS:
        assert _run(1, G, with_gs, kind, 0.1)[2][0] == np.float32(0.25)
        assert _run(4, G, with_gs, kind, 0.1)[2][0] == np.float32(1.0)
    for kind in ("linear", "cosine"):
        assert _run(20, G, with_gs, kind, 0.1)[2][0] == np.float32(0.1)
        assert _run(12, G, with_gs, kind, 0.0)[2][0] == np.float32(0.5)
    assert _run(16, G, with_gs, "rsqrt", 0.1)[2][0] == np.float32(0.5)
    assert _run(16777215, G, with_gs, "rsqrt", 0.1)[2][0] == np.float32(0.1)
    assert _run(16777215, G, with_gs, "constant", 0.1)[2][0] == np.float32(1.0)


@pytest.mark.parametrize("G,with_gs", [(1, False), (16, True)])
def test_the_skipped_verdict_writes_nothing_and_skipped_steps_do_not_count(G, with_gs):
    for kind in LR_SCHEDULE_KINDS:
        for t in (3, 7, 22, 16777215):
            # ok = 0: every output keeps its sentinel
            state, gs, ss = _run(t, G, with_gs, kind, 0.1, clip=_clip_state(0, 2))
            assert state.tolist() == [float(t), 123.0] and ss.tolist() == [7.0] * 4, (kind, t)
            if with_gs:
                assert np.array_equal(gs, _group_state(G).cpu().numpy()), (kind, t)
            # ok = 1 after two skipped steps: the factor is that of t - 2, the step counter itself is not touched
            state, gs, ss = _run(t, G, with_gs, kind, 0.1, clip=_clip_state(1, 2))
            _check(t - 2, G, with_gs, kind, 0.1, state, gs, ss, t)
            if t == 7:
                assert ss[0] != _run(t, G, with_gs, kind, 0.1)[2][0] or kind == "constant"


# ---------------------------------------------------------------------------------------- 2. in front of Adam
OMD = 1e-3


def _adam(form, bufs, grad, state, gstate, table, es, cs):
    ops = _ops()
    p, m, v, ema = bufs
    if form == "groups":
        ops.flat_adam_groups_dev_step(p, grad, m, v, state, gstate, table, grad_scale=GS, **BETAS)
    elif form == "ema":
        ops.flat_adam_ema_dev_step(p, grad, m, v, ema, state, es, None, grad_scale=GS, one_minus_decay=OMD,
                                   warmup=True, weight_decay=0.02, **BETAS)
    elif form == "clip":
        ops.flat_adam_clip_dev_step(p, grad, m, v, state, cs, grad_scale=GS, weight_decay=0.02, **BETAS)
    else:
        ops.flat_adam_dev_step(p, grad, m, v, state, grad_scale=GS, weight_decay=0.02, **BETAS)


@pytest.mark.parametrize("form", ["plain", "clip", "ema", "groups"])
@pytest.mark.parametrize("n", [64, 12288])
def test_schedule_then_adam_is_bitwise_adam_with_the_lr_written_from_the_host(n, form):
    ops = _ops()
    gen = torch.Generator(device="cuda").manual_seed(99 + n)
    start = [torch.randn(n, device="cuda", generator=gen), torch.randn(n, device="cuda", generator=gen) * 0.1,
             torch.rand(n, device="cuda", generator=gen) * 0.1, torch.randn(n, device="cuda", generator=gen)]
    grad = torch.randn(n, device="cuda", generator=gen)
    G = 4 if form == "groups" else 1
    base = np.array(_base_lrs(G), dtype=np.float32)
    table = (torch.arange(n // 64) % G).to(torch.uint8).cuda()
    wds = [0.02 * (g + 1) for g in range(G)]
    cs = None
    if form == "clip":
        cs = torch.zeros(8, device="cuda")
        pt = torch.zeros(ops.gradnorm_partials(n), dtype=torch.float64, device="cuda")
        norm = float(grad.double().pow(2).sum().sqrt()) * GS
        ops.grad_norm_clip_(grad, cs, pt, max_norm=0.5 * norm, grad_scale=GS, skip_nonfinite=True)
        cs[3] = 1.0                                                  # one earlier skipped step: t = 7 - 1
    t, t_eff = 7.0, (6.0 if form == "clip" else 7.0)
    mk_gs = lambda col0: torch.tensor([[l, w, 0.0, 0.0] for l, w in zip(col0, wds)], dtype=torch.float32, device="cuda")
    # the device path: the schedule op, then the existing Adam op
    got = [x.clone() for x in start]
    state = torch.tensor([t, 999.0], device="cuda")
    gstate = mk_gs([555.0] * G) if form == "groups" else None
    ss, es = torch.zeros(4, device="cuda"), torch.zeros(4, device="cuda")
    ops.lr_schedule_dev(state, torch.from_numpy(base).cuda(), ss, group_state=gstate, clip_state=cs, kind="cosine",
                        warmup_steps=W, decay_steps=N, min_lr_ratio=0.1)
    _adam(form, got, grad, state, gstate, table, es, cs)
    f = ss.cpu().numpy()[0]
    assert _ulps(f, np.float32(lr_factor("cosine", t_eff, W, N, 0.1))) <= 1 and 0.1 < f < 1.0
    # the same Adam op on clones whose lr the host wrote
    want = [x.clone() for x in start]
    state_h = torch.tensor([t, float(base[0] * f)], device="cuda")
    gstate_h = mk_gs([float(x) for x in base * f]) if form == "groups" else None
    es_h = torch.zeros(4, device="cuda")
    _adam(form, want, grad, state_h, gstate_h, table, es_h, cs)
    torch.cuda.synchronize()
    assert torch.equal(state, state_h)
    if form == "groups":
        assert torch.equal(gstate, gstate_h)
    for k, (a, b, s) in enumerate(zip(got, want, start)):
        assert torch.equal(a, b), f"n={n} {form}: buffer {'pmve'[k]} differs in {int((a != b).sum())} elements"
        if k < 3:
            assert not torch.equal(a, s)
    assert torch.equal(es, es_h)


# ---------------------------------------------------------------------------------------- 3. binding refusals
def test_binding_refusals_name_the_argument():
    from pytorch_rt1_for_distributed_training_amd.ops import load
    ops = _ops()
    state = torch.tensor([5.0, 123.0], device="cuda")
    lr_base = torch.tensor(_base_lrs(2), dtype=torch.float32, device="cuda")
    gs = _group_state(2)
    ss = torch.full((4,), 7.0, device="cuda")
    ok = dict(kind="cosine", warmup_steps=W, decay_steps=N, min_lr_ratio=0.1)
    call = lambda state=state, lr_base=lr_base, ss=ss, gs=gs, cs=None, **kw: ops.lr_schedule_dev(
        state, lr_base, ss, group_state=gs, clip_state=cs, **dict(ok, **kw))
    with pytest.raises(ValueError, match="kind is 'step'"):
        call(kind="step")
    with pytest.raises(RuntimeError, match="kind is 7"):
        load().lr_schedule_dev(state, lr_base, ss, gs, None, 7, W, N, 0.1)
    with pytest.raises(RuntimeError, match="kind is -1"):
        load().lr_schedule_dev(state, lr_base, ss, gs, None, -1, W, N, 0.1)
    for kind in ("linear", "cosine"):
        with pytest.raises(RuntimeError, match=r"decay_steps is 4, expected > warmup_steps \(4\)"):
            call(kind=kind, decay_steps=W)
        with pytest.raises(RuntimeError, match="decay_steps is 0"):
            call(kind=kind, decay_steps=0)
    with pytest.raises(RuntimeError, match="warmup_steps is -1"):
        call(warmup_steps=-1)
    for bad in (-0.01, 1.01, float("nan")):
        with pytest.raises(RuntimeError, match="min_lr_ratio is"):
            call(min_lr_ratio=bad)
    with pytest.raises(RuntimeError, match="lr_base has 17 entries"):
        call(lr_base=torch.zeros(17, device="cuda"), gs=None)
    with pytest.raises(RuntimeError, match="lr_base has 0 entries"):
        call(lr_base=torch.zeros(0, device="cuda"), gs=None)
    with pytest.raises(RuntimeError, match="lr_base has dtype"):
        call(lr_base=lr_base.double())
    with pytest.raises(RuntimeError, match="lr_base must be a GPU tensor"):
        call(lr_base=lr_base.cpu())
    with pytest.raises(RuntimeError, match="lr_base must be contiguous"):
        call(lr_base=torch.zeros(4, device="cuda")[::2])
    with pytest.raises(RuntimeError, match="group_state has 12 entries, expected 4 per group for the 2 groups"):
        call(gs=_group_state(3))
    with pytest.raises(RuntimeError, match="group_state has dtype"):
        call(gs=gs.double())
    with pytest.raises(RuntimeError, match="state has 1 entries"):
        call(state=torch.ones(1, device="cuda"))
    with pytest.raises(RuntimeError, match="state has dtype"):
        call(state=state.double())
    with pytest.raises(RuntimeError, match="sched_state must be fp32"):
        call(ss=torch.zeros(3, device="cuda"))
    with pytest.raises(RuntimeError, match="sched_state must be fp32"):
        call(ss=torch.zeros(8, device="cuda")[1:5])              # not 16-byte aligned
    with pytest.raises(RuntimeError, match="sched_state has dtype"):
        call(ss=ss.double())
    with pytest.raises(RuntimeError, match="alias"):
        call(ss=gs.view(-1)[:4])
    with pytest.raises(RuntimeError, match="clip_state"):
        call(cs=torch.zeros(4, device="cuda"))
    torch.cuda.synchronize()
    assert state.tolist() == [5.0, 123.0] and ss.tolist() == [7.0] * 4 and torch.equal(gs, _group_state(2))
    # the limits themselves pass: 16 groups, r = 0 and 1, W = 0, the kinds without an end at any decay_steps
    call(lr_base=torch.zeros(16, device="cuda"), gs=_group_state(16), min_lr_ratio=1.0, warmup_steps=0, decay_steps=1)
    call(kind="rsqrt", decay_steps=0, min_lr_ratio=0.0)
    call(kind="constant", decay_steps=0)
    torch.cuda.synchronize()
    assert ss.tolist() == [1.0, 5.0, 0.0, 0.0]


# ---------------------------------------------------------------------------------------- 4. the engine
SCHED = dict(kind="cosine", warmup_steps=2, decay_steps=6, min_lr_ratio=0.0)


def _sched_state(eng, base=True):
    """Weights, moments and everything the schedule op reads or writes.  ``base=False`` leaves out ``lr_base``, the
    device copy of the host's base lrs, which the host refreshes lazily (before an optimizer step, at a capture)."""
    opt = eng.optimizer
    out = [eng.flat.data, opt.exp_avg, opt.exp_avg_sq, opt.dev_state, opt.sched_state]
    out += [opt.lr_base] if base else []
    return out + ([opt.group_state] if opt.group_state is not None else [])


def _expected_lrs(eng, t):
    f = np.float32(lr_factor(t=t, kind=SCHED["kind"], warmup=SCHED["warmup_steps"], decay=SCHED["decay_steps"],
                             min_ratio=SCHED["min_lr_ratio"]))
    return [np.float32(g["lr"]) * f for g in eng.optimizer.param_groups]


@pytest.mark.parametrize("case", ["plain", "accumulate", "skipped"])
def test_graph_equals_eager_across_a_scheduler_step(case):
    """Six optimizer steps, warm-up of two, cosine to zero at the sixth, the MultiStepLR milestone after the third."""
    cfg = _cfg()
    k = 2 if case == "accumulate" else 1
    kw = dict(lr_schedule=SCHED, milestones=(1,))
    if case == "accumulate":
        kw.update(accumulate_grad_batches=2, grouped=False)          # one group: no group_state
    if case == "skipped":
        kw.update(skip_nonfinite=True)
    batches = _batches(cfg, 6 * k + (case == "skipped"))
    if case == "skipped":
        batches[3]["train_observation"]["natural_language_embedding"].fill_(float("nan"))
    eager, graphed = _engine(cfg, graph=False, **kw), _engine(cfg, graph=True, **kw)
    G = len(eager.optimizer.param_groups)
    assert G == (1 if case == "accumulate" else 4)
    assert (eager.optimizer.group_state is None) == (G == 1)
    applied, seen = 0, []
    for i, batch in enumerate(batches):
        le, lg = eager.train_step(batch), graphed.train_step(batch)
        torch.cuda.synchronize()
        bad = case == "skipped" and i == 3
        assert torch.equal(le, lg) or bad
        for a, b in zip(_sched_state(eager, eager.stepped), _sched_state(graphed, eager.stepped)):
            assert torch.equal(a, b), f"{case}: batch {i}"
        assert torch.equal(eager.optimizer.current_lr, graphed.optimizer.current_lr)
        if not eager.stepped:
            assert eager.optimizer.sched_state.tolist() == [seen[-1][0] if seen else 0.0, float(applied), 0.0, 0.0]
            continue
        if bad:
            assert eager.optimizer.skipped_steps == 1 and float(eager.optimizer.sched_state[1]) == applied
            continue
        applied += 1
        # the factor advances per applied optimizer step; the lr is the host formula times the base, within an ulp
        assert float(graphed.optimizer.sched_state[1]) == applied
        assert graphed.global_step == applied + (case == "skipped" and i > 3)
        want = _expected_lrs(graphed, applied)
        got = [float(v) for v in graphed.optimizer.current_lrs.values()]
        assert len(got) == G and got[0] == float(graphed.optimizer.current_lr) == graphed.lr_now
        for a, b in zip(got, want):
            assert _ulps(a, b) <= 1, f"{case}: step {applied}: lr {a!r} against {float(b)!r}"
        assert list(graphed.lrs_now.values()) == got
        seen.append((float(graphed.optimizer.lr_factor_now), got[0]))
        if applied == 3:
            for eng in (eager, graphed):
                eng.epoch_end()                                      # every base lr times 0.1
            assert graphed.lr == pytest.approx(LR * 0.1)
    assert applied == 6 and graphed._graph is not None, "capture did not happen"
    assert [f for f, _ in seen] == pytest.approx([0.5, 1.0, 0.8535534, 0.5, 0.1464466, 0.0], abs=1e-7)
    # the milestone and the schedule compose: step 4 runs at a tenth of step 2's rate times its own factor
    assert seen[3][1] == pytest.approx(seen[1][1] * 0.1 * 0.5, rel=1e-6)
    # the last update ran at lr 0 (cosine to r = 0 at N = 6)
    assert seen[5][1] == 0.0


def test_graph_eager_check_mid_schedule():
    cfg = _cfg()
    eng = _engine(cfg, graph=True, lr_schedule=dict(kind="linear", warmup_steps=3, decay_steps=10, min_lr_ratio=0.1))
    bs = _batches(cfg, 3)
    eng.train_step(bs[0])
    eng.train_step(bs[1])
    torch.cuda.synchronize()
    before = [t.clone() for t in _sched_state(eng)]
    res = eng.graph_eager_check(bs[2])
    assert res is not None and res["equal"], res
    for a, b in zip(before, _sched_state(eng)):
        assert torch.equal(a, b)
    f, t = eng.optimizer.sched_state.tolist()[:2]
    assert _ulps(f, np.float32(2 / 3)) <= 1 and t == 2.0


def test_default_engine_never_launches_the_schedule_op():
    adam = _ops()
    cfg = _cfg()
    eng = _engine(cfg, grouped=False, graph=True)
    opt = eng.optimizer
    assert opt.lr_schedule is None and opt.lr_base is None and opt.sched_state is None
    with mock.patch.object(adam, "lr_schedule_dev", wraps=adam.lr_schedule_dev) as new, \
            mock.patch.object(adam, "flat_adam_dev_step", wraps=adam.flat_adam_dev_step) as old:
        for b in _batches(cfg, 3):
            eng.train_step(b)
        torch.cuda.synchronize()
    assert new.call_count == 0 and old.call_count >= 1
    assert eng.lr_now == eng.lr == LR and eng.lrs_now == {"all": LR}
    assert "lr_schedule" not in opt.state_dict()
    # with a schedule the op runs once per optimizer step
    on = _engine(cfg, grouped=False, lr_schedule=SCHED)
    with mock.patch.object(adam, "lr_schedule_dev", wraps=adam.lr_schedule_dev) as new:
        for b in _batches(cfg, 2):
            on.train_step(b)
        torch.cuda.synchronize()
    assert new.call_count == 2


def test_resume_continues_the_lr_sequence_bitwise(tmp_path):
    from pytorch_rt1_for_distributed_training_amd.engine.trainer import Trainer
    from pytorch_rt1_for_distributed_training_amd.utils.checkpoint import build_checkpoint, save_checkpoint
    cfg = _cfg()
    batches = _batches(cfg, 6)
    kw = dict(lr_schedule=dict(kind="cosine", warmup_steps=2, decay_steps=8, min_lr_ratio=0.1), milestones=(1,))
    run = _engine(cfg, **kw)
    for b in batches[:3]:
        run.train_step(b)
    run.epoch_end()
    torch.cuda.synchronize()
    path = str(tmp_path / "last.ckpt")
    save_checkpoint(path, build_checkpoint(run.model, run.optimizer, run.scheduler, epoch=0,
                                           global_step=run.global_step))
    fresh = _engine(cfg, **kw)
    Trainer(fresh, verbose=False).resume(path)
    assert fresh.optimizer.step_count == 3 and fresh.lrs == pytest.approx(run.lrs)
    assert torch.equal(fresh.optimizer.sched_state, run.optimizer.sched_state)
    lrs = []
    for b in batches[3:]:
        la, lb = run.train_step(b), fresh.train_step(b)
        torch.cuda.synchronize()
        assert torch.equal(la, lb)
        for x, y in zip(_sched_state(run), _sched_state(fresh)):
            assert torch.equal(x, y)
        lrs.append(fresh.lr_now)
    assert len(set(lrs)) == 3 and float(fresh.optimizer.sched_state[1]) == 6.0
    # another schedule in the resumed run: a warning that names both, and the run's own schedule holds
    other = _engine(cfg, lr_schedule=dict(kind="linear", warmup_steps=2, decay_steps=8, min_lr_ratio=0.1),
                    milestones=(1,))
    with pytest.warns(UserWarning, match="lr schedule") as rec:
        Trainer(other, verbose=False).resume(path)
    assert "cosine" in str(rec[0].message) and "linear" in str(rec[0].message)
    assert other.optimizer.lr_schedule["kind"] == "linear" and other.optimizer.step_count == 3
