"""Parameter groups inside the fused Adam launch, on the GPU: flat_adam_kernel's GROUPS forms against the existing
ungrouped kernels group by group (bitwise), across steps and a skipped step, with equal groups, against an fp64
reference, the binding's refusals, and the engine's eager / one-graph steps, defaults and resume.

The bitwise oracle: the grouped kernel calls the same adam_elem with the same operands as the ungrouped kernel of the
same form run over the whole buffer with (lr_g, wd_g), so the elements of group g must be identical; the oracle runs
that ungrouped kernel once per group on copies and assembles each group's chunks."""
from unittest import mock

import pytest
import torch

pytestmark = pytest.mark.gpu

GS = 0.25
LR = 5e-4
BETAS = dict(beta1=0.9, beta2=0.999, eps=1e-8)
# 64: one chunk; 128: two chunks of different groups inside one wave's first 32 lanes; 12288: 12 waves of one
# workgroup; N_BIG: every lane makes two trips past the 2048-workgroup cap, 48 lanes of workgroup 0 a third
N_BIG = 2 * 2048 * 1024 + 192
SIZES = [64, 128, 12288, N_BIG]
FORMS = ["plain", "ema", "clip_inactive", "clip_active", "ema_clip_inactive", "ema_clip_active"]
OMD = 1e-3


def _ops():
    from pytorch_rt1_for_distributed_training_amd.ops import adam
    return adam


def _hyper(G):
    """Distinct (lr, wd) per group; with more than one group the last has lr = 0 and every odd one wd = 0."""
    lrs = [LR * (1 + g) / 2 for g in range(G)]
    wds = [0.0 if g % 2 else 0.02 * (g + 1) for g in range(G)]
    if G > 1:
        lrs[-1] = 0.0
    return lrs, wds


def _layouts(n):
    """(name, G, chunk table on the host) for G in {1, 2, 4, 16}: alternating every chunk, seeded random chunks, runs
    of 1 to 40 chunks, and one layout in which a group owns no chunk."""
    c = n // 64
    out = []
    gen = torch.Generator().manual_seed(77 + c % 1000)
    for G in (1, 2, 4, 16):
        out.append((f"alt{G}", G, (torch.arange(c) % G).to(torch.uint8)))
        out.append((f"rand{G}", G, torch.randint(0, G, (c,), generator=gen).to(torch.uint8)))
        runs, total = [], 0
        while total < c:
            r = int(torch.randint(1, 41, (1,), generator=gen))
            runs.append(torch.full((r,), len(runs) % G, dtype=torch.uint8))
            total += r
        out.append((f"runs{G}", G, torch.cat(runs)[:c].clone()))
    t = torch.randint(0, 3, (c,), generator=gen)
    out.append(("empty_group", 4, torch.where(t >= 1, t + 1, t).to(torch.uint8)))       # groups 0, 2, 3: 1 owns nothing
    return out


_BASE = {}


def _base(n):
    """Seeded gradient and start buffers of n floats, computed once per size and never modified."""
    if n not in _BASE:
        g = torch.Generator(device="cuda").manual_seed(4321 + n % 1000)
        scale = torch.pow(10.0, torch.rand(n, device="cuda", generator=g) * 6 - 3)
        p = torch.randn(n, device="cuda", generator=g) * scale
        _BASE[n] = dict(grad=torch.randn(n, device="cuda", generator=g), p=p,
                        m=torch.randn(n, device="cuda", generator=g) * 0.1,
                        v=torch.rand(n, device="cuda", generator=g) * 0.1,
                        ema=p * (1 + 1e-2 * torch.randn(n, device="cuda", generator=g)))
    return _BASE[n]


def _start(n):
    b = _base(n)
    return [b[k].clone() for k in ("p", "m", "v", "ema")]


def _group_state(lrs, wds):
    return torch.tensor([[l, w, 0.0, 0.0] for l, w in zip(lrs, wds)], dtype=torch.float32, device="cuda")


def _clip(form, grad):
    """clip_state for the form (None without CLIP): coefficient 1 when inactive, about 0.5 when active."""
    if "clip" not in form:
        return None
    ops = _ops()
    cs = torch.zeros(8, device="cuda")
    pt = torch.zeros(ops.gradnorm_partials(grad.numel()), dtype=torch.float64, device="cuda")
    norm = float(grad.double().pow(2).sum().sqrt()) * GS
    ops.grad_norm_clip_(grad, cs, pt, max_norm=1e30 if "inactive" in form else 0.5 * norm, grad_scale=GS,
                        skip_nonfinite=True)
    if "inactive" in form:
        assert float(cs[1]) == 1.0
    else:
        assert 0.49 < float(cs[1]) < 0.51
    return cs


def _ungrouped(form, bufs, grad, state, es, cs, wd):
    """The existing kernel of the form over the whole buffer."""
    ops = _ops()
    p, m, v, ema = bufs
    if "ema" in form:
        ops.flat_adam_ema_dev_step(p, grad, m, v, ema, state, es, cs, grad_scale=GS, one_minus_decay=OMD, warmup=True,
                                   weight_decay=wd, **BETAS)
    elif cs is not None:
        ops.flat_adam_clip_dev_step(p, grad, m, v, state, cs, grad_scale=GS, weight_decay=wd, **BETAS)
    else:
        ops.flat_adam_dev_step(p, grad, m, v, state, grad_scale=GS, weight_decay=wd, **BETAS)


def _grouped(form, bufs, grad, state, gstate, table, es, cs):
    p, m, v, ema = bufs
    on = "ema" in form
    _ops().flat_adam_groups_dev_step(p, grad, m, v, state, gstate, table, ema=ema if on else None,
                                     ema_state=es if on else None, clip_state=cs, grad_scale=GS, one_minus_decay=OMD,
                                     warmup=True, **BETAS)


def _elem_mask(table_dev, g):
    return (table_dev == g).repeat_interleave(64)


# ---------------------------------------------------------------------------------------- 1. per-group bitwise oracle
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", SIZES)
def test_each_group_is_bitwise_the_ungrouped_kernel(n, form):
    grad = _base(n)["grad"]
    cs = _clip(form, grad)
    t0 = 3.0
    for name, G, table in _layouts(n):
        lrs, wds = _hyper(G)
        table_dev = table.cuda()
        got = _start(n)
        state = torch.tensor([t0 + 1, 123.0], device="cuda")        # the grouped kernel does not read state[1]
        es = torch.full((4,), 7.0, device="cuda")
        _grouped(form, got, grad, state, _group_state(lrs, wds), table_dev, es, cs)
        want = _start(n)
        untouched = [t.clone() for t in want]
        es_ref = None
        for g in range(G):
            mask = _elem_mask(table_dev, g)
            if not bool(mask.any()):
                continue
            ref = _start(n)
            es_g = torch.full((4,), 7.0, device="cuda")
            _ungrouped(form, ref, grad, torch.tensor([t0 + 1, lrs[g]], device="cuda"), es_g, cs, wds[g])
            for w, r in zip(want, ref):
                w.copy_(torch.where(mask, r, w))
            es_ref = es_g
        for k, (a, b, u) in enumerate(zip(got, want, untouched)):
            if k == 3 and "ema" not in form:
                assert torch.equal(a, u), f"{name}: the average moved without EMA"
                continue
            assert torch.equal(a, b), (f"n={n} {form} {name}: buffer {'pmve'[k]} differs in "
                                       f"{int((a != b).sum())} elements")
        if "ema" in form:
            assert torch.equal(es, es_ref) and float(es[1]) == t0 + 1, (name, es.tolist())
        else:
            assert es.tolist() == [7.0] * 4
        if name.startswith("alt"):                                   # chunk 0 is group 0's: lr > 0
            assert not torch.equal(got[0][:64], untouched[0][:64])


# ---------------------------------------------------------------------------------------- 2. steps, then a skipped one
@pytest.mark.parametrize("form", ["clip_active", "ema_clip_active"])
@pytest.mark.parametrize("n", SIZES)
def test_two_steps_a_skipped_step_and_the_effective_step(n, form):
    ops = _ops()
    grad = _base(n)["grad"]
    bad = grad.clone()
    bad[n - 1] = float("nan")
    name, G, table = _layouts(n)[7]                                 # seeded random chunks over 4 groups
    assert name == "rand4"
    lrs, wds = _hyper(G)
    table_dev = table.cuda()
    gstate = _group_state(lrs, wds)
    got = _start(n)
    refs = [_start(n) for _ in range(G)]
    state = torch.zeros(2, device="cuda")
    states = [torch.tensor([0.0, lrs[g]], device="cuda") for g in range(G)]
    es = torch.zeros(4, device="cuda")
    es_refs = [torch.zeros(4, device="cuda") for _ in range(G)]
    cs = torch.zeros(8, device="cuda")
    pt = torch.zeros(ops.gradnorm_partials(n), dtype=torch.float64, device="cuda")
    norm = float(grad.double().pow(2).sum().sqrt()) * GS

    def step(gr):
        state[0:1].add_(1.0)                                        # the device step, as FlatAdam advances it
        ops.grad_norm_clip_(gr, cs, pt, max_norm=0.5 * norm, grad_scale=GS, skip_nonfinite=True)
        _grouped(form, got, gr, state, gstate, table_dev, es, cs)
        for g in range(G):
            states[g][0:1].add_(1.0)
            _ungrouped(form, refs[g], gr, states[g], es_refs[g], cs, wds[g])

    def check(what):
        for k in range(4 if "ema" in form else 3):
            want = got[k].clone()
            for g in range(G):
                want = torch.where(_elem_mask(table_dev, g), refs[g][k], want)
            assert torch.equal(got[k], want), f"{what}: buffer {'pmve'[k]}"
        if "ema" in form:
            assert torch.equal(es, es_refs[0]), what

    step(grad)
    step(grad)
    check("after two steps")
    assert float(state[0]) == 2.0 and (float(es[1]) == 2.0 or "ema" not in form)
    before = [t.clone() for t in got] + [es.clone()]
    step(bad)
    assert float(cs[2]) == 0.0 and float(cs[3]) == 1.0
    for a, b in zip(got + [es], before):
        assert torch.equal(a, b), "the skipped step touched something"
    step(grad)
    check("after the skipped step")
    assert float(state[0]) == 4.0
    if "ema" in form:
        assert float(es[1]) == 3.0                                  # t = step - skipped steps
    assert not torch.equal(got[0], before[0])


# ---------------------------------------------------------------------------------------- 3. equal groups
@pytest.mark.parametrize("form", ["plain", "ema", "clip_active", "ema_clip_active"])
@pytest.mark.parametrize("n", SIZES)
def test_equal_groups_are_bitwise_the_ungrouped_kernel(n, form):
    grad = _base(n)["grad"]
    cs = _clip(form, grad)
    for name, G, table in _layouts(n)[6:9]:                         # the three 4-group layouts
        got, want = _start(n), _start(n)
        es, es_ref = torch.zeros(4, device="cuda"), torch.zeros(4, device="cuda")
        state = torch.tensor([5.0, LR], device="cuda")
        _grouped(form, got, grad, state, _group_state([LR] * G, [0.03] * G), table.cuda(), es, cs)
        _ungrouped(form, want, grad, state, es_ref, cs, 0.03)
        for a, b in zip(got, want):
            assert torch.equal(a, b), f"n={n} {form} {name}"
        assert torch.equal(es, es_ref)


# ---------------------------------------------------------------------------------------- 4. fp64 reference
@pytest.mark.parametrize("n", SIZES)
def test_matches_the_fp64_reference(n):
    """An independent check at the tolerances of test_kernels_gpu.py::test_flat_adam_matches_reference."""
    ops = _ops()
    g = torch.Generator(device="cuda").manual_seed(11)
    p = torch.randn(n, device="cuda", generator=g)
    grad = torch.randn(n, device="cuda", generator=g)
    m = torch.randn(n, device="cuda", generator=g) * 0.1
    v = torch.rand(n, device="cuda", generator=g) * 0.1
    name, G, table = _layouts(n)[7]
    lrs, wds = _hyper(G)
    table_dev = table.cuda()
    ref = [t.double() for t in (p, m, v)]
    state = torch.zeros(2, device="cuda")
    for step in (1, 2, 7):
        state[0] = float(step)
        ops.flat_adam_groups_dev_step(p, grad, m, v, state, _group_state(lrs, wds), table_dev, grad_scale=GS, **BETAS)
        ops.reference_adam_groups_step(ref[0], grad.double(), ref[1], ref[2], table_dev, lrs, wds, step=step,
                                       grad_scale=GS, **BETAS)
    for got, want, atol, what in zip((p, m, v), ref, (1e-6, 1e-7, 1e-8), "pmv"):
        err = (got.double() - want).abs()
        print(f"n={n} {what}: max err {float(err.max()):.3e}")
        torch.testing.assert_close(got.double(), want, rtol=1e-5, atol=atol)


# ---------------------------------------------------------------------------------------- 5. binding refusals
def test_binding_refusals_name_the_argument():
    ops = _ops()
    n = 4096
    p, m, v, ema = _start(12288)
    p, m, v, ema = p[:n], m[:n], v[:n], ema[:n]
    grad = _base(12288)["grad"][:n]
    state = torch.tensor([1.0, LR], device="cuda")
    gstate = _group_state(*_hyper(4))
    table = (torch.arange(n // 64) % 4).to(torch.uint8).cuda()
    before = [t.clone() for t in (p, m, v)]
    call = lambda p=p, grad=grad, m=m, v=v, gstate=gstate, table=table, **kw: ops.flat_adam_groups_dev_step(
        p, grad, m, v, state, gstate, table, grad_scale=GS, **BETAS, **kw)
    with pytest.raises(RuntimeError, match="param has 4000 elements, not a positive multiple of 64"):
        call(p=p[:4000], grad=grad[:4000], m=m[:4000], v=v[:4000], table=table[:62])
    with pytest.raises(RuntimeError, match="chunk_group has 63 entries, expected 64"):
        call(table=table[:63])
    with pytest.raises(RuntimeError, match="chunk_group has 65 entries, expected 64"):
        call(table=torch.zeros(65, dtype=torch.uint8, device="cuda"))
    with pytest.raises(RuntimeError, match="chunk_group has dtype"):
        call(table=table.to(torch.int32))
    with pytest.raises(RuntimeError, match="chunk_group must be a GPU tensor"):
        call(table=table.cpu())
    with pytest.raises(RuntimeError, match="chunk_group must be contiguous"):
        call(table=torch.zeros(128, dtype=torch.uint8, device="cuda")[::2])
    with pytest.raises(RuntimeError, match="group_state has 0 entries"):
        call(gstate=torch.zeros(0, 4, device="cuda"))
    with pytest.raises(RuntimeError, match="group_state has 68 entries"):
        call(gstate=torch.zeros(17, 4, device="cuda"))
    with pytest.raises(RuntimeError, match="group_state has 6 entries"):
        call(gstate=torch.zeros(6, device="cuda"))
    with pytest.raises(RuntimeError, match="group_state has dtype"):
        call(gstate=gstate.double())
    with pytest.raises(RuntimeError, match="ema and ema_state go together"):
        call(ema=ema)
    with pytest.raises(RuntimeError, match="alias"):
        call(ema=p, ema_state=torch.zeros(4, device="cuda"))
    with pytest.raises(RuntimeError, match="clip_state"):
        call(clip_state=torch.zeros(4, device="cuda"))
    torch.cuda.synchronize()
    for a, b in zip((p, m, v), before):
        assert torch.equal(a, b)
    call(gstate=torch.zeros(16, 4, device="cuda"))                  # 16 groups are allowed (lr = 0: p stays)
    torch.cuda.synchronize()
    assert torch.equal(p, before[0]) and not torch.equal(m, before[1])


# ---------------------------------------------------------------------------------------- engine
WD = 0.05
MULT = 0.1


def _cfg():
    from pytorch_rt1_for_distributed_training_amd.config import RT1Config
    return RT1Config(height=96, width=96, seq_len=2, num_layers=2, backend="hip", dropout_rate=0.0,
                     drop_connect_rate=0.0, crop_ratio=0.0)


def _engine(cfg, graph=False, grouped=True, weight_decay=WD, **kw):
    from pytorch_rt1_for_distributed_training_amd.engine.step import TrainEngine
    from pytorch_rt1_for_distributed_training_amd.models import build_rt1, load_pretrained_backbone
    from pytorch_rt1_for_distributed_training_amd.models.efficientnet import pretrained_keys
    from pytorch_rt1_for_distributed_training_amd.ops import rng
    rng._COUNTERS.clear()
    torch.manual_seed(0)
    model = build_rt1(cfg)
    if grouped:
        # the multiplier asks for pretrained weights: a backbone state dict (here the backbone's own values)
        net = model._image_tokenizer._tokenizer.net
        sd = net.state_dict()
        load_pretrained_backbone(model, {k: sd[k].clone() for k in pretrained_keys(net)})
        kw = dict(dict(no_decay_norm_bias=True, backbone_lr_mult=MULT), **kw)
    return TrainEngine(model, cfg, order_probe=False, graph=graph, lr=LR, weight_decay=weight_decay, **kw)


def _batches(cfg, n, b=2):
    from pytorch_rt1_for_distributed_training_amd.data.synthetic import make_batch
    torch.manual_seed(123)
    return [make_batch(b, cfg.seq_len, cfg.height, cfg.width, device="cuda") for _ in range(n)]


def _copy_state(dst, src):
    """dst continues from src's weights, moments and BN buffers (the groups' lr / wd stay dst's own)."""
    with torch.no_grad():
        dst.flat.data.copy_(src.flat.data)
        dst.optimizer.exp_avg.copy_(src.optimizer.exp_avg)
        dst.optimizer.exp_avg_sq.copy_(src.optimizer.exp_avg_sq)
        for a, b in zip(dst.model.buffers(), src.model.buffers()):
            a.copy_(b)


def test_eager_steps_decay_only_the_decay_groups():
    """Three eager steps with weight_decay = 0.05 next to the same engine with weight_decay = 0.  The weights couple
    through the forward, so from the second step on two free runs see different gradients and nothing stays equal;
    each step of the second engine therefore starts from the first engine's state.  Then, step by step, every
    no-decay parameter is bitwise the weight_decay = 0 result, and at the end every decay parameter differs (at step 1
    the zero-initialised FiLM weights are 0 and decay to 0)."""
    cfg = _cfg()
    a, b = _engine(cfg), _engine(cfg, weight_decay=0.0)
    assert a.optimizer.group_names == ["new", "new_no_decay", "backbone", "backbone_no_decay"]
    assert a.lrs == pytest.approx(dict(new=LR, new_no_decay=LR, backbone=LR * MULT, backbone_no_decay=LR * MULT))
    assert not a.optimizer.groups_uniform() and not b.optimizer.groups_uniform()
    no_decay = {id(p) for g in a.optimizer.param_groups if g["weight_decay"] == 0.0 for p in g["params"]}
    assert 0 < len(no_decay) < len(a.flat.params)
    for step, batch in enumerate(_batches(cfg, 3), 1):
        _copy_state(b, a)
        la, lb = a.train_step(batch), b.train_step(batch)
        torch.cuda.synchronize()
        assert torch.equal(la, lb)
        same = differ = 0
        for pa, pb in zip(a.flat.params, b.flat.params):
            if id(pa) in no_decay:
                assert torch.equal(pa, pb), f"step {step}: a no-decay parameter {tuple(pa.shape)} was decayed"
                same += 1
            elif not torch.equal(pa, pb):
                differ += 1
        assert same == len(no_decay - {id(p) for p in a.model.parameters() if not p.requires_grad})
        if step == 3:
            assert differ == len(a.flat.params) - same, f"{len(a.flat.params) - same - differ} decay parameters equal"


@pytest.mark.parametrize("case", ["distinct", "uniform_at_capture", "ema_clip"])
def test_graph_equals_eager_and_survives_a_scheduler_step(case):
    cfg = _cfg()
    kw = dict(weight_decay=WD)
    if case == "uniform_at_capture":
        # two groups holding one (lr, wd): the eager step takes the ungrouped route, the capture the grouped kernel
        kw = dict(weight_decay=0.0, backbone_lr_mult=1.0)
    if case == "ema_clip":
        kw.update(ema_decay=0.999, max_grad_norm=1e-3, skip_nonfinite=True)
    batches = _batches(cfg, 5)
    eager, graphed = _engine(cfg, graph=False, **kw), _engine(cfg, graph=True, **kw)
    assert len(eager.optimizer.param_groups) == (2 if case == "uniform_at_capture" else 4)
    assert eager.optimizer.groups_uniform() == (case == "uniform_at_capture")

    def both(batch):
        le, lg = eager.train_step(batch), graphed.train_step(batch)
        torch.cuda.synchronize()
        assert torch.equal(le, lg)
        assert torch.equal(graphed.flat.data, eager.flat.data)
        assert torch.equal(graphed.optimizer.exp_avg, eager.optimizer.exp_avg)
        assert torch.equal(graphed.optimizer.exp_avg_sq, eager.optimizer.exp_avg_sq)
        if case == "ema_clip":
            assert torch.equal(graphed.optimizer.ema, eager.optimizer.ema)
            assert torch.equal(graphed.optimizer.ema_state, eager.optimizer.ema_state)

    for batch in batches[:3]:
        both(batch)
    assert graphed._graph is not None, "capture did not happen"
    captured = graphed._graph
    if case == "ema_clip":
        assert graphed.optimizer.clipped_steps == 3
    # a different lr on one group, from the host, as a scheduler would set it
    for eng in (eager, graphed):
        eng.optimizer.param_groups[1]["lr"] = LR * 0.37
    before = graphed.flat.data.clone()
    both(batches[3])
    both(batches[4])
    assert graphed._graph is captured, "the graph was recaptured"
    assert graphed.optimizer.group_state[1].tolist() == pytest.approx([LR * 0.37, 0.0, 0.0, 0.0])
    assert not torch.equal(graphed.flat.data, before)
    # and the new lr took effect: the same replay with the old lr ends elsewhere
    res = graphed.graph_eager_check(batches[0])
    assert res is not None and res["equal"], res


def _parent_step(opt, grad_scale=1.0):
    """The optimizer step of an engine without groups, clipping or the EMA, as it was before parameter groups."""
    opt.step_count += 1
    t = opt.step_count
    opt.flat.gather_grads()
    lr = opt.param_groups[0]["lr"]
    if float(opt.dev_state[0]) != t - 1 or float(opt.dev_state[1]) != float(torch.tensor(lr, dtype=torch.float32)):
        opt.dev_state.copy_(torch.tensor([float(t - 1), float(lr)]))
    opt.dev_state[0:1].add_(1.0)
    opt._dev_step = t
    _ops().flat_adam_dev_step(opt.flat.data, opt.flat.grad, opt.exp_avg, opt.exp_avg_sq, opt.dev_state, beta1=0.9,
                              beta2=0.999, eps=1e-8, weight_decay=opt.param_groups[0]["weight_decay"],
                              grad_scale=grad_scale)


def test_default_engine_stays_on_the_ungrouped_kernel():
    adam = _ops()
    cfg = _cfg()
    batches = _batches(cfg, 3)
    eng = _engine(cfg, grouped=False)
    opt = eng.optimizer
    assert len(opt.param_groups) == 1 and opt.chunk_group is None and opt.group_state is None
    assert "name" not in opt.param_groups[0] and eng.lrs == {"all": LR}
    # the one op carries every form: group_state and chunk_group select the grouped kernel, None the ungrouped one
    with mock.patch.object(adam, "flat_adam_dev_step", wraps=adam.flat_adam_dev_step) as step:
        for b in batches:
            eng.train_step(b)
        torch.cuda.synchronize()
    assert step.call_count == 3
    assert all(c.kwargs["group_state"] is None and c.kwargs["chunk_group"] is None for c in step.call_args_list)
    # the same engine on the parent's optimizer step
    ref = _engine(cfg, grouped=False)
    ref.optimizer.step = lambda closure=None, grad_scale=1.0: _parent_step(ref.optimizer, grad_scale)
    for b in batches:
        ref.train_step(b)
    torch.cuda.synchronize()
    assert torch.equal(eng.flat.data, ref.flat.data)
    assert torch.equal(opt.exp_avg, ref.optimizer.exp_avg) and torch.equal(opt.exp_avg_sq, ref.optimizer.exp_avg_sq)
    assert torch.equal(opt.dev_state, ref.optimizer.dev_state)
    # with groups the grouped form is the only Adam launch
    on = _engine(cfg)
    with mock.patch.object(adam, "flat_adam_dev_step", wraps=adam.flat_adam_dev_step) as step:
        on.train_step(batches[0])
        torch.cuda.synchronize()
    assert step.call_count == 1
    kw = step.call_args.kwargs
    assert kw["group_state"] is on.optimizer.group_state and kw["chunk_group"] is on.optimizer.chunk_group


def test_resume_restores_the_groups(tmp_path):
    from pytorch_rt1_for_distributed_training_amd.engine.trainer import Trainer
    from pytorch_rt1_for_distributed_training_amd.utils.checkpoint import build_checkpoint, save_checkpoint
    cfg = _cfg()
    batches = _batches(cfg, 3)
    run = _engine(cfg, milestones=(1,))
    for b in batches[:2]:
        run.train_step(b)
    run.epoch_end()                                                 # the milestone: every group's lr times 0.1
    torch.cuda.synchronize()
    want_lrs = dict(new=LR * 0.1, new_no_decay=LR * 0.1, backbone=LR * MULT * 0.1, backbone_no_decay=LR * MULT * 0.1)
    assert run.lrs == pytest.approx(want_lrs)
    path = str(tmp_path / "last.ckpt")
    save_checkpoint(path, build_checkpoint(run.model, run.optimizer, run.scheduler, epoch=0,
                                           global_step=run.global_step))
    fresh = _engine(cfg, milestones=(1,))
    assert fresh.lrs["new"] == LR
    Trainer(fresh, verbose=False).resume(path)
    assert fresh.lrs == pytest.approx(want_lrs) and list(fresh.lrs) == list(want_lrs)
    assert fresh.optimizer.step_count == 2 and fresh.global_step == 2
    assert fresh.scheduler.get_last_lr() == pytest.approx(list(want_lrs.values()))
    la, lb = run.train_step(batches[2]), fresh.train_step(batches[2])
    torch.cuda.synchronize()
    assert torch.equal(la, lb)
    assert torch.equal(run.flat.data, fresh.flat.data)
    assert torch.equal(run.optimizer.exp_avg_sq, fresh.optimizer.exp_avg_sq)
    assert torch.equal(run.optimizer.group_state, fresh.optimizer.group_state)
    # other flags, another layout: the run stops and names both
    other = _engine(cfg, backbone_lr_mult=1.0)
    with pytest.raises(ValueError, match="parameter groups") as e:
        Trainer(other, verbose=False).resume(path)
    assert "backbone_no_decay" in str(e.value) and "('new_no_decay'" in str(e.value)
    plain = _engine(cfg, grouped=False)
    with pytest.raises(ValueError, match="parameter groups") as e:
        Trainer(plain, verbose=False).resume(path)
    assert "'all'" in str(e.value) and "backbone" in str(e.value)
