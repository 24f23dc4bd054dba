"""Layer-wise trust ratios (FlatAdam(layer_adapt=True), TrainEngine(optimizer="lamb")) on the CPU: the torch fallback
against the fp64 oracle ops.adam.reference_lamb_step on the kernel tests' layouts A and D, the tensor tables against
flat.offsets, the flag build_param_groups gives each group, the arguments, the state dict in torch-AdamW's layout and
the resume message.

Tolerances: the fallback works in fp32 with fp64 norms, so an element of p carries a few fp32 roundings of
lr * r * u on top of the rounding of p itself: rtol 1e-5 with atol 1e-6 (the GPU test's bound for p), and 1e-6 relative
on the trust ratios and norms (fp32 roundings of fp64 sums of exactly representable squares)."""
import math

import pytest
import torch
import torch.nn as nn

import pytorch_rt1_for_distributed_training_amd as rt1
from pytorch_rt1_for_distributed_training_amd.data.synthetic import make_batch
from pytorch_rt1_for_distributed_training_amd.engine.optim import FlatAdam, build_param_groups
from pytorch_rt1_for_distributed_training_amd.ops.adam import reference_lamb_step
from pytorch_rt1_for_distributed_training_amd.parallel.flat import FlatParameters

A = [1, 63, 64, 65, 200, 4097]
BETAS = (0.9, 0.999)
EPS = 1e-8
LR = 1e-2


def _layout(case):
    """FlatParameters over tensors of the sizes A with seeded values; layout D: tensor 2 all-zero, tensor 3 never gets
    a gradient, tensor 4 in a group that is not adapted; wd = 0 for those three."""
    gen = torch.Generator().manual_seed(11)
    params = [nn.Parameter(torch.randn(n, generator=gen) * 10.0 ** float(torch.randint(-2, 2, (1,), generator=gen)))
              for n in A]
    groups = None
    if case == "D":
        with torch.no_grad():
            params[2].zero_()
        groups = [dict(name="decay", params=[params[i] for i in (0, 1, 5)], lr=LR, weight_decay=0.1),
                  dict(name="plain", params=[params[2], params[3]], lr=LR, weight_decay=0.0),
                  dict(name="fixed", params=[params[4]], lr=LR, weight_decay=0.0, layer_adapt=False)]
    flat = FlatParameters(params)
    opt = FlatAdam(flat, lr=LR, betas=BETAS, eps=EPS, weight_decay=0.1, use_kernel=False, groups=groups,
                   layer_adapt=True)
    return params, flat, opt


@pytest.mark.parametrize("case", ["A", "D"])
def test_torch_fallback_matches_the_fp64_oracle(case):
    params, flat, opt = _layout(case)
    starts = opt.tensor_chunk_start.tolist()
    adapt = opt.tensor_adapt.tolist()
    assert adapt == ([1, 1, 1, 1, 0, 1] if case == "D" else [1] * 6)
    p64 = flat.data.double().clone()
    m64, v64 = torch.zeros_like(p64), torch.zeros_like(p64)
    gen = torch.Generator().manual_seed(5)
    p_start = flat.data.clone()
    for step in range(1, 4):
        grad = torch.zeros(flat.numel)
        for i, (p, o) in enumerate(zip(flat.params, flat.offsets)):      # the padding carries no gradient
            if not (case == "D" and i == 3):
                grad[o:o + p.numel()] = torch.randn(p.numel(), generator=gen)
        flat.grad.copy_(grad)
        opt.step()
        if case == "D":
            lrs, wds = [LR, LR, LR], [0.1, 0.0, 0.0]
            trust, norms = reference_lamb_step(p64, grad.double(), m64, v64, starts, adapt, lr=lrs, beta1=BETAS[0],
                                               beta2=BETAS[1], eps=EPS, weight_decay=wds, step=step,
                                               chunk_group=opt.chunk_group)
        else:
            trust, norms = reference_lamb_step(p64, grad.double(), m64, v64, starts, adapt, lr=LR, beta1=BETAS[0],
                                               beta2=BETAS[1], eps=EPS, weight_decay=0.1, step=step)
        for name, got, want, rtol, atol in (("p", flat.data, p64, 1e-5, 1e-6), ("m", opt.exp_avg, m64, 1e-5, 1e-7),
                                            ("v", opt.exp_avg_sq, v64, 1e-5, 1e-8),
                                            ("trust", opt.trust, trust, 1e-6, 0.0),
                                            ("norms", opt.norms, norms, 1e-6, 0.0)):
            err = (got.double() - want).abs()
            tol = atol + rtol * want.abs()
            print(f"{case} step {step} {name}: max err {float(err.max()):.3e}, worst err - tol "
                  f"{float((err - tol).max()):.3e}")
            assert bool((err <= tol).all()), f"{case} step {step} {name}: {int((err > tol).sum())} beyond tolerance"
        if case == "D":
            # tensor 2 has ||p|| = 0 only until its first update moves it
            assert opt.trust[[3, 4]].tolist() == [1.0, 1.0] and (step > 1 or float(opt.trust[2]) == 1.0)
            o = flat.offsets[3]
            assert torch.equal(flat.data[o:o + 128], p_start[o:o + 128])       # ||u|| = 0: untouched
    for p, o in zip(flat.params, flat.offsets):                                  # the padding stays zero
        pad = slice(o + p.numel(), o + (p.numel() + 63) // 64 * 64)
        for buf in (flat.data, opt.exp_avg, opt.exp_avg_sq):
            assert not buf[pad].any()
    names = list(opt.trust_ratios())
    # names without a model: the state dict's indices, which follow the groups
    assert names == ([str(i) for i in range(6)] if case == "A" else ["0", "1", "3", "4", "5", "2"])
    assert opt.trust_ratios()["5"].dim() == 0
    pn, un = opt.last_update_norms()[names[5]]
    assert float(pn) > 0 and float(un) > 0 and float(opt.trust[5]) == pytest.approx(float(pn) / float(un), rel=1e-6)


class Small(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(3, 7, 3)
        self.bn = nn.BatchNorm2d(7)
        self.emb = nn.Embedding(11, 13)
        self.fc = nn.Linear(13, 70)
        self.frozen = nn.Linear(4, 4)
        for p in self.frozen.parameters():
            p.requires_grad_(False)


def test_tensor_tables_follow_the_flat_offsets():
    torch.manual_seed(0)
    model = Small()
    trainable = [p for p in model.parameters() if p.requires_grad]
    flat = FlatParameters(list(reversed(trainable)))
    groups = build_param_groups(model, 1e-3, 0.05, no_decay_norm_bias=True)
    assert {g["name"]: g.get("layer_adapt", True) for g in groups} == {"new": True, "new_no_decay": False}
    opt = FlatAdam(flat, lr=1e-3, weight_decay=0.05, all_params=list(model.parameters()), use_kernel=False,
                   groups=groups, layer_adapt=True)
    starts = opt.tensor_chunk_start.tolist()
    assert opt.tensor_chunk_start.dtype == torch.int32 and opt.tensor_adapt.dtype == torch.uint8
    assert len(starts) == len(flat.params) + 1 and starts[0] == 0 and starts[-1] == flat.numel // 64
    for i, (p, o) in enumerate(zip(flat.params, flat.offsets)):
        assert starts[i] * 64 == o and (starts[i + 1] - starts[i]) * 64 == (p.numel() + 63) // 64 * 64
    emb = model.emb.weight
    want = [0 if (p.ndim <= 1 or p is emb) else 1 for p in flat.params]
    assert opt.tensor_adapt.tolist() == want and 0 in want and 1 in want
    assert opt.trust.shape == (len(flat.params),) and opt.norms.shape == (len(flat.params), 2)
    # the flag stays with the optimizer: param_groups, and with them checkpoints, hold the keys they always held
    assert all("layer_adapt" not in g for g in opt.param_groups)
    assert all("layer_adapt" not in g for g in opt.state_dict()["param_groups"])
    # without groups every tensor adapts; with the option off nothing is built
    every = FlatAdam(FlatParameters([nn.Parameter(torch.randn(n)) for n in A]), use_kernel=False, layer_adapt=True)
    assert every.tensor_adapt.tolist() == [1] * 6 and every.tensor_chunk_start.tolist() == [0, 1, 2, 3, 5, 9, 74]
    off = FlatAdam(FlatParameters([nn.Parameter(torch.randn(n)) for n in A]), use_kernel=False)
    assert off.trust is None and off.norms is None and off.tensor_chunk_start is None and off.kind == "adam"
    with pytest.raises(RuntimeError, match="layer_adapt"):
        off.trust_ratios()


def test_optimizer_argument():
    import distribute_train
    p = distribute_train.build_parser()
    assert p.parse_args([]).optimizer == "adam"
    assert p.parse_args(["--optimizer", "lamb"]).optimizer == "lamb"
    with pytest.raises(SystemExit):
        p.parse_args(["--optimizer", "lars"])
    from pytorch_rt1_for_distributed_training_amd.engine.step import TrainEngine
    from pytorch_rt1_for_distributed_training_amd.models import build_rt1
    cfg = _cfg()
    with pytest.raises(ValueError, match="optimizer"):
        TrainEngine(build_rt1(cfg), cfg, order_probe=False, optimizer="lars")


def test_state_dict_round_trips_through_torch_adamw():
    """The state is Adam's: a torch.optim.AdamW over the same parameters loads it, and its own state dict loads back
    into a LAMB optimizer and into an Adam one."""
    params, flat, opt = _layout("A")
    gen = torch.Generator().manual_seed(3)
    for _ in range(2):
        for p in params:                                      # through the views: the padding carries no gradient
            p.grad.copy_(torch.randn(p.shape, generator=gen))
        opt.step()
    sd = opt.state_dict()
    assert sd["optimizer_kind"] == "lamb" and set(sd) == {"state", "param_groups", "optimizer_kind"}
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    adamw = torch.optim.AdamW(params, lr=LR, betas=BETAS, eps=EPS, weight_decay=0.1)
    adamw.load_state_dict(sd)                 # the stock optimizer takes the dict as it is: it reads two keys
    assert "optimizer_kind" not in adamw.state_dict()
    back = adamw.state_dict()
    for kind in (True, False):
        other_params = [nn.Parameter(p.detach().clone()) for p in params]
        other = FlatAdam(FlatParameters(other_params), lr=LR, betas=BETAS, eps=EPS, weight_decay=0.1,
                         use_kernel=False, layer_adapt=kind)
        other.load_state_dict(back)
        assert other.step_count == 2
        assert torch.equal(other.exp_avg, opt.exp_avg) and torch.equal(other.exp_avg_sq, opt.exp_avg_sq)
        assert ("optimizer_kind" in other.state_dict()) == kind
    # an Adam optimizer's state dict is what it always was
    plain = FlatAdam(FlatParameters([nn.Parameter(torch.randn(n)) for n in A]), use_kernel=False)
    plain.flat.grad.normal_()
    plain.step()
    assert set(plain.state_dict()) == {"state", "param_groups"}


def _cfg():
    return rt1.preset("tiny").replace(seq_len=2, dropout_rate=0.0, drop_connect_rate=0.0, crop_ratio=0.0)


def _engine(**kw):
    from pytorch_rt1_for_distributed_training_amd.engine.step import TrainEngine
    from pytorch_rt1_for_distributed_training_amd.models import build_rt1
    torch.manual_seed(0)
    cfg = _cfg()
    return TrainEngine(build_rt1(cfg), cfg, order_probe=False, **kw)


class _MemoryLogger:
    def __init__(self):
        self.rows = []

    def log(self, metrics, step, epoch):
        self.rows.append(dict(metrics, step=step))

    def flush(self):
        pass


def test_resume_message_and_trust_logging(tmp_path, capsys):
    from pytorch_rt1_for_distributed_training_amd.engine.trainer import Trainer
    from pytorch_rt1_for_distributed_training_amd.utils import checkpoint as C
    from pytorch_rt1_for_distributed_training_amd.utils.logging import MultiLogger
    g = torch.Generator().manual_seed(123)
    batches = [make_batch(2, 2, 64, 64, uint8=False, generator=g) for _ in range(3)]
    adam = _engine(no_decay_norm_bias=True, weight_decay=0.05)
    assert adam.optimizer.trust is None and adam.optimizer.kind == "adam"
    for b in batches[:2]:
        adam.train_step(b)
    path = str(tmp_path / "adam.ckpt")
    C.save_checkpoint(path, C.build_checkpoint(adam.model, adam.optimizer, adam.scheduler, epoch=0,
                                               global_step=adam.global_step))
    assert "optimizer_kind" not in C.load_checkpoint(path)["optimizer_states"][0]
    # an Adam checkpoint continues under LAMB: one line says so, the moments and the step are the checkpoint's
    lamb = _engine(optimizer="lamb", no_decay_norm_bias=True, weight_decay=0.05)
    log = _MemoryLogger()
    tr = Trainer(lamb, max_epochs=2, log_every_n_steps=1, logger=MultiLogger([log]), num_sanity_val_steps=0,
                 verbose=True)
    capsys.readouterr()
    tr.resume(path)
    lines = [l for l in capsys.readouterr().out.splitlines() if "optimizer" in l]
    assert len(lines) == 1 and "adam" in lines[0] and "lamb" in lines[0]
    assert lamb.optimizer.step_count == 2
    assert torch.equal(lamb.optimizer.exp_avg, adam.optimizer.exp_avg)
    assert torch.equal(lamb.optimizer.exp_avg_sq, adam.optimizer.exp_avg_sq)
    # the same kind: no line
    again = _engine(no_decay_norm_bias=True, weight_decay=0.05)
    Trainer(again, max_epochs=2, verbose=True).resume(path)
    assert not [l for l in capsys.readouterr().out.splitlines() if "was written by" in l]
    # training under LAMB logs the trust ratios at the log point, and the no-decay tensors keep ratio 1
    tr.fit(batches, None)
    rows = [r for r in log.rows if "trust/min" in r]
    assert rows and all(math.isfinite(r["train_loss_step"]) for r in rows)
    assert all(r["trust/min"] <= r["trust/median"] <= r["trust/max"] for r in rows)
    opt = lamb.optimizer
    small = [i for i, p in enumerate(lamb.flat.params) if p.ndim <= 1]
    assert small and opt.trust[small].tolist() == [1.0] * len(small)
    assert any(float(t) != 1.0 for t in opt.trust)
    # and the reverse: a LAMB checkpoint records its kind and continues under Adam with one line
    path2 = str(tmp_path / "lamb.ckpt")
    C.save_checkpoint(path2, C.build_checkpoint(lamb.model, opt, lamb.scheduler, epoch=0, global_step=lamb.global_step))
    assert C.load_checkpoint(path2)["optimizer_states"][0]["optimizer_kind"] == "lamb"
    back = _engine(no_decay_norm_bias=True, weight_decay=0.05)
    capsys.readouterr()
    Trainer(back, max_epochs=2, verbose=True).resume(path2)
    lines = [l for l in capsys.readouterr().out.splitlines() if "was written by" in l]
    assert len(lines) == 1 and "lamb" in lines[0]
    assert torch.equal(back.optimizer.exp_avg, opt.exp_avg) and back.optimizer.step_count == opt.step_count
