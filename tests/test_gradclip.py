"""Global-norm gradient clipping and the non-finite step skip on the CPU (torch fallback of the clip kernels):
FlatAdam against torch, skip semantics, the engine and trainer on the tiny preset, two gloo ranks, the CLI flags."""
import math
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

import pytorch_rt1_for_distributed_training_amd as rt1
from pytorch_rt1_for_distributed_training_amd.data.synthetic import make_batch
from pytorch_rt1_for_distributed_training_amd.engine.optim import FlatAdam
from pytorch_rt1_for_distributed_training_amd.parallel.flat import FlatParameters

SHAPES = [(7,), (64, 40), (1000,)]


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(*s, generator=g)) for s in SHAPES]


def _grads(step, scale=1.0):
    g = torch.Generator().manual_seed(100 + step)
    return [torch.randn(*s, generator=g) * scale for s in SHAPES]


def _flat_adam(**kw):
    params = _params()
    flat = FlatParameters(params)
    return params, flat, FlatAdam(flat, lr=5e-4, **kw)


def _feed(params, opt, grads):
    with torch.no_grad():
        for p, g in zip(params, grads):
            p.grad.copy_(g)
    opt.step()


def _state(flat, opt):
    return flat.data.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------- 1. FlatAdam vs torch
def test_flat_adam_clip_matches_torch_clip_grad_norm():
    params, flat, opt = _flat_adam(max_grad_norm=0.1)
    ref = [torch.nn.Parameter(p.detach().clone()) for p in _params()]
    ref_opt = torch.optim.Adam(ref, lr=5e-4)
    for step in range(1, 6):
        grads = _grads(step)                      # norm ~ sqrt(3567) >> 0.1
        _feed(params, opt, grads)
        for p, g in zip(ref, grads):
            p.grad = g.clone()
        total = torch.nn.utils.clip_grad_norm_(ref, 0.1)
        assert float(total) > 10.0
        torch.testing.assert_close(float(opt.last_grad_norm), float(total), rtol=1e-5, atol=0)
        ref_opt.step()
    assert opt.clipped_steps == 5 and opt.skipped_steps == 0
    for p, r in zip(params, ref):
        torch.testing.assert_close(p.detach(), r.detach(), rtol=1e-5, atol=1e-6)
    for i, (r, o) in enumerate(zip(ref, flat.offsets)):
        n = r.numel()
        st = ref_opt.state[r]
        torch.testing.assert_close(opt.exp_avg[o:o + n].view_as(r), st["exp_avg"], rtol=1e-5, atol=1e-7)
        torch.testing.assert_close(opt.exp_avg_sq[o:o + n].view_as(r), st["exp_avg_sq"], rtol=1e-5, atol=1e-8)


def test_flat_adam_inactive_clip_is_bitwise_the_plain_optimizer():
    params, flat, opt = _flat_adam(max_grad_norm=1e30)
    params0, flat0, opt0 = _flat_adam()
    assert opt0.clip_state is None and not opt0.clip_enabled
    for step in range(1, 6):
        _feed(params, opt, _grads(step))
        _feed(params0, opt0, _grads(step))
    assert opt.clipped_steps == 0
    assert _same(_state(flat, opt), _state(flat0, opt0))
    assert float(opt.clip_state[1]) == 1.0 and float(opt.clip_state[2]) == 1.0


# ---------------------------------------------------------------------------------------------- 2. skip semantics
def test_skipped_step_leaves_no_trace_and_checkpoint_carries_the_effective_step():
    params, flat, opt = _flat_adam(skip_nonfinite=True)
    clean_p, clean_flat, clean = _flat_adam()              # only ever given steps 1, 2, 4, 5
    after2 = None
    for step in range(1, 6):
        grads = _grads(step)
        if step == 3:
            grads[1][5, 7] = float("nan")
        else:
            _feed(clean_p, clean, _grads(step))
        _feed(params, opt, grads)
        if step == 2:
            after2 = _state(flat, opt)
        if step == 3:
            assert _same(_state(flat, opt), after2)
            assert float(opt.clip_state[2]) == 0.0 and float(opt.clip_state[5]) == 1.0
            assert not math.isfinite(float(opt.last_grad_norm))
    assert _same(_state(flat, opt), _state(clean_flat, clean))
    assert opt.skipped_steps == 1 and opt.step_count == 5
    assert float(opt.clip_state[5]) == 0.0
    sd = opt.state_dict()
    assert float(sd["state"][0]["step"]) == 4
    # round trip: a fresh optimizer continues exactly like the uninterrupted ones
    params2, flat2, opt2 = _flat_adam(skip_nonfinite=True)
    with torch.no_grad():
        flat2.data.copy_(flat.data)
    opt2.load_state_dict(sd)
    assert opt2.step_count == 4 and opt2.skipped_steps == 0
    for ps, o in ((params, opt), (params2, opt2), (clean_p, clean)):
        _feed(ps, o, _grads(6))
    assert _same(_state(flat2, opt2), _state(flat, opt))
    assert _same(_state(flat2, opt2), _state(clean_flat, clean))


def test_nonfinite_gradient_without_skip_is_not_hidden():
    params, flat, opt = _flat_adam(max_grad_norm=1.0)
    grads = _grads(1)
    grads[2][-1] = float("inf")
    _feed(params, opt, grads)
    assert float(opt.clip_state[1]) == 1.0 and float(opt.clip_state[2]) == 1.0 and opt.skipped_steps == 0
    assert not torch.isfinite(flat.data).all()


# ---------------------------------------------------------------------------------------------- 3. engine, tiny preset
def _cfg():
    return rt1.preset("tiny").replace(seq_len=2)


def _engine(**kw):
    from pytorch_rt1_for_distributed_training_amd.engine.step import TrainEngine
    from pytorch_rt1_for_distributed_training_amd.models import build_rt1
    torch.manual_seed(0)
    cfg = _cfg()
    return TrainEngine(build_rt1(cfg), cfg, order_probe=False, **kw)


def _loader(nan_at=(1,), n=3):
    g = torch.Generator().manual_seed(123)
    out = []
    for i in range(n):
        b = make_batch(2, 2, 64, 64, uint8=False, generator=g)
        if i in nan_at:
            b["train_observation"]["natural_language_embedding"].fill_(float("nan"))
        out.append(b)
    return out


def _running_stats(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()
            if k.endswith("running_mean") or k.endswith("running_var")}


def test_engine_skips_a_nan_batch_and_rolls_bn_statistics_back():
    batches = _loader()
    eng = _engine(skip_nonfinite=True)
    assert eng._bn_flat is not None and eng._bn_flat.numel() >= 87_296
    l1 = eng.train_step(batches[0])
    assert math.isfinite(float(l1))
    params1, stats1 = eng.flat.data.clone(), _running_stats(eng.model)
    assert stats1
    l2 = eng.train_step(batches[1])
    assert not math.isfinite(float(l2))
    assert torch.equal(eng.flat.data, params1) and torch.isfinite(eng.flat.data).all()
    stats2 = _running_stats(eng.model)
    for k, v in stats1.items():
        assert torch.isfinite(stats2[k]).all() and torch.equal(stats2[k], v), k
    assert eng.optimizer.skipped_steps == 1
    l3 = eng.train_step(batches[2])
    assert math.isfinite(float(l3))
    assert not torch.equal(eng.flat.data, params1)
    # what it protects against: the same sequence without the option
    plain = _engine()
    for b in batches:
        plain.train_step(b)
    assert not torch.isfinite(plain.flat.data).all()
    assert any(not torch.isfinite(v).all() for v in _running_stats(plain.model).values())


# ---------------------------------------------------------------------------------------------- 4. Trainer.fit
class _MemoryLogger:
    def __init__(self):
        self.rows = []

    def log(self, metrics, step, epoch):
        self.rows.append(dict(metrics, step=step))

    def flush(self):
        pass


def _fit(loader, **kw):
    from pytorch_rt1_for_distributed_training_amd.engine.trainer import Trainer
    from pytorch_rt1_for_distributed_training_amd.utils.logging import MultiLogger
    eng = _engine(skip_nonfinite=True, **kw)
    log = _MemoryLogger()
    tr = Trainer(eng, max_epochs=1, log_every_n_steps=1, logger=MultiLogger([log]), verbose=False)
    tr.fit(loader)
    return tr, log


def test_trainer_survives_one_bad_batch_and_logs_it():
    tr, log = _fit(_loader(), max_grad_norm=1e3)
    steps = [r for r in log.rows if "skipped_steps" in r]
    assert [r["step"] for r in steps] == [1, 2, 3]
    assert [r["skipped_steps"] for r in steps] == [0, 1, 1]
    assert all("clipped_steps" in r and "grad_norm" in r for r in steps)
    assert math.isfinite(steps[0]["train_loss_step"]) and math.isfinite(steps[2]["train_loss_step"])
    assert "train_loss_step" not in steps[1]
    epoch = tr.history["train_loss_epoch"]
    assert len(epoch) == 1 and math.isfinite(epoch[0])
    # the epoch mean is the mean over the two finite steps
    torch.testing.assert_close(epoch[0], (steps[0]["train_loss_step"] + steps[2]["train_loss_step"]) / 2,
                               rtol=1e-6, atol=0)


def test_trainer_raises_when_every_batch_is_bad():
    from pytorch_rt1_for_distributed_training_amd.engine.trainer import NonFiniteLoss
    with pytest.raises(NonFiniteLoss):
        _fit(_loader(nan_at=(0, 1, 2)))


# ---------------------------------------------------------------------------------------------- 5. two gloo ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_cfg():
    return _cfg().replace(dropout_rate=0.0, drop_connect_rate=0.0, crop_ratio=0.0)


def _dp_worker(rank, world, port, out_dir):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    torch.set_num_threads(2)
    from pytorch_rt1_for_distributed_training_amd.engine.step import TrainEngine, split_batch
    from pytorch_rt1_for_distributed_training_amd.models import build_rt1
    from pytorch_rt1_for_distributed_training_amd.parallel import dist as pdist
    pdist.init_distributed("cpu")
    torch.manual_seed(1000 + rank)
    cfg = _dp_cfg()
    eng = TrainEngine(build_rt1(cfg), cfg, order_probe=True, max_grad_norm=0.05, skip_nonfinite=True)
    g = torch.Generator().manual_seed(7 + rank)                  # a different batch per rank
    batch = make_batch(2, 2, 64, 64, uint8=False, generator=g)
    # this rank's unclipped gradient, on a clone of the (broadcast) initial state
    ref = build_rt1(cfg)
    ref.load_state_dict(eng.model.state_dict())
    ref.train()
    loss_bt, _ = ref.train_forward(*split_batch(batch), with_aux=False)
    loss_bt.mean().backward()
    names = [n for n, p in eng.model.named_parameters() if p.requires_grad]
    ref_params = dict(ref.named_parameters())
    grad = torch.cat([(ref_params[n].grad if ref_params[n].grad is not None else torch.zeros_like(ref_params[n]))
                      .reshape(-1) for n in names])
    eng.train_step(batch)
    params = torch.cat([p.detach().reshape(-1) for n, p in eng.model.named_parameters()])
    torch.save({"grad": grad, "params": params, "clip": eng.optimizer.clip_state.clone()},
               os.path.join(out_dir, f"rank{rank}.pt"))
    pdist.shutdown()


def test_two_ranks_take_the_same_clip_decision_without_another_collective(tmp_path):
    world = 2
    mp.start_processes(_dp_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True,
                       start_method="spawn")
    r0 = torch.load(tmp_path / "rank0.pt", weights_only=True)
    r1 = torch.load(tmp_path / "rank1.pt", weights_only=True)
    assert torch.equal(r0["params"], r1["params"])
    assert torch.equal(r0["clip"], r1["clip"])
    assert not torch.equal(r0["grad"], r1["grad"])
    want = float(((r0["grad"].double() + r1["grad"].double()) / 2).pow(2).sum().sqrt())
    assert want > 0.05
    torch.testing.assert_close(float(r0["clip"][0]), want, rtol=1e-5, atol=0)
    assert float(r0["clip"][1]) < 1.0 and float(r0["clip"][2]) == 1.0 and float(r0["clip"][4]) == 1.0


# ---------------------------------------------------------------------------------------------- 6. CLI
def test_cli_flags_default_off():
    import distribute_train
    p = distribute_train.build_parser()
    a = p.parse_args([])
    assert a.gradient_clip_val == 0 and a.skip_nonfinite_steps is False
    a = p.parse_args(["--gradient_clip_val", "0.5", "--skip_nonfinite_steps"])
    assert a.gradient_clip_val == 0.5 and a.skip_nonfinite_steps is True
