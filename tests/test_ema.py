"""Exponential moving average of the weights (TrainEngine(ema_decay=...)) on the CPU, torch backend, tiny preset: the
torch fallback of the fused update against the fp64 oracle, its skip and accumulation semantics, the checkpoint entry
and its round trip through Trainer.resume, loading the averaged weights for evaluation, and the arguments.

The element-wise bound is the GPU test's: 2^-23 * (|want| + omd_t * |p - ema|).  The fallback rounds three times
(subtraction, product, sum: at most 2^-24 * (|want| + 2 omd_t |p - ema|)), which is within it."""
import json

import pytest
import torch

import pytorch_rt1_for_distributed_training_amd as rt1
from pytorch_rt1_for_distributed_training_amd.data.synthetic import make_batch
from pytorch_rt1_for_distributed_training_amd.ops.adam import reference_ema_step
from pytorch_rt1_for_distributed_training_amd.utils import checkpoint as C

EPS23 = 2.0 ** -23


def _cfg():
    return rt1.preset("tiny").replace(seq_len=2, dropout_rate=0.0, drop_connect_rate=0.0, crop_ratio=0.0)


def _engine(**kw):
    from pytorch_rt1_for_distributed_training_amd.engine.step import TrainEngine
    from pytorch_rt1_for_distributed_training_amd.models import build_rt1
    torch.manual_seed(0)
    cfg = _cfg()
    return TrainEngine(build_rt1(cfg), cfg, order_probe=False, **kw)


def _batches(n, seed=123):
    g = torch.Generator().manual_seed(seed)
    return [make_batch(2, 2, 64, 64, uint8=False, generator=g) for _ in range(n)]


def _assert_ema(got, e_prev, p_new, omd_t):
    want = reference_ema_step(e_prev, p_new, omd_t)
    assert want.dtype == torch.float64
    bound = EPS23 * (want.abs() + omd_t * (p_new.double() - e_prev.double()).abs())
    err = (got.double() - want).abs()
    assert bool((err <= bound).all()), f"{int((err > bound).sum())} elements beyond the bound, max {float(err.max())}"


def _trainable_names(model):
    return {"model." + n for n, p in model.named_parameters() if p.requires_grad}


class _MemoryLogger:
    def __init__(self):
        self.rows = []

    def log(self, metrics, step, epoch):
        self.rows.append(dict(metrics, step=step))

    def flush(self):
        pass


# ------------------------------------------------------------------------------------------------ 14. torch fallback
@pytest.mark.parametrize("decay,warmup", [(0.999, True), (0.9, False)])
def test_fallback_follows_the_recurrence(decay, warmup):
    eng = _engine(ema_decay=decay, ema_warmup=warmup)
    opt = eng.optimizer
    assert opt._kernel is None and torch.equal(opt.ema, eng.flat.data)
    assert opt.ema.data_ptr() != eng.flat.data.data_ptr()
    omd32 = float(torch.tensor(1.0 - decay, dtype=torch.float32))
    for step, b in enumerate(_batches(3), 1):
        e_prev = opt.ema.clone()
        eng.train_step(b)
        omd_t = float(opt.ema_state[0])
        if warmup:
            assert omd_t == pytest.approx(max(1.0 - decay, 9.0 / (10.0 + step)), rel=1e-6, abs=0)
        else:
            assert omd_t == omd32
        assert opt.ema_state.tolist()[1:] == [float(step), 0.0, 0.0]
        assert float(opt.ema_decay_now) == pytest.approx(1.0 - omd_t, rel=1e-6)
        _assert_ema(opt.ema, e_prev, eng.flat.data, omd_t)
        assert not torch.equal(opt.ema, e_prev) and not torch.equal(opt.ema, eng.flat.data)


def test_fallback_skipped_step_leaves_the_average_alone():
    bs = _batches(5)
    bs[2]["train_observation"]["image"].fill_(float("nan"))
    eng = _engine(skip_nonfinite=True, ema_decay=0.999)
    opt = eng.optimizer
    for i, b in enumerate(bs):
        before = (opt.ema.clone(), opt.ema_state.clone())
        eng.train_step(b)
        if i == 2:
            assert opt.skipped_steps == 1
            assert torch.equal(opt.ema, before[0]) and torch.equal(opt.ema_state, before[1])
        else:
            assert not torch.equal(opt.ema, before[0])
    assert opt.step_count == 5 and float(opt.ema_state[1]) == 4.0 and opt.ema_num_updates == 4
    clean = _engine(ema_decay=0.999)
    for i in (0, 1, 3, 4):
        clean.train_step(bs[i])
    assert torch.equal(opt.ema, clean.optimizer.ema)
    assert torch.equal(opt.ema_state, clean.optimizer.ema_state)
    assert torch.equal(eng.flat.data, clean.flat.data)


def test_fallback_accumulation_updates_the_average_once_per_window():
    eng = _engine(accumulate_grad_batches=2, ema_decay=0.999)
    opt = eng.optimizer
    for i, b in enumerate(_batches(6)):
        before = (opt.ema.clone(), opt.ema_state.clone())
        eng.train_step(b)
        if i % 2 == 0:
            assert not eng.stepped
            assert torch.equal(opt.ema, before[0]) and torch.equal(opt.ema_state, before[1])
            with pytest.raises(RuntimeError, match="accumulation window"):
                with eng.ema_weights():
                    pass
        else:
            assert eng.stepped and not torch.equal(opt.ema, before[0])
    assert float(opt.ema_state[1]) == 3.0 and eng.global_step == 3


def test_ema_weights_swaps_contents_and_restores_them():
    eng = _engine(ema_decay=0.9, ema_warmup=False)
    bs = _batches(4)
    for b in bs[:3]:
        eng.train_step(b)
    live, ptr = eng.flat.data.clone(), eng.flat.data.data_ptr()
    loss_live = eng.eval_step(bs[3])
    with eng.ema_weights():
        assert torch.equal(eng.flat.data, eng.optimizer.ema) and eng.flat.data.data_ptr() == ptr
        loss_ema = eng.eval_step(bs[3])
    assert torch.equal(eng.flat.data, live) and not torch.equal(loss_ema, loss_live)
    with pytest.raises(ZeroDivisionError):
        with eng.ema_weights():
            1 / 0
    assert torch.equal(eng.flat.data, live)                  # restored when the body raises, too
    with pytest.raises(RuntimeError, match="EMA is off"):
        with _engine().ema_weights():
            pass


# ------------------------------------------------------------------------------------------------ 15. checkpoint
def _fit(tmp, ema_decay, skip=False):
    from pytorch_rt1_for_distributed_training_amd.engine.trainer import Trainer
    from pytorch_rt1_for_distributed_training_amd.utils.logging import MultiLogger
    kw = dict(ema_decay=ema_decay) if ema_decay else {}
    eng = _engine(milestones=[1], skip_nonfinite=skip, **kw)
    log = _MemoryLogger()
    tr = Trainer(eng, max_epochs=2, log_every_n_steps=1, checkpoint=C.ModelCheckpoint(str(tmp)),
                 logger=MultiLogger([log]), num_sanity_val_steps=0, verbose=False)
    train = _batches(3)
    if skip:
        train[1]["train_observation"]["image"].fill_(float("nan"))
    tr.fit(train, _batches(2, seed=5))
    return dict(eng=eng, tr=tr, rows=log.rows, last=str(tmp / "last.ckpt"))


@pytest.fixture(scope="module")
def ema_run(tmp_path_factory):
    """Two epochs of three batches with the EMA and the non-finite skip on (one batch per epoch is skipped)."""
    return _fit(tmp_path_factory.mktemp("ema_on"), 0.999, skip=True)


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    return _fit(tmp_path_factory.mktemp("ema_off"), 0.0)


def test_checkpoint_entry_layout(ema_run, plain_run):
    eng = ema_run["eng"]
    ck, plain = C.load_checkpoint(ema_run["last"]), C.load_checkpoint(plain_run["last"])
    assert "ema" not in plain
    assert set(ck) == set(plain) | {"ema"}
    for k in plain:
        assert type(ck[k]) is type(plain[k]), k
    assert list(ck["state_dict"]) == list(plain["state_dict"])
    ema = ck["ema"]
    assert set(ema) == {"decay", "warmup", "num_updates", "state_dict"}
    assert ema["decay"] == 0.999 and ema["warmup"] is True
    opt = eng.optimizer
    assert opt.step_count == 6 and opt.skipped_steps == 2
    assert ema["num_updates"] == opt.step_count - opt.skipped_steps == 4
    assert set(ema["state_dict"]) == _trainable_names(eng.model)
    assert "model._action_token_emb.weight" not in ema["state_dict"]
    assert not any("running_" in k or "num_batches" in k for k in ema["state_dict"])
    sd = opt.ema_state_dict()
    for k, v in ema["state_dict"].items():
        assert v.device.type == "cpu" and v.shape == ck["state_dict"][k].shape
        assert torch.equal(v, sd[k[len("model."):]]), k
    assert any(not torch.equal(v, ck["state_dict"][k]) for k, v in ema["state_dict"].items())


def test_resume_restores_the_average_and_continues_bitwise(ema_run):
    from pytorch_rt1_for_distributed_training_amd.engine.trainer import Trainer
    eng = ema_run["eng"]
    fresh = _engine(milestones=[1], skip_nonfinite=True, ema_decay=0.999)
    with torch.no_grad():
        fresh.optimizer.ema.mul_(2.0)                       # anything but the answer
    tr = Trainer(fresh, max_epochs=3, verbose=False)
    tr.resume(ema_run["last"])
    assert tr.current_epoch == 2 and fresh.global_step == eng.global_step
    assert torch.equal(fresh.flat.data, eng.flat.data)
    assert torch.equal(fresh.optimizer.ema, eng.optimizer.ema)
    assert float(fresh.optimizer.ema_state[1]) == float(eng.optimizer.ema_state[1]) == 4.0
    assert fresh.optimizer.ema_num_updates == 4
    # one more step: the resumed engine and a copy of the uninterrupted one agree bitwise (the uninterrupted engine's
    # state is restored afterwards: other tests read the fixture)
    snap = eng._snapshot()
    b = _batches(1, seed=9)[0]
    la, lb = eng.train_step(b), fresh.train_step(b)
    try:
        assert torch.equal(la, lb)
        assert torch.equal(fresh.flat.data, eng.flat.data)
        assert torch.equal(fresh.optimizer.ema, eng.optimizer.ema)
        assert torch.equal(fresh.optimizer.ema_state, eng.optimizer.ema_state)
        assert float(fresh.optimizer.ema_state[1]) == 5.0
    finally:
        eng._restore(snap)


# ------------------------------------------------------------------------------------------------ 16. mixed resumes
def test_resume_without_the_entry_starts_the_average_at_the_weights(plain_run):
    from pytorch_rt1_for_distributed_training_amd.engine.trainer import Trainer
    fresh = _engine(milestones=[1], ema_decay=0.999)
    with torch.no_grad():
        fresh.optimizer.ema.mul_(2.0)
    Trainer(fresh, max_epochs=3, verbose=False).resume(plain_run["last"])
    assert torch.equal(fresh.flat.data, plain_run["eng"].flat.data)
    assert torch.equal(fresh.optimizer.ema, fresh.flat.data)


def test_resume_with_the_entry_into_an_engine_without_ema_ignores_it(ema_run):
    from pytorch_rt1_for_distributed_training_amd.engine.trainer import Trainer
    fresh = _engine(milestones=[1], skip_nonfinite=True)
    tr = Trainer(fresh, max_epochs=3, verbose=False)
    tr.resume(ema_run["last"])
    assert fresh.optimizer.ema is None and "eval_loss_ema" not in tr.history
    assert torch.equal(fresh.flat.data, ema_run["eng"].flat.data)
    fresh.train_step(_batches(1, seed=9)[0])


# ------------------------------------------------------------------------------------------------ 17. loading, logging
def test_load_model_state_overlays_the_average(ema_run, plain_run):
    from pytorch_rt1_for_distributed_training_amd.models import build_rt1
    eng = ema_run["eng"]
    ck = C.load_checkpoint(ema_run["last"])
    m = build_rt1(_cfg())
    C.load_model_state(m, ck, use_ema=True)
    avg = eng.optimizer.ema_state_dict()
    live = eng.model.state_dict()
    assert set(avg) < set(live)
    for k, v in m.state_dict().items():
        assert torch.equal(v, avg[k] if k in avg else live[k]), k
    m2 = build_rt1(_cfg())
    C.load_model_state(m2, ema_run["last"])                    # the default stays the live weights
    for k, v in m2.state_dict().items():
        assert torch.equal(v, live[k]), k
    with pytest.raises(KeyError, match="no 'ema' entry"):
        C.load_model_state(build_rt1(_cfg()), plain_run["last"], use_ema=True)


def test_policy_and_eval_cli_load_the_average(ema_run, plain_run, capsys):
    import eval_rt1
    from pytorch_rt1_for_distributed_training_amd.eval import RT1Policy
    eng = ema_run["eng"]
    pol = RT1Policy.from_checkpoint(ema_run["last"], _cfg(), device="cpu", use_ema=True)
    avg = eng.optimizer.ema_state_dict()
    got = dict(pol.model.named_parameters())
    for k, v in avg.items():
        assert torch.equal(got[k].detach(), v), k
    with pytest.raises(KeyError, match="no 'ema' entry"):
        RT1Policy.from_checkpoint(plain_run["last"], _cfg(), device="cpu", use_ema=True)
    argv = ["--env", "toy", "--episodes", "1", "--max_episode_steps", "2", "--height", "64", "--width", "64",
            "--seq_len", "2", "--num_layers", "2", "--device", "cpu", "--no_video"]
    assert eval_rt1.main(["--ckpt", ema_run["last"], "--ema"] + argv) == 0
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["episodes"] == 1
    with pytest.raises(KeyError, match="no 'ema' entry"):
        eval_rt1.main(["--ckpt", plain_run["last"], "--ema"] + argv)


def test_validation_logs_eval_loss_ema_only_when_on(ema_run, plain_run):
    on, off = ema_run, plain_run
    assert not any("eval_loss_ema" in r for r in off["rows"])
    assert "eval_loss_ema" not in off["tr"].history and off["tr"].last_ema_loss is None
    rows = [r for r in on["rows"] if "eval_loss_ema" in r]
    assert len(rows) == 2 and len(on["tr"].history["eval_loss_ema"]) == 2
    assert [r["eval_loss_ema"] for r in rows] == on["tr"].history["eval_loss_ema"]
    assert len(on["tr"].history["eval_loss"]) == 2
    assert set(off["tr"].history) == set(on["tr"].history) - {"eval_loss_ema"}
    assert on["tr"].history["eval_loss_ema"] != on["tr"].history["eval_loss"]
    # the file names are those of the live weights
    import os
    names = sorted(os.listdir(os.path.dirname(on["last"])))
    assert len(names) == 3 and all("ema" not in n for n in names)
    # a direct call logs it too, under the pass's name
    tr = on["tr"]
    n = len(on["rows"])
    tr.validate(_batches(1, seed=5), name="test_loss")
    assert [k for r in on["rows"][n:] for k in r if k.endswith("_ema")] == ["test_loss_ema"]


def test_cli_flags():
    import distribute_train
    p = distribute_train.build_parser()
    a = p.parse_args([])
    assert a.ema_decay == 0.0 and a.no_ema_warmup is False
    a = p.parse_args(["--ema_decay", "0.9999", "--no_ema_warmup"])
    assert a.ema_decay == 0.9999 and a.no_ema_warmup is True


# ------------------------------------------------------------------------------------------------ 18. arguments
@pytest.mark.parametrize("bad", [1.0, -0.1, 1.5])
def test_decay_outside_the_unit_interval_raises(bad):
    from pytorch_rt1_for_distributed_training_amd.engine.optim import FlatAdam
    from pytorch_rt1_for_distributed_training_amd.parallel.flat import FlatParameters
    flat = FlatParameters([torch.nn.Parameter(torch.zeros(8))])
    with pytest.raises(ValueError, match="ema_decay"):
        FlatAdam(flat, ema_decay=bad)
    with pytest.raises(ValueError, match="ema_decay"):
        _engine(ema_decay=bad)


def test_ema_off_by_default_and_state_dict_without_names():
    from pytorch_rt1_for_distributed_training_amd.engine.optim import FlatAdam
    from pytorch_rt1_for_distributed_training_amd.parallel.flat import FlatParameters
    ps = [torch.nn.Parameter(torch.randn(5)), torch.nn.Parameter(torch.randn(2, 3))]
    off = FlatAdam(FlatParameters(ps))
    assert off.ema is None and off.ema_state is None and off.ema_decay_now is None
    with pytest.raises(RuntimeError, match="EMA is off"):
        off.ema_state_dict()
    assert C.ema_entry(off) is None
    on = FlatAdam(FlatParameters(ps), ema_decay=0.5, ema_warmup=False)
    sd = on.ema_state_dict()
    assert [tuple(v.shape) for v in sd.values()] == [(5,), (2, 3)]
    with torch.no_grad():
        on.ema.zero_()
    on.load_ema_state_dict(sd, num_updates=3)
    assert torch.equal(on.ema, on.flat.data) and on.ema_state.tolist() == [0.5, 3.0, 0.0, 0.0]
    on.ema.zero_()
    on.reset_ema()
    assert torch.equal(on.ema, on.flat.data)
    with pytest.raises(KeyError):
        on.load_ema_state_dict({})
