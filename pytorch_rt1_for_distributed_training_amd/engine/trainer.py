"""Epoch loop with Lightning-equivalent semantics (no Lightning dependency).

Mirrors what ``lightning.Trainer.fit`` + ``test`` do for the reference
(``distribute_train.py:192-247``): per-epoch ``DistributedSampler`` reshuffle,
``train_loss`` logged every ``log_every_n_steps`` and as an epoch mean
(``train_loss_step`` / ``train_loss_epoch``), a validation pass each epoch
(``eval_loss``), ``lr-Adam`` at epoch granularity (``LearningRateMonitor``),
MultiStepLR stepped per epoch, ``ModelCheckpoint`` on rank 0, resume from a
checkpoint (commented out in the reference, ``:240``, supported here), and a
final ``test`` pass (``test_loss``).

Differences: losses are accumulated on device and reduced across ranks only at
log points (the reference's ``sync_dist=True`` all-reduces a scalar every
step); ``eval_loss`` / ``test_loss`` are averaged over all ranks instead of
reporting rank 0's shard; a non-finite training loss aborts the run with the
step number (failure detection; the reference has none).  With the engine's
``skip_nonfinite`` a step with a non-finite gradient is skipped on the device
instead: the loss means are taken over the finite steps, ``grad_norm`` /
``clipped_steps`` / ``skipped_steps`` are logged at each log interval, and the
run aborts only when a whole log window (at least ``MIN_SKIPS_TO_ABORT``
consecutive steps) was skipped.

With the engine's ``accumulate_grad_batches=k`` a ``train_step`` is one micro-batch: steps, log points and
``global_step`` count optimizer steps (as Lightning does), ``train_loss_step`` is the mean over the micro-batches of
the logged windows, and a window left open when an epoch's batches run out is applied (``engine.flush_window``) before
validation, the LR scheduler and checkpointing, so no checkpoint ever holds a half-accumulated gradient.

With the engine's ``ema_decay > 0`` every validation also runs on the averaged weights and logs ``eval_loss_ema``,
checkpoints carry the average under one more top-level key, ``"ema"``, and ``resume`` restores it (or starts it at the
restored weights when the checkpoint has none).  ``eval_loss`` and the checkpoint file names are those of the live weights.

With more than one parameter group (the engine's ``no_decay_norm_bias`` / ``backbone_lr_mult``) each epoch also logs
``lr/<group>``; checkpoints carry the groups in the optimizer and scheduler states, and ``resume`` restores their names
and learning rates -- into the same group layout only: the resumed run's flags must reproduce it.

With the engine's ``lr_schedule`` the ``log_every_n_steps`` log point also logs ``lr-Adam`` (and ``lr/<group>`` with
several groups) as the last applied update used them, read back from the device at the point that already synchronises
for the loss; the per-epoch ``lr-Adam`` stays the base learning rate that ``MultiStepLR`` scales.

With the engine's ``optimizer="lamb"`` the same log point also logs ``trust/min``, ``trust/median`` and ``trust/max``,
the layer-wise trust ratios of the last applied update (one small device-to-host copy, never per step); ``resume``
says in one line when the checkpoint was written by the other optimizer kind (the state is the same).

With the engine's ``label_smoothing`` / ``z_loss`` the logged training loss is the regularised objective, so each log
point also logs ``train_nll_step``, the plain CE of the same batches; ``eval_loss`` / ``test_loss`` are the plain CE in
any case (the objective applies in training mode only).  With the engine's ``token_accuracy`` each log point logs
``train_acc_step`` = hits / rows of the action tokens since the last log point, summed over ranks (one more small
all-reduce), every validation logs ``eval_acc`` / ``test_acc`` (and ``..._ema`` where the EMA pass runs), and each of
these comes with its per-slot values ``<name>/tok0 .. tok{A-1}``.  The device counters are zeroed at each read; what
the training steps counted before a validation is set aside and put back after it.
"""
from __future__ import annotations

import math
import os
import time
from typing import Dict, Iterable, Optional

import torch

from ..data.prefetch import DevicePrefetcher
from ..parallel import dist as pdist
from ..utils.checkpoint import (PREFIX, ModelCheckpoint, build_checkpoint, ema_entry, load_checkpoint,
                                load_model_state)
from ..utils.logging import MultiLogger
from .step import TrainEngine


class NonFiniteLoss(RuntimeError):
    pass


# skip_nonfinite: consecutive skipped steps below which a log window made only of skipped steps is not yet fatal.  With
# log_every_n_steps=1 every skipped step is such a window, and surviving one bad batch is what the option is for.
MIN_SKIPS_TO_ABORT = 2


class Trainer:
    def __init__(self, engine: TrainEngine, max_epochs: int = 100, log_every_n_steps: int = 500,
                 checkpoint: Optional[ModelCheckpoint] = None, logger: Optional[MultiLogger] = None,
                 limit_train_batches: Optional[int] = None, limit_val_batches: Optional[int] = None,
                 num_sanity_val_steps: int = 2, verbose: bool = True, batch_transform=None):
        self.engine = engine
        self.batch_transform = batch_transform   # device-side batch transform (GPU crop+resize of raw frames)
        self.max_epochs = max_epochs
        self.log_every = max(1, log_every_n_steps)
        self.ckpt = checkpoint
        self.logger = logger or MultiLogger([])
        self.limit_train = limit_train_batches
        self.limit_val = limit_val_batches
        self.sanity = num_sanity_val_steps
        self.verbose = verbose and pdist.context().is_main
        self.current_epoch = 0
        self.history: Dict[str, list] = {"train_loss_epoch": [], "eval_loss": [], "samples_per_sec": []}
        self.last_ema_loss = None                # validate(): loss on the averaged weights (engine EMA on)
        if getattr(engine.optimizer, "ema", None) is not None:
            self.history["eval_loss_ema"] = []
        self.acc_on = getattr(engine, "token_counters", None) is not None
        self.nll_on = bool(getattr(engine, "regularised", False))
        self.last_acc: Dict[str, float] = {}     # validate(): the accuracy metrics it logged (token_accuracy on)
        if self.acc_on:
            self.history["eval_acc"] = []
        self.graph_checked = False
        self.graph_check = None

    # ------------------------------------------------------------------ helpers
    def _iter(self, loader, limit):
        pf = self.prefetcher = DevicePrefetcher(loader, self.engine.device, transform=self.batch_transform)
        it = iter(pf)
        try:
            for i, b in enumerate(it):
                if limit is not None and i >= limit:
                    break
                yield b
        finally:
            it.close()                       # stops the loader thread and fills pf.stats (input-path timing)

    def _mean_across(self, total: torch.Tensor, count: int) -> float:
        t = torch.stack([total.detach().double().reshape(()),
                         torch.tensor(float(count), dtype=torch.float64, device=total.device)])
        t = pdist.all_reduce_mean(t)
        return float(t[0] / t[1]) if float(t[1]) > 0 else float("nan")

    def _acc_metrics(self, name: str) -> Dict[str, float]:
        """Read and zero the engine's token counters: ``{name: hits / rows, name/tok<a>: per slot}`` over all ranks
        (the mean over ranks of both columns: their ratio is that of the sums).  Empty without rows."""
        c = pdist.all_reduce_mean(self.engine.read_token_counters().double())
        hits, rows = c[:, 0], c[:, 1]
        if float(rows.sum()) <= 0:
            return {}
        out = {name: float(hits.sum() / rows.sum())}
        for a in range(c.shape[0]):
            if float(rows[a]) > 0:
                out[f"{name}/tok{a}"] = float(hits[a] / rows[a])
        return out

    def _log(self, metrics, step=None):
        step = self.engine.global_step if step is None else step
        if pdist.context().is_main:
            self.logger.log(metrics, step, self.current_epoch)

    def _make_ckpt(self, callbacks):
        e = self.engine
        return build_checkpoint(e.model, e.optimizer, e.scheduler, epoch=self.current_epoch,
                                global_step=e.global_step, callbacks=callbacks, ema=ema_entry(e.optimizer))

    def _check_graph(self, batch):
        """Once, right after the hipGraph step is captured: one replayed step and one eager step on the same batch from
        the same state (TrainEngine.graph_eager_check, the engine is left untouched) must agree bitwise on every rank;
        otherwise training continues on the eager (hook-driven, bucketed) step.  This is what makes the segmented
        graph-DP step safe to use under RCCL by default."""
        e = self.engine
        self.graph_checked = True
        res = e.graph_eager_check(batch)
        if res is None:
            return
        ok = pdist.all_true(res["equal"])
        self.graph_check = dict(res, all_ranks_equal=ok)
        if self.verbose:
            print(f"[trainer] hipGraph step vs eager step on one batch: {'bitwise equal' if ok else 'DIFFERENT'} "
                  f"({res})", flush=True)
        if not ok:
            if self.verbose:
                print("[trainer] falling back to the eager step", flush=True)
            e.drop_graph()

    # ------------------------------------------------------------------ public
    def resume(self, path: str):
        ck = load_checkpoint(path, map_location="cpu")
        load_model_state(self.engine.model, ck)
        if ck.get("optimizer_states"):
            opt, saved = self.engine.optimizer, ck["optimizer_states"][0]
            if opt.group_layout(saved["param_groups"]) != opt.group_layout():
                raise ValueError(f"{path} was written with the parameter groups (name, parameters) "
                                 f"{opt.group_layout(saved['param_groups'])}, this run has {opt.group_layout()}: "
                                 f"resume with the --no_decay_norm_bias / --backbone_lr_mult of the run that wrote it")
            opt.load_state_dict(saved)
            # Adam and LAMB keep the same state (m, v, step): either continues from the other's checkpoint
            was, now = saved.get("optimizer_kind", "adam"), getattr(opt, "kind", "adam")
            if was != now and self.verbose:
                print(f"[trainer] {path} was written by the {was} optimizer, this run continues with {now} from its "
                      f"moments and step {opt.step_count}", flush=True)
        if ck.get("lr_schedulers"):
            self.engine.scheduler.load_state_dict(ck["lr_schedulers"][0])
        self.engine.global_step = int(ck.get("global_step", 0))
        self.current_epoch = int(ck.get("epoch", -1)) + 1
        if self.engine.ddp.enabled:
            self.engine.ddp.broadcast_parameters()
        self.engine.refresh_buffer_shadow()
        opt = self.engine.optimizer
        if getattr(opt, "ema", None) is not None:
            # every rank reads the same file, so the restored average needs no broadcast; a checkpoint without one
            # (trained with the EMA off) starts the average at the restored weights
            ema = ck.get("ema")
            if isinstance(ema, dict) and ema.get("state_dict"):
                opt.load_ema_state_dict({k[len(PREFIX):] if k.startswith(PREFIX) else k: v
                                         for k, v in ema["state_dict"].items()},
                                        num_updates=int(ema.get("num_updates", 0)))
            else:
                opt.reset_ema()

    def _eval_mean(self, loader, limit) -> float:
        total, n = None, 0
        for batch in self._iter(loader, limit):
            loss = self.engine.eval_step(batch)
            total = loss if total is None else total + loss
            n += 1
        if total is None:
            total = torch.zeros((), device=self.engine.device)
        return self._mean_across(total, n)

    def validate(self, loader, limit=None, name="eval_loss") -> float:
        """Mean loss over ``loader`` with the live weights (the return value).  With the engine's EMA on the pass
        runs once more on the averaged weights (``TrainEngine.ema_weights``) and logs ``<name>_ema``; the value is
        kept in ``last_ema_loss``."""
        acc_name = name[:-len("_loss")] + "_acc" if name.endswith("_loss") else name + "_acc"
        self.last_acc = {}
        # what the training steps counted since the last log point waits aside while the passes below count
        held = self.engine.read_token_counters() if self.acc_on else None
        loss = self._eval_mean(loader, limit)
        if self.acc_on:
            self.last_acc.update(self._acc_metrics(acc_name))
        self.last_ema_loss = None
        if getattr(self.engine.optimizer, "ema", None) is not None:
            with self.engine.ema_weights():
                self.last_ema_loss = self._eval_mean(loader, limit)
            self._log({name + "_ema": self.last_ema_loss})
            if self.acc_on:
                self.last_acc.update(self._acc_metrics(acc_name + "_ema"))
        if self.acc_on:
            self.engine.token_counters.add_(held)
            if self.last_acc:
                self._log(self.last_acc)
        return loss

    def fit(self, train_loader: Iterable, val_loader: Optional[Iterable] = None):
        """Train on a high-priority HIP stream when batches are decoded on the device: the prefetch stream's decode
        kernels (data/resident.py, data/shards.py) then only take workgroup slots the step leaves free instead of
        competing with it for the CUs (the step is one graph launch that keeps the chip busy).
        ``RT1_TRAIN_STREAM=normal`` keeps the default stream instead (A/B: a high-priority queue in the process has a
        cost of its own, ~1 ms per bench step measured for an idle one, profiles/r6_graph_dp_world1.log)."""
        e = self.engine
        if (e.device.type == "cuda" and self.batch_transform is not None
                and os.environ.get("RT1_TRAIN_STREAM", "high") != "normal"):
            _, hi = torch.cuda.Stream.priority_range()
            s = torch.cuda.Stream(device=e.device, priority=hi)
            s.wait_stream(torch.cuda.current_stream(e.device))
            try:
                with torch.cuda.stream(s):
                    self._fit(train_loader, val_loader)
            finally:
                torch.cuda.current_stream(e.device).wait_stream(s)
            return
        self._fit(train_loader, val_loader)

    def _fit(self, train_loader: Iterable, val_loader: Optional[Iterable] = None):
        e = self.engine
        if val_loader is not None and self.sanity > 0 and self.current_epoch == 0:
            self.validate(val_loader, self.sanity)
        for epoch in range(self.current_epoch, self.max_epochs):
            self.current_epoch = epoch
            sampler = getattr(train_loader, "sampler", None)
            if hasattr(sampler, "set_epoch"):
                sampler.set_epoch(epoch)
            elif hasattr(train_loader, "set_epoch"):
                train_loader.set_epoch(epoch)
            self._log({"lr-Adam": e.lr})
            if len(e.lrs) > 1:
                self._log({f"lr/{name}": v for name, v in e.lrs.items()})
            total, n, window, wn = None, 0, None, 0
            nwindow = None                           # plain CE of the window's batches (regularised objective)
            wsteps = 0                               # optimizer steps since the last log point (wn counts batches)
            samples = 0
            opt = e.optimizer
            clip_on = bool(getattr(opt, "clip_enabled", False))
            skip_on = bool(getattr(opt, "skip_nonfinite", False))
            sched_on = getattr(opt, "lr_schedule", None) is not None
            # skip_nonfinite: means over the finite-loss steps only (device-side masked sums and counts, no sync)
            tcount = wcount = None
            t0 = time.perf_counter()

            def log_point():
                # after a train_step (or the epoch-end flush) that applied the optimizer
                nonlocal window, wn, wcount, wsteps, nwindow
                wsteps += 1
                if e.global_step % self.log_every == 0:
                    step_loss = self._mean_across(window, wcount if skip_on else wn)
                    if skip_on:
                        # a skipped step is survived, a dead run is not: every step of this window skipped
                        # (MIN_SKIPS_TO_ABORT: a one-step window cannot tell the two apart)
                        streak = int(opt.clip_state[5])
                        if streak >= max(wsteps, MIN_SKIPS_TO_ABORT):
                            raise NonFiniteLoss(f"{streak} consecutive non-finite steps skipped up to step "
                                                f"{e.global_step}")
                    elif not math.isfinite(step_loss):
                        raise NonFiniteLoss(f"non-finite train loss at step {e.global_step}: {step_loss}")
                    metrics = {"train_loss_step": step_loss} if math.isfinite(step_loss) else {}
                    if clip_on:
                        metrics.update(grad_norm=float(opt.last_grad_norm), clipped_steps=opt.clipped_steps,
                                       skipped_steps=opt.skipped_steps)
                    if self.nll_on and nwindow is not None:
                        metrics["train_nll_step"] = self._mean_across(nwindow, wcount if skip_on else wn)
                    if self.acc_on:
                        metrics.update(self._acc_metrics("train_acc_step"))
                    lr_shown = e.lr
                    if sched_on:
                        # the scheduled values of the last applied update, from the device (this point has synchronised)
                        now = e.lrs_now
                        lr_shown = metrics["lr-Adam"] = next(iter(now.values()))
                        if len(now) > 1:
                            metrics.update({f"lr/{name}": v for name, v in now.items()})
                    if getattr(opt, "trust", None) is not None:
                        # layer-wise trust ratios of the last applied update: one small D2H at this synchronised point
                        tr = opt.trust.float().cpu()
                        metrics.update({"trust/min": float(tr.min()), "trust/median": float(tr.median()),
                                        "trust/max": float(tr.max())})
                    self._log(metrics)
                    window, wn, wcount, wsteps, nwindow = None, 0, None, 0, None
                    if self.verbose:
                        extra = (f" grad_norm {metrics['grad_norm']:.4g} clipped {metrics['clipped_steps']} "
                                 f"skipped {metrics['skipped_steps']}") if clip_on else ""
                        print(f"epoch {epoch} step {e.global_step} train_loss {step_loss:.6f} lr {lr_shown:.2e}{extra}",
                              flush=True)

            for batch in self._iter(train_loader, self.limit_train):
                loss = e.train_step(batch)
                if e.graph and not self.graph_checked and (e._graph is not None or e._segments is not None):
                    self._check_graph(batch)
                nll = e.last_nll.detach() if self.nll_on and e.last_nll is not None else None
                if skip_on:
                    fin = torch.isfinite(loss)
                    one = fin.to(torch.float32)
                    loss = torch.where(fin, loss, torch.zeros_like(loss))
                    tcount = one if tcount is None else tcount + one
                    wcount = one if wcount is None else wcount + one
                    if nll is not None:
                        nll = torch.where(fin, nll, torch.zeros_like(nll))
                if nll is not None:
                    nwindow = nll if nwindow is None else nwindow + nll
                total = loss if total is None else total + loss
                window = loss if window is None else window + loss
                n += 1
                wn += 1
                samples += int(batch["action_label"]["action"].shape[0]) * pdist.context().world_size
                if e.stepped:
                    log_point()
            if e.flush_window():                     # a partial accumulation window: one more optimizer step
                log_point()
            if e.device.type == "cuda":
                torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            metrics = {"train_loss_epoch": (self._mean_across(total, tcount if skip_on else n) if total is not None
                                            else float("nan")),
                       "samples_per_sec": samples / dt if dt > 0 else 0.0}
            io = dict(getattr(getattr(self, "prefetcher", None), "stats", {}) or {})
            if io and n:
                io["step_ms"] = 1e3 * dt / n
                self.input_stats = io
                if self.verbose:
                    print(f"epoch {epoch} input path (per batch): " +
                          " ".join(f"{k} {v:.2f}" for k, v in io.items() if k != "batches"), flush=True)
            if not math.isfinite(metrics["train_loss_epoch"]) and n > 0:
                raise NonFiniteLoss(f"non-finite epoch loss at epoch {epoch}")
            if val_loader is not None:
                metrics["eval_loss"] = self.validate(val_loader, self.limit_val)
            self._log(metrics)
            if val_loader is not None and self.last_ema_loss is not None:
                metrics["eval_loss_ema"] = self.last_ema_loss        # validate() logged it already
            if val_loader is not None and self.last_acc:
                metrics.update(self.last_acc)                        # likewise
            for k in self.history:
                if k in metrics:
                    self.history[k].append(metrics[k])
            if self.verbose:
                print(f"epoch {epoch} " + " ".join(f"{k} {v:.6g}" for k, v in metrics.items()), flush=True)
            e.epoch_end()
            if self.ckpt is not None and pdist.context().is_main:
                self.ckpt.on_epoch_end(epoch, metrics, self._make_ckpt)
            self.logger.flush()
            pdist.barrier()
        self.current_epoch = self.max_epochs

    def test(self, loader, limit=None) -> float:
        loss = self.validate(loader, limit, "test_loss")
        self._log({"test_loss": loss})
        self.logger.flush()
        if self.verbose:
            print(f"test_loss {loss:.6g}", flush=True)
        return loss
