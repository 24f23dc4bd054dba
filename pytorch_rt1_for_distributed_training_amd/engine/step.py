"""One optimisation step of RT-1 (forward, backward, DP all-reduce, Adam).

Replaces ``RT1_Lightning.training_step`` + Lightning's automatic optimisation
(``distribute_train.py:59-73,99-118``).  Per step:

1. ``ddp.prepare()``  — reset bucket counters, (optionally) broadcast BN buffers;
2. forward under the compute dtype (bf16 on MI355X), loss = mean of the
   per-(b,t) actor loss exactly as ``loss_fn`` (``:112-118``);
3. backward — bucket all-reduces fire from gradient hooks while the rest of
   the backward runs;
4. ``ddp.finish()`` then ONE fused Adam launch over the flat buffer with the
   1/world average folded in.

``graph=True`` (hip backend, one GPU) runs the whole step -- forward, backward,
gradient gather and Adam -- as ONE captured hipGraph (``torch.cuda.CUDAGraph``
is hipGraph on ROCm): the first call runs an eager step and captures, later
calls copy the batch into the static input buffers and replay.  Everything the
step needs from the host is device-resident: the random-shift offsets and
drop-path masks come from torch's graph-safe RNG, dropout seeds from the
``ops.rng`` device counter, Adam's step/lr from ``FlatAdam.dev_state``.
With data parallelism (``graph=True``, world > 1) forward + backward is captured as a CHAIN of graphs cut where
each gradient bucket completes (``engine.graphs.SegmentedCapture``); a step replays segment i, issues bucket i's
RCCL all-reduce on the comm stream, replays segment i+1 while that all-reduce runs, ... then one fused Adam
launch.  Collectives are never captured; they overlap the backward exactly where DDP's hooks would fire them.

``max_grad_norm`` / ``skip_nonfinite`` (both off by default, and then nothing here changes): the optimizer takes the
global norm of the all-reduced flat gradient on the device (``csrc/kernels/gradnorm.hip``), the clip variant of the
fused Adam scales the gradient or leaves a non-finite step untouched, and ``buffer_guard_`` rolls the BN running
statistics of such a step back -- all inside the captured graph, with no host read.  The norm's summation order
depends only on the buffer length, so every rank takes the same decision without another collective.

``accumulate_grad_batches=k`` (Lightning's name; 1 = off, and then nothing here changes): ``train_step`` runs one
micro-batch -- release the gradients, forward, backward, ACCUMULATING gather into the flat gradient -- and the optimizer
runs on the k-th with ``grad_scale / k``, so the update uses the mean gradient over micro-batches and ranks.  The
window starts with the one memset of the flat gradient.  With ``graph=True`` the captured graph is the micro-step
(no memset, no optimizer); the memset and the optimizer / clip / guard launches run eagerly around the replays.  Under
data parallelism only the final micro-batch all-reduces.  BN running statistics advance once per micro-batch; their
shadow is the state before the window, so a skipped window rolls all of it back.

``ema_decay=d`` (0 = off, and then nothing here changes): the optimizer keeps an exponential moving average of the
trainable weights in one more flat fp32 buffer, updated by the Adam launch itself (``ops.adam.flat_adam_dev_step`` given ``ema``:
``ema += omd_t * (p - ema)``, the warm-up schedule formed on the device from the same step the bias corrections use), so
every step path above carries it and a skipped step leaves it untouched.  BN running statistics and the frozen
``_action_token_emb`` are not averaged: ``ema_weights()`` runs the averaged weights with the live BN buffers
(``torch.optim.swa_utils.AveragedModel``'s default).  The buffer is fp32: at decay 0.9999 an update whose ``|p - ema|`` is
below about ``1e-3 |ema|`` moves it by less than an ulp.

``no_decay_norm_bias`` / ``backbone_lr_mult`` (off / 1, and then nothing here changes): the optimizer gets up to four
parameter groups (``engine.optim.build_param_groups``: no weight decay on norms, biases and embeddings; a smaller
learning rate on the pretrained backbone) and the Adam launch looks the group up per 64-element chunk
(``ops.adam.flat_adam_dev_step`` given ``group_state``), on every step path above and together with clipping and the EMA.  Each group's
``{lr, wd}`` is device state like the step: a scheduler step rewrites it from the host before the next replay, so the
captured graph stays valid.  ``backbone_lr_mult != 1`` asks for pretrained weights (``pretrained``, else the model's
``backbone_pretrained`` mark that ``models.load_pretrained_backbone`` leaves).  ``lrs`` gives every group's lr by name.

``lr_schedule=dict(kind, warmup_steps, decay_steps, min_lr_ratio)`` (None = off, and then nothing here changes): a
per-step factor on every group's base lr -- linear warm-up, then constant / linear / cosine / inverse-sqrt decay
(``engine.optim.lr_factor``) -- formed on the device by one tiny launch inside ``optimizer.step()``
(``ops.adam.lr_schedule_dev``), from the effective Adam step the bias corrections use, so every step path above carries
it, a skipped step does not advance it and no step waits for a host write.  ``lr`` / ``lrs`` stay the base learning
rates that ``MultiStepLR`` scales per epoch; ``lr_now`` / ``lrs_now`` read the scheduled values back from the device.

``label_smoothing`` / ``z_loss`` / ``token_accuracy`` (0 / 0 / off, and then nothing here changes): the training
objective becomes ``(1 - eps) nll + eps mean_c(-log p_c) + zeta logsumexp^2`` (``models.policy.token_losses``; on the
fused head one kernel, ``ops.head``), applied only while the model is in training mode, so ``eval_step`` stays
the plain CE; ``last_nll`` is then the plain CE of the last training batch (the engine's own copy: a replay clones the
graph's tensor, and a capture, which records a forward without running it, leaves the eager step's figure in place).
With ``token_accuracy`` every forward adds {pred == label, rows} per action-token slot to ``token_counters`` (one small
launch, part of the captured step; every micro-batch of an accumulation window counts); ``read_token_counters`` reads
and zeroes them.

``optimizer="lamb"`` (``"adam"`` = off, and then nothing here changes): ``FlatAdam(layer_adapt=True)``, layer-wise trust
ratios on Adam's moments -- three launches (``ops.adam.flat_lamb_dev_step``) where the Adam launch was, so every step
path and every option above carries them unchanged; the no-decay groups of ``no_decay_norm_bias`` are not adapted.

No ``network_state`` is fabricated (the reference samples a random one on the
CPU and copies it to the GPU every step only to read its shape).
"""
from __future__ import annotations

import contextlib
import time
from typing import Dict, Optional

import torch
import torch.nn as nn

from ..config import RT1Config
from ..parallel import dist as pdist
from ..parallel.ddp import DataParallel, gradient_ready_order
from ..parallel.flat import deferred_sums
from ..parallel.flat import FlatParameters
from .optim import FlatAdam, build_param_groups, multistep_lr


def split_batch(batch: Dict) -> tuple:
    obs = batch["train_observation"]
    return obs["image"], obs.get("natural_language_embedding"), batch["action_label"]


def _clone_tree(batch):
    if isinstance(batch, dict):
        return {k: _clone_tree(v) for k, v in batch.items()}
    return batch.clone() if isinstance(batch, torch.Tensor) else batch


def _copy_into(dst, src):
    if isinstance(dst, dict):
        for k in dst:
            _copy_into(dst[k], src[k])
    elif isinstance(dst, torch.Tensor):
        dst.copy_(src, non_blocking=True)


def _same_shapes(a, b) -> bool:
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same_shapes(a[k], b[k]) for k in a)
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.shape == b.shape and a.dtype == b.dtype
    return True


def to_device(batch, device, non_blocking=True):
    if isinstance(batch, dict):
        return {k: to_device(v, device, non_blocking) for k, v in batch.items()}
    if isinstance(batch, torch.Tensor):
        return batch.to(device, non_blocking=non_blocking)
    return batch


def synthetic_probe_batch(cfg: RT1Config, b: int, device) -> Dict:
    return {"train_observation": {"image": torch.rand(b, cfg.seq_len, 3, cfg.height, cfg.width, device=device),
                                  "natural_language_embedding": torch.randn(b, cfg.seq_len, 512, device=device)},
            "action_label": {"terminate_episode": torch.zeros(b, cfg.seq_len, dtype=torch.long, device=device),
                             "action": torch.zeros(b, cfg.seq_len, 2, device=device)}}


# Diagnostic knobs of the graph-DP step (RT1_DP_DIAG, comma list; for same-box A/B of its per-step costs only):
#   nosync   -- no per-step BN-buffer broadcast before the replay
#   noreduce -- no bucket all-reduces (world 1 only: the sums are the identity there)
#   relaxed1 -- the one-graph step captured in relaxed mode (as the graph-DP segments are)
#   globalseg -- the graph-DP segments captured in global mode
#   emptycache -- empty_cache() before the segmented capture
_DP_DIAG = set(filter(None, __import__("os").environ.get("RT1_DP_DIAG", "").split(",")))


def _test_capture_failure():
    """Test hook (GPU rehearsals): RT1_TEST_CAPTURE_FAIL=<rank> makes that rank's segmented capture raise, so the
    collective capture decision and the eager fallback of every rank are exercised."""
    import os
    r = os.environ.get("RT1_TEST_CAPTURE_FAIL")
    if r is not None and torch.distributed.is_initialized() and int(r) == torch.distributed.get_rank():
        raise RuntimeError("capture failure forced by RT1_TEST_CAPTURE_FAIL")


OPTIMIZERS = ("adam", "lamb")     # lamb: FlatAdam(layer_adapt=True), layer-wise trust ratios on the same state


class TrainEngine:
    def __init__(self, model: nn.Module, cfg: RT1Config, lr: float = 5e-4, milestones=(50, 75, 90),
                 gamma: float = 0.1, weight_decay: float = 0.0, bucket_cap_mb: float = 32.0,
                 broadcast_buffers: bool = True, device: Optional[torch.device] = None,
                 grad_comm_dtype: torch.dtype = torch.float32, order_probe: bool = True, comm: str = "torch",
                 graph: bool = False, max_grad_norm: Optional[float] = None, skip_nonfinite: bool = False,
                 accumulate_grad_batches: int = 1, ema_decay: float = 0.0, ema_warmup: bool = True,
                 no_decay_norm_bias: bool = False, backbone_lr_mult: float = 1.0,
                 pretrained: Optional[bool] = None, lr_schedule: Optional[dict] = None,
                 label_smoothing: float = 0.0, z_loss: float = 0.0, token_accuracy: bool = False,
                 optimizer: str = "adam"):
        from ..models.policy import checked_objective
        if optimizer not in OPTIMIZERS:
            raise ValueError(f"optimizer must be one of {OPTIMIZERS}, got {optimizer!r}")
        label_smoothing, z_loss = checked_objective(label_smoothing, z_loss)
        if not isinstance(backbone_lr_mult, (int, float)) or not backbone_lr_mult > 0:
            raise ValueError(f"backbone_lr_mult must be a number > 0, got {backbone_lr_mult!r}")
        if pretrained is None:
            pretrained = bool(getattr(model, "backbone_pretrained", False))
        if float(backbone_lr_mult) != 1.0 and not pretrained:
            raise ValueError(f"backbone_lr_mult={backbone_lr_mult} needs pretrained weights to protect: load them "
                             f"(--pretrained, models.load_pretrained_backbone) or resume a checkpoint (--resume; "
                             f"pretrained=True)")
        if int(accumulate_grad_batches) != accumulate_grad_batches or accumulate_grad_batches < 1:
            raise ValueError(f"accumulate_grad_batches must be an integer >= 1, got {accumulate_grad_batches!r}")
        ctx = pdist.context()
        self.cfg = cfg
        self.device = device or pdist.default_device()
        self.model = model.to(self.device)
        # training objective and token accuracy (models/policy.py): plain attributes of the model; the {hits, rows}
        # counters per action-token slot are this engine's device state, not a buffer of the model, so neither the
        # checkpoint nor the data-parallel buffer broadcast sees them
        self.model.label_smoothing, self.model.z_loss = label_smoothing, z_loss
        self.regularised = label_smoothing != 0.0 or z_loss != 0.0
        self.token_accuracy = bool(token_accuracy)
        self.token_counters = None
        if self.token_accuracy:
            self.token_counters = torch.zeros(self.model._tokens_per_action, 2, dtype=torch.int64, device=self.device)
        self.model.track_token_accuracy = self.token_accuracy
        self.model.token_counters = self.token_counters
        self.last_nll = None       # mean plain CE of the last train_step's batch (regularised objective only)
        self.compute_dtype = torch.bfloat16 if (cfg.dtype == "bf16" and self.device.type == "cuda") else torch.float32
        self.backend = self._select_backend(cfg)
        if self.backend == "hip":
            from ..ops import install
            install(self.model, cfg)
        elif self.device.type == "cuda" and cfg.channels_last:
            self.model._image_tokenizer.to(memory_format=torch.channels_last)

        trainable = [p for p in self.model.parameters() if p.requires_grad]
        if order_probe:
            order = self._gradient_order(trainable)
        else:
            order = list(reversed(trainable))
        if self.token_counters is not None:
            self.token_counters.zero_()            # the order probe's forward counted its synthetic rows
        self.flat = FlatParameters(order, device=self.device)
        # weight-gradient split-K sums folded into the flat gather (parallel/flat.py deferred_sums): one backward per
        # step into an fp32 gradient buffer on the GPU
        self._defer_sums = self.flat.grad.is_cuda and self.flat.grad.dtype == torch.float32
        fused = getattr(self.model, "fused", None)
        if fused is not None and hasattr(fused, "attach_flat"):
            fused.attach_flat(self.flat)
        native = None
        if comm == "native":
            if self.device.type != "cuda":
                raise ValueError("comm='native' (RCCL) needs GPU tensors")
            from ..parallel.native_comm import NativeComm
            dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
            # world 1: a single-rank RCCL communicator, so the bucketed DP path runs (and is testable) on one GPU
            native = (NativeComm(device=dev_index) if ctx.world_size > 1 else NativeComm.single(dev_index))
        elif comm not in ("torch", "native"):
            raise ValueError(f"unknown comm backend {comm!r}")
        self.ddp = DataParallel(self.model, self.flat, bucket_cap_mb=bucket_cap_mb,
                                broadcast_buffers=broadcast_buffers, grad_comm_dtype=grad_comm_dtype, comm=native)
        # parameter groups (engine/optim.py build_param_groups); with both rules off the one default group, and then
        # nothing here changes
        groups = None
        if no_decay_norm_bias or float(backbone_lr_mult) != 1.0:
            groups = build_param_groups(self.model, lr, weight_decay, bool(no_decay_norm_bias),
                                        float(backbone_lr_mult))
        self.optimizer = FlatAdam(self.flat, lr=lr, weight_decay=weight_decay,
                                  all_params=list(self.model.parameters()), max_grad_norm=max_grad_norm,
                                  skip_nonfinite=skip_nonfinite, ema_decay=ema_decay, ema_warmup=ema_warmup,
                                  param_names={id(p): n for n, p in self.model.named_parameters()}, groups=groups,
                                  lr_schedule=lr_schedule, layer_adapt=optimizer == "lamb")
        # skip_nonfinite: the forward of a bad batch has already written the BN running statistics when the norm
        # kernel notices, so they live in one flat buffer (the data-parallel one when there is one) with a shadow copy
        # of the last good state; buffer_guard_ advances or rolls back right after the optimizer step
        self.skip_nonfinite = bool(skip_nonfinite)
        self._bn_flat = self._bn_shadow = None
        if self.skip_nonfinite:
            from ..parallel.flat import flatten_buffers
            self._bn_flat = self.ddp.buffers if self.ddp.buffers is not None else flatten_buffers(self.model)
            if self._bn_flat is not None:
                self._bn_shadow = self._bn_flat.clone()
        self.scheduler = multistep_lr(self.optimizer, list(milestones), gamma)
        self.global_step = 0       # optimizer steps (Lightning's meaning), not micro-batches
        # gradient accumulation: micro_step = micro-batches already in the open window, stepped = whether the last
        # train_step applied the optimizer (always, without accumulation)
        self.accumulate_grad_batches = int(accumulate_grad_batches)
        self.micro_step = 0
        self.stepped = True
        self.ddp.accumulate = self.accumulate_grad_batches > 1
        # one GPU: the whole step is one graph; data parallel: forward+backward is the graph, the gradient
        # all-reduce and Adam run after each replay (collectives are never captured)
        self.graph = bool(graph) and self.backend == "hip" and self.device.type == "cuda"
        self._graph = None
        self._segments = None      # SegmentedCapture of the data-parallel graph step
        self._static_batch = None
        self._static_loss = None
        self._static_nll = None    # forward_loss's last_nll as the captured step wrote it
        # graph-DP comm timing (bench.py): (event before the final waits, event after) per replayed step
        self.comm_timing = None
        self.comm_host_wait_s = 0.0
        self.bucket_timing = []    # per replayed step: [(bucket, launch event, ready event)] while comm_timing is on

    # ------------------------------------------------------------------ setup helpers
    def _select_backend(self, cfg: RT1Config) -> str:
        if cfg.backend == "torch" or self.device.type != "cuda":
            return "torch"
        if cfg.backend == "hip":
            return "hip"
        from ..ops import available
        return "hip" if available() else "torch"

    def _gradient_order(self, trainable):
        """Probe gradient-ready order on rank 0 with a 1-sample batch; broadcast it."""
        index = {id(p): i for i, p in enumerate(trainable)}
        order_idx = None
        if pdist.context().is_main:
            probe = synthetic_probe_batch(self.cfg, 1, self.device)

            def run():
                with self.autocast():
                    loss, _ = self.model.train_forward(*split_batch(probe), with_aux=False)
                loss.mean().backward()
            was = self.model.training
            self.model.train()
            order = gradient_ready_order(self.model, run, trainable)
            self.model.train(was)
            order_idx = [index[id(p)] for p in order]
        order_idx = pdist.broadcast_object(order_idx)
        return [trainable[i] for i in order_idx]

    def refresh_buffer_shadow(self):
        """The BN running statistics were replaced from outside the step (checkpoint load, parameter broadcast):
        they are the good state now."""
        if self._bn_shadow is not None:
            self._bn_shadow.copy_(self._bn_flat)

    def _guard_buffers(self):
        if self._bn_shadow is None:
            return
        opt = self.optimizer
        if opt._kernel is not None:
            opt._kernel.buffer_guard_(self._bn_flat, self._bn_shadow, opt.clip_state)
        elif float(opt.clip_state[2]) != 0.0:
            self._bn_shadow.copy_(self._bn_flat)
        else:
            self._bn_flat.copy_(self._bn_shadow)

    def autocast(self):
        if self.compute_dtype == torch.float32 or self.backend == "hip":
            return contextlib.nullcontext()
        return torch.autocast(device_type=self.device.type, dtype=self.compute_dtype)

    # ------------------------------------------------------------------ steps
    def forward_loss(self, batch: Dict):
        images, ctx, actions = split_batch(batch)
        with self.autocast():
            loss_bt, aux = self.model.train_forward(images, ctx, actions, with_aux=False)
        nll = aux.get("action_nll")
        self.last_nll = nll.mean() if nll is not None else None
        return loss_bt.mean(), aux

    def _step_body(self, batch: Dict) -> torch.Tensor:
        self.model.train()
        self.ddp.prepare()
        self.optimizer.zero_grad()
        loss, _ = self.forward_loss(batch)
        with deferred_sums(self._defer_sums):
            loss.backward()
        self.ddp.finish()
        self.optimizer.step(grad_scale=self.ddp.grad_scale)
        self._guard_buffers()
        return loss.detach()

    def train_step(self, batch: Dict) -> torch.Tensor:
        if self.accumulate_grad_batches > 1:
            return self._accum_step(batch)
        if self.graph and self._static_batch is not None and not _same_shapes(self._static_batch, batch):
            # a batch of another shape (e.g. a short last batch) cannot replay the captured graph: run it eagerly
            loss = self._step_body(batch)
            self.optimizer._dev_step = None            # the eager Adam advanced the device state; re-sync next replay
            self.global_step += 1
            return loss
        if self.graph and self.ddp.enabled:
            return self._graph_dp_step(batch)
        if self.graph:
            return self._graph_step(batch)
        loss = self._step_body(batch)
        self.global_step += 1
        return loss

    # ------------------------------------------------------------------ gradient accumulation (k > 1)
    def _window_begin(self):
        self.flat.grad.zero_()
        if "nosync" in _DP_DIAG and self._segments is not None:
            self.ddp.reset_buckets()                 # diagnostic, as in _graph_dp_step: no BN-buffer broadcast
        else:
            self.ddp.prepare()                       # bucket counters, one BN-buffer broadcast per window

    def _window_end(self):
        """Optimizer on the accumulated (and, under DP, all-reduced) gradient of ``micro_step`` micro-batches."""
        self.optimizer.step(grad_scale=self.ddp.grad_scale / self.micro_step)
        self._guard_buffers()
        self.micro_step = 0
        self.global_step += 1
        self.stepped = True

    def _micro_body(self, batch: Dict) -> torch.Tensor:
        """Release, forward, backward, accumulating gather: what the one-GPU micro-step graph holds."""
        self.model.train()
        self.flat.release_grads()
        loss, _ = self.forward_loss(batch)
        with deferred_sums(self._defer_sums):
            loss.backward()
        self.ddp.finish()
        return loss.detach()

    def _eager_micro_step(self, batch: Dict) -> torch.Tensor:
        if self.micro_step == 0:
            self._window_begin()
        else:
            # the window's earlier micro-batches may have left the bucket counters anywhere (a segmented capture
            # marks every bucket launched; so does a replayed or dropped graph's window): this backward's hooks
            # must find them fresh, or a final micro-batch would gather and never all-reduce
            self.ddp.reset_buckets()
        final = self.micro_step + 1 == self.accumulate_grad_batches
        # a non-final micro-batch launches no bucket and gathers its whole gradient at the end of the backward
        with contextlib.nullcontext() if final else self.ddp.no_sync():
            loss = self._micro_body(batch)
        self.micro_step += 1
        if final:
            self._window_end()
        return loss

    def _accum_step(self, batch: Dict) -> torch.Tensor:
        self.stepped = False
        if not self.graph or (self._static_batch is not None and not _same_shapes(self._static_batch, batch)):
            return self._eager_micro_step(batch)
        dp = self.ddp.enabled
        if (self._segments if dp else self._graph) is None:
            loss = self._eager_micro_step(batch)     # real micro-step, also warms up lazily-initialised state
            if dp:
                self._capture_dp_collectively(batch)
            else:
                try:
                    self._capture(batch)
                except Exception as e:
                    self._capture_failed(e)
            return loss
        if self.micro_step == 0:
            self._window_begin()
        final = self.micro_step + 1 == self.accumulate_grad_batches
        _copy_into(self._static_batch, batch)
        if not dp:
            self._graph.replay()
        else:
            self._replay_segments(launch=final)      # only the final micro-batch all-reduces its buckets
        self.micro_step += 1
        if final:
            self._window_end()
        self.last_nll = self._static_nll.clone() if self._static_nll is not None else None
        return self._static_loss.clone()

    def flush_window(self) -> bool:
        """Apply a partial accumulation window (an epoch ended inside it): the optimizer runs on the mean of the
        ``micro_step`` micro-batches gathered so far.  No-op (False) on an empty window."""
        if self.accumulate_grad_batches <= 1 or self.micro_step == 0:
            return False
        self.ddp.all_reduce_grads()                  # none of these micro-batches was the window's final one
        self._window_end()
        return True

    # ------------------------------------------------------------------ hipGraph step
    def _graph_step(self, batch: Dict) -> torch.Tensor:
        if self._graph is None:
            loss = self._step_body(batch)            # real step, also warms up lazily-initialised state
            self.global_step += 1
            try:
                self._capture(batch)
            except Exception as e:   # capture is an optimisation: never lose the run to it
                self._capture_failed(e)
            return loss
        _copy_into(self._static_batch, batch)
        opt = self.optimizer
        if opt.device_state_stale():
            opt.sync_device_state()
        self._graph.replay()
        opt.step_count += 1
        opt._dev_step = opt.step_count
        self.global_step += 1
        self.last_nll = self._static_nll.clone() if self._static_nll is not None else None
        return self._static_loss.clone()

    def _capture_failed(self, e: Exception):
        import sys
        print(f"[rt1] hipGraph capture failed ({type(e).__name__}: {e}); continuing eagerly",
              file=sys.stderr, flush=True)
        self.graph = False
        self._graph = None

    def _capture(self, batch: Dict):
        self._static_batch = _clone_tree(batch)
        torch.cuda.synchronize(self.device)
        self.optimizer.sync_device_state()
        g = torch.cuda.CUDAGraph()
        steps_before = self.optimizer.step_count
        # the capture records the step without running it: the nll tensor that its forward_loss leaves in last_nll is
        # unwritten graph memory until a replay, so last_nll keeps the eager step's figure, capture failed or not
        nll_eager = self.last_nll
        try:
            with torch.cuda.graph(g, capture_error_mode="relaxed" if "relaxed1" in _DP_DIAG else "global"):
                if self.accumulate_grad_batches > 1:
                    self._static_loss = self._micro_body(self._static_batch)     # no memset, no optimizer
                else:
                    self._static_loss = self._step_body(self._static_batch)
        finally:
            # the capture recorded the step; it did not run it (restore even when the capture failed, so an eager
            # fallback continues from the right Adam step and re-syncs the device copy)
            self.optimizer.step_count = steps_before
            self.optimizer._dev_step = None
            nll_static, self.last_nll = self.last_nll, nll_eager
        self.optimizer.sync_device_state()
        self._static_nll = nll_static
        self._graph = g

    # ------------------------------------------------------------------ hipGraph data-parallel step
    def _graph_dp_step(self, batch: Dict) -> torch.Tensor:
        if self._segments is None:
            loss = self._step_body(batch)            # eager step (bucketed, overlapped DP) warms everything up
            self.global_step += 1
            self._capture_dp_collectively(batch)
            return loss
        _copy_into(self._static_batch, batch)
        if "nosync" not in _DP_DIAG:
            self.ddp.sync_buffers()                  # rank-0 BN buffers before the forward (DDP parity)
        self._replay_segments()
        self.optimizer.step(grad_scale=self.ddp.grad_scale)
        self._guard_buffers()
        self.global_step += 1
        self.last_nll = self._static_nll.clone() if self._static_nll is not None else None
        return self._static_loss.clone()

    def _replay_segments(self, launch: bool = True):
        """Replay the captured segments, issuing each completed bucket's all-reduce between them, and wait for all of
        them.  ``launch=False`` (a non-final micro-batch of an accumulation window): replay only, no collective and
        no comm-timing record (``comm_timing`` / ``bucket_timing`` hold one entry per replay that all-reduced)."""
        if not launch:
            self._segments.replay_with(lambda buckets: None)
            return
        works = []
        timing = self.comm_timing is not None
        launched = []                                # (bucket indices, event after the segment that completed them)

        def on_buckets(buckets):
            if "noreduce" in _DP_DIAG and self.ddp.world == 1:
                return
            works.extend(self.ddp.launch_bucket(b) for b in buckets)
            if timing:
                ev = torch.cuda.Event(enable_timing=True)
                ev.record()
                launched.append((list(buckets), ev))
        # segment i replays on the compute stream; bucket i's all-reduce then runs on the comm stream while
        # segment i+1 computes
        self._segments.replay_with(on_buckets)
        if timing:
            # exposed communication: compute-stream time between the last segment and the end of the last wait;
            # per bucket: its launch point (end of the segment that completed it) -> the compute stream passing its
            # wait (an upper bound on the all-reduce: max(backward left, all-reduce))
            e0 = torch.cuda.Event(enable_timing=True)
            e0.record()
            h0 = time.perf_counter()
            done = []
            for w in works:
                if w is not None:
                    w.wait()
                ev = torch.cuda.Event(enable_timing=True)
                ev.record()
                done.append(ev)
            self.comm_host_wait_s += time.perf_counter() - h0
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            self.comm_timing.append((e0, e1))
            per_bucket = []
            k = 0
            for buckets, ev in launched:
                for b in buckets:
                    per_bucket.append((b, ev, done[k]))
                    k += 1
            self.bucket_timing.append(per_bucket)
        else:
            self.ddp.wait_all(works)

    def _capture_dp_collectively(self, batch: Dict):
        err = None
        try:
            _test_capture_failure()
            self._capture_segments(batch)
        except Exception as e:
            err = e
        # capture success is a COLLECTIVE decision: a rank whose capture failed runs eager steps, whose bucket
        # all-reduces are issued from hooks in a different order and count than the graph-DP replay's, so every
        # rank must take the same path or the collectives stop lining up (summing buckets of different steps, or
        # hanging).  No collective runs during the capture itself, so every rank reaches this all-reduce.
        if not pdist.all_true(err is None):
            import sys
            why = f"{type(err).__name__}: {err}" if err is not None else "failed on another rank"
            print(f"[rt1] segmented hipGraph capture {why}; every rank continues eagerly", file=sys.stderr,
                  flush=True)
            self.drop_graph()

    def _capture_segments(self, batch: Dict):
        from .graphs import SegmentedCapture
        import gc
        self._static_batch = _clone_tree(batch)
        torch.cuda.synchronize(self.device)
        gc.collect()
        if "emptycache" in _DP_DIAG:
            # diagnostic: as torch.cuda.graph does before a capture (measured 0.3-0.6 ms/step SLOWER for the
            # segments, profiles/r6_graph_dp_world1.log)
            torch.cuda.empty_cache()
        side = torch.cuda.Stream(self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        seg = SegmentedCapture(side, mode="global" if "globalseg" in _DP_DIAG else "relaxed")
        seg.expected_last = len(self.ddp.buckets)
        nll_eager = self.last_nll                    # as in _capture: the captured forward's nll is not yet written
        try:
            with torch.cuda.stream(side):
                seg.begin()
                self.model.train()
                if self.accumulate_grad_batches > 1:
                    self.flat.release_grads()        # the window's memset stays outside the segments
                else:
                    self.optimizer.zero_grad()
                with self.ddp.capture_cuts(seg):
                    loss, _ = self.forward_loss(self._static_batch)
                    with deferred_sums(self._defer_sums):
                        loss.backward()
                rest = self.ddp.unlaunched_buckets()
                # buckets that never completed (a param without a gradient)
                self.flat.gather_grads(accumulate=self.ddp.accumulate)
                self._static_loss = loss.detach()
                self._static_nll = self.last_nll
                seg.end(extra_buckets=rest)
        except BaseException:
            seg.abort()
            raise
        finally:
            self.last_nll = nll_eager
        torch.cuda.current_stream(self.device).wait_stream(side)
        torch.cuda.synchronize(self.device)
        self._segments = seg

    def drop_graph(self):
        """Leave the hipGraph step for good (capture failure, or a failed graph == eager check): every later step
        runs the eager hook-driven step.  Call it on every rank (it changes which collectives a step issues)."""
        self.graph = False
        self._graph = None
        self._segments = None
        self.flat.reattach_grads()

    def bucket_report(self):
        """Mean launch -> ready time (ms) per bucket over the timed graph-DP steps, and the buckets' sizes (MB)."""
        if not self.bucket_timing:
            return None
        acc = {}
        for step in self.bucket_timing:
            for b, l, d in step:
                acc.setdefault(b, []).append(l.elapsed_time(d))
        el = 4 if self.flat.grad.dtype == torch.float32 else 2
        return [{"bucket": b, "mb": round((self.ddp.buckets[b].end - self.ddp.buckets[b].start) * el / 2 ** 20, 2),
                 "launch_to_ready_ms": round(sum(v) / len(v), 3)} for b, v in sorted(acc.items())]

    # ------------------------------------------------------------------ graph == eager self-check
    def _snapshot(self) -> Dict:
        from ..ops import rng as _rng
        opt = self.optimizer
        with torch.no_grad():
            return dict(data=self.flat.data.clone(), m=opt.exp_avg.clone(), v=opt.exp_avg_sq.clone(),
                        dev=opt.dev_state.clone(), step=opt.step_count, dev_step=opt._dev_step,
                        dev_groups=opt._dev_groups,
                        group_state=(opt.group_state.clone() if opt.group_state is not None else None),
                        bufs=[b.detach().clone() for b in self.model.buffers()],
                        rng=(torch.cuda.get_rng_state(self.device) if self.device.type == "cuda" else None),
                        cpu_rng=torch.get_rng_state(),
                        ctr={d: t.clone() for d, t in _rng._COUNTERS.items()}, gstep=self.global_step,
                        clip=(opt.clip_state.clone() if opt.clip_state is not None else None),
                        shadow=(self._bn_shadow.clone() if self._bn_shadow is not None else None),
                        # an open accumulation window is state too: what it gathered so far and its position
                        grad=(self.flat.grad.clone() if self.accumulate_grad_batches > 1 else None),
                        micro=self.micro_step, stepped=self.stepped,
                        ema=(opt.ema.clone() if opt.ema is not None else None),
                        ema_state=(opt.ema_state.clone() if opt.ema_state is not None else None),
                        lr_base=(opt.lr_base.clone() if opt.lr_base is not None else None),
                        sched_state=(opt.sched_state.clone() if opt.sched_state is not None else None),
                        hits=(self.token_counters.clone() if self.token_counters is not None else None),
                        nll=(self.last_nll.clone() if self.last_nll is not None else None))

    def _restore(self, s: Dict):
        from ..ops import rng as _rng
        opt = self.optimizer
        with torch.no_grad():
            self.flat.data.copy_(s["data"])
            opt.exp_avg.copy_(s["m"])
            opt.exp_avg_sq.copy_(s["v"])
            opt.dev_state.copy_(s["dev"])
            if s["group_state"] is not None:
                opt.group_state.copy_(s["group_state"])
            for b, c in zip(self.model.buffers(), s["bufs"]):
                b.copy_(c)
            for d, t in s["ctr"].items():
                _rng._COUNTERS[d].copy_(t)
            if s["clip"] is not None:
                opt.clip_state.copy_(s["clip"])
            if s["shadow"] is not None:
                self._bn_shadow.copy_(s["shadow"])
            if s["grad"] is not None:
                self.flat.grad.copy_(s["grad"])
            if s["ema"] is not None:
                opt.ema.copy_(s["ema"])
                opt.ema_state.copy_(s["ema_state"])
            if s["lr_base"] is not None:
                opt.lr_base.copy_(s["lr_base"])
                opt.sched_state.copy_(s["sched_state"])
            if s["hits"] is not None:
                self.token_counters.copy_(s["hits"])
        self.micro_step, self.stepped = s["micro"], s["stepped"]
        self.last_nll = s["nll"].clone() if s["nll"] is not None else None
        opt.step_count, opt._dev_step, opt._dev_groups = s["step"], s["dev_step"], s["dev_groups"]
        if s["rng"] is not None:
            torch.cuda.set_rng_state(s["rng"], self.device)
        torch.set_rng_state(s["cpu_rng"])
        self.global_step = s["gstep"]

    def graph_eager_check(self, batch: Dict) -> Optional[Dict]:
        """One captured-graph step and one eager step on ``batch`` from the SAME state (parameters, Adam moments, BN
        running statistics, RNG states, dropout counter); the reduced flat gradients, the updated parameters and the
        losses must be bitwise equal (every kernel is deterministic and the random draws replay identically).  The
        engine is left in the pre-check state.  None when no graph has been captured (nothing to compare).
        With ``accumulate_grad_batches > 1`` the two are one replayed and one eager MICRO-step from the same state,
        the flat gradient gathered so far and the window position included."""
        if not self.graph or (self._graph is None and self._segments is None):
            return None
        if not _same_shapes(self._static_batch, batch):
            return None
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        snap = self._snapshot()
        timing, self.comm_timing = self.comm_timing, None
        try:
            loss_g = self.train_step(batch).clone()
            if self.device.type == "cuda":
                torch.cuda.synchronize(self.device)
            grad_g, data_g = self.flat.grad.clone(), self.flat.data.clone()
            opt = self.optimizer
            ema_g = (opt.ema.clone(), opt.ema_state.clone()) if opt.ema is not None else None
            self._restore(snap)
            loss_e = (self._eager_micro_step(batch) if self.accumulate_grad_batches > 1 else self._step_body(batch))
            if self.device.type == "cuda":
                torch.cuda.synchronize(self.device)
            res = dict(grads=bool(torch.equal(grad_g, self.flat.grad)),
                       params=bool(torch.equal(data_g, self.flat.data)),
                       loss=bool(torch.equal(loss_g, loss_e)))
            if ema_g is not None:
                res["ema"] = bool(torch.equal(ema_g[0], opt.ema) and torch.equal(ema_g[1], opt.ema_state))
            if not res["grads"]:
                res["max_grad_diff"] = float((grad_g - self.flat.grad).abs().max())
        finally:
            self._restore(snap)
            self.comm_timing = timing
            if self.device.type == "cuda":
                torch.cuda.synchronize(self.device)
        res["equal"] = res["grads"] and res["params"] and res["loss"] and res.get("ema", True)
        return res

    # ------------------------------------------------------------------ averaged weights
    @contextlib.contextmanager
    def ema_weights(self):
        """Run the model on the exponential moving average of its weights: inside the context ``flat.data`` holds
        ``optimizer.ema``, on exit the live weights are copied back.  Content copies only, so every address -- and
        with it a captured graph and the bf16 weight shadow, which is refreshed from the flat buffer on each
        forward -- stays valid.  Only the trainable parameters are averaged: BN running statistics and the frozen
        ``_action_token_emb`` are the live ones (``torch.optim.swa_utils.AveragedModel``'s default).  For evaluation;
        a ``train_step`` inside the context would train the average."""
        opt = self.optimizer
        if opt.ema is None:
            raise RuntimeError("ema_weights(): the EMA is off (ema_decay = 0)")
        if self.micro_step != 0:
            raise RuntimeError(f"ema_weights(): an accumulation window is open ({self.micro_step} micro-batches); "
                               f"finish or flush it first")
        with torch.no_grad():
            saved = self.flat.data.clone()
            self.flat.data.copy_(opt.ema)
        try:
            yield self
        finally:
            with torch.no_grad():
                self.flat.data.copy_(saved)

    @torch.no_grad()
    def eval_step(self, batch: Dict) -> torch.Tensor:
        self.model.eval()
        loss, _ = self.forward_loss(batch)
        return loss.detach()

    def read_token_counters(self, reset: bool = True) -> Optional[torch.Tensor]:
        """This rank's {hits, rows} per action-token slot since the last read, int64 [A, 2] on the host side of a sync
        (None with ``token_accuracy`` off); ``reset`` zeroes the device counters, in place, so a captured graph keeps
        adding to the same memory."""
        if self.token_counters is None:
            return None
        out = self.token_counters.clone()
        if reset:
            self.token_counters.zero_()
        return out

    def epoch_end(self):
        self.scheduler.step()

    @property
    def lr(self) -> float:
        return self.optimizer.param_groups[0]["lr"]

    @property
    def lrs(self) -> Dict[str, float]:
        """Learning rate of every parameter group by name (``lr`` is the first group's)."""
        return {n: g["lr"] for n, g in zip(self.optimizer.group_names, self.optimizer.param_groups)}

    @property
    def lr_now(self) -> float:
        """The first group's learning rate as the last applied update used it: ``lr`` without a per-step schedule, else
        the scheduled value read back from the device (a sync: for log points)."""
        if self.optimizer.lr_schedule is None:
            return self.lr
        return float(self.optimizer.current_lr)

    @property
    def lrs_now(self) -> Dict[str, float]:
        """``lr_now`` of every parameter group by name."""
        if self.optimizer.lr_schedule is None:
            return self.lrs
        return {n: float(v) for n, v in self.optimizer.current_lrs.items()}
