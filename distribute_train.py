"""RT-1 training entrypoint (MI355X / ROCm).

Same flags as the reference ``distribute_train.py:270-293`` (``--device --gpus
--max_epochs --batch_size --num_workers --milestones --lr --exp_name --log_dir
--ckpt_dir --log_every_n_steps --ckpt_every_n_epochs --dataset_dir
--train_episode --test_episode --eval_episode --random_crop_factor --height
--width --seq_len``) plus framework flags (``--mode``, ``--synthetic``,
``--resume``, ``--dtype``, ``--backend``, ...).

Launch:
  single GPU / CPU:   python distribute_train.py --gpus 0 ...
  one node, N GPUs:   python distribute_train.py --gpus 0,1,2,3 ...   (spawns one process per GPU)
                  or  torchrun --nproc-per-node N --master-addr 127.0.0.1 distribute_train.py ...
``--mode debug`` reproduces the reference's default smoke test (``debug()``,
``:250-266``): one train-mode forward at B=2 and one inference step at B=1.
"""
from __future__ import annotations

import argparse
import os

import numpy as np
import subprocess
import sys


LR_SCHEDULES = ("constant", "linear", "cosine", "rsqrt")
PHOTOMETRIC_NEEDS_SHARD = ("--photometric runs on the GPU decode path and needs the packed-shard format "
                           "(tools/pack_shards.py): .npz episodes and --synthetic decode on CPU workers")
DEFAULT_MILESTONES = [50, 75, 90]


def resolve_milestones(args):
    """--milestones as given; left out: the reference's 50 75 90, or none under a decaying --lr_schedule."""
    if args.milestones is not None:
        return list(args.milestones)
    return list(DEFAULT_MILESTONES) if args.lr_schedule in ("none", "constant") else []


def resolve_lr_schedule(args, train_loader=None):
    """The engine's ``lr_schedule`` dict (None for ``none``).  ``--lr_decay_steps 0`` with linear / cosine means the
    whole run, which needs the number of batches per epoch: a loader without a length is refused."""
    if args.lr_schedule == "none":
        return None
    decay = int(args.lr_decay_steps)
    if decay == 0 and args.lr_schedule in ("linear", "cosine"):
        try:
            batches = len(train_loader)
        except TypeError:
            raise SystemExit(f"--lr_schedule {args.lr_schedule} with --lr_decay_steps 0 needs the length of the "
                             f"training loader, and this one has none: pass --lr_decay_steps")
        if args.limit_train_batches is not None:
            batches = min(batches, args.limit_train_batches)
        decay = args.max_epochs * -(-batches // args.accumulate_grad_batches)
    return dict(kind=args.lr_schedule, warmup_steps=int(args.warmup_steps), decay_steps=decay,
                min_lr_ratio=float(args.min_lr_ratio))


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    # ---- reference flags
    p.add_argument("--device", type=str, default="gpu")
    p.add_argument("--gpus", type=str, default="0")
    p.add_argument("--max_epochs", type=int, default=100)
    p.add_argument("--batch_size", type=int, default=8)
    p.add_argument("--num_workers", type=int, default=15)
    p.add_argument("--milestones", type=int, nargs="+", default=None,
                   help="epochs at which MultiStepLR multiplies every lr by 0.1 (default: 50 75 90, or none with a "
                        "decaying --lr_schedule; explicit milestones always apply)")
    p.add_argument("--lr", type=float, default=5e-4)
    p.add_argument("--exp_name", type=str, default="exp_rt1")
    p.add_argument("--log_dir", type=str, default="./exp/logs")
    p.add_argument("--ckpt_dir", type=str, default="./exp/ckpt")
    p.add_argument("--log_every_n_steps", type=int, default=500)
    p.add_argument("--ckpt_every_n_epochs", type=int, default=1)
    p.add_argument("--dataset_dir", type=str, default="./data/language_table_b2b_npz")
    p.add_argument("--train_episode", type=int, default=7800)
    p.add_argument("--test_episode", type=int, default=50)
    p.add_argument("--eval_episode", type=int, default=50)
    p.add_argument("--random_crop_factor", type=float, default=0.95)
    p.add_argument("--height", type=int, default=256)
    p.add_argument("--width", type=int, default=456)
    p.add_argument("--seq_len", type=int, default=6)
    # ---- framework flags
    p.add_argument("--mode", choices=["train", "debug"], default="train")
    p.add_argument("--synthetic", action="store_true", help="synthetic windows of the real shapes (no dataset)")
    p.add_argument("--synthetic_samples", type=int, default=4096)
    p.add_argument("--resume", type=str, default=None, help="checkpoint to resume from (e.g. .../last.ckpt)")
    p.add_argument("--dtype", choices=["bf16", "fp32"], default="bf16")
    p.add_argument("--backend", choices=["auto", "hip", "torch"], default="auto")
    p.add_argument("--num_layers", type=int, default=8)
    p.add_argument("--weight_decay", type=float, default=0.0, help="AdamW decoupled decay (0 = Adam, reference)")
    p.add_argument("--optimizer", choices=["adam", "lamb"], default="adam",
                   help="lamb: layer-wise trust ratios (LAMB) on Adam's moments -- every tensor's update is scaled to "
                        "lr * ||p|| / ||update||, for large effective batches; the --no_decay_norm_bias groups keep "
                        "the plain step; checkpoints are interchangeable with adam's")
    p.add_argument("--no_decay_norm_bias", action="store_true",
                   help="--weight_decay skips BatchNorm / LayerNorm scales and shifts, every bias and the embeddings "
                        "(their own parameter group inside the one fused Adam launch)")
    p.add_argument("--backbone_lr_mult", type=float, default=1.0,
                   help="learning rate of the pretrained EfficientNet-B3 backbone as a multiple of --lr (> 0; needs "
                        "--pretrained or --resume: without pretrained weights there is nothing to protect)")
    p.add_argument("--gradient_clip_val", type=float, default=0.0,
                   help="clip the global gradient norm to this value on the device (Lightning's name; 0 = off)")
    p.add_argument("--skip_nonfinite_steps", action="store_true",
                   help="a step whose gradient norm is not finite changes nothing: no Adam update, BN running "
                        "statistics rolled back")
    p.add_argument("--accumulate_grad_batches", type=int, default=1,
                   help="optimizer step every N batches on the mean of their gradients (Lightning's name; N x "
                        "--batch_size on one GPU computes the mean gradient of N data-parallel ranks)")
    p.add_argument("--ema_decay", type=float, default=0.0,
                   help="exponential moving average of the trainable weights, updated inside the fused Adam launch "
                        "(0 = off; 0.999-0.9999 is usual); validation also logs eval_loss_ema, checkpoints carry the "
                        "average under 'ema', eval_rt1.py --ema evaluates it")
    p.add_argument("--no_ema_warmup", action="store_true",
                   help="use --ema_decay from the first step instead of min(decay, (1 + t) / (10 + t))")
    p.add_argument("--lr_schedule", choices=["none"] + list(LR_SCHEDULES), default="none",
                   help="per-step learning-rate factor on every group's lr, formed on the device from the effective "
                        "Adam step (skipped steps do not count): linear warm-up over --warmup_steps, then constant, "
                        "linear or cosine decay to --min_lr_ratio at --lr_decay_steps, or inverse-sqrt decay")
    p.add_argument("--warmup_steps", type=int, default=0, help="optimizer steps of linear warm-up (the first uses 1/W)")
    p.add_argument("--lr_decay_steps", type=int, default=0,
                   help="optimizer step at which linear / cosine reach --min_lr_ratio (0 = the whole run: max_epochs * "
                        "ceil(batches per epoch / accumulate_grad_batches))")
    p.add_argument("--min_lr_ratio", type=float, default=0.0, help="floor of the decay as a fraction of the lr")
    p.add_argument("--label_smoothing", type=float, default=0.0,
                   help="training objective: label smoothing in [0, 1) over all vocab bins (torch's cross_entropy "
                        "convention); validation and test stay the plain cross-entropy; train_nll_step is logged")
    p.add_argument("--z_loss", type=float, default=0.0,
                   help="training objective: + z_loss * logsumexp(logits)^2 per action token (PaLM's auxiliary loss; "
                        "1e-4 is usual); validation and test stay the plain cross-entropy")
    p.add_argument("--token_accuracy", action="store_true",
                   help="log the action-token accuracy: train_acc_step, eval_acc, test_acc and per-slot .../tok<a>")
    p.add_argument("--bucket_cap_mb", type=float, default=32.0)
    p.add_argument("--no_broadcast_buffers", action="store_true")
    p.add_argument("--comm", choices=["torch", "native"], default="torch",
                    help="gradient collectives: torch ProcessGroup (RCCL) or the native C++ RCCL communicator")
    p.add_argument("--limit_train_batches", type=int, default=None)
    p.add_argument("--limit_val_batches", type=int, default=None)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--graph", choices=["auto", "on", "off"], default="auto",
                   help="hipGraph training step (auto = on for the hip backend on GPU; the step bench.py measures)")
    p.add_argument("--pretrained", type=str, default=None,
                   help="torchvision efficientnet_b3 state dict for the backbone (reference weights='imagenet')")
    p.add_argument("--data_format", choices=["auto", "npz", "shard"], default="auto",
                   help="episode storage: per-episode .npz (CPU PIL crop) or a packed shard (GPU crop+resize)")
    p.add_argument("--data_residency", choices=["auto", "host", "hbm"], default="auto",
                   help="packed shards: 'hbm' keeps each rank's episodes resident on its GPU (one copy at start, no "
                        "per-step frame H2D; data/resident.py), 'host' gathers raw frames into pinned batches every "
                        "step; 'auto' = hbm on GPU when the rank's frames fit --hbm_data_gb")
    p.add_argument("--hbm_data_gb", type=float, default=96.0,
                   help="HBM budget per rank for resident training frames (of 288 GB per MI355X)")
    p.add_argument("--photometric", action="store_true",
                   help="colour augmentation of the training frames on the GPU decode path (packed shards only; one "
                        "draw per window; validation and test never get it): brightness +-0.1, saturation x[0.8, "
                        "1.2], hue +-0.03 turns, contrast x[0.8, 1.2] unless the flags below say otherwise")
    p.add_argument("--photometric_brightness", type=float, default=None, metavar="D",
                   help="brightness delta drawn in [-D, D] (0 <= D <= 1)")
    p.add_argument("--photometric_saturation", type=float, nargs=2, default=None, metavar=("LO", "HI"),
                   help="saturation factor drawn in [LO, HI] (0 <= LO <= HI)")
    p.add_argument("--photometric_hue", type=float, default=None, metavar="D",
                   help="hue delta in turns drawn in [-D, D] (0 <= D <= 0.5)")
    p.add_argument("--photometric_contrast", type=float, nargs=2, default=None, metavar=("LO", "HI"),
                   help="contrast factor drawn in [LO, HI] (0 <= LO <= HI)")
    return p


def photometric_spec(args):
    """The ``PhotometricDistortions`` range spec the --photometric flags ask for (None: off).  Raises ValueError on a
    range the transform has no meaning for."""
    if not getattr(args, "photometric", False):
        return None
    from pytorch_rt1_for_distributed_training_amd.data.augment import PhotometricDistortions
    from pytorch_rt1_for_distributed_training_amd.data.photometric import check_spec
    spec = PhotometricDistortions()
    if args.photometric_brightness is not None:
        spec.brightness_max_delta = args.photometric_brightness
    if args.photometric_saturation is not None:
        spec.saturation_lower, spec.saturation_upper = args.photometric_saturation
    if args.photometric_hue is not None:
        spec.hue_max_delta = args.photometric_hue
    if args.photometric_contrast is not None:
        spec.contrast_lower, spec.contrast_upper = args.photometric_contrast
    return check_spec(spec)


def _spawn_local(args) -> int:
    """One process per listed GPU (what Lightning's DDP launcher does for the reference), via the shared
    launcher (``parallel/launch.py``): children are fresh processes, the parent never touches the GPU."""
    from pytorch_rt1_for_distributed_training_amd.parallel.launch import spawn_local
    gpus = [g for g in args.gpus.split(",") if g.strip() != ""]
    return spawn_local(len(gpus), sys.argv, {"CUDA_VISIBLE_DEVICES": ",".join(gpus)})


def make_config(args):
    from pytorch_rt1_for_distributed_training_amd.config import RT1Config
    return RT1Config(height=args.height, width=args.width, seq_len=args.seq_len, num_layers=args.num_layers,
                     dtype=args.dtype, backend=args.backend, pretrained=getattr(args, "pretrained", None))


def make_loaders(args, cfg, ctx):
    import torch
    from torch.utils.data import DataLoader
    from torch.utils.data.distributed import DistributedSampler
    from pytorch_rt1_for_distributed_training_amd import data as D

    def loader(ds, shuffle):
        sampler = DistributedSampler(ds, ctx.world_size, ctx.rank, shuffle=shuffle) if ctx.distributed else None
        return DataLoader(ds, batch_size=args.batch_size, shuffle=(shuffle and sampler is None), sampler=sampler,
                          collate_fn=D.collate_fn, num_workers=args.num_workers,
                          pin_memory=ctx.device.type == "cuda", drop_last=shuffle,
                          persistent_workers=args.num_workers > 0)

    if args.synthetic:
        mk = lambda n, seed: D.SyntheticDataset(n, cfg.seq_len, cfg.height, cfg.width, seed=seed, uint8=True)
        return (loader(mk(args.synthetic_samples, 0), True), loader(mk(max(args.batch_size * 2, 16), 1), False),
                loader(mk(max(args.batch_size * 2, 16), 2), False))
    root = args.dataset_dir
    fmt = getattr(args, "data_format", "auto")
    if fmt == "shard" or (fmt == "auto" and D.is_shard(os.path.join(root, "train"))):
        # packed shards: raw frames gathered into pinned batches by threads; crop+resize on the GPU
        def shard(split, shuffle, bs):
            return D.ShardBatchLoader(os.path.join(root, split), bs, cfg.seq_len, args.random_crop_factor,
                                      shuffle=shuffle, rank=ctx.rank, world=ctx.world_size, seed=args.seed,
                                      drop_last=shuffle, threads=max(2, min(args.num_workers, 16)),
                                      pin=ctx.device.type == "cuda",
                                      photometric=photometric_spec(args) if split == "train" else None)
        train = _resident_train_loader(args, cfg, ctx, os.path.join(root, "train"))
        if train is None:
            train = shard("train", True, args.batch_size)
        return train, shard("test", False, args.batch_size), shard("val", False, args.batch_size)
    if getattr(args, "photometric", False):
        raise SystemExit(PHOTOMETRIC_NEEDS_SHARD)
    tf = D.DecodeAndRandomResizedCrop(args.random_crop_factor, (args.width, args.height), as_uint8=True)
    for split in ("train", "test", "val"):
        if not os.path.isdir(os.path.join(root, split)):
            raise SystemExit(f"dataset split {os.path.join(root, split)} not found (use --synthetic, or convert the "
                             f"Language-Table episodes with data.convert_reference_episodes)")
    train = D.EpisodeWindowDataset(os.path.join(root, "train"), range(args.train_episode), cfg.seq_len, tf)
    test = D.EpisodeWindowDataset(os.path.join(root, "test"), range(args.test_episode), cfg.seq_len, tf)
    val = D.EpisodeWindowDataset(os.path.join(root, "val"), range(args.eval_episode), cfg.seq_len, tf)
    return loader(train, True), loader(test, False), loader(val, False)


def _resident_train_loader(args, cfg, ctx, path):
    """The HBM-resident training loader (data/resident.py) when --data_residency asks for it (or 'auto' finds the
    rank's frames within --hbm_data_gb on a GPU); None selects the host-gather loader."""
    from pytorch_rt1_for_distributed_training_amd.data import resident as R
    from pytorch_rt1_for_distributed_training_amd.data.shards import Shard
    mode = getattr(args, "data_residency", "auto")
    if mode == "host" or (mode == "auto" and ctx.device.type != "cuda"):
        return None
    sh = Shard(path)
    try:
        eps = R.assign_episodes(sh.lengths, ctx.world_size, args.seed)[ctx.rank]
    except ValueError as e:          # fewer episodes than ranks
        if mode == "hbm":
            raise
        if ctx.is_main:
            print(f"[data] {e}: host-gather path", flush=True)
        return None
    need_gb = float(sh.lengths[eps].sum()) * float(np.prod(sh.frame_shape)) / 2 ** 30
    if mode == "auto" and need_gb > args.hbm_data_gb:
        if ctx.is_main:
            print(f"[data] {need_gb:.1f} GB of frames per rank > --hbm_data_gb {args.hbm_data_gb}: host-gather path",
                  flush=True)
        return None
    res = R.ResidentShard(path, ctx.device, rank=ctx.rank, world=ctx.world_size, max_gb=args.hbm_data_gb,
                          seed=args.seed)
    if ctx.is_main:
        print(f"[data] resident training frames: {res.frames.shape[0]} frames, {res.nbytes / 2 ** 30:.2f} GB per rank, "
              f"loaded in {res.load_s:.1f} s", flush=True)
    return R.ResidentBatchLoader(res, args.batch_size, cfg.seq_len, args.random_crop_factor, shuffle=True,
                                 seed=args.seed, drop_last=True, photometric=photometric_spec(args))


def _batch_transform(train_loader, cfg):
    from pytorch_rt1_for_distributed_training_amd.data.resident import ResidentBatchLoader, decode_resident
    from pytorch_rt1_for_distributed_training_amd.data.shards import decode_on_device
    res = train_loader.res if isinstance(train_loader, ResidentBatchLoader) else None

    def transform(b):
        if res is not None and "plan_rows" in b:
            return decode_resident(res, b, cfg.height, cfg.width)
        return decode_on_device(b, cfg.height, cfg.width)
    return transform


def train(args):
    import torch
    from pytorch_rt1_for_distributed_training_amd.engine.step import TrainEngine
    from pytorch_rt1_for_distributed_training_amd.engine.trainer import Trainer
    from pytorch_rt1_for_distributed_training_amd.models import build_rt1
    from pytorch_rt1_for_distributed_training_amd.parallel import dist as pdist
    from pytorch_rt1_for_distributed_training_amd.utils.checkpoint import ModelCheckpoint
    from pytorch_rt1_for_distributed_training_amd.utils.logging import CSVLogger, MultiLogger, TensorBoardLogger

    ctx = pdist.init_distributed("cpu" if args.device == "cpu" else "auto")
    torch.manual_seed(args.seed + ctx.rank)
    cfg = make_config(args)
    train_loader, test_loader, eval_loader = make_loaders(args, cfg, ctx)
    if ctx.is_main:
        print(f"Building RT-1 (world={ctx.world_size}, device={ctx.device}, dtype={cfg.dtype})", flush=True)
    torch.manual_seed(args.seed)  # identical init on every rank (rank 0 broadcasts anyway)
    model = build_rt1(cfg)
    # --graph auto: the hipGraph step (segmented graph-DP with several ranks), the step bench.py measures.  The trainer
    # checks it once against the eager bucketed DP step on the first batch (bitwise, every rank) and falls back to the
    # eager step if they differ (Trainer._check_graph)
    use_graph = args.graph in ("on", "auto")
    lr_schedule = resolve_lr_schedule(args, train_loader)
    engine = TrainEngine(model, cfg, lr=args.lr, milestones=resolve_milestones(args), weight_decay=args.weight_decay,
                         bucket_cap_mb=args.bucket_cap_mb, broadcast_buffers=not args.no_broadcast_buffers,
                         comm=args.comm, graph=use_graph,
                         max_grad_norm=args.gradient_clip_val if args.gradient_clip_val > 0 else None,
                         skip_nonfinite=args.skip_nonfinite_steps,
                         accumulate_grad_batches=args.accumulate_grad_batches, ema_decay=args.ema_decay,
                         ema_warmup=not args.no_ema_warmup, no_decay_norm_bias=args.no_decay_norm_bias,
                         backbone_lr_mult=args.backbone_lr_mult, pretrained=bool(args.pretrained or args.resume),
                         lr_schedule=lr_schedule, label_smoothing=args.label_smoothing, z_loss=args.z_loss,
                         token_accuracy=args.token_accuracy, optimizer=args.optimizer)
    if ctx.is_main:
        if args.optimizer != "adam":
            off = [n for n in engine.optimizer.group_names if n.endswith("no_decay")]
            print(f"[train] optimizer {args.optimizer}: layer-wise trust ratios on {len(engine.flat.params)} tensors"
                  + (f", not on the groups {off}" if off else ""), flush=True)
        print(f"[train] gradient_clip_val {args.gradient_clip_val if args.gradient_clip_val > 0 else 'off'}, "
              f"skip_nonfinite_steps {'on' if args.skip_nonfinite_steps else 'off'}, "
              f"accumulate_grad_batches {args.accumulate_grad_batches}", flush=True)
        if len(engine.lrs) > 1:
            print("[train] parameter groups: " + ", ".join(
                f"{g.get('name')} ({len(g['params'])} tensors, lr {g['lr']:.3g}, weight_decay {g['weight_decay']:g})"
                for g in engine.optimizer.param_groups), flush=True)
        if lr_schedule is not None:
            print(f"[train] lr_schedule {lr_schedule}, milestones {resolve_milestones(args)}", flush=True)
        if args.ema_decay > 0:
            print(f"[train] ema_decay {args.ema_decay} (warm-up {'off' if args.no_ema_warmup else 'on'})", flush=True)
        if args.photometric:
            ps = photometric_spec(args)
            print(f"[train] photometric brightness +-{ps.brightness_max_delta:g}, saturation "
                  f"[{ps.saturation_lower:g}, {ps.saturation_upper:g}], hue +-{ps.hue_max_delta:g} turns, contrast "
                  f"[{ps.contrast_lower:g}, {ps.contrast_upper:g}] (one draw per window, training frames only)",
                  flush=True)
        if args.label_smoothing or args.z_loss or args.token_accuracy:
            print(f"[train] label_smoothing {args.label_smoothing:g}, z_loss {args.z_loss:g} (training mode only: "
                  f"eval_loss / test_loss stay the plain CE), token_accuracy {'on' if args.token_accuracy else 'off'}",
                  flush=True)
    ckpt = ModelCheckpoint(os.path.join(args.ckpt_dir, args.exp_name), every_n_epochs=args.ckpt_every_n_epochs)
    loggers = []
    if ctx.is_main:
        loggers = [CSVLogger(os.path.join(args.log_dir, "csv"), args.exp_name),
                   TensorBoardLogger(os.path.join(args.log_dir, "tb"), args.exp_name)]
    trainer = Trainer(engine, args.max_epochs, args.log_every_n_steps, ckpt, MultiLogger(loggers),
                      args.limit_train_batches, args.limit_val_batches,
                      batch_transform=_batch_transform(train_loader, cfg))
    if args.resume:
        trainer.resume(args.resume)
    if ctx.is_main:
        print("Start Training ...", flush=True)
    trainer.fit(train_loader, eval_loader)
    if ctx.is_main:
        print("Start Final Testing ...", flush=True)
    trainer.test(test_loader, args.limit_val_batches)
    pdist.shutdown()


def debug(args):
    """Reference ``debug()``: train-mode forward (B=2) then one inference step (B=1)."""
    import torch
    from pytorch_rt1_for_distributed_training_amd.models import build_rt1
    from pytorch_rt1_for_distributed_training_amd.engine.step import TrainEngine
    from pytorch_rt1_for_distributed_training_amd.parallel import dist as pdist

    ctx = pdist.init_distributed("cpu" if args.device == "cpu" else "auto")
    cfg = make_config(args)
    model = build_rt1(cfg)
    eng = TrainEngine(model, cfg, order_probe=False)
    dev, T, H, W = ctx.device, cfg.seq_len, cfg.height, cfg.width
    batch = {"train_observation": {"image": torch.full((2, T, 3, H, W), 0.5, device=dev),
                                   "natural_language_embedding": torch.full((2, T, 512), 1.0, device=dev)},
             "action_label": {"terminate_episode": torch.full((2, T), 1, device=dev),
                              "action": torch.zeros(2, T, 2, device=dev)}}
    print("=========Training Debug=========")
    eng.model.train()
    with eng.autocast():
        eng.model.set_actions(batch["action_label"])
        loss_bt, aux = eng.model.train_forward(batch["train_observation"]["image"],
                                               batch["train_observation"]["natural_language_embedding"],
                                               batch["action_label"])
    pred = eng.model._action_tokenizer.detokenize(aux["predicted_tokens_for_output"])
    print(f"pred_action:{tuple(pred['action'].shape)}")
    print(f"is_terminate:{tuple(pred['terminate_episode'].shape)}")
    print(f"action_loss:{tuple(loss_bt.shape)}, mean_loss:{float(loss_bt.mean()):.6f}")
    print("=========Inference Debug=========")
    eng.model.eval()
    state = eng.model.initial_state(1, dev)
    with eng.autocast():
        pred, state = eng.model({"image": torch.full((1, 3, H, W), 0.5, device=dev),
                                 "natural_language_embedding": torch.full((1, 512), 1.0, device=dev)}, state)
    print(f"pred_action:{tuple(pred['action'].shape)}")
    print(f"is_terminate:{tuple(pred['terminate_episode'].shape)}")
    print(f"seq_idx:{state['seq_idx'].tolist()}")


def check_args(parser, args):
    """Refusals that need no model: a flag combination that cannot mean what it says."""
    if not args.backbone_lr_mult > 0:
        parser.error(f"--backbone_lr_mult must be > 0, got {args.backbone_lr_mult}")
    if args.backbone_lr_mult != 1.0 and not (args.pretrained or args.resume):
        parser.error("--backbone_lr_mult needs --pretrained or --resume: a randomly initialised backbone has no "
                     "pretrained weights to protect with a smaller learning rate")
    if not 0.0 <= args.label_smoothing < 1.0:                # NaN fails both comparisons
        parser.error(f"--label_smoothing must be in [0, 1), got {args.label_smoothing}")
    if not 0.0 <= args.z_loss < float("inf"):
        parser.error(f"--z_loss must be finite and >= 0, got {args.z_loss}")
    if args.warmup_steps < 0:
        parser.error(f"--warmup_steps must be >= 0, got {args.warmup_steps}")
    if args.lr_decay_steps < 0:
        parser.error(f"--lr_decay_steps must be >= 0 (0 = the whole run), got {args.lr_decay_steps}")
    if not 0.0 <= args.min_lr_ratio <= 1.0:
        parser.error(f"--min_lr_ratio must be in [0, 1], got {args.min_lr_ratio}")
    if args.lr_schedule in ("linear", "cosine") and 0 < args.lr_decay_steps <= args.warmup_steps:
        parser.error(f"--lr_decay_steps ({args.lr_decay_steps}) must be greater than --warmup_steps "
                     f"({args.warmup_steps}) for --lr_schedule {args.lr_schedule}")
    if args.lr_schedule == "none" and (args.warmup_steps or args.lr_decay_steps or args.min_lr_ratio):
        parser.error("--warmup_steps / --lr_decay_steps / --min_lr_ratio need --lr_schedule")
    ranges = (args.photometric_brightness, args.photometric_saturation, args.photometric_hue,
              args.photometric_contrast)
    if not args.photometric and any(v is not None for v in ranges):
        parser.error("--photometric_brightness / _saturation / _hue / _contrast need --photometric")
    if args.photometric:
        if args.synthetic or args.data_format == "npz":
            parser.error(PHOTOMETRIC_NEEDS_SHARD)
        try:
            photometric_spec(args)
        except ValueError as e:
            parser.error(str(e))


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    check_args(parser, args)
    gpus = [g for g in args.gpus.split(",") if g.strip() != ""]
    if args.mode == "train" and args.device != "cpu" and len(gpus) > 1 and "RANK" not in os.environ:
        return _spawn_local(args)
    if "RANK" not in os.environ and args.device != "cpu" and len(gpus) == 1:
        os.environ.setdefault("CUDA_VISIBLE_DEVICES", gpus[0])
    if args.device != "cpu":
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        from pytorch_rt1_for_distributed_training_amd.utils.tuned_gemms import enable_tuned_gemms
        enable_tuned_gemms()          # recorded hipBLASLt solutions (before the first GEMM)
    if args.mode == "debug":
        debug(args)
    else:
        train(args)
    return 0


if __name__ == "__main__":
    sys.exit(main())
