#!/usr/bin/env python3
"""Cost of the exponential moving average of the weights (csrc/kernels/adam.hip, the EMA forms) on the GPU.

  python tools/bench_ema.py kernels      # (a) at the full model's size, in one process: the unchanged flat_adam_dev,
                                         #     flat_adam_dev + torch's lerp_ (the two-launch alternative), and the
                                         #     fused flat_adam_ema_dev, plain and clip form
  python tools/bench_ema.py step_ab      # (b) the bench step (full model, 300x300, T6, b128, graph) with the EMA off
                                         #     and on, alternated three times, one child process per run
  python tools/bench_ema.py step --on    # one such run

(a) times 200 back-to-back repetitions between two device events after a warm-up, three passes over the variants in
turn, and reports microseconds and GB/s against the bytes each must move: 28n for Adam (read p, g, m, v; write p, m,
v), 28n + 12n for Adam followed by lerp_ (read ema, p; write ema), 36n fused.  The five buffers are 141 MB each at the
full model's size, so no call finds its operands in the 256 MB last-level cache.  The baselines are flat_adam_dev --
the kernel every run without the option launches, unchanged -- and torch's lerp_; the fused kernel is never compared
with itself.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_FLAT = 35_200_128      # flat parameter floats of the full model (parallel.FlatParameters.numel, 64-float aligned)


def _time_us(fn, reps=200, warm=20):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


def kernels(a):
    import torch
    from pytorch_rt1_for_distributed_training_amd.ops import adam as ops
    assert torch.cuda.is_available(), "needs a GPU"
    n = a.n
    g = torch.Generator(device="cuda").manual_seed(0)
    p = torch.randn(n, device="cuda", generator=g)
    grad = torch.randn(n, device="cuda", generator=g) * 1e-3
    m, v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    ema = p.clone()
    state = torch.tensor([1.0, 5e-4], device="cuda")
    es = torch.zeros(4, device="cuda")
    cs = torch.zeros(8, device="cuda")
    pt = torch.zeros(ops.gradnorm_partials(n), dtype=torch.float64, device="cuda")
    ops.grad_norm_clip_(grad, cs, pt, max_norm=1.0, grad_scale=1.0, skip_nonfinite=True)      # a verdict to obey
    kw = dict(beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, grad_scale=1.0)
    omd = 1.0 - a.decay
    ekw = dict(one_minus_decay=omd, warmup=True, **kw)

    def adam():
        ops.flat_adam_dev_step(p, grad, m, v, state, **kw)

    def adam_then_lerp():
        ops.flat_adam_dev_step(p, grad, m, v, state, **kw)
        ema.lerp_(p, omd)

    def lerp():
        ema.lerp_(p, omd)

    def fused():
        ops.flat_adam_ema_dev_step(p, grad, m, v, ema, state, es, None, **ekw)

    def clip():
        ops.flat_adam_clip_dev_step(p, grad, m, v, state, cs, **kw)

    def fused_clip():
        ops.flat_adam_ema_dev_step(p, grad, m, v, ema, state, es, cs, **ekw)

    print(f"n = {n} floats ({4 * n / 1e6:.1f} MB per buffer), 200 repetitions each, 3 passes, "
          f"{torch.cuda.get_device_name(0)}", flush=True)
    rows = [("flat_adam_dev (baseline, unchanged)", adam, 28 * n),
            ("flat_adam_dev + torch lerp_ (two launches)", adam_then_lerp, 40 * n),
            ("torch lerp_ alone", lerp, 12 * n),
            ("flat_adam_ema_dev (fused)", fused, 36 * n),
            ("flat_adam_clip_dev (baseline, unchanged)", clip, 28 * n),
            ("flat_adam_ema_dev, clip form (fused)", fused_clip, 36 * n)]
    best = {}
    for rep in range(3):
        for name, fn, nbytes in rows:
            us = _time_us(fn)
            best.setdefault(name, []).append(us)
            print(f"pass {rep + 1}  {name:44s} {us:9.2f} us  {nbytes / us / 1e3:9.1f} GB/s over {nbytes / 1e6:9.3f} MB",
                  flush=True)
    med = {k: sorted(x)[1] for k, x in best.items()}
    base, two, fus = (med[rows[i][0]] for i in (0, 1, 3))
    print(f"median of 3: adam {base:.2f} us, adam + lerp_ {two:.2f} us, fused {fus:.2f} us", flush=True)
    print(f"fused / adam = {fus / base:.3f} (byte model 36/28 = {36 / 28:.3f}); fused / two-launch = {fus / two:.3f} "
          f"(byte model 36/40 = {36 / 40:.3f}); fused {'beats' if fus < two else 'DOES NOT beat'} the two launches",
          flush=True)
    print(f"clip form: fused {med[rows[5][0]]:.2f} us against {med[rows[4][0]]:.2f} us", flush=True)
    print(f"ema_state after the runs: {es.tolist()}", flush=True)


def step(a):
    import torch
    from pytorch_rt1_for_distributed_training_amd.config import RT1Config
    from pytorch_rt1_for_distributed_training_amd.data.prefetch import DevicePrefetcher
    from pytorch_rt1_for_distributed_training_amd.data.synthetic import SyntheticStream
    from pytorch_rt1_for_distributed_training_amd.engine.step import TrainEngine
    from pytorch_rt1_for_distributed_training_amd.models import build_rt1
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    cfg = RT1Config(height=a.height, width=a.width, seq_len=a.seq_len, backend="hip")
    torch.manual_seed(0)
    kw = dict(ema_decay=a.decay) if a.on else {}
    eng = TrainEngine(build_rt1(cfg), cfg, order_probe=False, graph=True, device=dev, **kw)
    stream = SyntheticStream(a.batch, cfg.seq_len, cfg.height, cfg.width, ring=2, uint8=True, seed=0)
    batches = iter(DevicePrefetcher(stream, dev, depth=2))
    for _ in range(a.warmup):
        eng.train_step(next(batches))
        torch.cuda.synchronize()
    assert eng._graph is not None, "the step was not captured"
    t0 = time.perf_counter()
    for _ in range(a.steps):
        loss = eng.train_step(next(batches))
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / a.steps
    out = dict(ema="on" if a.on else "off", ms_per_step=round(ms, 3), steps=a.steps, loss=float(loss))
    if a.on:
        opt = eng.optimizer
        out.update(ema_decay_now=float(opt.ema_decay_now), ema_updates=opt.ema_num_updates)
    print(json.dumps(out), flush=True)


def step_ab(a):
    """off, on, off, on, off, on: a fresh child process per run (nothing is shared but the GPU)."""
    res = {"off": [], "on": []}
    for rep in range(3):
        for on in (False, True):
            cmd = [sys.executable, os.path.abspath(__file__), "step", "--steps", str(a.steps), "--warmup",
                   str(a.warmup), "--batch", str(a.batch), "--height", str(a.height), "--width", str(a.width),
                   "--seq_len", str(a.seq_len), "--decay", str(a.decay)] + (["--on"] if on else [])
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.child_timeout)
            if r.returncode != 0:
                print(r.stdout[-2000:], r.stderr[-4000:], flush=True)
                raise SystemExit(f"child failed with {r.returncode}; stopping")
            line = r.stdout.strip().splitlines()[-1]
            print(f"rep {rep + 1} {line}", flush=True)
            res["on" if on else "off"].append(json.loads(line)["ms_per_step"])
    off, on = res["off"], res["on"]
    mean = lambda x: sum(x) / len(x)
    print(f"off: {off} ms/step (mean {mean(off):.3f})", flush=True)
    print(f"on : {on} ms/step (mean {mean(on):.3f})", flush=True)
    print(f"on-cost: {1e3 * (mean(on) - mean(off)):.1f} us/step "
          f"(ranges off {min(off):.3f}-{max(off):.3f}, on {min(on):.3f}-{max(on):.3f})", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["kernels", "step", "step_ab"])
    ap.add_argument("--n", type=int, default=N_FLAT)
    ap.add_argument("--decay", type=float, default=0.9999)
    ap.add_argument("--on", action="store_true", help="step: EMA on (ema_decay = --decay, warm-up on)")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--height", type=int, default=300)
    ap.add_argument("--width", type=int, default=300)
    ap.add_argument("--seq_len", type=int, default=6)
    ap.add_argument("--child_timeout", type=float, default=240.0)
    a = ap.parse_args()
    {"kernels": kernels, "step": step, "step_ab": step_ab}[a.mode](a)


if __name__ == "__main__":
    main()
