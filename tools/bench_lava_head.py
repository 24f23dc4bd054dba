#!/usr/bin/env python3
"""Time LAVA's policy head (DenseResnet 1024 x 2 blocks + action projection, din = 128) forward + backward, eager torch
against the HIP head (csrc/kernels/lavahead.hip, ops/lava_head.dense_resnet_head), in one process on one GPU.

Rows: B = 4, 32, 256 windows.  The modes share weights and inputs and are timed alternately, round by round, with
device events around `iters` calls; the median, minimum and maximum over the rounds are printed.  Then, in a separate
pass, the device kernels one forward + backward launches, counted from a profiler trace, and per hip kernel the bytes
it must move (computed from the shapes: operands read once, results written once) over its time in that trace.

    python tools/bench_lava_head.py [--out profiles/lava_head.log]
"""
from __future__ import annotations

import argparse
import copy
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_rt1_for_distributed_training_amd.models.lava import DenseResnet, _dense, policy_head  # noqa: E402
from pytorch_rt1_for_distributed_training_amd.ops.lava_head import resolve_backend  # noqa: E402

DIN, WIDTH, BLOCKS, ACT = 128, 1024, 2, 2
MODES = ("torch", "hip")


def _step(head, proj, x, dout):
    x.grad = None
    (policy_head(x, head, proj) * dout).sum().backward()


def _time(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters                        # us per call


def _heads(dev):
    torch.manual_seed(0)
    head, proj = DenseResnet(DIN, WIDTH, BLOCKS).to(dev), _dense(WIDTH, ACT).to(dev)
    heads = {m: (copy.deepcopy(head), copy.deepcopy(proj)) for m in MODES}
    heads["hip"][0].backend = "hip"
    return heads


def _kernel_bytes(b):
    """Bytes each hip launch must move, in launch order: forward then backward."""
    lin = [(DIN, WIDTH, False)] + [(WIDTH, WIDTH // 4, False), (WIDTH // 4, WIDTH // 4, False),
                                   (WIDTH // 4, WIDTH, True)] * BLOCKS
    fwd = [4 * (b * k + n * k + n + b * n * (2 if res else 1)) for k, n, res in lin]
    fwd.append(4 * (b * WIDTH + ACT * WIDTH + ACT + b * ACT))
    bwd = [4 * (b * ACT + b * WIDTH + ACT * WIDTH + b * WIDTH + ACT * WIDTH + ACT)]
    for i, (k, n, _) in reversed(list(enumerate(lin))):
        carry = i % 3 == 1                                               # a block's first linear adds the residual's
        bwd.append(4 * (b * n + b * k + n * k + b * k * (2 if carry else 1) + n * k + n))
    return fwd + bwd


def _trace(step):
    """(name, us) of the device kernels of one call (copies and memsets are not kernels and are not counted)."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
          and not e.name.lower().startswith(("memcpy", "memset", "copy"))]
    ev.sort(key=lambda e: e.time_range.start)
    return [(e.name, e.device_time) for e in ev]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default="", help="also append the rows to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_lava_head needs a GPU")
    resolve_backend("hip", DIN, WIDTH, ACT)
    dev = torch.device("cuda", 0)
    def emit(line):                                                      # a row is out before the next measurement starts
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")

    emit(f"# {torch.cuda.get_device_name(0)}; policy head din={DIN} width={WIDTH} blocks={BLOCKS} action={ACT} fwd+bwd, "
         f"us per call, median [min, max] of {a.rounds} rounds x {a.iters} calls, modes alternated")
    heads = _heads(dev)
    for b in (4, 32, 256):
        x = torch.randn(b, DIN, device=dev, requires_grad=True)
        dout = torch.randn(b, ACT, device=dev)
        times = {m: [] for m in MODES}
        for m in MODES:                                                  # warm-up: code objects, library algorithms
            for _ in range(5):
                _step(*heads[m], x, dout)
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for m in MODES:
                times[m].append(_time(lambda: _step(*heads[m], x, dout), a.iters))
        med = {m: statistics.median(v) for m, v in times.items()}
        row = " ".join(f"{m} {med[m]:8.1f} [{min(v):8.1f}, {max(v):8.1f}]" for m, v in times.items())
        emit(f"B={b:4d}  {row}  torch/hip {med['torch'] / med['hip']:.2f}x")
    for b in (4, 32, 256):
        x = torch.randn(b, DIN, device=dev, requires_grad=True)
        dout = torch.randn(b, ACT, device=dev)
        traces = {m: _trace(lambda: _step(*heads[m], x, dout)) for m in MODES}
        emit(f"B={b:4d} kernels per call (fwd+bwd, loss and its backward included): "
             + ", ".join(f"{m} {len(t)}" for m, t in traces.items())
             + f"; device time of them, us: " + ", ".join(f"{m} {sum(u for _, u in t):.1f}" for m, t in traces.items()))
        ours = [(n, u) for n, u in traces["hip"] if "lava_head" in n]
        nbytes = _kernel_bytes(b)
        if len(ours) != len(nbytes):
            raise SystemExit(f"expected {len(nbytes)} lava_head launches, the trace has {len(ours)}")
        for (name, us), nb in zip(ours, nbytes):
            short = name.split("lava_head_")[1].split("(")[0][:40]
            emit(f"B={b:4d}   {short:40s} {nb / 1024:9.1f} KiB {us:7.1f} us {nb / us / 1e3 if us > 0 else 0.0:8.1f} GB/s")


if __name__ == "__main__":
    main()
