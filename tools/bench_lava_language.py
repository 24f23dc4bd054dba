#!/usr/bin/env python3
"""Time LAVA's cross stack (the pixel-language CrossLayers) forward + backward in three modes, in one process on one
GPU: all torch; attention on hip (csrc/kernels/lavaxattn.hip) with the language rows in eager torch, the path before
the language kernels; attention and language rows on hip (csrc/kernels/lavalang.hip, ops/lava_language.cross_stack).

Rows: one layer and the 4-layer stack at (N, S) = (16, 1150) -- the reference config's frames per device -- and
(256, 1150).  The modes share weights and inputs and are timed alternately, round by round, with device events around
`iters` calls; the median, minimum and maximum over the rounds are printed.  Then the device kernels one forward +
backward launches per layer, counted from a profiler trace of the 4-layer stack, for the two hip modes.

    python tools/bench_lava_language.py [--out profiles/lava_language.log]
"""
from __future__ import annotations

import argparse
import copy
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_rt1_for_distributed_training_amd.models.lava import CrossLayer  # noqa: E402
from pytorch_rt1_for_distributed_training_amd.ops.lava_attention import resolve_backend as resolve_attention  # noqa: E402
from pytorch_rt1_for_distributed_training_amd.ops.lava_language import cross_stack, resolve_backend  # noqa: E402

D = 128
MODES = ("torch", "attn_hip", "attn+lang_hip")


def _step(mode, layers, pixels, lang, dout):
    pixels.grad = None
    if mode == "attn+lang_hip":
        q = cross_stack(pixels, lang[:, 0], layers)[0][:, None]
    else:
        q = lang
        for layer in layers:
            q = layer(pixels, q)
    (q * dout).sum().backward()


def _time(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters                        # us per call


def _stacks(depth, dev):
    torch.manual_seed(0)
    ref = [CrossLayer(D, 2, D, 0.0).to(dev) for _ in range(depth)]
    stacks = {m: copy.deepcopy(ref) for m in MODES}
    for m in MODES[1:]:
        for layer in stacks[m]:
            layer.backend = "hip"
    return stacks


def _launches(step):
    """Device kernels of one call (copies and memsets are not kernels and are not counted)."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
               and not e.name.lower().startswith(("memcpy", "memset", "copy")))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default="", help="also append the rows to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_lava_language needs a GPU")
    resolve_attention("hip", D, 2)
    resolve_backend("hip")
    dev = torch.device("cuda", 0)
    def emit(line):                                                      # a row is out before the next measurement starts
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")

    emit(f"# {torch.cuda.get_device_name(0)}; cross stack fwd+bwd, us per call, median [min, max] of {a.rounds} "
             f"rounds x {a.iters} calls, modes alternated")
    for n, s in ((16, 1150), (256, 1150)):
        for depth in (1, 4):
            stacks = _stacks(depth, dev)
            pixels = torch.randn(n, s, D, device=dev, requires_grad=True)
            lang, dout = torch.randn(n, 1, D, device=dev), torch.randn(n, 1, D, device=dev)
            times = {m: [] for m in MODES}
            for m in MODES:                                              # warm-up: code objects, library algorithms
                for _ in range(5):
                    _step(m, stacks[m], pixels, lang, dout)
            torch.cuda.synchronize()
            for _ in range(a.rounds):
                for m in MODES:
                    times[m].append(_time(lambda: _step(m, stacks[m], pixels, lang, dout), a.iters))
            med = {m: statistics.median(v) for m, v in times.items()}
            row = " ".join(f"{m} {med[m]:8.1f} [{min(v):8.1f}, {max(v):8.1f}]" for m, v in times.items())
            emit(f"N={n:4d} S={s} layers={depth}  {row}  attn_hip/attn+lang_hip "
                         f"{med['attn_hip'] / med['attn+lang_hip']:.2f}x  per layer {med['attn+lang_hip'] / depth:.1f} us")
    for n in (16, 256):
        stacks = _stacks(4, dev)
        pixels = torch.randn(n, 1150, D, device=dev, requires_grad=True)
        lang, dout = torch.randn(n, 1, D, device=dev), torch.randn(n, 1, D, device=dev)
        counts = {m: _launches(lambda: _step(m, stacks[m], pixels, lang, dout)) for m in MODES[1:]}
        emit(f"N={n:4d} kernels per layer (4-layer stack fwd+bwd, loss and its backward included): "
             + ", ".join(f"{m} {c / 4:.1f}" for m, c in counts.items()))


if __name__ == "__main__":
    main()
