#!/usr/bin/env python3
"""Time LAVA's pixel-language CrossLayer forward + backward, backend hip (csrc/kernels/lavaxattn.hip) against torch
(eager nn.LayerNorm + nn.MultiheadAttention, the path of the parent commit), in one process on one GPU.

Rows: one layer and the 4-layer stack at (N, S) = (16, 1150) -- the reference config's frames per device -- and
(256, 1150).  The two backends share weights and inputs and are timed alternately, round by round, with device events
around `iters` calls; the median, minimum and maximum over the rounds are printed.  The byte floor is what the folded
attention alone must move per layer: forward N*S*d*4 B read, backward twice that read plus one write.

    python tools/bench_lava_xattn.py [--out profiles/lava_xattn.log]
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
from pytorch_rt1_for_distributed_training_amd.ops.lava_attention import resolve_backend  # noqa: E402

D = 128


def _step(layers, pixels, lang, dout):
    pixels.grad = None
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


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default="", help="also append the rows to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_lava_xattn needs a GPU")
    resolve_backend("hip", D, 2)
    dev = torch.device("cuda", 0)
    lines = [f"# {torch.cuda.get_device_name(0)}; CrossLayer fwd+bwd, us per call, median [min, max] of {a.rounds} "
             f"rounds x {a.iters} calls, backends alternated"]
    for n, s in ((16, 1150), (256, 1150)):
        floor = n * s * D * 4
        lines.append(f"# N={n} S={s}: byte floor per layer: forward {floor / 1e6:.2f} MB read, backward "
                     f"{2 * floor / 1e6:.2f} MB read + {floor / 1e6:.2f} MB written")
        for depth in (1, 4):
            torch.manual_seed(0)
            ref = [CrossLayer(D, 2, D, 0.0).to(dev) for _ in range(depth)]
            stacks = {"torch": ref, "hip": copy.deepcopy(ref)}
            for layer in stacks["hip"]:
                layer.backend = "hip"
            pixels = torch.randn(n, s, D, device=dev, requires_grad=True)
            lang, dout = torch.randn(n, 1, D, device=dev), torch.randn(n, 1, D, device=dev)
            times = {k: [] for k in stacks}
            for k, layers in stacks.items():                             # warm-up: code objects, library algorithms
                for _ in range(5):
                    _step(layers, pixels, lang, dout)
            torch.cuda.synchronize()
            for _ in range(a.rounds):
                for k, layers in stacks.items():
                    times[k].append(_time(lambda: _step(layers, pixels, lang, dout), a.iters))
            med = {k: statistics.median(v) for k, v in times.items()}
            row = " ".join(f"{k} {med[k]:9.1f} [{min(v):9.1f}, {max(v):9.1f}]" for k, v in times.items())
            lines.append(f"N={n:4d} S={s} layers={depth}  {row}  torch/hip {med['torch'] / med['hip']:.2f}x  "
                         f"hip moves the floor at {depth * 4 * floor / med['hip'] / 1e3:.1f} GB/s")
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
