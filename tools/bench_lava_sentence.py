#!/usr/bin/env python3
"""Time LAVA's visual sentence (level projections, scale, positions, cat, dropout) forward + backward at 180x320
frames: the fused kernels (csrc/kernels/lavasent.hip) against the eager chain of SequenceLAVMSE.encode they replace,
(a) in fp32 and (b) under bf16 autocast, in one process on one GPU, at 16 and 256 frames.  All three start from the hip
encoder's NHWC bf16 stage outputs (eager pays its permute(0, 3, 1, 2).float() views and the level-4 pool, as the model
does), share the weights, and are timed alternately, round by round, with device events around `iters` calls after a
warm-up; the median, minimum and maximum over the rounds are printed.

Then each kernel call alone against its minimum bytes (each operand read once, each result written once; the 160 KB of
weights left out) and the HBM bandwidth (data sheet: 8 TB/s).  The weight gradient's fp32 partial workspace, written
and read back once, is NOT in the minimum and is printed next to its row.

    python tools/bench_lava_sentence.py [--out profiles/lava_sentence.log]
"""
from __future__ import annotations

import argparse
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_rt1_for_distributed_training_amd.models.lava import ConvMaxpoolEncoder, _dense, sincos_2d  # noqa: E402
from pytorch_rt1_for_distributed_training_amd.ops import lava_sentence as ls  # noqa: E402

H, W, D, P_DROP = 180, 320, 128, 0.1
PEAK_BYTES = 8.0e12


def _time(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters                        # us per call


def _eager(l2, l3, proj, pos, autocast):
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        f3 = l3.permute(0, 3, 1, 2).float()
        sent = []
        for i, f in zip(ls.FUSE_LAYERS, (l2.permute(0, 3, 1, 2).float(), f3, F.max_pool2d(f3, 2))):
            sent.append(proj[str(i)](f.flatten(2).transpose(1, 2)) * math.sqrt(D) + pos[len(sent)])
        return F.dropout(torch.cat(sent, dim=1), P_DROP, True)


def _step(kind, l2, l3, proj, pos, dpix):
    for t in (l2, l3, *proj.parameters()):
        t.grad = None
    if kind == "hip":
        out = ls.visual_sentence(l2, l3, proj, pos, P_DROP, True)
    else:
        out = _eager(l2, l3, proj, pos, kind == "autocast")
    out.backward(dpix)


def _rows(n, rounds, iters, dev):
    torch.manual_seed(0)
    with torch.no_grad():
        x = torch.rand(n, H, W, 3, device=dev)
        l2, l3 = ConvMaxpoolEncoder(backend="hip").to(dev).stages_nhwc(x)[2:4]
    l2, l3 = l2.requires_grad_(), l3.requires_grad_()
    proj = torch.nn.ModuleDict({str(i): _dense(c, D) for i, c in zip(ls.FUSE_LAYERS, ls.CHANNELS)}).to(dev)
    (h2, w2), (h3, w3) = l2.shape[1:3], l3.shape[1:3]
    tables = [sincos_2d(D, h, w).to(dev) for h, w in ((h2, w2), (h3, w3), (h3 // 2, w3 // 2))]
    pos = {"hip": torch.cat(tables).contiguous(), "eager": tables, "autocast": tables}
    dpix = torch.randn(n, pos["hip"].shape[0], D, device=dev)
    times = {k: [] for k in ("eager", "autocast", "hip")}
    for k in times:                                                      # warm-up: code objects, library algorithms
        for _ in range(3):
            _step(k, l2, l3, proj, pos[k], dpix)
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k in times:
            times[k].append(_time(lambda: _step(k, l2, l3, proj, pos[k], dpix), iters))
    med = {k: statistics.median(v) for k, v in times.items()}
    row = "  ".join(f"{k} {med[k] / 1e3:8.3f} ms [{min(v) / 1e3:8.3f}, {max(v) / 1e3:8.3f}]" for k, v in times.items())
    rows = [f"N={n:4d} sentence fwd+bwd S={dpix.shape[1]}  {row}  eager/hip {med['eager'] / med['hip']:.2f}x  "
            f"autocast/hip {med['autocast'] / med['hip']:.2f}x"]

    lin = [proj[str(i)] for i in ls.FUSE_LAYERS]
    wts, bs = [m.weight.detach() for m in lin], [m.bias.detach() for m in lin]
    a2, a3 = l2.detach(), l3.detach()
    lv, px = (a2.numel() + a3.numel()) * 2, dpix.numel() * 4             # bytes of the levels and of pixels / dpix
    parts = ls.wgrad_partials(n, h2, w2, h3, w3)
    ws = 2 * 4 * sum(p * (D * c + D) for p, c in zip(parts, ls.CHANNELS))
    calls = {"fwd": (lambda: ls.lava_sentence_fwd(a2, a3, wts[0], bs[0], wts[1], bs[1], wts[2], bs[2], pos["hip"],
                                                  P_DROP, 7), lv + px, ""),
             "dgrad": (lambda: ls.lava_sentence_bwd(dpix, a2, a3, *wts, P_DROP, 7, True, False), px + a3.numel() * 2 + lv,
                       ""),
             "wgrad": (lambda: ls.lava_sentence_bwd(dpix, a2, a3, *wts, P_DROP, 7, False, True), px + lv,
                       f"  + {ws / 1e6:6.2f} MB of partials written and read (P={parts}), not in the minimum")}
    for name, (fn, nbytes, note) in calls.items():
        fn()
        torch.cuda.synchronize()
        us = statistics.median(_time(fn, iters) for _ in range(rounds))
        least = nbytes / PEAK_BYTES * 1e6
        rows.append(f"N={n:4d} sentence {name:5s} {us:9.1f} us  {nbytes / 1e6:8.2f} MB  {nbytes / us / 1e6:6.3f} TB/s  "
                    f"least {least:6.1f} us: {100 * least / us:5.1f} % of HBM peak{note}")
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default="", help="also append the rows to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_lava_sentence needs a GPU")
    ls.resolve_backend("hip")
    dev = torch.device("cuda", 0)
    lines = [f"# {torch.cuda.get_device_name(0)}; visual sentence at {H}x{W}, dropout {P_DROP}, median [min, max] of "
             f"{a.rounds} rounds x {a.iters} calls, backends alternated; kernel rows: every call includes its KB-sized "
             f"weight packs, dgrad its two launches, wgrad its partial reduce"]
    for n in (16, 256):
        lines += _rows(n, a.rounds, a.iters, dev)
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
