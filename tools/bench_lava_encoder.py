#!/usr/bin/env python3
"""Time LAVA's ConvMaxpoolEncoder forward + backward at 180x320 frames, encoder backend hip
(csrc/kernels/lavaconv.hip) against (a) eager fp32 and (b) eager under bf16 autocast with channels-last, in one process
on one GPU, at 16 and 256 frames.  The three share weights and fp32 NHWC frames and are timed alternately, round by
round, with device events around `iters` calls after a warm-up; the median, minimum and maximum over the rounds are
printed.  Every path starts from the NHWC frames the model receives, so eager pays its NCHW permute.

Then each stage's three kernels alone (forward, data gradient, weight gradient), with the FLOPs (2 * pixels * 9 * Cin *
Cout) and the minimum bytes (each operand read once, each result written once) computed from the shapes, and the share
of the hardware's least time -- the larger of FLOPs over the bf16 MFMA peak and bytes over the HBM bandwidth (data
sheet: 2.5 PFLOP/s dense, 8 TB/s) -- saying which of the two bounds the kernel.  The weight gradient also writes and
reads back its fp32 workgroup partials (P x (9 Cin Cout + Cout) floats, P capped by the CU count, not by the bytes);
that workspace is NOT in the minimum bytes and is printed next to the row: at few frames it is several times the
stage's minimum traffic and is part of why the weight gradient sits further from the peak there.

    python tools/bench_lava_encoder.py [--out profiles/lava_encoder.log]
"""
from __future__ import annotations

import argparse
import copy
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_rt1_for_distributed_training_amd.models.lava import ConvMaxpoolEncoder  # noqa: E402
from pytorch_rt1_for_distributed_training_amd.ops import lava_conv  # noqa: E402

H, W = 180, 320
PEAK_FLOPS, PEAK_BYTES = 2.5e15, 8.0e12
FUSED = (2, 3, 4)                                                        # pyramid levels the model reads


def _time(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters                        # us per call


def _step(enc, kind, frames, douts):
    for p in enc.parameters():
        p.grad = None
    if kind == "hip":
        levels = enc(frames)
    elif kind == "eager":
        levels = enc(frames.permute(0, 3, 1, 2).contiguous())
    else:                                                                # the NHWC frames are a channels-last NCHW view
        with torch.autocast("cuda", dtype=torch.bfloat16):
            levels = enc(frames.permute(0, 3, 1, 2))
    sum((levels[i].float() * douts[i]).sum() for i in FUSED).backward()


def _encoder_rows(n, rounds, iters, dev):
    torch.manual_seed(0)
    base = ConvMaxpoolEncoder().to(dev)
    encs = {"eager": base, "autocast": copy.deepcopy(base).to(memory_format=torch.channels_last),
            "hip": ConvMaxpoolEncoder(backend="hip").to(dev)}
    encs["hip"].load_state_dict(base.state_dict())
    frames = torch.rand(n, H, W, 3, device=dev)
    with torch.no_grad():
        douts = {i: torch.randn_like(l) for i, l in enumerate(base(frames.permute(0, 3, 1, 2).contiguous()))}
    times = {k: [] for k in encs}
    for k, e in encs.items():                                            # warm-up: code objects, library algorithms
        for _ in range(3):
            _step(e, k, frames, douts)
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, e in encs.items():
            times[k].append(_time(lambda: _step(e, k, frames, douts), iters))
    med = {k: statistics.median(v) for k, v in times.items()}
    row = "  ".join(f"{k} {med[k] / 1e3:8.3f} ms [{min(v) / 1e3:8.3f}, {max(v) / 1e3:8.3f}]" for k, v in times.items())
    return (f"N={n:4d} encoder fwd+bwd  {row}  eager/hip {med['eager'] / med['hip']:.2f}x  "
            f"autocast/hip {med['autocast'] / med['hip']:.2f}x")


def _kernel_rows(n, rounds, iters, dev):
    rows, h, w = [], H, W
    x = torch.rand(n, h, w, 3, device=dev)
    for cin, cout in lava_conv.STAGES:
        wt = torch.randn(cout, cin, 3, 3, device=dev) * (2.0 / (9 * cin)) ** 0.5
        b = torch.zeros(cout, device=dev)
        y, idx = lava_conv.lava_conv_fwd(x, wt, b)
        dy = torch.randn_like(y)
        flops = 2.0 * n * h * w * 9 * cin * cout
        xb, yb = x.numel() * x.element_size(), y.numel() * 3             # y bf16 + idx uint8
        calls = {"fwd": (lambda: lava_conv.lava_conv_fwd(x, wt, b), xb + yb),
                 "wgrad": (lambda: lava_conv.lava_conv_wgrad(x, dy, idx), xb + yb)}
        if cin != 3:
            calls["dgrad"] = (lambda: lava_conv.lava_conv_dgrad(dy, idx, wt, (h, w)), xb + yb)
        for name, (fn, nbytes) in calls.items():
            fn()
            torch.cuda.synchronize()
            us = statistics.median(_time(fn, iters) for _ in range(rounds))
            t_f, t_b = flops / PEAK_FLOPS * 1e6, nbytes / PEAK_BYTES * 1e6
            ws = ""
            if name == "wgrad":
                parts = lava_conv.wgrad_partials(n, h, w, cin, cout)
                ws = (f"  + {2 * parts * (9 * cin * cout + cout) * 4 / 1e6:7.2f} MB of partials written and read "
                      f"(P={parts}), not in the minimum")
            rows.append(f"N={n:4d} stage ({cin:3d},{cout:3d}) {h:3d}x{w:3d} {name:5s} {us:9.1f} us  "
                        f"{flops / 1e9:8.2f} GFLOP {nbytes / 1e6:8.2f} MB  {flops / us / 1e6:7.1f} TFLOP/s "
                        f"{nbytes / us / 1e6:6.3f} TB/s  least {max(t_f, t_b):7.1f} us "
                        f"({'MFMA' if t_f > t_b else 'HBM'}-bound): {100 * max(t_f, t_b) / us:5.1f} % of peak{ws}")
        x, h, w = y, h // 2, w // 2
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default="", help="also append the rows to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_lava_encoder needs a GPU")
    lava_conv.resolve_backend("hip")
    dev = torch.device("cuda", 0)
    lines = [f"# {torch.cuda.get_device_name(0)}; ConvMaxpoolEncoder at {H}x{W}, median [min, max] of {a.rounds} "
             f"rounds x {a.iters} calls, backends alternated; kernel rows: wgrad includes its partial reduce and "
             f"every kernel call its KB-sized weight pack"]
    for n in (16, 256):
        lines.append(_encoder_rows(n, a.rounds, a.iters, dev))
    for n in (16, 256):
        lines += _kernel_rows(n, a.rounds, a.iters, dev)
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
