#!/usr/bin/env python3
"""Time PixelLangMSE's ConvMaxpoolLanguageEncoder forward + backward at 180x320, sequence 4 (12 stacked channels),
encoder backend hip (csrc/kernels/lavaconv.hip, lavapix.hip) against (a) eager fp32 and (b) eager under bf16 autocast
with channels-last, in one process on one GPU, at 16 and 128 windows.  The three share weights, the fp32 NHWC stacked
frames and the language embedding and are timed alternately, round by round, with device events around `iters` calls
after a warm-up; the median, minimum and maximum over the rounds are printed.  Every path starts from the NHWC frames
the model receives, so eager pays its NCHW permute; the gate projections (nn.Linear) are inside every path.

Then each kernel alone against its byte floor -- each operand read once, each result written once, over the HBM
bandwidth (data sheet: 8 TB/s) -- next to its FLOPs over the bf16 MFMA peak (2.5 PFLOP/s dense); the larger of the two
is the hardware's least time.  The weight gradient's fp32 partials are not in the floor (see bench_lava_encoder.py).

    python tools/bench_lava_pixel.py [--out profiles/lava_pixel.log]
"""
from __future__ import annotations

import argparse
import copy
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_rt1_for_distributed_training_amd.models.lava import ConvMaxpoolLanguageEncoder  # noqa: E402
from pytorch_rt1_for_distributed_training_amd.ops import lava_conv, lava_pixel  # noqa: E402

H, W, CIN = 180, 320, 12
PEAK_FLOPS, PEAK_BYTES = 2.5e15, 8.0e12


def _time(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters                        # us per call


def _step(enc, kind, frames, lang, dout):
    for p in enc.parameters():
        p.grad = None
    if kind == "hip":
        out = enc(frames, lang)
    elif kind == "eager":
        out = enc(frames.permute(0, 3, 1, 2).contiguous(), lang)
    else:                                                                # the NHWC frames are a channels-last NCHW view
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = enc(frames.permute(0, 3, 1, 2), lang)
    (out.float() * dout).sum().backward()


def _encoder_rows(n, rounds, iters, dev):
    torch.manual_seed(0)
    base = ConvMaxpoolLanguageEncoder(CIN).to(dev)
    encs = {"eager": base, "autocast": copy.deepcopy(base).to(memory_format=torch.channels_last),
            "hip": ConvMaxpoolLanguageEncoder(CIN, backend="hip").to(dev)}
    encs["hip"].load_state_dict(base.state_dict())
    frames, lang = torch.rand(n, H, W, CIN, device=dev), torch.randn(n, 512, device=dev)
    dout = torch.randn(n, 256, device=dev)
    times = {k: [] for k in encs}
    for k, e in encs.items():                                            # warm-up: code objects, library algorithms
        for _ in range(3):
            _step(e, k, frames, lang, dout)
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, e in encs.items():
            times[k].append(_time(lambda: _step(e, k, frames, lang, dout), iters))
    med = {k: statistics.median(v) for k, v in times.items()}
    row = "  ".join(f"{k} {med[k] / 1e3:8.3f} ms [{min(v) / 1e3:8.3f}, {max(v) / 1e3:8.3f}]" for k, v in times.items())
    return (f"N={n:4d} pixel encoder fwd+bwd  {row}  eager/hip {med['eager'] / med['hip']:.2f}x  "
            f"autocast/hip {med['autocast'] / med['hip']:.2f}x")


def _kernel_rows(n, rounds, iters, dev):
    rows, h, w = [], H, W

    def add(name, fn, flops, nbytes):
        fn()
        torch.cuda.synchronize()
        us = statistics.median(_time(fn, iters) for _ in range(rounds))
        t_f, t_b = flops / PEAK_FLOPS * 1e6, nbytes / PEAK_BYTES * 1e6
        rows.append(f"N={n:4d} {name:28s} {us:9.1f} us  {flops / 1e9:8.2f} GFLOP {nbytes / 1e6:8.2f} MB  "
                    f"{nbytes / us / 1e6:6.3f} TB/s  byte floor {t_b:7.1f} us = {100 * t_b / us:5.1f} % of the time; "
                    f"least {max(t_f, t_b):7.1f} us ({'MFMA' if t_f > t_b else 'HBM'}-bound): "
                    f"{100 * max(t_f, t_b) / us:5.1f} % of peak")

    x = torch.rand(n, h, w, CIN, device=dev)
    for cin, cout in ((CIN, 32),) + lava_conv.STAGES[1:]:
        wt = torch.randn(cout, cin, 3, 3, device=dev) * (2.0 / (9 * cin)) ** 0.5
        b, g = torch.zeros(cout, device=dev), torch.randn(n, cout, device=dev)
        flops = 2.0 * n * h * w * 9 * cin * cout
        tag = f"({cin:3d},{cout:3d}) {h:3d}x{w:3d}"
        if cin < 32:
            y, idx = lava_conv.lava_conv_fwd(x, wt, b)
            dy = torch.randn_like(y)
            xb, yb = x.numel() * x.element_size(), y.numel() * 3         # y bf16 + idx uint8
            add(f"first {tag} fwd", lambda: lava_conv.lava_conv_fwd(x, wt, b), flops, xb + yb)
            add(f"first {tag} wgrad", lambda: lava_conv.lava_conv_wgrad(x, dy, idx), flops, xb + yb)
        else:
            y, idx = lava_conv.lava_conv_gated_fwd(x, wt, b, g)
            dy = torch.randn_like(y)
            xb, yb = x.numel() * x.element_size(), y.numel() * 3
            add(f"gated {tag} fwd", lambda: lava_conv.lava_conv_gated_fwd(x, wt, b, g), flops, xb + yb)
            add(f"gated {tag} dgrad", lambda: lava_conv.lava_conv_gated_dgrad(dy, idx, wt, g, (h, w)), flops, xb + yb)
            add(f"gated {tag} wgrad", lambda: lava_conv.lava_conv_gated_wgrad(x, dy, idx, g), flops, xb + yb)
            add(f"gated {tag} dgate", lambda: lava_conv.lava_conv_dgate(dy, y, g, cin, (h, w)), 2.0 * y.numel(),
                y.numel() * 4)
        x, h, w = y, h // 2, w // 2
    g, lw, lb = torch.randn(n, 256, device=dev), torch.ones(256, device=dev), torch.zeros(256, device=dev)
    out, mean, stat = lava_pixel.lava_pixel_tail_fwd(x, g, lw, lb, 1e-6)
    dout = torch.randn_like(out)
    add(f"tail {h:3d}x{w:3d} fwd", lambda: lava_pixel.lava_pixel_tail_fwd(x, g, lw, lb, 1e-6), 2.0 * x.numel(),
        x.numel() * 2)
    add(f"tail {h:3d}x{w:3d} bwd", lambda: lava_pixel.lava_pixel_tail_bwd(dout, mean, stat, g, lw, h, w),
        2.0 * x.numel(), x.numel() * 2)
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default="", help="also append the rows to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_lava_pixel needs a GPU")
    lava_pixel.resolve_backend("hip", CIN)
    dev = torch.device("cuda", 0)
    lines = [f"# {torch.cuda.get_device_name(0)}; ConvMaxpoolLanguageEncoder at {H}x{W}, {CIN} stacked channels, median "
             f"[min, max] of {a.rounds} rounds x {a.iters} calls, backends alternated; kernel rows: wgrad includes its "
             f"partial reduce and every conv call its KB-sized weight pack"]
    for n in (16, 128):
        lines.append(_encoder_rows(n, a.rounds, a.iters, dev))
    for n in (16, 128):
        lines += _kernel_rows(n, a.rounds, a.iters, dev)
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
