#!/usr/bin/env python3
"""Device-side cost of the HBM-resident input path per batch: plan H2D + gather/crop/resize kernel + per-frame vector
gathers, at the bench config (b128, T=6, 360x640 frames -> 300x300), over a synthetic resident frame table.

  python tools/gpu/resident_decode.py [--frames 8000] [--batches 50] [--photometric]

``--photometric`` times the same plans three ways in one run, alternating: decode alone, decode with a ``photometric``
row per window (data/photometric.py), and the photometric kernel alone on a decoded batch, set against its byte floor
(two reads and one write of the image).
"""
from __future__ import annotations

import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8000)
    ap.add_argument("--batches", type=int, default=50)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--seq", type=int, default=6)
    ap.add_argument("--out", type=int, nargs=2, default=[300, 300])
    ap.add_argument("--photometric", action="store_true", help="also time the decode with the colour augmentation")
    ap.add_argument("--rounds", type=int, default=3, help="--photometric: alternating rounds of each variant")
    args = ap.parse_args()
    import numpy as np
    import torch
    from pytorch_rt1_for_distributed_training_amd.data import resident as R
    from pytorch_rt1_for_distributed_training_amd.data.shards import crop_boxes

    class _Table:       # a ResidentShard without a file: random frames already on the device
        pass
    dev = torch.device("cuda", 0)
    res = _Table()
    res.device = dev
    res.frames = torch.randint(0, 256, (args.frames, 360, 640, 3), dtype=torch.uint8, device=dev)
    res.instruction = torch.randn(args.frames, 512, device=dev)
    res.action = torch.randn(args.frames, 2, device=dev)
    res.is_terminal = torch.zeros(args.frames, dtype=torch.int64, device=dev)
    rng = np.random.default_rng(0)
    B, T = args.batch, args.seq
    plans = []
    for _ in range(args.batches):
        rows = torch.from_numpy(rng.integers(0, args.frames, (B, T))).pin_memory()
        boxes = torch.from_numpy(crop_boxes(rng, B * T, 360, 640, 0.95).reshape(B, T, 4)).pin_memory()
        plans.append({"plan_rows": rows, "crop_boxes": boxes})
    H, W = args.out
    for p in plans[:3]:
        R.decode_resident(res, {k: v.to(dev, non_blocking=True) for k, v in p.items()}, H, W)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for p in plans:
        out = R.decode_resident(res, {k: v.to(dev, non_blocking=True) for k, v in p.items()}, H, W)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / len(plans)
    host = 1e3 * (time.perf_counter() - t0) / len(plans)
    img = out["train_observation"]["image"]
    if args.photometric:
        _photometric(args, R, res, plans, img, dev, rng)
    src_mb = B * T * 360 * 640 * 3 / 1e6
    print(f"resident decode b{B} T={T} 360x640 -> {H}x{W}: {ms:.3f} ms/batch on the GPU ({host:.3f} ms host), "
          f"{src_mb:.0f} MB of source frames (~{src_mb / ms:.0f} GB/s effective), image {tuple(img.shape)}; "
          f"host-gather path for comparison: h2d 9.5-9.8 ms + crop 1.4 ms per batch "
          f"(profiles/r3_realdata_shard_train_300_b128.log)", flush=True)


def _photometric(args, R, res, plans, img, dev, rng):
    import torch
    from pytorch_rt1_for_distributed_training_amd.data.augment import PhotometricDistortions
    from pytorch_rt1_for_distributed_training_amd.data.photometric import photometric_params, photometric_u8_
    H, W = args.out
    B, T = args.batch, args.seq
    on = [dict(p, photometric=torch.from_numpy(photometric_params(rng, B, PhotometricDistortions())).pin_memory())
          for p in plans]
    prm = on[0]["photometric"].to(dev)

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(n):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    decode = lambda ps: lambda i: R.decode_resident(res, {k: v.to(dev, non_blocking=True) for k, v in ps[i].items()},
                                                    H, W)
    variants = {"decode, option off": decode(plans), "decode, option on": decode(on),
                "photometric kernel alone": lambda i: photometric_u8_(img, prm, T)}
    for fn in variants.values():
        timed(fn, 3)
    ms = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            ms[k].append(timed(fn, len(plans)))
    gb = 3 * img.numel() / 1e9
    for k, v in ms.items():
        print(f"photometric b{B} T={T} {H}x{W}: {k}: " + ", ".join(f"{x:.3f}" for x in v) + " ms/batch per round",
              flush=True)
    k_ms = min(ms["photometric kernel alone"])
    print(f"photometric kernel: {k_ms:.3f} ms for 2 reads + 1 write of {img.numel() / 1e6:.0f} MB = {gb:.2f} GB: "
          f"{gb / k_ms * 1e3:.0f} GB/s against the ~6300 GB/s HBM rate (floor {gb / 6.3:.3f} ms)", flush=True)


if __name__ == "__main__":
    main()
