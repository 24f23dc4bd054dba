#!/usr/bin/env python3
"""Every csrc/kernels/wgrad.hip call of one eager hip-backend training step (shapes, prologue, call site captured by
wrapping the binding), re-timed in isolation with the configuration the step used and with every tile variant x
row-split count; prints the step's choice against the best few (median us, split partial sum included).  With
--bmm: the encoder's weight gradients that ops/linear.py plan_wgrad leaves to the library's split-K instead (random
operands at the step's shapes), against explicit plans with other split counts and the MFMA kernel's variants x splits.

  python tools/bench_wgrad_sites.py [--batch 128] [--top 4] [--bmm]
"""
from __future__ import annotations

import argparse
import os
import sys
import traceback

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.bench_dw_phases import timeit  # noqa: E402

PKG = "pytorch_rt1_for_distributed_training_amd"
SPLITS = (1, 2, 4, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256)


def _site() -> str:
    for fr in reversed(traceback.extract_stack()[:-2]):
        if PKG in fr.filename and "bench_wgrad_sites" not in fr.filename:
            return f"{fr.filename.split(PKG + '/')[-1]}:{fr.lineno}"
    return "?"


def Co_ci_bad(co: int, ci: int) -> bool:
    return co % 8 != 0 or ci % 8 != 0


def bmm_sites(a, mfma):
    """--bmm: every (M, Co, Ci) of the encoder's convs, the top and the TokenLearner at --batch x 6 frames whose plan
    is the library's; the planner's split against explicit ``Wgrad("bmm", splits=s)`` plans and the MFMA kernel."""
    from pytorch_rt1_for_distributed_training_amd.models.efficientnet import block_specs, conv_out_size
    from pytorch_rt1_for_distributed_training_amd.ops import linear
    N, H, W = a.batch * 6, 150, 150
    shapes = []
    for sp in block_specs():
        Ho, Wo = conv_out_size(H, sp.kernel, sp.stride), conv_out_size(W, sp.kernel, sp.stride)
        if sp.expand_ch != sp.in_ch:
            shapes.append((N * H * W, sp.expand_ch, sp.in_ch, f"blk{sp.index} expand"))
        shapes.append((N * Ho * Wo, sp.out_ch, sp.expand_ch, f"blk{sp.index} project"))
        H, W = Ho, Wo
    shapes += [(N * H * W, 1536, 384, "top"), (N * H * W, 512, 1536, "conv1x1"), (N * H * W, 64, 512, "token learner")]
    for M, Co, Ci, site in sorted(shapes, reverse=True):
        plan = linear.plan_wgrad(M, Co, Ci)
        if plan.kind not in ("bmm", "mm"):
            continue
        dy = torch.randn(M, Co, device="cuda").to(torch.bfloat16)
        x = torch.randn(M, Ci, device="cuda").to(torch.bfloat16)
        base = timeit(lambda: linear.wgrad(dy, x, plan=plan), a.iters)
        rows = [(timeit(lambda: linear.wgrad(dy, x, plan=linear.Wgrad("bmm", splits=s)), a.iters), "bmm", s)
                for s in SPLITS if 2 <= s and s * 256 <= M]
        if not Co_ci_bad(Co, Ci):
            for v in range(6):
                for s in SPLITS:
                    if s * 64 <= M:
                        try:
                            rows.append((timeit(lambda: mfma(dy, x, variant=v, splits=s), a.iters), v, s))
                        except RuntimeError:
                            pass
        rows.sort(key=lambda r: r[0])
        best = " ".join(f"v{v}/s{s}:{t:.1f}" for t, v, s in rows[:a.top])
        print(f"M={M:8d} Co={Co:5d} Ci={Ci:5d} step({plan.kind}/s{plan.splits}) {base:7.1f} | best {best} | {site}",
              flush=True)
        del dy, x
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--top", type=int, default=4)
    ap.add_argument("--bmm", action="store_true")
    a = ap.parse_args()
    from pytorch_rt1_for_distributed_training_amd.config import RT1Config
    from pytorch_rt1_for_distributed_training_amd.data.synthetic import make_batch
    from pytorch_rt1_for_distributed_training_amd.engine.step import TrainEngine, to_device
    from pytorch_rt1_for_distributed_training_amd.models import build_rt1
    from pytorch_rt1_for_distributed_training_amd.ops._ext import load

    ext = load()
    real = ext.wgrad
    calls = {}
    active = [False]

    def spy(dy, x, *args, **kw):
        if active[0]:
            key = (tuple(dy.shape), tuple(x.shape), len(args) > 0 and args[0] is not None, kw.get("variant", -1),
                   kw.get("splits", -1), _site())
            if key not in calls:
                calls[key] = (dy.clone(), x.clone(), args, dict(kw))
        return real(dy, x, *args, **kw)

    if a.bmm:
        return bmm_sites(a, real)
    ext.wgrad = spy
    dev = torch.device("cuda", 0)
    cfg = RT1Config(height=300, width=300, seq_len=6, backend="hip")
    eng = TrainEngine(build_rt1(cfg), cfg, order_probe=False, device=dev)
    eng.graph = False
    batch = to_device(make_batch(a.batch, cfg.seq_len, cfg.height, cfg.width), dev)
    eng.train_step(batch)
    active[0] = True
    eng.train_step(batch)
    active[0] = False
    ext.wgrad = real
    del eng
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    print(f"{len(calls)} distinct wgrad calls")
    for (ds, xs, pro, v0, s0, site), (dy, x, args, kw) in sorted(calls.items(), key=lambda kv: -kv[0][0][0]):
        M = dy.shape[0]
        rows = []
        base = timeit(lambda: real(dy, x, *args, **kw), a.iters)
        for v in range(6):
            for s in SPLITS:
                if s * 64 > M:
                    continue
                kw2 = dict(kw, variant=v, splits=s)
                if Co_ci_bad(ds[1], xs[1]):
                    continue
                try:
                    rows.append((timeit(lambda: real(dy, x, *args, **kw2), a.iters), v, s))
                except RuntimeError:
                    pass
        rows.sort(key=lambda r: r[0])
        best = " ".join(f"v{v}/s{s}:{t:.1f}" for t, v, s in rows[:a.top])
        print(f"M={M:8d} Co={ds[1]:5d} Ci={xs[1]:5d} pro={int(pro)} step(v{v0}/s{s0}) {base:7.1f} | best {best} | {site}",
              flush=True)
        del dy, x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
