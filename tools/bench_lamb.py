#!/usr/bin/env python3
"""Cost of the LAMB step (csrc/kernels/lamb.hip: lamb_moments, lamb_trust, lamb_apply) against the one fused Adam launch
it replaces (csrc/kernels/adam.hip), on the GPU.

  python tools/bench_lamb.py kernels   # at the full model's flat size, in one process

The layout is the real one: build_rt1(preset("full")) on the host, the engine's flat order without the probe (reversed
parameters), build_param_groups(no_decay_norm_bias, backbone_lr_mult = 0.1): four groups, of which the two no-decay
ones are not adapted, and one table entry per tensor.  Both optimizers run their grouped form, plain (Adam 28 B/elem,
LAMB 24 + 16 = 40) and with clip + EMA (36 against 24 + 24 = 48).  Each row is timed as 200 back-to-back launches
between two device events after a warm-up; the rows alternate over the passes, and the whole set is run twice.  The rows
are the Adam launch, the three LAMB launches together and each LAMB kernel alone (the extension's lamb_kernel_alone, an
entry point for this tool only) with its achieved bandwidth over the bytes it must move.

The yardstick is the Adam launch of the same form scaled by the byte ratio (40/28, 48/36); the tool prints the measured
ratio next to it, and the Adam launch's own run-to-run spread.  The buffers are 141 MB each, so no launch finds its
operands in the 256 MB last-level cache.
"""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_adam_groups import _time_us  # noqa: E402


def real_layout(lr=5e-4, weight_decay=0.05, mult=0.1):
    """(chunk_group uint8, tensor_chunk_start list, tensor_adapt list, [(name, lr, wd)]) of the full model."""
    import torch
    from pytorch_rt1_for_distributed_training_amd.config import preset
    from pytorch_rt1_for_distributed_training_amd.engine.optim import FlatAdam, build_param_groups
    from pytorch_rt1_for_distributed_training_amd.models import build_rt1
    from pytorch_rt1_for_distributed_training_amd.parallel.flat import FlatParameters
    torch.manual_seed(0)
    model = build_rt1(preset("full"))
    flat = FlatParameters(list(reversed([p for p in model.parameters() if p.requires_grad])), device="cpu")
    opt = FlatAdam(flat, lr=lr, weight_decay=weight_decay, all_params=list(model.parameters()), use_kernel=False,
                   groups=build_param_groups(model, lr, weight_decay, True, mult), layer_adapt=True)
    return (opt.chunk_group.clone(), opt.tensor_chunk_start.tolist(), opt.tensor_adapt.tolist(),
            [(g["name"], g["lr"], g["weight_decay"]) for g in opt.param_groups])


def kernels(a):
    import torch
    from pytorch_rt1_for_distributed_training_amd.ops import adam as ops
    assert torch.cuda.is_available(), "needs a GPU"
    table, starts, adapt, groups = real_layout()
    n, nT = table.numel() * 64, len(adapt)
    sizes = [b - c for c, b in zip(starts[:-1], starts[1:])]
    print(f"n = {n} floats ({4 * n / 1e6:.1f} MB per buffer), {nT} tensors ({sum(adapt)} adapted), largest "
          f"{max(sizes)} chunks, {a.reps} launches per timing, {a.passes} passes x {a.runs} runs, "
          f"{torch.cuda.get_device_name(0)}", flush=True)
    g = torch.Generator(device="cuda").manual_seed(0)
    p = torch.randn(n, device="cuda", generator=g)
    grad = torch.randn(n, device="cuda", generator=g) * 1e-3
    m, v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    ema = p.clone()
    state = torch.tensor([1.0, 5e-4], device="cuda")
    gstate = torch.tensor([[lr * 1e-2, wd, 0.0, 0.0] for _, lr, wd in groups], device="cuda")   # small steps: p stays sane
    tab = table.cuda()
    tcs, ta, ct = ops.lamb_tables(starts, adapt, n, "cuda")
    work = dict(chunk_sums=torch.zeros(n // 64, 2, device="cuda"), trust=torch.ones(nT, device="cuda"),
                norms=torch.zeros(nT, 2, device="cuda"))
    es = torch.zeros(4, device="cuda")
    cs = torch.zeros(8, device="cuda")
    pt = torch.zeros(ops.gradnorm_partials(n), dtype=torch.float64, device="cuda")
    ops.grad_norm_clip_(grad, cs, pt, max_norm=1.0, grad_scale=1.0, skip_nonfinite=True)      # a verdict to obey
    kw = dict(beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0)
    omd = 1.0 - 0.9999
    full = dict(ema=ema, ema_state=es, clip_state=cs, one_minus_decay=omd, warmup=True)

    def lamb(**form):
        return lambda: ops.flat_lamb_dev_step(p, grad, m, v, state, tensor_chunk_start=tcs, tensor_adapt=ta,
                                              chunk_tensor=ct, group_state=gstate, chunk_group=tab, **work, **form,
                                              **kw)

    def alone(kernel, ema=None, ema_state=None, clip_state=None, one_minus_decay=1.0, warmup=True):
        ext = ops.load()
        return lambda: ext.lamb_kernel_alone(kernel, p, grad, m, v, state, ema, ema_state, clip_state, gstate, tab,
                                             tcs, ta, ct, work["chunk_sums"], work["trust"], work["norms"], 0.9,
                                             0.999, 1e-8, 0.0, 1.0, float(one_minus_decay), bool(warmup))

    def adam(**form):
        return lambda: ops.flat_adam_groups_dev_step(p, grad, m, v, state, gstate, tab, **form, **kw)

    c = n // 64
    forms = []
    for what, form, adam_b, s1, s3 in (("plain", {}, 28, 24, 16), ("clip + EMA", full, 36, 24, 24)):
        forms.append((what, adam_b, s1 + s3, [
            (f"adam, {what}", adam(**form), adam_b * n + c),
            (f"lamb, {what}: three launches", lamb(**form), (s1 + s3) * n + 16 * c + 3 * c),
            (f"lamb_moments, {what}", alone(1, **form), s1 * n + 8 * c + c),
            (f"lamb_trust, {what}", alone(2, **form), 8 * c),
            (f"lamb_apply, {what}", alone(3, **form), s3 * n + 3 * c)]))
    med = lambda x: sorted(x)[len(x) // 2]
    for run in range(a.runs):
        for what, adam_b, lamb_b, rows in forms:
            times = {name: [] for name, _, _ in rows}
            for rep in range(a.passes):
                for name, fn, nbytes in rows:
                    us = _time_us(fn, a.reps)
                    times[name].append(us)
                    print(f"run {run + 1} pass {rep + 1}  {name:44s} {us:9.2f} us  {nbytes / us / 1e6:7.3f} TB/s over "
                          f"{nbytes / 1e6:9.3f} MB", flush=True)
            b, l = times[rows[0][0]], times[rows[1][0]]
            parts = sum(med(times[rows[i][0]]) for i in (2, 3, 4))
            ratio, bytes_ratio = med(l) / med(b), lamb_b / adam_b
            print(f"run {run + 1} {what}: adam median {med(b):.2f} us (spread {100 * (max(b) - min(b)) / med(b):.2f} %), "
                  f"lamb median {med(l):.2f} us (its kernels alone: {parts:.2f} us); lamb / adam = {ratio:.4f}, byte "
                  f"ratio {lamb_b}/{adam_b} = {bytes_ratio:.4f}, measured / byte ratio = {ratio / bytes_ratio:.4f}",
                  flush=True)
    print(f"finite weights after the run: {bool(torch.isfinite(p).all())}", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["kernels"])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--runs", type=int, default=2)
    a = ap.parse_args()
    {"kernels": kernels}[a.mode](a)


if __name__ == "__main__":
    main()
