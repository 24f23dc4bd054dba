#!/usr/bin/env python3
"""Cost of the per-element group lookup in the fused Adam (csrc/kernels/adam.hip, the GROUPS forms) on the GPU.

  python tools/bench_adam_groups.py kernels   # at the full model's flat size, in one process: the ungrouped kernel and
                                              # the grouped one over the real model's four-group layout, in the plain
                                              # form (28 B/elem) and in the clip + EMA form (36 B/elem)

The chunk table is the real one: build_rt1(preset("full")) on the host, the engine's flat order without the probe
(reversed parameters), build_param_groups(no_decay_norm_bias, backbone_lr_mult = 0.1).  Each variant is timed as 200
back-to-back launches between two device events after a warm-up; the variants alternate over 5 passes, so each pass
times the grouped kernel right after the ungrouped one of the same form.  Both move the same 28 or 36 B per element;
the table adds 1/256 B per element and the group constants stay in cache, so the expectation is parity: the grouped /
ungrouped ratio of the medians is judged against the run-to-run spread of the UNGROUPED kernel's own five repeats
((max - min) / median), which the tool prints next to it.  The buffers are 141 MB each, so no launch finds its
operands in the 256 MB last-level cache.  The baselines are the kernels every run without groups launches, unchanged.
"""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def real_layout(lr=5e-4, weight_decay=0.05, mult=0.1):
    """(chunk table uint8 on the host, [(name, lr, wd, chunks)]) of the full model's four groups in the flat order."""
    import torch
    from pytorch_rt1_for_distributed_training_amd.config import preset
    from pytorch_rt1_for_distributed_training_amd.engine.optim import FlatAdam, build_param_groups
    from pytorch_rt1_for_distributed_training_amd.models import build_rt1
    from pytorch_rt1_for_distributed_training_amd.parallel.flat import FlatParameters
    torch.manual_seed(0)
    model = build_rt1(preset("full"))
    flat = FlatParameters(list(reversed([p for p in model.parameters() if p.requires_grad])), device="cpu")
    opt = FlatAdam(flat, lr=lr, weight_decay=weight_decay, all_params=list(model.parameters()), use_kernel=False,
                   groups=build_param_groups(model, lr, weight_decay, True, mult))
    table = opt.chunk_group.clone()
    counts = torch.bincount(table.long(), minlength=len(opt.param_groups)).tolist()
    return table, [(g["name"], g["lr"], g["weight_decay"], c) for g, c in zip(opt.param_groups, counts)]


def kernels(a):
    import torch
    from pytorch_rt1_for_distributed_training_amd.ops import adam as ops
    assert torch.cuda.is_available(), "needs a GPU"
    table, groups = real_layout()
    n = table.numel() * 64
    changes = int((table[1:] != table[:-1]).sum())
    print(f"n = {n} floats ({4 * n / 1e6:.1f} MB per buffer), table {table.numel()} B, {changes} group changes along "
          f"the buffer, {a.reps} launches per timing, {a.passes} passes, {torch.cuda.get_device_name(0)}", flush=True)
    for name, lr, wd, c in groups:
        print(f"  group {name:18s} lr {lr:.3g} wd {wd:g}: {c} chunks ({100.0 * c / table.numel():.2f} %)", flush=True)
    g = torch.Generator(device="cuda").manual_seed(0)
    p = torch.randn(n, device="cuda", generator=g)
    grad = torch.randn(n, device="cuda", generator=g) * 1e-3
    m, v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    ema = p.clone()
    state = torch.tensor([1.0, 5e-4], device="cuda")
    gstate = torch.tensor([[lr, wd, 0.0, 0.0] for _, lr, wd, _ in groups], device="cuda")
    tab = table.cuda()
    es = torch.zeros(4, device="cuda")
    cs = torch.zeros(8, device="cuda")
    pt = torch.zeros(ops.gradnorm_partials(n), dtype=torch.float64, device="cuda")
    ops.grad_norm_clip_(grad, cs, pt, max_norm=1.0, grad_scale=1.0, skip_nonfinite=True)      # a verdict to obey
    kw = dict(beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0)
    omd = 1.0 - 0.9999
    rows = [("flat_adam_dev (ungrouped, unchanged)",
             lambda: ops.flat_adam_dev_step(p, grad, m, v, state, weight_decay=0.05, **kw), 28 * n),
            ("flat_adam_groups_dev, plain form",
             lambda: ops.flat_adam_groups_dev_step(p, grad, m, v, state, gstate, tab, **kw), 28 * n + n // 64),
            ("flat_adam_ema_dev, clip form (ungrouped, unchanged)",
             lambda: ops.flat_adam_ema_dev_step(p, grad, m, v, ema, state, es, cs, weight_decay=0.05,
                                                one_minus_decay=omd, warmup=True, **kw), 36 * n),
            ("flat_adam_groups_dev, clip + EMA form",
             lambda: ops.flat_adam_groups_dev_step(p, grad, m, v, state, gstate, tab, ema=ema, ema_state=es,
                                                   clip_state=cs, one_minus_decay=omd, warmup=True, **kw),
             36 * n + n // 64)]
    times = {name: [] for name, _, _ in rows}
    for rep in range(a.passes):
        for name, fn, nbytes in rows:
            us = _time_us(fn, a.reps)
            times[name].append(us)
            print(f"pass {rep + 1}  {name:52s} {us:9.2f} us  {nbytes / us / 1e3:9.1f} GB/s over {nbytes / 1e6:9.3f} MB",
                  flush=True)
    med = lambda x: sorted(x)[len(x) // 2]
    for base, new, what in ((rows[0][0], rows[1][0], "plain"), (rows[2][0], rows[3][0], "clip + EMA")):
        b, g_ = times[base], times[new]
        spread = (max(b) - min(b)) / med(b)
        ratio = med(g_) / med(b)
        verdict = ("within" if abs(ratio - 1.0) <= spread else
                   "FASTER than the ungrouped kernel by more than" if ratio < 1.0 else
                   "SLOWER than the ungrouped kernel by more than")
        print(f"{what}: ungrouped median {med(b):.2f} us (min {min(b):.2f}, max {max(b):.2f}, spread "
              f"{100 * spread:.2f} %), grouped median {med(g_):.2f} us (min {min(g_):.2f}, max {max(g_):.2f}); "
              f"grouped / ungrouped = {ratio:.4f}, {verdict} the ungrouped kernel's own spread", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["kernels"])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--passes", type=int, default=5)
    a = ap.parse_args()
    {"kernels": kernels}[a.mode](a)


if __name__ == "__main__":
    main()
