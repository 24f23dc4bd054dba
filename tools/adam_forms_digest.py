#!/usr/bin/env python3
"""sha256 digests of what every form of the fused Adam (csrc/kernels/adam.hip) leaves behind, on the GPU.

  python tools/adam_forms_digest.py > digest.txt

For each of the nine forms -- host arguments, device state, and the device-state update under clip_state, with the
EMA of the weights, with parameter groups, and their combinations -- at each size and setting below, the script builds
p, g, m, v (and ema) on the CPU from a seeded generator, copies them to the device, runs three consecutive steps with
the device step advanced as FlatAdam.step does it (``state[0:1].add_(1.0)`` before the launch) and prints one sha256
per output buffer: p, m, v, ema, ema_state.  It calls only the ``ops.adam`` wrappers, so two builds of the kernels can
be compared line for line with ``diff``: a differing line names the form, the size, the setting and the buffer.

Sizes, the smallest that reach every code path of the kernel:

  ungrouped  4099                         one pass of the float4 loop, a 3-element scalar tail
  ungrouped  2 * 2048 * 256 * 4 + 1203    the grid-stride loop taken twice, then a partial pass, then the tail
  grouped    64 * 65                      one pass
  grouped    64 * (2 * 32768 + 5)         the grid-stride loop taken twice, then a partial pass

Settings: weight_decay 0 and 0.01 (ungrouped; the grouped runs hold G = 3 groups with distinct lrs, one wd = 0 and two
wd > 0, and one table entry >= G, which the kernel reads as G - 1), grad_scale 1 and 0.5, the EMA warm-up on and off,
and for the clip forms a verdict with coef = 1, one with coef < 1, and a skipped step (ok = 0, skipped counter 1)
between two applied ones.  The inputs hold v >= 0, a few exact zeros in g, m and v and a few denormal-scale gradients.
"""
from __future__ import annotations

import hashlib
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = 3
LR = 5e-4
BETAS = dict(beta1=0.9, beta2=0.999, eps=1e-8)
OMD = 1e-3                                                   # one minus the EMA decay
UNGROUPED_N = (4099, 2 * 2048 * 256 * 4 + 1203)
GROUPED_N = (64 * 65, 64 * (2 * 32768 + 5))
GROUP_LR_WD = ((1e-3, 0.0), (3e-4, 0.01), (2e-3, 0.05))
# clip_state {norm, coef, ok, skipped steps, 0...} of the three steps
VERDICTS = {"coef1": [(0.5, 1.0, 1.0, 0.0)] * 3,
            "coef<1": [(4.0, 0.25, 1.0, 0.0)] * 3,
            "skip": [(0.5, 1.0, 1.0, 0.0), (float("inf"), 1.0, 0.0, 1.0), (2.0, 0.5, 1.0, 1.0)]}


def inputs(n: int):
    """p, m, v, ema and one gradient per step on the CPU, a function of n alone."""
    import torch
    gen = torch.Generator().manual_seed(1234 + n)
    p = torch.randn(n, generator=gen)
    m = torch.randn(n, generator=gen) * 1e-3
    v = torch.rand(n, generator=gen) * 1e-6
    ema = p + torch.randn(n, generator=gen) * 1e-2
    grads = torch.randn(STEPS, n, generator=gen) * 1e-3
    idx = torch.randperm(n, generator=gen)[:24]
    grads[:, idx[0:4]] = 0.0
    grads[:, idx[4:8]] = 1e-40                               # denormal in fp32
    grads[:, idx[8:12]] = -3e-39
    m[idx[0:2]] = 0.0
    v[idx[0:2]] = 0.0                                        # g = m = v = 0: the denominator is eps alone
    v[idx[12:16]] = 0.0
    m[idx[16:20]] = 0.0
    table = torch.randint(0, len(GROUP_LR_WD), (max(n // 64, 1),), generator=gen, dtype=torch.uint8)
    table[len(table) // 2] = 7                               # >= G: read as G - 1
    return dict(p=p, m=m, v=v, ema=ema, grads=grads, table=table)


def sha(t) -> str:
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def run(ops, base, *, host=False, clip=None, ema=False, groups=False, wd=0.0, gs=1.0, warmup=True):
    import torch
    dev = lambda t: t.clone().to("cuda")
    p, m, v = dev(base["p"]), dev(base["m"]), dev(base["v"])
    grads = [dev(g) for g in base["grads"]]     # an allocation each: every gradient is 16-byte aligned
    e = dev(base["ema"]) if ema else None
    es = torch.zeros(4, device="cuda") if ema else None
    cs = torch.zeros(8, device="cuda") if clip else None
    state = torch.tensor([0.0, LR], device="cuda")
    gstate = table = None
    if groups:
        gstate = torch.tensor([[lr, w, 0.0, 0.0] for lr, w in GROUP_LR_WD], device="cuda")
        table = base["table"].to("cuda")
    for k in range(STEPS):
        g = grads[k]
        state[0:1].add_(1.0)
        if clip:
            cs[:4].copy_(torch.tensor(VERDICTS[clip][k]))
        if host:
            ops.flat_adam_step(p, g, m, v, lr=LR, weight_decay=wd, step=k + 1, grad_scale=gs, **BETAS)
        elif groups:
            ops.flat_adam_groups_dev_step(p, g, m, v, state, gstate, table, ema=e, ema_state=es, clip_state=cs,
                                          grad_scale=gs, one_minus_decay=OMD, warmup=warmup, **BETAS)
        elif ema:
            ops.flat_adam_ema_dev_step(p, g, m, v, e, state, es, cs, weight_decay=wd, grad_scale=gs,
                                       one_minus_decay=OMD, warmup=warmup, **BETAS)
        elif clip:
            ops.flat_adam_clip_dev_step(p, g, m, v, state, cs, weight_decay=wd, grad_scale=gs, **BETAS)
        else:
            ops.flat_adam_dev_step(p, g, m, v, state, weight_decay=wd, grad_scale=gs, **BETAS)
    torch.cuda.synchronize()
    out = dict(p=p, m=m, v=v)
    if ema:
        out.update(ema=e, ema_state=es)
    return out


def main():
    import torch
    from pytorch_rt1_for_distributed_training_amd.ops import adam as ops
    assert torch.cuda.is_available(), "needs a GPU"
    forms = [("host", dict(host=True)), ("dev", {}), ("dev+clip", dict(clip=True)), ("dev+ema", dict(ema=True)),
             ("dev+clip+ema", dict(clip=True, ema=True)), ("groups", dict(groups=True)),
             ("groups+clip", dict(groups=True, clip=True)), ("groups+ema", dict(groups=True, ema=True)),
             ("groups+clip+ema", dict(groups=True, clip=True, ema=True))]
    cache = {}
    lines = 0
    for name, f in forms:
        grouped = f.get("groups", False)
        for n in (GROUPED_N if grouped else UNGROUPED_N):
            if n not in cache:
                cache[n] = inputs(n)
            wds = (None,) if grouped else (0.0, 0.01)
            warmups = (True, False) if f.get("ema") else (None,)
            verdicts = tuple(VERDICTS) if f.get("clip") else (None,)
            for wd, gs, warmup, verdict in itertools.product(wds, (1.0, 0.5), warmups, verdicts):
                kw = dict(host=f.get("host", False), ema=f.get("ema", False), groups=grouped, gs=gs, clip=verdict)
                tag = f"form={name} n={n} gs={gs}"
                if wd is not None:
                    kw["wd"] = wd
                    tag += f" wd={wd}"
                if warmup is not None:
                    kw["warmup"] = warmup
                    tag += f" warmup={int(warmup)}"
                if verdict is not None:
                    tag += f" verdict={verdict}"
                for buf, t in run(ops, cache[n], **kw).items():
                    print(f"{tag} buf={buf} sha256={sha(t)}", flush=True)
                    lines += 1
    print(f"# {lines} digests, {len(forms)} forms, {STEPS} steps each, {torch.cuda.get_device_name(0)}", flush=True)


if __name__ == "__main__":
    main()
