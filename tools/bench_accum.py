#!/usr/bin/env python3
"""Cost of gradient accumulation (TrainEngine(accumulate_grad_batches=k)) on the GPU, at the bench configuration
(full model, 300x300, T6, b128, bf16, graph).

  python tools/bench_accum.py kernels        # (a) multi_add_ / multi_reduce_add_ next to multi_copy_ /
                                             #     multi_reduce_copy_ on the step's real gather lists
  python tools/bench_accum.py step_all       # (b) ms per micro-step and per window for k = 1, 2, 4, one child each
  python tools/bench_accum.py step --k 4     # one such run

(a) runs one eager forward + backward under ``deferred_sums``, forms the two lists ``FlatParameters.gather_grads``
would form (stolen gradients; deferred split-K partial sets) and times 100 back-to-back repetitions of each kernel on
them between two device events after a warm-up.  Bytes: the copy moves 2n (read source, write destination), the add 3n
(the destination is read as well), so bytes alone predict 1.5x; the reduce forms read splits x n and write n, plus n
for the accumulating form.  The destinations are the flat gradient's views and stay finite throughout (a copy, or
120 repeated adds of one fixed source).
(b) k = 1 is the one-graph step bench.py measures; for k > 1 a window is k replays of the micro-step graph between the
eager memset and the eager optimizer launches.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time_us(fn, reps=100, warm=20):
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


def _engine(a, k):
    import torch
    from pytorch_rt1_for_distributed_training_amd.config import RT1Config
    from pytorch_rt1_for_distributed_training_amd.engine.step import TrainEngine
    from pytorch_rt1_for_distributed_training_amd.models import build_rt1
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    cfg = RT1Config(height=a.height, width=a.width, seq_len=a.seq_len, backend="hip")
    torch.manual_seed(0)
    return TrainEngine(build_rt1(cfg), cfg, order_probe=False, graph=a.graph, device=dev,
                       accumulate_grad_batches=k), cfg, dev


def _stream(a, cfg, dev):
    from pytorch_rt1_for_distributed_training_amd.data.prefetch import DevicePrefetcher
    from pytorch_rt1_for_distributed_training_amd.data.synthetic import SyntheticStream
    stream = SyntheticStream(a.batch, cfg.seq_len, cfg.height, cfg.width, ring=2, uint8=True, seed=0)
    return iter(DevicePrefetcher(stream, dev, depth=2))


def kernels(a):
    import torch
    from pytorch_rt1_for_distributed_training_amd.ops import load
    from pytorch_rt1_for_distributed_training_amd.parallel import flat as flat_mod
    a.graph = False
    eng, cfg, dev = _engine(a, 2)
    ext = load()
    batch = next(_stream(a, cfg, dev))
    eng.model.train()
    eng.flat.grad.zero_()
    eng.flat.release_grads()
    loss, _ = eng.forward_loss(batch)
    with flat_mod.deferred_sums(eng._defer_sums):
        loss.backward()
    torch.cuda.synchronize()
    # the lists gather_grads forms (read-only here: the pending table is left for the real gather below)
    dst, src, red = [], [], []
    for p, v in zip(eng.flat.params, eng.flat.views):
        g = p.grad
        if g is None:
            continue
        pend = flat_mod._pending_of(g)
        if pend is not None:
            red.append((v, g, pend[1], pend[2]))
        else:
            assert g.dtype == torch.float32 and g.is_contiguous()
            dst.append(v)
            src.append(g)
    n_copy = sum(d.numel() for d in dst)
    n_red = sum(r[0].numel() for r in red)
    n_red_in = sum(r[0].numel() * r[2] for r in red)
    rd, rs, rk, rss = [r[0] for r in red], [r[1] for r in red], [r[2] for r in red], [r[3] for r in red]
    print(f"{torch.cuda.get_device_name(0)}: {a.height}x{a.width} T{a.seq_len} b{a.batch}, flat gradient "
          f"{eng.flat.numel} floats; stolen gradients: {len(dst)} entries, {4 * n_copy / 1e6:.2f} MB; deferred partial "
          f"sets: {len(red)} entries, {4 * n_red / 1e6:.2f} MB out of {4 * n_red_in / 1e6:.2f} MB of partials "
          f"(splits {min(rk) if rk else 0}-{max(rk) if rk else 0}); 100 repetitions each", flush=True)
    rows = [("multi_copy_", lambda: ext.multi_copy_(dst, src), 8 * n_copy),
            ("multi_add_", lambda: ext.multi_add_(dst, src), 12 * n_copy)]
    if red:
        rows += [("multi_reduce_copy_", lambda: ext.multi_reduce_copy_(rd, rs, rk, rss), 4 * (n_red_in + n_red)),
                 ("multi_reduce_add_", lambda: ext.multi_reduce_add_(rd, rs, rk, rss), 4 * (n_red_in + 2 * n_red))]
    res = {}
    for rep in range(2):
        for name, fn, nbytes in rows:
            us = _time_us(fn)
            res.setdefault(name, []).append(us)
            print(f"pass {rep + 1}  {name:20s} {us:9.2f} us  {nbytes / us / 1e3:9.1f} GB/s over {nbytes / 1e6:9.3f} MB",
                  flush=True)
    best = {k: min(v) for k, v in res.items()}
    print(f"multi_add_ / multi_copy_ = {best['multi_add_'] / best['multi_copy_']:.2f}x (bytes alone: 1.50x)", flush=True)
    if red:
        print(f"multi_reduce_add_ / multi_reduce_copy_ = {best['multi_reduce_add_'] / best['multi_reduce_copy_']:.2f}x "
              f"(bytes alone: {(n_red_in + 2 * n_red) / (n_red_in + n_red):.2f}x)", flush=True)
    eng.flat.grad.zero_()
    eng.flat.gather_grads(accumulate=True)         # the real gather: consumes the pending table
    torch.cuda.synchronize()
    assert not flat_mod._PENDING and bool(torch.isfinite(eng.flat.grad).all())


def step(a):
    import torch
    a.graph = True
    eng, cfg, dev = _engine(a, a.k)
    batches = _stream(a, cfg, dev)
    for _ in range(a.warmup * a.k):
        eng.train_step(next(batches))
        torch.cuda.synchronize()
    assert eng._graph is not None, "the step was not captured"
    assert eng.micro_step == 0
    check = None
    if a.check:
        # the replayed (micro-)step against the eager one from the same state, bitwise; the engine is left untouched
        eng.train_step(next(batches))
        check = eng.graph_eager_check(next(batches))
        for _ in range(a.k - 1):
            eng.train_step(next(batches))
        torch.cuda.synchronize()
        assert eng.micro_step == 0
    t0 = time.perf_counter()
    for _ in range(a.windows * a.k):
        loss = eng.train_step(next(batches))
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0)
    print(json.dumps(dict(k=a.k, ms_per_micro_step=round(ms / (a.windows * a.k), 3),
                          ms_per_window=round(ms / a.windows, 3), windows=a.windows, batch=a.batch,
                          samples_per_s=round(a.batch * a.windows * a.k / ms * 1e3, 1), loss=float(loss),
                          optimizer_steps=eng.global_step,
                          graph_eq_eager=(check["equal"] if check is not None else None))), flush=True)


def step_all(a):
    """k = 1, 2, 4: a fresh child process per run (nothing is shared but the GPU)."""
    for k in a.ks:
        windows = max(1, a.micro_steps // k)
        cmd = [sys.executable, os.path.abspath(__file__), "step", "--k", str(k), "--windows", str(windows), "--warmup",
               str(a.warmup), "--batch", str(a.batch), "--height", str(a.height), "--width", str(a.width),
               "--seq_len", str(a.seq_len)] + (["--check"] if a.check else [])
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.child_timeout)
        if r.returncode != 0:
            print(r.stdout[-2000:], r.stderr[-4000:], flush=True)
            raise SystemExit(f"child failed with {r.returncode}; stopping")
        print(r.stdout.strip().splitlines()[-1], flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["kernels", "step", "step_all"])
    ap.add_argument("--k", type=int, default=2, help="step: accumulate_grad_batches")
    ap.add_argument("--ks", type=int, nargs="+", default=[1, 2, 4], help="step_all: the values of k")
    ap.add_argument("--windows", type=int, default=10, help="step: timed windows")
    ap.add_argument("--micro_steps", type=int, default=20, help="step_all: timed micro-steps per run")
    ap.add_argument("--warmup", type=int, default=3, help="warm-up windows")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--height", type=int, default=300)
    ap.add_argument("--width", type=int, default=300)
    ap.add_argument("--seq_len", type=int, default=6)
    ap.add_argument("--check", action="store_true",
                    help="step: TrainEngine.graph_eager_check of one (micro-)step after the warm-up (mid-window for k > 1)")
    ap.add_argument("--child_timeout", type=float, default=240.0)
    a = ap.parse_args()
    {"kernels": kernels, "step": step, "step_all": step_all}[a.mode](a)


if __name__ == "__main__":
    main()
