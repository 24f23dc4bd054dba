"""LAVA's policy head on csrc/kernels/lavahead.hip (ops/lava_head.py) against the modules' own expression -- plain
F.linear, relu, add and autograd -- in fp64 on the CPU.

Per tensor the metric is max |got - ref64| / max |ref64| and the bound is 4x the same metric of that expression in fp32
eager on the GPU (tests/test_lava_language_gpu.py's rule).  Every output must be bitwise equal over two runs.  Both
metrics are printed (pytest -s).  Checked: the action, dx and every dW and db, for the loss (action * dout).sum().

B = 1 (one row), 3 (a partial M-tile), 16 (one tile), 17 (a second tile holding one row) and row_chunk() + 1 (a second
chunk holding one row; the 64-row chunks of the 256-column layers hold four full chunks and one row).

The ReLU condition is asserted on the fp64 reference alone, so a bad seed fails as a bad seed: no ReLU input with a
non-zero incoming gradient may lie within gate(B) of zero, or a gate that legitimately flips in fp32 could fail the
bound.  gate is 1e-4 for B = 1, 3, 16 and 17, with the seeds below found for it on the CPU (the smallest seed that
meets it; at B = 16 and 17 most seeds leave one to a few inputs inside 1e-4).  Only B = row_chunk() + 1 = 257 cannot
meet 1e-4: with 257 x 1536 ReLU inputs per block, 98 to 113 of them lie inside 1e-4 for (128, 2, 2) and 32 to 46 for
(256, 1, 3) at every seed 0 .. 7.  There gate is 1e-6, the rounding error of an fp32 sum of 1024 such products
(sqrt(1024) 2^-24 0.6), and the two seeds used keep every ReLU input at least 2e-6 away from zero.
"""
import pytest
import torch
import torch.nn.functional as F

SHAPES = [(128, 2, 2), (256, 1, 3)]                                       # (din, blocks, action_size)
SEEDS = {(128, 2, 2): [1, 1, 177, 1805, 0], (256, 1, 3): [0, 0, 18, 6, 5]}    # per B case, picked on the CPU (see gate)
WIDTH = 1024


def gate(b):
    return 1e-4 if b <= 17 else 1e-6


def _sizes():
    from pytorch_rt1_for_distributed_training_amd.ops.lava_head import row_chunk
    return [1, 3, 16, 17, row_chunk() + 1]


def _inputs(b, din, blocks, act, seed):
    gen = torch.Generator().manual_seed(seed)
    r = lambda *shape: torch.randn(*shape, generator=gen)
    dims = [(din, WIDTH)] + [(WIDTH, WIDTH // 4), (WIDTH // 4, WIDTH // 4), (WIDTH // 4, WIDTH)] * blocks + [(WIDTH, act)]
    t = {"x": r(b, din), "dout": r(b, act)}
    for i, (k, n) in enumerate(dims):
        t[f"w{i}"], t[f"b{i}"] = 0.05 * r(n, k), 0.05 * r(n)
    t["dres"] = r(b, WIDTH)                                              # the loss weights of dense_resnet alone
    return t, len(dims)


def _eager(t, n, dtype, dev, proj=True, gates=None):
    """DenseResnet.forward and the projection written out; ``gates`` collects (ReLU input, ReLU output)."""
    v = {k: t[k].to(dev, dtype).requires_grad_() for k in t if k[0] != "d"}
    def relu(p):
        q = F.relu(p)
        if gates is not None:
            q.retain_grad()
            gates.append((p, q))
        return q
    h = F.linear(v["x"], v["w0"], v["b0"])
    for i in range(1, n - 1, 3):
        y = F.linear(relu(h), v[f"w{i}"], v[f"b{i}"])
        y = F.linear(relu(y), v[f"w{i + 1}"], v[f"b{i + 1}"])
        h = h + F.linear(relu(y), v[f"w{i + 2}"], v[f"b{i + 2}"])
    return _finish(t, v, n, F.linear(h, v[f"w{n - 1}"], v[f"b{n - 1}"]) if proj else h, proj, dev, dtype)


def _finish(t, v, n, out, proj, dev, dtype):
    dout = t["dout" if proj else "dres"].to(dev, dtype)
    names = ["x"] + [f"{p}{i}" for i in range(n if proj else n - 1) for p in "wb"]
    grads = torch.autograd.grad((out * dout).sum(), [v[k] for k in names], retain_graph=True)
    return ["out"] + ["d" + k for k in names], [a.detach().double().cpu() for a in [out] + list(grads)]


def _hip(t, n, proj=True):
    from pytorch_rt1_for_distributed_training_amd.models.lava import DenseResnet
    from pytorch_rt1_for_distributed_training_amd.ops.lava_head import dense_resnet, dense_resnet_head
    head = DenseResnet(t["x"].shape[1], WIDTH, (n - 2) // 3)
    lins = [head.inp] + [l for b in head.blocks for l in (b[1], b[3], b[5])] + [torch.nn.Linear(WIDTH, t["dout"].shape[1])]
    for i, lin in enumerate(lins):
        lin.weight.data, lin.bias.data = t[f"w{i}"].clone(), t[f"b{i}"].clone()
    head, last = head.cuda(), lins[-1].cuda()
    x = t["x"].cuda().requires_grad_()
    v = {"x": x, **{f"{p}{i}": getattr(lin, a) for i, lin in enumerate(lins) for p, a in (("w", "weight"), ("b", "bias"))}}
    out = dense_resnet_head(x, head, last) if proj else dense_resnet(x, head)
    return _finish(t, v, n, out, proj, "cuda", torch.float32)[1]


def _reference(t, n, proj=True):
    gates = []
    names, ref = _eager(t, n, torch.float64, "cpu", proj, gates)
    eps = gate(t["x"].shape[0])
    near = sum(int(((p.abs() < eps) & (q.grad != 0)).sum()) for p, q in gates)
    assert near == 0, f"bad seed: {near} ReLU inputs within {eps} of zero carry a gradient"
    return names, ref


def _check(tag, names, ref, eag, got, again):
    failures = []
    for name, r, e, g, g2 in zip(names, ref, eag, got, again):
        assert torch.isfinite(g).all(), name
        assert torch.equal(g, g2), f"{name}: two runs differ"
        scale = float(r.abs().max())
        err_e, err_g = float((e - r).abs().max()) / scale, float((g - r).abs().max()) / scale
        print(f"lava_head {tag} {name:5s} max|ref|={scale:.3e} eager={err_e:.3e} hip={err_g:.3e}")
        if not err_g <= 4 * err_e:
            failures.append(f"{name}: hip {err_g:.3e} > bound from eager {err_e:.3e}")
    assert not failures, failures


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "din%d-blocks%d-act%d" % s)
@pytest.mark.parametrize("case", range(5))
def test_head_matches_fp64(case, shape):
    b = _sizes()[case]
    t, n = _inputs(b, *shape, SEEDS[shape][case])
    names, ref = _reference(t, n)
    _check(f"B={b} {shape}", names, ref, _eager(t, n, torch.float32, "cuda")[1], _hip(t, n), _hip(t, n))


@pytest.mark.gpu
def test_dense_resnet_alone_matches_fp64():
    t, n = _inputs(3, 128, 2, 2, SEEDS[(128, 2, 2)][1])
    names, ref = _reference(t, n, proj=False)
    _check("resnet B=3", names, ref, _eager(t, n, torch.float32, "cuda", False)[1], _hip(t, n, False), _hip(t, n, False))
