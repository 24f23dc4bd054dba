"""tl_fwd and tl_bwd (csrc/kernels/tokenlearner.hip) against the element-wise fp64 oracle of tests/tl_oracle.py, stage
by stage from the stored intermediates: P below one 16-row block, either side of every block edge, either side of the
switch from tl_bwd_kernel<128> to <256> (P = 128 / 129) and at the LDS limit P = 256, with N = 1 and 3 frames, rows of
different means and scales, a near-one-hot and a nearly flat softmax.  P = 257 is refused by tl_supported and by both
bindings.  Every case repeats bitwise.  Run with -s for one line per case and one summary per entry point
(profiles/se_stem_tl_oracle_gpu.log)."""
import pytest
import torch

import gemm_oracle as gm
import glue_oracle as go
import tl_oracle as tlo

pytestmark = pytest.mark.gpu

DEV = "cuda"
TABLES = {}
PS = [1, 15, 16, 17, 63, 64, 65, 100, 127, 128, 129, 225, 255, 256]
CASES = [(N, P, "normal") for P in PS for N in (1, 3)] + [(3, P, k) for P in (100, 256) for k in ("onehot", "flat")]
CASES.append((8, 225, "normal"))      # 115,200 elements of z1: enough for the bias statistic of its store


@pytest.fixture(scope="module")
def ext():
    from pytorch_rt1_for_distributed_training_amd import ops
    yield ops.load()
    for t in TABLES.values():
        t.summary()
    print()


def table(entry):
    return TABLES.setdefault(entry, gm.Table(entry))


def gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31)
    return torch.Generator(device="cpu").manual_seed(seed)


def inputs(N, P, kind, device=DEV):
    return tlo.make_inputs(N, P, gen(N, P, len(kind)), device, kind)


@pytest.mark.parametrize("N,P,kind", CASES, ids=[f"N{n}-P{p}-{k}" for n, p, k in CASES])
def test_token_learner_every_block_edge(ext, N, P, kind):
    d = inputs(N, P, kind)
    name = f"N{N} P{P} {kind} bwd<{tlo.bwd_template(P)}>"
    assert ext.tl_supported(P, 512, 64, 8) and tlo.bwd_template(P) == (128 if P <= 128 else 256)
    args = (d["x"], d["gamma"], d["beta"], d["eps"], d["W1"], d["b1"], d["W2"], d["b2"])
    fw = ext.tl_fwd(*args)
    assert all(torch.equal(a, b) for a, b in zip(fw, ext.tl_fwd(*args))), f"{name}: tl_fwd does not repeat bitwise"
    st = table("tl_fwd").add(name, tlo.check_fwd(*args, fw, "tl_fwd " + name))
    out, mu, rs, z1, s = fw
    if kind == "onehot":
        assert s.amax(-1).max().item() > 0.5, f"{name}: the softmax is not peaked"
    if kind == "flat":
        assert (s.amax(-1) / s.amin(-1)).max().item() < 1.01, f"{name}: the softmax is not flat"
    bargs = (d["x"], d["dO"], s, z1, mu, rs, d["gamma"], d["beta"], d["W1"].t().contiguous(), d["W2"])
    bw = ext.tl_bwd(*bargs)
    assert all(torch.equal(a, b) for a, b in zip(bw, ext.tl_bwd(*bargs))), f"{name}: tl_bwd does not repeat bitwise"
    table("tl_bwd").add(name, tlo.check_bwd(d["x"], d["dO"], s, z1, mu, rs, d["gamma"], d["beta"], d["W1"], d["W2"], bw,
                                            "tl_bwd " + name))
    assert st["worst_hard"] <= 1.0
    if N * P * 64 >= go.BIAS_MIN_COUNT:
        assert st["count"] >= go.BIAS_MIN_COUNT, f"{name}: too few elements entered the bias statistic"


def test_p_257_is_refused(ext):
    assert ext.tl_supported(256, 512, 64, 8) and not ext.tl_supported(257, 512, 64, 8) and not ext.tl_supported(0, 512, 64, 8)
    d = inputs(1, 257, "normal")
    with pytest.raises(RuntimeError, match="unsupported P"):
        ext.tl_fwd(d["x"], d["gamma"], d["beta"], d["eps"], d["W1"], d["b1"], d["W2"], d["b2"])
    z = lambda *s, dt=torch.float32: torch.zeros(*s, device=DEV, dtype=dt)
    with pytest.raises(RuntimeError, match="unsupported P"):
        ext.tl_bwd(d["x"], d["dO"], z(1, 8, 257), z(1, 257, 64, dt=torch.bfloat16), z(1, 257), z(1, 257), d["gamma"],
                   d["beta"], d["W1"].t().contiguous(), d["W2"])
