"""The glue oracle (tests/glue_oracle.py) can fail: an fp32-math, bf16-store emulation of bn_bwd_apply and block_tail on
the CPU passes it clean and is caught with each of five planted faults.  The truncating store has a relative Frobenius
error of 0.003, well inside the 1e-2 that the older kernel tests accept; the frame-index slip over 7 of 6000 rows comes to
0.012 / 0.017 at this shape and falls below 1e-2 as soon as the map has a few thousand more rows.

Run with -s to see the table: fault, Frobenius error, worst err/bound, mean signed ulp error, verdict."""
import pytest
import torch

import glue_oracle as go

BF = torch.bfloat16
N, HW, C = 3, 2000, 136
FAULTS = ["trunc", "frame", "tail", "keep", "const"]
# (a) trunc: truncating bf16 store                    (b) frame: last 7 rows of frame 1 read frame 2's per-frame rows
# (c) tail:  last vector left equal to its input       (d) keep:  keep[n] also applied to rb / to skip
# (e) const: one channel's k0 / shift taken from its neighbour


@pytest.fixture(scope="module")
def inp():
    d = go.make_inputs(N, HW, C, 20240, "cpu")
    d["keep"] = torch.tensor([0.0, 1.0 / 0.7, 1.0 / 0.7])      # the frame boundary of fault (b) lies between kept frames
    return d


def _store(o, fault):
    if fault == "trunc":
        return (o.contiguous().view(torch.int32) & ~0xFFFF).view(torch.float32).to(BF)
    return o.to(BF)


def _frames(fault):
    fr = torch.arange(N)[:, None].expand(N, HW).clone()
    if fault == "frame":
        fr[1, -7:] = 2
    return fr


def emu_bn_bwd_apply(d, fault=None):
    fr = _frames(fault)
    g, yv = d["G"].float(), d["y"].float()
    kp = d["keep"][fr][..., None]
    gv = g * (d["rs"][fr] * kp)
    gv = gv + (d["rb"][fr] * kp if fault == "keep" else d["rb"][fr])
    z = yv * d["scale"] + d["shift"]
    s = torch.sigmoid(z)
    gv = gv * (s * (1 + z * (1 - s)))
    k1 = d["gamma"] * d["rstd"]
    k2 = -k1 * d["rstd"] * d["mdzx"]
    k0 = -k1 * (d["mdz"] - d["mean"] * d["rstd"] * d["mdzx"])
    if fault == "const":
        k0 = k0.clone()
        k0[5] = k0[6]
    out = _store(k1 * gv + (k2 * yv + k0), fault)
    if fault == "tail":
        out[-1, -1, -8:] = d["G"][-1, -1, -8:]
    return out


def emu_block_tail(d, fault=None):
    fr = _frames(fault)
    sh = d["shift"]
    if fault == "const":
        sh = sh.clone()
        sh[5] = sh[6]
    kp = d["keep"][fr][..., None]
    f = (d["y"].float() * d["scale"] + sh) * kp
    f = f + (d["skip"].float() * kp if fault == "keep" else d["skip"].float())
    out = _store(f * d["fmul"][fr] + d["fadd"][fr], fault)
    if fault == "tail":
        out[-1, -1, -8:] = d["y"][-1, -1, -8:]
    return out


def _ref(op, d):
    if op == "bn_bwd_apply":
        return go.ref_bn_bwd_apply(d["G"], d["y"], d["scale"], d["shift"], d["mean"], d["rstd"], d["gamma"], 1,
                                   d["mdz"], d["mdzx"], d["rs"], d["rb"], d["keep"])
    return go.ref_block_tail(d["y"], d["scale"], d["shift"], d["keep"], d["skip"], d["fmul"], d["fadd"])


EMU = {"bn_bwd_apply": emu_bn_bwd_apply, "block_tail": emu_block_tail}


def _figures(out, ref, S):
    chk = go.Bf16Check("figures")
    chk.add(out, ref, S)
    return chk.worst, chk.mean_ulp


def _report(op, fault, out, ref, S, verdict):
    worst, ulp = _figures(out, ref, S)
    fro = go.frob(out, ref)
    print(f"\nglue oracle | {op:12s} | {fault or 'clean':6s} | frobenius {fro:.5f} | worst err/bound {worst:8.3f} | "
          f"mean signed ulp {ulp:+.4f} | {verdict}")
    return fro


@pytest.mark.parametrize("op", list(EMU))
def test_clean_emulation_passes(inp, op):
    ref, S = _ref(op, inp)
    out = EMU[op](inp)
    stats = go.assert_bf16_exact(out, ref, S, op)
    assert stats["count"] >= go.BIAS_MIN_COUNT      # the bias assertion was not skipped
    _report(op, None, out, ref, S, "passes")


@pytest.mark.parametrize("fault", FAULTS)
@pytest.mark.parametrize("op", list(EMU))
def test_planted_fault_is_caught(inp, op, fault):
    ref, S = _ref(op, inp)
    out = EMU[op](inp, fault)
    with pytest.raises(AssertionError) as e:
        go.assert_bf16_exact(out, ref, S, op)
    fro = _report(op, fault, out, ref, S, "caught: " + str(e.value)[:110])
    if fault == "trunc":
        assert fro < 1e-2       # the Frobenius check of the older tests lets a biased store through


def test_failure_names_the_element(inp):
    ref, S = _ref("block_tail", inp)
    out = emu_block_tail(inp)
    out[2, 1234, 77] = out[2, 1234, 77].float() * 1.02
    with pytest.raises(AssertionError, match=r"\(2, 1234, 77\)"):
        go.assert_bf16_exact(out, ref, S, "block_tail")
    out[0, 3, 9] = float("nan")
    with pytest.raises(AssertionError, match=r"non-finite.*\(0, 3, 9\)"):
        go.assert_bf16_exact(out, ref, S, "block_tail")


def test_exact_zero_needs_exact_zero():
    ref = torch.zeros(1, 2, 8, dtype=torch.float64)
    out = torch.zeros(1, 2, 8, dtype=BF)
    go.assert_bf16_exact(out, ref, ref.clone(), "zeros")
    out[0, 1, 3] = 1e-30
    with pytest.raises(AssertionError):
        go.assert_bf16_exact(out, ref, ref.clone(), "zeros")


def test_bf16_ulp():
    x = torch.tensor([1.0, 1.99, 2.0, -0.75, 3e-5], dtype=torch.float64)
    e = torch.floor(torch.log2(x.abs()))
    assert torch.equal(go.bf16_ulp(x), torch.pow(2.0, e - 7))
