"""Layer-wise trust ratios (csrc/kernels/lamb.hip, ops.adam.flat_lamb_dev_step) on the GPU: the moments against the
fused Adam, every buffer against an fp64 oracle element by element, the applied update against the measured one,
degenerate tensors and the padding, a skipped step, the clip forms, parameter groups against the ungrouped form, bitwise
determinism eager and replayed, the bindings' refusals, and the engine (eager, one graph, every option, resume).

Layouts (tensor sizes in floats; every tensor is padded with zeros to a multiple of 64):
  A  1, 63, 64, 65, 200, 4097: every padding length, tensor boundaries inside one wave's 256-float row
  B  forty 64-float tensors, then one of 300000: many one-chunk tensors per wave, then a tensor whose 4688 chunk pairs
     lamb_trust splits into runs of 19 per lane
  C  one tensor of 2 * 2048 * 1024 + 192 floats: every lane makes more than one grid-stride trip
  D  A with tensor 2 all-zero (||p|| = 0), tensor 3 without gradient or momentum (||u|| = 0), tensor 4 not adapted; wd = 0

Tolerances.  m, v: those of the fused Adam's fp64 test (rtol 1e-5, atol 1e-7 / 1e-8); p and ema: rtol 1e-5, atol 1e-6.
trust and norms: rtol 1e-5 -- 64 non-negative fp32 terms per chunk bound the error of a squared norm by
64 * 2^-24 = 3.8e-6, half of that on a norm, twice that in the ratio, plus a few ulp from forming u in fp32; everything
after the chunk sums is fp64.  Measured on an MI355X: trust and ||u|| lie 6e-6 to 7e-6 from the oracle, always to the
same side.  That is the hyperparameter, not the sums: the kernels receive beta2 = 0.999 in fp32, whose 1 - beta2 is
1.3e-5 off, so the bias correction 1 - beta2^t is, and u by half of it (the fused Adam carries the same constant); the
oracle is given the double.  ||p|| agrees to 1e-7."""
import math
from unittest import mock

import pytest
import torch

pytestmark = pytest.mark.gpu

GS = 0.25
LR = 1e-2
WD = 0.02
OMD = 1e-3
BETAS = dict(beta1=0.9, beta2=0.999, eps=1e-8)
N_BIG = 2 * 2048 * 1024 + 192
SIZES = {"A": [1, 63, 64, 65, 200, 4097], "B": [64] * 40 + [300000], "C": [N_BIG]}
SIZES["D"] = SIZES["A"]
FORMS = ["plain", "ema", "clip_inactive", "clip_active", "ema_clip_active"]


def _ops():
    from pytorch_rt1_for_distributed_training_amd.ops import adam
    return adam


def _align(n):
    return (n + 63) // 64 * 64


def _starts(name):
    out = [0]
    for s in SIZES[name]:
        out.append(out[-1] + _align(s) // 64)
    return out


def _numel(name):
    return _starts(name)[-1] * 64


def _real(name):
    """Mask of the elements that belong to a tensor (False on the padding)."""
    mask = torch.zeros(_numel(name), dtype=torch.bool, device="cuda")
    for s, c in zip(SIZES[name], _starts(name)):
        mask[c * 64:c * 64 + s] = True
    return mask


def _seg(name, i):
    c = _starts(name)
    return slice(c[i] * 64, c[i + 1] * 64)


_BASE = {}


def _base(name):
    """Seeded start buffers of the layout with zero padding, computed once and never modified.  Every tensor has its
    own scale in [1e-2, 1]; v stays above 1e-3 so that no single element dominates a tensor's update norm."""
    if name not in _BASE:
        n, real = _numel(name), _real(name)
        g = torch.Generator(device="cuda").manual_seed(977 + n % 1000)
        scale = torch.ones(n, device="cuda")
        for i in range(len(SIZES[name])):
            scale[_seg(name, i)] = 10.0 ** (-2.0 * ((i * 7) % 5) / 4.0)
        z = lambda t: torch.where(real, t, torch.zeros_like(t))
        p = z(torch.randn(n, device="cuda", generator=g) * scale)
        b = dict(grad=z(torch.randn(n, device="cuda", generator=g)), p=p,
                 m=z(torch.randn(n, device="cuda", generator=g) * 0.1),
                 v=z(torch.rand(n, device="cuda", generator=g) * 0.1 + 1e-3),
                 ema=z(p * (1 + 1e-2 * torch.randn(n, device="cuda", generator=g))))
        if name == "D":
            b["p"][_seg(name, 2)] = 0
            b["ema"][_seg(name, 2)] = 0
            b["grad"][_seg(name, 3)] = 0
            b["m"][_seg(name, 3)] = 0
        _BASE[name] = b
    return _BASE[name]


def _start(name):
    b = _base(name)
    return [b[k].clone() for k in ("p", "m", "v", "ema")]


def _adapt(name):
    a = [1] * len(SIZES[name])
    if name == "D":
        a[4] = 0
    return a


_TABLES = {}


def _tables(name, adapt=None):
    adapt = tuple(_adapt(name) if adapt is None else adapt)
    if (name, adapt) not in _TABLES:
        _TABLES[name, adapt] = _ops().lamb_tables(_starts(name), list(adapt), _numel(name), "cuda")
    return _TABLES[name, adapt]


def _work(name):
    nT = len(SIZES[name])
    return dict(chunk_sums=torch.zeros(_numel(name) // 64, 2, device="cuda"), trust=torch.ones(nT, device="cuda"),
                norms=torch.zeros(nT, 2, device="cuda"))


def _clip(form, grad, coef=None):
    """clip_state for the form (None without CLIP): the verdict of the norm kernels with a bound far away (inactive,
    coefficient 1) or at half the norm (active, about 0.5); ``coef``: a hand-written verdict with that coefficient."""
    if "clip" not in form:
        return None
    if coef is not None:
        return torch.tensor([1.0, coef, 1.0, 0, 0, 0, 0, 0], device="cuda")
    ops = _ops()
    cs = torch.zeros(8, device="cuda")
    pt = torch.zeros(ops.gradnorm_partials(grad.numel()), dtype=torch.float64, device="cuda")
    norm = float(grad.double().pow(2).sum().sqrt()) * GS
    ops.grad_norm_clip_(grad, cs, pt, max_norm=1e30 if "inactive" in form else 0.5 * norm, grad_scale=GS,
                        skip_nonfinite=True)
    assert float(cs[1]) == 1.0 if "inactive" in form else 0.49 < float(cs[1]) < 0.51
    return cs


def _lamb(name, form, bufs, grad, state, work, cs=None, es=None, wd=WD, tables=None, gstate=None, table=None):
    p, m, v, ema = bufs
    tcs, ta, ct = tables if tables is not None else _tables(name)
    on = "ema" in form
    _ops().flat_lamb_dev_step(p, grad, m, v, state, tensor_chunk_start=tcs, tensor_adapt=ta,
                              chunk_tensor=ct, ema=ema if on else None,
                              ema_state=es if on else None, clip_state=cs, group_state=gstate, chunk_group=table,
                              weight_decay=wd, grad_scale=GS, one_minus_decay=OMD, warmup=True, **work, **BETAS)


def _adam(form, bufs, grad, state, cs=None, es=None, wd=WD):
    p, m, v, ema = bufs
    on = "ema" in form
    _ops().flat_adam_dev_step(p, grad, m, v, state, ema=ema if on else None, ema_state=es if on else None,
                              clip_state=cs, weight_decay=wd, grad_scale=GS, one_minus_decay=OMD, warmup=True, **BETAS)


def _state(step, lr=LR):
    return torch.tensor([float(step), lr], device="cuda")


def _es():
    return torch.zeros(4, device="cuda")


def _close(got, want, rtol, atol, what):
    """Element-wise over the whole buffer; prints the worst element."""
    got, want = got.double().reshape(-1), want.double().reshape(-1)
    assert got.shape == want.shape
    err = (got - want).abs()
    tol = atol + rtol * want.abs()
    k = int((err - tol).argmax())
    print(f"{what}: {got.numel()} elements, max err {float(err.max()):.3e}; worst vs tolerance at [{k}]: got "
          f"{float(got[k]):.9e} want {float(want[k]):.9e} err {float(err[k]):.3e} tol {float(tol[k]):.3e}")
    assert bool((err <= tol).all()), f"{what}: {int((err > tol).sum())} elements beyond rtol {rtol} atol {atol}"


# ------------------------------------------------------------------------------------- 1. the moments are Adam's
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_moments_are_adams(name, form):
    grad = _base(name)["grad"]
    cs = _clip(form, grad)
    a, b, c = _start(name), _start(name), _start(name)
    _lamb(name, form, a, grad, _state(3), _work(name), cs=cs, es=_es())
    _adam(form, b, grad, _state(3), cs=cs, es=_es())
    c[0].mul_(-3.0).add_(0.5)                                   # other weights: the moments do not depend on p
    c[3].copy_(c[0])
    _lamb(name, form, c, grad, _state(3), _work(name), cs=cs, es=_es())
    torch.cuda.synchronize()
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), "m, v differ from flat_adam_dev_step's"
    assert torch.equal(a[1], c[1]) and torch.equal(a[2], c[2]), "m, v depend on p"
    assert not torch.equal(a[1], _base(name)["m"]) and not torch.equal(a[0], _base(name)["p"])
    assert torch.equal(grad, _base(name)["grad"])


# ------------------------------------------------------------------------------------- 2. fp64 oracle
def _oracle_steps(name, form, steps, wd=WD, lr=LR, cs=None, adapt=None, table=None, lrs=None, wds=None):
    """Runs ``steps`` on copies with the kernels and with the fp64 oracle; returns (bufs, work, ref, trust64, norms64)."""
    ops = _ops()
    grad = _base(name)["grad"]
    bufs, work, es = _start(name), _work(name), _es()
    ref = [t.double() for t in bufs]
    tables = _tables(name, adapt)
    coef = float(cs[1]) if cs is not None else 1.0
    skipped = float(cs[3]) if cs is not None else 0.0
    gstate = None
    if table is not None:
        gstate = torch.tensor([[l, w, 0.0, 0.0] for l, w in zip(lrs, wds)], dtype=torch.float32, device="cuda")
    trust = norms = None
    for step in steps:
        _lamb(name, form, bufs, grad, _state(step, lr), work, cs=cs, es=es, wd=wd, tables=tables, gstate=gstate,
              table=table)
        t = step - skipped
        trust, norms = ops.reference_lamb_step(ref[0], grad.double(), ref[1], ref[2], _starts(name),
                                               _adapt(name) if adapt is None else adapt,
                                               lr=lrs if table is not None else lr, beta1=0.9, beta2=0.999, eps=1e-8,
                                               weight_decay=wds if table is not None else wd, step=t,
                                               grad_scale=GS * coef, chunk_group=table)
        if "ema" in form:
            ref[3] = ops.reference_ema_step(ref[3], ref[0], max(OMD, 9.0 / (10.0 + t)))
    torch.cuda.synchronize()
    return bufs, work, ref, trust, norms


def _check_oracle(tag, form, bufs, work, ref, trust, norms):
    for got, want, atol, what in zip(bufs[:3], ref[:3], (1e-6, 1e-7, 1e-8), "pmv"):
        _close(got, want, 1e-5, atol, f"{tag} {what}")
    if "ema" in form:
        _close(bufs[3], ref[3], 1e-5, 1e-6, f"{tag} ema")
    _close(work["trust"], trust, 1e-5, 0.0, f"{tag} trust")
    _close(work["norms"], norms, 1e-5, 0.0, f"{tag} norms")


@pytest.mark.parametrize("form", ["plain", "ema", "clip_active", "ema_clip_active"])
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_matches_the_fp64_oracle(name, form):
    cs = _clip(form, _base(name)["grad"])
    _check_oracle(f"{name} {form}", form, *_oracle_steps(name, form, (1, 2, 7), cs=cs))


# ------------------------------------------------------------------------------------- 3. applied u = measured u
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_the_applied_update_is_the_measured_one(name):
    """lr = 1, wd = 0: p_new = p - r u with r = ||p|| / ||u||, so ||p_old - p_new|| / ||p_old|| = 1 for every tensor."""
    grad = _base(name)["grad"]
    bufs, work = _start(name), _work(name)
    _lamb(name, "plain", bufs, grad, _state(2, lr=1.0), work, wd=0.0)
    torch.cuda.synchronize()
    old = _base(name)["p"].double()
    moved = old - bufs[0].double()
    for i in range(len(SIZES[name])):
        s = _seg(name, i)
        ratio = float(moved[s].pow(2).sum().sqrt() / old[s].pow(2).sum().sqrt())
        print(f"{name} tensor {i} ({SIZES[name][i]} floats): |dp| / |p| = {ratio:.9f}, trust {float(work['trust'][i]):.6e}")
        assert abs(ratio - 1.0) <= 1e-5


# ------------------------------------------------------------------------------------- 4. degenerate tensors, padding
def _group_layout(name, G, adapt_off=None):
    """Group of tensor i is i % G (runs aligned to tensors); (chunk table on the device, lrs, wds, tensor_adapt): the
    last group has lr = 0, odd groups wd = 0, the tensors of group ``adapt_off`` are not adapted."""
    starts = _starts(name)
    table = torch.zeros(starts[-1], dtype=torch.uint8)
    for i in range(len(SIZES[name])):
        table[starts[i]:starts[i + 1]] = i % G
    lrs = [LR * (1 + g) / 2 for g in range(G)]
    lrs[-1] = 0.0
    wds = [0.0 if g % 2 else 0.02 * (g + 1) for g in range(G)]
    adapt = [0 if i % G == adapt_off else 1 for i in range(len(SIZES[name]))]
    return table.cuda(), lrs, wds, adapt


@pytest.mark.parametrize("form", FORMS + ["grouped", "ema_grouped"])
def test_degenerate_tensors_and_padding(form):
    name = "D"
    grad = _base(name)["grad"]
    cs = _clip(form, grad)
    bufs, work, es = _start(name), _work(name), _es()
    kw = dict(wd=0.0)
    if "grouped" in form:
        # three groups, every one with wd = 0 (so that ||u|| = 0 holds for tensor 3); tensor 4 alone in the group whose
        # flag is off
        table = torch.zeros(_numel(name) // 64, dtype=torch.uint8)
        starts = _starts(name)
        for i, gi in enumerate([0, 1, 0, 1, 2, 0]):
            table[starts[i]:starts[i + 1]] = gi
        kw.update(table=table.cuda(),
                  gstate=torch.tensor([[LR, 0, 0, 0], [2 * LR, 0, 0, 0], [LR / 2, 0, 0, 0]], device="cuda"))
    for step in (1, 2, 3):
        _lamb(name, form, bufs, grad, _state(step), work, cs=cs, es=es, **kw)
        if step == 1:
            torch.cuda.synchronize()
            assert work["trust"][[2, 3, 4]].tolist() == [1.0, 1.0, 1.0]      # ||p|| = 0, ||u|| = 0, not adapted
            assert work["norms"][2, 0] == 0 and work["norms"][3, 1] == 0 and work["norms"][4].min() > 0
            assert all(float(work["trust"][i]) != 1.0 for i in (0, 1, 5))
    torch.cuda.synchronize()
    assert work["trust"][[3, 4]].tolist() == [1.0, 1.0]
    assert torch.equal(bufs[0][_seg(name, 3)], _base(name)["p"][_seg(name, 3)]), "the ||u|| = 0 tensor moved"
    assert not torch.equal(bufs[0][_seg(name, 2)], _base(name)["p"][_seg(name, 2)])
    pad = ~_real(name)
    assert int(pad.sum()) == 63 + 1 + 0 + 63 + 56 + 63
    for buf, what in zip(bufs if "ema" in form else bufs[:3], ("p", "m", "v", "ema")):
        assert not bool(buf[pad].any()), f"padding of {what} is not zero"


# ------------------------------------------------------------------------------------- 5. a skipped step
@pytest.mark.parametrize("form", ["clip_active", "ema_clip_active"])
def test_skipped_step_touches_nothing_and_does_not_count(form):
    name = "A"
    ops = _ops()
    grad = _base(name)["grad"]
    bufs, work, es = _start(name), _work(name), _es()
    _lamb(name, form, bufs, grad, _state(1), work, cs=_clip(form, grad, coef=1.0), es=es)     # one good step first
    torch.cuda.synchronize()
    everything = bufs + [work["chunk_sums"], work["trust"], work["norms"], es]
    before = [t.clone() for t in everything]
    skip = torch.tensor([float("inf"), 1.0, 0.0, 1.0, 0.0, 1.0, 0.0, 0.0], device="cuda")
    _lamb(name, form, bufs, grad, _state(2), work, cs=skip, es=es)
    torch.cuda.synchronize()
    for t, b in zip(everything, before):
        assert torch.equal(t, b)
    # the next good step: the device counter says 3, one step was skipped, so this is Adam step 2
    ref = [t.double() for t in bufs]
    good = torch.tensor([1.0, 0.5, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0], device="cuda")
    _lamb(name, form, bufs, grad, _state(3), work, cs=good, es=es)
    trust, norms = ops.reference_lamb_step(ref[0], grad.double(), ref[1], ref[2], _starts(name), _adapt(name), lr=LR,
                                           beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=WD, step=2,
                                           grad_scale=GS * 0.5)
    if "ema" in form:
        ref[3] = ops.reference_ema_step(ref[3], ref[0], max(OMD, 9.0 / 12.0))
        assert es.tolist()[1] == 2.0
    torch.cuda.synchronize()
    _check_oracle(f"after a skipped step, {form}", form, bufs, work, ref, trust, norms)


# ------------------------------------------------------------------------------------- 6. the clip forms
@pytest.mark.parametrize("name", ["A", "B"])
def test_clip_forms(name):
    grad = _base(name)["grad"]
    # a verdict with coef == 1 is no verdict, bit for bit
    a, b, wa, wb = _start(name), _start(name), _work(name), _work(name)
    _lamb(name, "ema", a, grad, _state(2), wa, es=_es())
    _lamb(name, "ema_clip_inactive", b, grad, _state(2), wb, cs=_clip("clip_inactive", grad), es=_es())
    torch.cuda.synchronize()
    for x, y in zip(a + [wa["trust"], wa["norms"], wa["chunk_sums"]], b + [wb["trust"], wb["norms"], wb["chunk_sums"]]):
        assert torch.equal(x, y)
    # coef = 0.5 is the plain form on 0.5 g, within the oracle tolerances
    c, d, wc, wd_ = _start(name), _start(name), _work(name), _work(name)
    _lamb(name, "clip_active", c, grad, _state(2), wc, cs=_clip("clip_active", grad, coef=0.5))
    _lamb(name, "plain", d, grad * 0.5, _state(2), wd_)
    torch.cuda.synchronize()
    for got, want, atol, what in zip(c[:3], d[:3], (1e-6, 1e-7, 1e-8), "pmv"):
        _close(got, want, 1e-5, atol, f"{name} coef 0.5 vs half the gradient, {what}")
    _close(wc["trust"], wd_["trust"], 1e-5, 0.0, f"{name} coef 0.5 vs half the gradient, trust")


# ------------------------------------------------------------------------------------- 7. parameter groups
@pytest.mark.parametrize("form", ["plain", "ema_clip_active"])
@pytest.mark.parametrize("G", [2, 4])
@pytest.mark.parametrize("name", ["A", "B"])
def test_each_group_is_bitwise_the_ungrouped_form(name, G, form):
    grad = _base(name)["grad"]
    cs = _clip(form, grad)
    table, lrs, wds, adapt = _group_layout(name, G, adapt_off=1)
    tables = _tables(name, adapt)
    gstate = torch.tensor([[l, w, 0.0, 0.0] for l, w in zip(lrs, wds)], dtype=torch.float32, device="cuda")
    got, work, es = _start(name), _work(name), _es()
    _lamb(name, form, got, grad, _state(2), work, cs=cs, es=es, tables=tables, gstate=gstate, table=table)
    torch.cuda.synchronize()
    elem = table.repeat_interleave(64)
    tensor_group = torch.tensor([i % G for i in range(len(SIZES[name]))], device="cuda")
    for g in range(G):
        want, wwork, wes = _start(name), _work(name), _es()
        _lamb(name, form, want, grad, _state(2, lr=lrs[g]), wwork, cs=cs, es=wes, wd=wds[g], tables=tables)
        torch.cuda.synchronize()
        mask = elem == g
        for a, b, what in zip(got if "ema" in form else got[:3], want, ("p", "m", "v", "ema")):
            assert torch.equal(a[mask], b[mask]), f"group {g} {what}"
        tmask = tensor_group == g
        assert torch.equal(work["trust"][tmask], wwork["trust"][tmask])
        assert torch.equal(work["norms"][tmask], wwork["norms"][tmask])
        assert torch.equal(es, wes)
    assert bool((work["trust"][tensor_group == 1] == 1.0).all())             # the group whose flag is off
    assert bool((work["trust"][tensor_group == 0] != 1.0).all())
    last = elem == G - 1                                                      # lr = 0: p stays, m and v advance
    assert torch.equal(got[0][last], _base(name)["p"][last])
    assert not torch.equal(got[1][last], _base(name)["m"][last])
    assert not torch.equal(got[2][last], _base(name)["v"][last])


@pytest.mark.parametrize("name", ["A", "B"])
def test_groups_match_the_fp64_oracle(name):
    table, lrs, wds, adapt = _group_layout(name, 4, adapt_off=1)
    _check_oracle(f"{name} grouped", "ema", *_oracle_steps(name, "ema", (1, 2, 7), adapt=adapt, table=table, lrs=lrs,
                                                           wds=wds))


# ------------------------------------------------------------------------------------- 8. determinism
@pytest.mark.parametrize("name", ["B", "C"])
def test_two_runs_are_bitwise_equal(name):
    grad = _base(name)["grad"]
    runs = []
    for _ in range(2):
        bufs, work = _start(name), _work(name)
        _lamb(name, "plain", bufs, grad, _state(2), work)
        runs.append(bufs + [work["trust"], work["norms"], work["chunk_sums"]])
    torch.cuda.synchronize()
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_graph_replays_equal_eager_calls():
    name, form = "B", "ema_clip_active"
    grad = _base(name)["grad"]
    cs = _clip(form, grad)

    def make():
        return dict(bufs=_start(name), work=_work(name), es=_es(), state=_state(0))

    def step(r):
        r["state"][0:1].add_(1.0)                   # the device op the engine advances the step with
        _lamb(name, form, r["bufs"], grad, r["state"], r["work"], cs=cs, es=r["es"])

    eager, graphed, scratch = make(), make(), make()
    for _ in range(3):
        step(eager)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(scratch)                               # warm-up on other buffers
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step(graphed)
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    assert graphed["state"].tolist()[0] == 3.0
    for a, b in zip(eager["bufs"] + [eager["es"]] + list(eager["work"].values()),
                    graphed["bufs"] + [graphed["es"]] + list(graphed["work"].values())):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------- 9. refusals
def test_binding_refusals_name_the_argument():
    ops = _ops()
    name = "A"
    n, starts = _numel(name), _starts(name)
    tables = lambda s=starts, a=_adapt(name), n=n: ops.lamb_tables(s, a, n, "cuda")
    with pytest.raises(RuntimeError, match="tensor_chunk_start starts at 1, expected 0"):
        tables(s=[1] + starts[1:])
    with pytest.raises(RuntimeError, match=f"tensor_chunk_start ends at {starts[-1] - 1}, expected n / 64 = {starts[-1]}"):
        tables(s=starts[:-1] + [starts[-1] - 1])
    with pytest.raises(RuntimeError, match="tensor_chunk_start decreases at entry 3"):
        tables(s=starts[:3] + [1] + starts[4:])
    with pytest.raises(RuntimeError, match="tensor_adapt has 5 entries, expected 6"):
        tables(a=[1] * 5)
    with pytest.raises(RuntimeError, match="n is 100, not a positive multiple of 64"):
        tables(n=100)
    with pytest.raises(RuntimeError, match="describes 65536 tensors, chunk_tensor .uint16. holds at most 65535"):
        ops.lamb_tables(list(range(65537)), [1] * 65536, 65536 * 64, "cuda")
    tcs, ta, ct = ops.lamb_tables(list(range(65536)), [1] * 65535, 65535 * 64, "cuda")        # the most it holds
    assert ct.dtype == torch.uint16 and ct.numel() == 65535 and int(ct[-1].cpu()) == 65534

    tcs, ta, ct = _tables(name)
    assert tcs.tolist() == starts and tcs.dtype == torch.int32 and ta.dtype == torch.uint8
    want_ct = torch.repeat_interleave(torch.arange(6), torch.tensor(starts[1:]) - torch.tensor(starts[:-1]))
    assert ct.cpu().to(torch.int64).tolist() == want_ct.tolist()
    bufs, work = _start(name), _work(name)
    grad = _base(name)["grad"]
    before = [t.clone() for t in bufs]

    def call(cut=None, **kw):
        p, m, v, ema = bufs
        g = grad
        if cut is not None:
            p, g, m, v = p[:cut], g[:cut], m[:cut], v[:cut]
        args = dict(tensor_chunk_start=tcs, tensor_adapt=ta, chunk_tensor=ct, weight_decay=WD, grad_scale=GS, **work,
                    **BETAS)
        args.update(kw)
        ops.flat_lamb_dev_step(p, g, m, v, _state(1), **args)

    with pytest.raises(RuntimeError, match="param has 4000 elements, not a positive multiple of 64"):
        call(cut=4000)
    with pytest.raises(RuntimeError, match="tensor_chunk_start has dtype"):
        call(tensor_chunk_start=tcs.to(torch.int64))
    with pytest.raises(RuntimeError, match="tensor_chunk_start must be a GPU tensor"):
        call(tensor_chunk_start=tcs.cpu())
    with pytest.raises(RuntimeError, match="tensor_adapt has 5 entries, expected 6"):
        call(tensor_adapt=ta[:5])
    with pytest.raises(RuntimeError, match="tensor_adapt has dtype"):
        call(tensor_adapt=ta.to(torch.int32))
    with pytest.raises(RuntimeError, match="chunk_tensor has 73 entries, expected 74"):
        call(chunk_tensor=ct[:73])
    with pytest.raises(RuntimeError, match="chunk_tensor has dtype"):
        call(chunk_tensor=ct.to(torch.int32))
    with pytest.raises(RuntimeError, match="chunk_sums has 146 entries, expected 148"):
        call(chunk_sums=work["chunk_sums"][:73])
    with pytest.raises(RuntimeError, match="chunk_sums has dtype"):
        call(chunk_sums=work["chunk_sums"].double())
    with pytest.raises(RuntimeError, match="trust has 5 entries, expected 6"):
        call(trust=work["trust"][:5])
    with pytest.raises(RuntimeError, match="norms has 6 entries, expected 12"):
        call(norms=torch.zeros(6, device="cuda"))
    with pytest.raises(RuntimeError, match="ema and ema_state go together"):
        call(ema=bufs[3])
    with pytest.raises(RuntimeError, match="group_state and chunk_group go together"):
        call(group_state=torch.zeros(2, 4, device="cuda"))
    with pytest.raises(RuntimeError, match="chunk_group has 73 entries, expected 74"):
        call(group_state=torch.zeros(2, 4, device="cuda"), chunk_group=torch.zeros(73, dtype=torch.uint8, device="cuda"))
    with pytest.raises(RuntimeError, match="clip_state"):
        call(clip_state=torch.zeros(4, device="cuda"))
    with pytest.raises(RuntimeError, match="alias"):
        call(trust=bufs[0][:6])
    with pytest.raises(RuntimeError, match="chunk_tensor must be a GPU tensor"):
        call(chunk_tensor=ct.cpu())
    torch.cuda.synchronize()
    for a, b in zip(bufs, before):
        assert torch.equal(a, b)
    call()
    torch.cuda.synchronize()
    assert not torch.equal(bufs[0], before[0])


# ------------------------------------------------------------------------------------- 10. engine
# The configuration is the one the other engine GPU tests of the suite build (96 x 96 frames, two windows of two frames,
# two transformer layers, bf16, hip backend), not preset("tiny") itself: that preset is the CPU plumbing configuration
# (64 x 64, fp32, torch backend); this is its size class on the backend under test.
ENGINE_WD = 0.05


def _cfg():
    from pytorch_rt1_for_distributed_training_amd.config import RT1Config
    return RT1Config(height=96, width=96, seq_len=2, num_layers=2, backend="hip", dropout_rate=0.0,
                     drop_connect_rate=0.0, crop_ratio=0.0)


def _engine(cfg, graph=False, **kw):
    from pytorch_rt1_for_distributed_training_amd.engine.step import TrainEngine
    from pytorch_rt1_for_distributed_training_amd.models import build_rt1
    from pytorch_rt1_for_distributed_training_amd.ops import rng
    rng._COUNTERS.clear()
    torch.manual_seed(0)
    kw = dict(dict(lr=5e-4, weight_decay=ENGINE_WD), **kw)
    return TrainEngine(build_rt1(cfg), cfg, order_probe=False, graph=graph, **kw)


def _batches(cfg, n, b=2):
    from pytorch_rt1_for_distributed_training_amd.data.synthetic import make_batch
    torch.manual_seed(123)
    return [make_batch(b, cfg.seq_len, cfg.height, cfg.width, device="cuda") for _ in range(n)]


@pytest.mark.parametrize("no_decay", [False, True])
def test_engine_graph_equals_eager(no_decay):
    cfg = _cfg()
    batches = _batches(cfg, 3)
    eager = _engine(cfg, optimizer="lamb", no_decay_norm_bias=no_decay)
    graphed = _engine(cfg, graph=True, optimizer="lamb", no_decay_norm_bias=no_decay)
    start = eager.flat.data.clone()
    for b in batches:
        le, lg = eager.train_step(b), graphed.train_step(b)
        torch.cuda.synchronize()
        assert torch.equal(le, lg)
    assert graphed._graph is not None, "capture did not happen"
    assert torch.equal(eager.flat.data, graphed.flat.data) and not torch.equal(eager.flat.data, start)
    assert torch.equal(eager.optimizer.exp_avg, graphed.optimizer.exp_avg)
    assert torch.equal(eager.optimizer.trust, graphed.optimizer.trust)
    assert torch.equal(eager.optimizer.norms, graphed.optimizer.norms)
    opt = graphed.optimizer
    trust = opt.trust.tolist()
    assert all(math.isfinite(t) and t > 0 for t in trust)
    vectors = [i for i, p in enumerate(graphed.flat.params) if p.ndim <= 1]
    matrices = [i for i, p in enumerate(graphed.flat.params) if p.ndim >= 2]
    assert vectors and matrices
    if no_decay:
        emb = {id(m.weight) for m in graphed.model.modules() if isinstance(m, torch.nn.Embedding)}
        off = [i for i, p in enumerate(graphed.flat.params) if p.ndim <= 1 or id(p) in emb]
        assert opt.tensor_adapt.tolist() == [0 if i in set(off) else 1 for i in range(len(trust))]
        assert [trust[i] for i in off] == [1.0] * len(off), "a norm / bias / embedding tensor was adapted"
    else:
        assert opt.tensor_adapt.tolist() == [1] * len(trust)
    assert sum(trust[i] != 1.0 for i in matrices) > len(matrices) // 2
    names = list(opt.trust_ratios())
    assert len(names) == len(trust) and all(isinstance(n, str) and not n.isdigit() for n in names)


def test_graph_dp_path_world1_with_lamb():
    """The segmented graph-DP step (a single-rank RCCL communicator drives the bucketed path) against the eager one."""
    import pytorch_rt1_for_distributed_training_amd as rt1
    from pytorch_rt1_for_distributed_training_amd.data.synthetic import make_batch
    from pytorch_rt1_for_distributed_training_amd.engine.step import TrainEngine
    from pytorch_rt1_for_distributed_training_amd.models import build_rt1
    cfg = rt1.RT1Config(height=128, width=128, seq_len=6, backend="hip", dropout_rate=0.0, drop_connect_rate=0.0,
                        crop_ratio=0.0)
    engines = []
    for graph in (True, False):
        torch.manual_seed(0)
        engines.append(TrainEngine(build_rt1(cfg), cfg, order_probe=True, bucket_cap_mb=4.0, comm="native",
                                   graph=graph, optimizer="lamb", weight_decay=ENGINE_WD))
    eg, ee = engines
    assert eg.ddp.enabled and len(eg.ddp.buckets) > 1
    g = torch.Generator().manual_seed(7)
    try:
        for step in range(3):
            batch = make_batch(4, cfg.seq_len, 128, 128, device="cuda", generator=g)
            lg, le = float(eg.train_step(batch)), float(ee.train_step(batch))
            torch.cuda.synchronize()
            assert lg == le, (step, lg, le)
            assert torch.equal(eg.flat.data, ee.flat.data), step
            assert torch.equal(eg.optimizer.trust, ee.optimizer.trust), step
        assert eg._segments is not None and eg._segments.num_segments > 1
        assert float(eg.optimizer.dev_state[0]) == 3.0 and not bool((eg.optimizer.trust == 1.0).all())
    finally:
        eg.ddp.comm.destroy()
        ee.ddp.comm.destroy()


class _MemoryLogger:
    def __init__(self):
        self.rows = []

    def log(self, metrics, step, epoch):
        self.rows.append(dict(metrics, step=step))

    def flush(self):
        pass


def test_engine_with_every_option_on():
    from pytorch_rt1_for_distributed_training_amd.engine.trainer import Trainer
    from pytorch_rt1_for_distributed_training_amd.utils.logging import MultiLogger
    cfg = _cfg()
    eng = _engine(cfg, graph=True, optimizer="lamb", no_decay_norm_bias=True, max_grad_norm=1.0, skip_nonfinite=True,
                  ema_decay=0.999, accumulate_grad_batches=2,
                  lr_schedule=dict(kind="cosine", warmup_steps=2, decay_steps=10, min_lr_ratio=0.1))
    log = _MemoryLogger()
    tr = Trainer(eng, max_epochs=1, log_every_n_steps=1, logger=MultiLogger([log]), num_sanity_val_steps=0,
                 verbose=False)
    start = eng.flat.data.clone()
    tr.fit(_batches(cfg, 6), None)
    torch.cuda.synchronize()
    assert eng.global_step == 3 and eng.optimizer.skipped_steps == 0
    rows = [r for r in log.rows if "train_loss_step" in r]
    assert len(rows) == 3 and all(math.isfinite(r["train_loss_step"]) for r in rows)
    for r in rows:
        assert 0 < r["trust/min"] <= r["trust/median"] <= r["trust/max"] and math.isfinite(r["trust/max"])
    assert not torch.equal(eng.flat.data, start) and bool(torch.isfinite(eng.flat.data).all())
    assert not torch.equal(eng.optimizer.ema, eng.flat.data)


def test_resume_from_an_adam_checkpoint_continues_under_lamb(tmp_path):
    from pytorch_rt1_for_distributed_training_amd.engine.trainer import Trainer
    from pytorch_rt1_for_distributed_training_amd.utils.checkpoint import build_checkpoint, save_checkpoint
    ops = _ops()
    cfg = _cfg()
    batches = _batches(cfg, 3)
    run = _engine(cfg)
    for b in batches[:2]:
        run.train_step(b)
    torch.cuda.synchronize()
    path = str(tmp_path / "adam.ckpt")
    save_checkpoint(path, build_checkpoint(run.model, run.optimizer, run.scheduler, epoch=0,
                                           global_step=run.global_step))
    fresh = _engine(cfg, optimizer="lamb")
    Trainer(fresh, verbose=False).resume(path)
    opt = fresh.optimizer
    assert opt.step_count == 2 and fresh.global_step == 2
    assert torch.equal(fresh.flat.data, run.flat.data)
    assert torch.equal(opt.exp_avg, run.optimizer.exp_avg) and torch.equal(opt.exp_avg_sq, run.optimizer.exp_avg_sq)
    ref = [t.double().clone() for t in (fresh.flat.data, opt.exp_avg, opt.exp_avg_sq)]
    fresh.train_step(batches[2])
    torch.cuda.synchronize()
    assert opt.step_count == 3 and float(opt.dev_state[0]) == 3.0
    trust, norms = ops.reference_lamb_step(ref[0], fresh.flat.grad.double(), ref[1], ref[2],
                                           opt.tensor_chunk_start.tolist(), opt.tensor_adapt.tolist(), lr=5e-4,
                                           beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=ENGINE_WD, step=3,
                                           grad_scale=fresh.ddp.grad_scale)
    for got, want, atol, what in zip((fresh.flat.data, opt.exp_avg, opt.exp_avg_sq), ref, (1e-6, 1e-7, 1e-8), "pmv"):
        _close(got, want, 1e-5, atol, f"first LAMB step after an Adam checkpoint, {what}")
    _close(opt.trust, trust, 1e-5, 0.0, "first LAMB step after an Adam checkpoint, trust")


def test_default_engine_builds_no_lamb_tensor_and_calls_no_lamb_op():
    adam = _ops()
    cfg = _cfg()
    batches = _batches(cfg, 2)
    with mock.patch.object(adam, "flat_lamb_dev_step", wraps=adam.flat_lamb_dev_step) as step, \
            mock.patch.object(adam, "lamb_tables", wraps=adam.lamb_tables) as tables, \
            mock.patch.object(adam, "flat_adam_dev_step", wraps=adam.flat_adam_dev_step) as adam_step:
        eng = _engine(cfg)
        for b in batches:
            eng.train_step(b)
        torch.cuda.synchronize()
    opt = eng.optimizer
    assert opt.trust is None and opt.norms is None and opt.chunk_sums is None and opt.tensor_chunk_start is None
    assert opt.chunk_tensor is None and opt.tensor_adapt is None and opt.kind == "adam"
    assert step.call_count == 0 and tables.call_count == 0 and adam_step.call_count == 2
    assert set(opt.state_dict()) == {"state", "param_groups"}
    # and with the option on the Adam op is not launched
    with mock.patch.object(adam, "flat_lamb_dev_step", wraps=adam.flat_lamb_dev_step) as step, \
            mock.patch.object(adam, "flat_adam_dev_step", wraps=adam.flat_adam_dev_step) as adam_step:
        on = _engine(cfg, optimizer="lamb")
        on.train_step(batches[0])
        torch.cuda.synchronize()
    assert step.call_count == 1 and adam_step.call_count == 0
