"""The regularised action head on the GPU (csrc/kernels/head.hip: head_ce_loss_fwd_kernel, head_token_hits_kernel)
against the element-wise fp64 oracle of tests/head_loss_oracle.py, against the plain head_ce_fwd bit for bit where the
two must agree, through the autograd function, and through a one-GPU engine with the captured step.  Run with -s for
one line per kernel case."""
import pytest
import torch

import decoder_oracle as do
import gemm_oracle as gm
import head_loss_oracle as ho

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
DEV = "cuda"
EPS, ZETA = 0.1, 1e-4


@pytest.fixture(scope="module")
def ext():
    from pytorch_rt1_for_distributed_training_amd import ops
    return ops.load()


@pytest.fixture(scope="module")
def plain(ext):
    """head_ce_fwd's outputs and the operands of every (V, R) of the grid, computed once and left unchanged."""
    out = {}
    for V in ho.VOCABS:
        for R in ho.HEAD_R:
            ops, _ = ho.head_inputs(V, R, ho.gen(V, R), DEV)
            out[V, R] = (ops, ext.head_ce_fwd(*ops))
    return out


def test_operands_are_the_decoder_oracle_tests(plain):
    import test_decoder_oracle_gpu as t
    assert (t.HEAD_R, t.HEAD_S) == (ho.HEAD_R, ho.HEAD_S)
    for V, R in ((256, 1), (512, 17), (1024, 90)):
        theirs, _ = t.head_inputs(V, R, t.gen(V, R))
        assert all(torch.equal(a, b) for a, b in zip(theirs, plain[V, R][0]))


@pytest.mark.parametrize("R", sorted(ho.HEAD_R))
@pytest.mark.parametrize("V", ho.VOCABS)
def test_kernel_grid_against_the_oracle_and_the_plain_kernel(ext, plain, V, R):
    (hidden, pos, W, bias, target), (ce0, pred0, G0, hb0) = plain[V, R]
    assert int(target.min()) == 0 or int(target.max()) == V - 1
    for eps, zeta in ho.OBJECTIVES:
        name = f"V{V} R{R} eps {eps} zeta {zeta}"
        loss, ce, pred, G, hb = ext.head_ce_loss_fwd(hidden, pos, W, bias, target, eps, zeta)
        again = ext.head_ce_loss_fwd(hidden, pos, W, bias, target, eps, zeta)
        r = ho.ref_head_loss(hb, W, bias, target, eps, zeta)
        rl, rg = ho.ratios(loss, G, r)
        print(f"\nhead loss oracle | {name:40s} | loss / bound {rl:8.5f} | G / bound {rg:6.3f}", end="")
        ho.check_head_loss(loss, ce, G, r, name)
        assert torch.equal(ce, ce0) and torch.equal(pred, pred0) and torch.equal(hb, hb0), \
            f"{name}: ce / pred / hb are not head_ce_fwd's bits"
        assert all(torch.equal(u, v) for u, v in zip((loss, ce, pred, G, hb), again)), f"{name}: no bitwise repeat"
        assert not torch.equal(G, G0) and not torch.equal(loss, ce)


@pytest.mark.parametrize("V", ho.VOCABS)
def test_zero_options_reproduce_the_plain_kernel_bit_for_bit(ext, plain, V):
    ops, (ce0, pred0, G0, hb0) = plain[V, 17]
    loss, ce, pred, G, hb = ext.head_ce_loss_fwd(*ops, 0.0, 0.0)
    assert torch.equal(ce, ce0) and torch.equal(pred, pred0) and torch.equal(G, G0) and torch.equal(hb, hb0)
    assert torch.equal(loss, ce)


@pytest.mark.parametrize("bad", [(1.0, 0.0), (-0.1, 0.0), (0.0, -1e-4), (float("nan"), 0.0), (0.0, float("nan")),
                                 (0.0, float("inf"))])
def test_binding_refuses_bad_options(ext, plain, bad):
    with pytest.raises(RuntimeError, match="label_smoothing|z_loss"):
        ext.head_ce_loss_fwd(*plain[256, 1][0], *bad)


def test_autograd_function_gradients_against_fp64_autograd(ext):
    """HeadCEFn with the options at B = 5, T = 6 and the model's positions (R = 90).  The loss and the plain CE are held
    to the oracle.  The gradients of hidden, W and bias are held twice:
      * as products, the way the decoder oracle tests hold theirs: against the fp64 product of the STORED bf16 operands
        (dz = head_ce_scale(G, dce), which is deterministic, so the test recomputes the bits the backward used) through
        gemm_oracle.assert_gemm / assert_f32, reduction lengths V (dh) and R (dW, dbias);
      * end to end against fp64 autograd of the objective on the bf16-rounded operands, with the operand's own error
        carried into the bound: the stored dz is off the fp64 dz by e_dz = dce bound_G + REL |dz| (the oracle's bound
        of G, then the one bf16 rounding of the scale kernel), which reaches a product through the other operand's
        absolute values.
    The gradient of hidden is exactly 0 on the unscored positions."""
    from pytorch_rt1_for_distributed_training_amd.models.transformer import action_prediction_positions
    from pytorch_rt1_for_distributed_training_amd.ops.head import head_ce
    torch.manual_seed(7)
    B, T, K, A, V, E = 5, 6, 8, 3, 256, 512
    S = T * (K + A)
    lin = torch.nn.Linear(E, V).to(DEV)
    hidden = torch.randn(B, S, E, device=DEV, requires_grad=True)
    pos = action_prediction_positions(T, K, A).to(DEV)
    targets = torch.randint(0, V, (B, T * A), device=DEV)
    t32 = targets.reshape(-1).int()
    R = B * T * A
    loss, pred, nll = head_ce(lin, hidden, pos, targets, None, EPS, ZETA)
    assert loss.requires_grad and not nll.requires_grad and not pred.requires_grad and loss.shape == (R,)
    Wb = lin.weight.detach().to(BF)
    bias = lin.bias.detach()
    _, _, pred2, G, hb = ext.head_ce_loss_fwd(hidden.detach(), pos.int(), Wb, bias, t32, EPS, ZETA)
    assert torch.equal(hb, hidden.detach()[:, pos].reshape(R, E).to(BF)) and torch.equal(pred, pred2)
    r = ho.ref_head_loss(hb, Wb, bias, t32, EPS, ZETA)
    do.check_f32(loss.detach(), r["loss"], r["bound_loss"], "HeadCEFn loss")
    do.check_f32(nll, r["ce"], r["bound_ce"], "HeadCEFn nll")
    do.check_bf16(G, r["G"], r["bound_G"], "HeadCEFn G", None, r["S_G"])
    w = torch.rand(R, device=DEV) + 0.5
    (loss * w).sum().backward()
    dh = hidden.grad[:, pos].reshape(R, E)
    dW, db = lin.weight.grad, lin.bias.grad
    assert torch.equal(dh.to(BF).float(), dh)
    # ---- products of the stored operands
    dz = ext.head_ce_scale(G, w).double()
    Wd, hd = Wb.double(), hb.double()
    gm.assert_gemm(dh.to(BF), dz @ Wd, dz.abs() @ Wd.abs(), V, "HeadCEFn dh = dz W")
    gm.assert_f32(dW, dz.t() @ hd, dz.abs().t() @ hd.abs(), R, "HeadCEFn dW = dz^T hb")
    gm.assert_f32(db, dz.sum(0), dz.abs().sum(0), R, "HeadCEFn dbias = colsum dz")
    # ---- end to end against fp64 autograd on the bf16-rounded operands
    h64, W64, b64 = hd.clone().requires_grad_(True), Wd.clone().requires_grad_(True), bias.double().requires_grad_(True)
    z = h64 @ W64.t() + b64
    ref = (torch.nn.functional.cross_entropy(z, targets.reshape(-1), reduction="none", label_smoothing=ho.f32(EPS))
           + ho.f32(ZETA) * torch.logsumexp(z, 1) ** 2)
    (ref * w.double()).sum().backward()
    dz64 = r["G"] * w.double()[:, None]
    e_dz = r["bound_G"] * w.double()[:, None] + do.REL * dz64.abs() + do.U32 * dz64.abs()
    sl = do.slack
    gm.assert_within(dh.to(BF), h64.grad, do.REL * h64.grad.abs() + sl(V) * (dz64.abs() @ Wd.abs()) + e_dz @ Wd.abs(),
                     "HeadCEFn dhidden vs autograd")
    gm.assert_within(dW, W64.grad, do.U32 * W64.grad.abs() + sl(R) * (dz64.abs().t() @ hd.abs()) + e_dz.t() @ hd.abs(),
                     "HeadCEFn dW vs autograd")
    gm.assert_within(db, b64.grad, do.U32 * b64.grad.abs() + sl(R) * dz64.abs().sum(0) + e_dz.sum(0),
                     "HeadCEFn dbias vs autograd")
    untouched = torch.ones(S, dtype=torch.bool, device=DEV)
    untouched[pos] = False
    assert float(hidden.grad[:, untouched].abs().max()) == 0.0


@pytest.mark.parametrize("A", [1, 3])
@pytest.mark.parametrize("R", [1, 17, 2304])
def test_token_hits_kernel_counts_exactly_and_accumulates(ext, A, R):
    g = torch.Generator().manual_seed(A * 10007 + R)
    pred = torch.randint(0, 3, (R,), generator=g, dtype=torch.int32).to(DEV)
    target = torch.randint(0, 3, (R,), generator=g, dtype=torch.int32).to(DEV)
    counters = torch.zeros(A, 2, dtype=torch.int64, device=DEV)
    slot = torch.arange(R, device=DEV) % A
    for calls in (1, 2):
        ext.head_token_hits_(pred, target, counters)
        want = torch.stack([torch.stack([(pred == target)[slot == a].sum(), (slot == a).sum()]) for a in range(A)])
        assert torch.equal(counters, calls * want), (A, R, calls, counters.tolist(), want.tolist())


def test_token_hits_from_the_kernels_own_predictions(ext, plain):
    (hidden, pos, W, bias, target), _ = plain[256, 90]
    _, _, pred, _, _ = ext.head_ce_loss_fwd(hidden, pos, W, bias, target, EPS, ZETA)
    target = torch.where(torch.arange(90, device=DEV) % 2 == 0, pred, target)      # some hits for certain
    counters = torch.zeros(3, 2, dtype=torch.int64, device=DEV)
    ext.head_token_hits_(pred, target, counters)
    slot = torch.arange(90, device=DEV) % 3
    assert counters[:, 0].tolist() == [int((pred == target)[slot == a].sum()) for a in range(3)]
    assert counters[:, 1].tolist() == [30, 30, 30] and int(counters[:, 0].sum()) >= 45


# ---------------------------------------------------------------------------------------------------- one-GPU engine
QUIET = dict(dropout_rate=0.0, drop_connect_rate=0.0, crop_ratio=0.0)      # no random draw: two engines can interleave


def _engine(cfg, graph, fresh=True, **kw):
    from pytorch_rt1_for_distributed_training_amd.engine.step import TrainEngine
    from pytorch_rt1_for_distributed_training_amd.models import build_rt1
    from pytorch_rt1_for_distributed_training_amd.ops import rng
    if fresh:
        rng._COUNTERS.clear()
    torch.manual_seed(0)
    return TrainEngine(build_rt1(cfg), cfg, order_probe=False, graph=graph, **kw)


def test_engine_graph_step_counts_and_eval_stays_plain():
    from test_graph_gpu import _batches, _cfg
    cfg = _cfg()
    eng = _engine(cfg, True, label_smoothing=EPS, z_loss=ZETA, token_accuracy=True)
    assert eng.model.fused.fused_head
    bs = _batches(cfg, 4)
    A = eng.model._tokens_per_action
    rows = 4 * cfg.seq_len                                     # rows per slot and step (b = 4)
    eng.train_step(bs[0])                                      # eager step + capture
    assert eng._graph is not None
    eng.train_step(bs[1])                                      # one replay
    torch.cuda.synchronize()
    before, nll_before = eng.token_counters.clone(), eng.last_nll.clone()
    assert before[:, 1].tolist() == [2 * rows] * A
    res = eng.graph_eager_check(bs[2])
    assert res is not None and res["equal"], res
    assert torch.equal(eng.token_counters, before)             # the check leaves the counters as it found them
    assert torch.equal(eng.last_nll, nll_before)               # ... and the last step's nll
    eng.read_token_counters()
    for b in bs[1:]:
        eng.train_step(b)                                      # three replays
    c = eng.read_token_counters()
    assert c[:, 1].tolist() == [3 * rows] * A and int(c[:, 1].sum()) == 3 * rows * A
    assert bool((c[:, 0] <= c[:, 1]).all()) and eng.last_nll is not None
    assert float(eng.last_nll) != float(eng._static_loss)
    # eval: the plain CE, bitwise that of an engine without the options on the same weights
    off = _engine(cfg, False)
    with torch.no_grad():
        off.flat.data.copy_(eng.flat.data)
        for a, b in zip(off.model.buffers(), eng.model.buffers()):
            a.copy_(b)
    losses = []
    for e in (eng, off):
        torch.manual_seed(11)                                  # the random crop shift is drawn in eval mode too
        losses.append(e.eval_step(bs[3]))
    assert torch.equal(*losses)
    assert eng.read_token_counters()[:, 1].tolist() == [rows] * A      # validation counts as well


def test_last_nll_is_the_steps_own_figure_across_capture_and_replay():
    """The capturing step runs eagerly and then records a second forward whose nll tensor nothing has written yet:
    last_nll must stay the eager figure.  After a replay it is the plain CE of the replayed batch.  The yardstick is an
    engine that never captures, on the same batches (no dropout, drop-path or shift, so the two can interleave)."""
    from test_graph_gpu import _batches, _cfg
    cfg = _cfg(**QUIET)
    eng = _engine(cfg, True, label_smoothing=EPS, z_loss=ZETA)
    ref = _engine(cfg, False, fresh=False, label_smoothing=EPS, z_loss=ZETA)
    bs = _batches(cfg, 3)
    l0, r0 = eng.train_step(bs[0]), ref.train_step(bs[0])     # eager step + capture
    assert eng._graph is not None and eng._static_nll is not None
    assert torch.equal(l0, r0) and torch.equal(eng.last_nll, ref.last_nll)
    for b in bs[1:]:                                           # replays
        lg, le = eng.train_step(b), ref.train_step(b)
        assert torch.equal(lg, le) and torch.equal(eng.last_nll, ref.last_nll)
        assert eng.last_nll is not eng._static_nll and float(eng.last_nll) != float(lg)


def test_failed_capture_keeps_the_eager_nll():
    """A capture that raises leaves last_nll the eager step's value, and the engine goes on eagerly."""
    from test_graph_gpu import _batches, _cfg
    cfg = _cfg(**QUIET)
    eng = _engine(cfg, True, label_smoothing=EPS, z_loss=ZETA)
    ref = _engine(cfg, False, fresh=False, label_smoothing=EPS, z_loss=ZETA)
    bs = _batches(cfg, 2)
    body, calls = eng._step_body, []

    def step_body(batch):
        calls.append(1)
        if len(calls) == 2:                                    # the call under capture, before it records anything
            eng.last_nll = torch.full((), float("nan"), device=DEV)
            raise RuntimeError("capture failure forced by the test")
        return body(batch)

    eng._step_body = step_body
    l0, r0 = eng.train_step(bs[0]), ref.train_step(bs[0])
    assert len(calls) == 2 and not eng.graph and eng._graph is None
    assert torch.equal(l0, r0) and torch.equal(eng.last_nll, ref.last_nll)
    l1, r1 = eng.train_step(bs[1]), ref.train_step(bs[1])
    assert torch.equal(l1, r1) and torch.equal(eng.last_nll, ref.last_nll)


def test_token_hits_takes_the_kernel_for_any_integer_rows(ext, monkeypatch):
    """ops.head.token_hits_ on GPU counters: int64 rows are converted and counted by the kernel, never by torch, and
    more than 32 slots are refused."""
    from pytorch_rt1_for_distributed_training_amd.models import policy
    from pytorch_rt1_for_distributed_training_amd.ops.head import token_hits_

    def no_torch(*a):
        raise AssertionError("the torch count ran for GPU counters")

    monkeypatch.setattr(policy, "token_hits_torch_", no_torch)
    pred = torch.tensor([[1, 2, 3], [1, 0, 3]], device=DEV)                      # int64 (b, A)
    target = torch.tensor([[1, 2, 0], [0, 0, 3]], device=DEV)
    counters = torch.zeros(3, 2, dtype=torch.int64, device=DEV)
    token_hits_(counters, pred, target.int())
    assert counters.tolist() == [[1, 2], [2, 2], [1, 2]]
    with pytest.raises(ValueError, match="32"):
        token_hits_(torch.zeros(33, 2, dtype=torch.int64, device=DEV), pred, target)


def test_default_engine_runs_the_plain_kernel_only(monkeypatch):
    from test_graph_gpu import _batches, _cfg
    from pytorch_rt1_for_distributed_training_amd.ops import head
    real = head.load()
    calls = []

    class Spy:
        def __getattr__(self, name):
            if name.startswith("head_"):
                calls.append(name)
            return getattr(real, name)

    monkeypatch.setattr(head, "load", lambda: Spy())
    cfg = _cfg()
    eng = _engine(cfg, False)
    b = _batches(cfg, 1)[0]
    eng.train_step(b)
    eng.eval_step(b)
    assert "head_ce_fwd" in calls
    assert "head_ce_loss_fwd" not in calls and "head_token_hits_" not in calls
    assert eng.token_counters is None and eng.last_nll is None
