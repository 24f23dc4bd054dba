"""GEMM and weight-gradient dispatch (ops/linear.py planners) on the CPU against the recorded decisions of the
dispatchers they replaced: backbone._lin / _lin_bn / wgrad / wgrad_bmm / gram_moments and attention._proj / _wgrad /
_wgrad_bias.  tests/fixtures/gemm_plans.txt holds one line per query of ``queries()``; it was recorded at the commit
before ops/linear.py existed, from what those dispatchers called, and is never regenerated from the code under test.
The capability queries are host functions of the extension: no GPU."""
import dataclasses
import os

import pytest

from pytorch_rt1_for_distributed_training_amd.config import preset
from pytorch_rt1_for_distributed_training_amd.models.efficientnet import block_specs, conv_out_size
from pytorch_rt1_for_distributed_training_amd.ops import _ext
from test_backbone_gpu import BLOCKS_NHW

pytestmark = pytest.mark.skipif(not _ext.available(), reason="HIP extension not built (python build.py)")

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fixtures", "gemm_plans.txt")
# the leaf switches, off one at a time, for the planners that read them
FLAG_SETS = {"product": ("default", "pw_tall=0", "g256=0"), "wgrad": ("default", "wgrad_mfma=0"),
             "gram": ("default", "wgrad_mfma=0", "gram_sx=0")}
STEP = (768, 150, 150, 128)         # the benchmark: frames, block 0's input, decoder batch
SMALL = (*BLOCKS_NHW, 2)            # the per-block GPU test's shape; the decoder at batch 2


def queries():
    """Every distinct query the call sites of MBConvFn, TopFn, expand_bwd_z_wide, the TokenLearner, the decoder layers,
    the embedding and the action head make at the two sizes, as sorted tuples (planner, ints...)."""
    cfg = preset("full")
    q = set()

    def conv(M, K, N, pro=False):           # forward product (plain, + BN in training / eval), dgrad, weight gradient
        q.update(("product", M, K, N, stats, p) for stats in (0, 1) for p in ({0, int(pro)}))
        q.add(("product", M, N, K, 0, 0))
        q.update(("wgrad", M, N, K, form) for form in ("plain", "raw"))

    for N, H, W, B in (STEP, SMALL):
        for sp in block_specs():
            H2, W2 = conv_out_size(H, sp.kernel, sp.stride), conv_out_size(W, sp.kernel, sp.stride)
            if sp.expand_ratio != 1:
                conv(N * H * W, sp.in_ch, sp.expand_ch)
                q.add(("gram", N * H * W, sp.in_ch))
            conv(N * H2 * W2, sp.expand_ch, sp.out_ch, pro=_ext.load().pw_gemm_supported(sp.expand_ch, sp.out_ch))
            H, W = H2, W2
        conv(N * H * W, sp.out_ch, 1536)                                            # TopFn
        conv(N * H * W, 1536, cfg.token_embedding_size)
        q.update(("wgrad", N * H * W, 64, cfg.token_embedding_size, form) for form in ("plain", "raw"))  # TokenLearner
        E, HD = cfg.feed_forward_size, cfg.num_heads * cfg.layer_size
        T = B * cfg.seq_len * (cfg.num_image_tokens + cfg.tokens_per_action)
        for K, N in ((HD, E), (E, E)):                                              # out projection, FF / embedding
            q.update({("token_product", T, K, N, 0), ("token_product", T, N, K, 1), ("token_wgrad", T, N, K, 0)})
        q.update({("token_product", T, 3 * HD, E, 1), ("token_wgrad", T, 3 * HD, E, 1)})      # fused Q/K/V
        q.add(("token_wgrad", B * cfg.seq_len * cfg.tokens_per_action, cfg.vocab_size, E, 0))  # action head
    return sorted(q)


def lines(plan):
    """``plan(planner, args, flag set) -> plan``: the fixture's lines, one per query and flag set."""
    out = []
    for name, *args in queries():
        for fs in FLAG_SETS.get(name, ("default",)):
            p = plan(name, args, fs)
            out.append(f"{name} {' '.join(map(str, args))} [{fs}] : {' '.join(map(str, dataclasses.astuple(p)))}")
    return out


def plan_now(name, args, fs):
    from pytorch_rt1_for_distributed_training_amd.ops import linear, switches
    flags = linear.RouteFlags.from_switches(switches.DEFAULTS.__getitem__)
    if fs != "default":
        flags = dataclasses.replace(flags, **{fs.split("=")[0]: False})
    if name == "product":
        M, K, N, stats, pro = args
        return linear.plan_product(M, K, N, bool(stats), bool(pro), flags)
    if name == "wgrad":
        return linear.plan_wgrad(*args[:3], flags)
    if name == "gram":
        return linear.plan_wgrad(args[0], args[1], args[1], flags, gram=True)
    if name == "token_product":
        return linear.plan_token_product(*args[:3], bool(args[3]))
    return linear.plan_token_wgrad(*args[:3], bool(args[3]))


@pytest.mark.skipif(bool(os.environ.get("RT1_AB")), reason="the decoder's switches are import-time constants")
def test_plans_match_recorded_decisions():
    with open(FIXTURE) as f:
        want = [ln for ln in f.read().splitlines() if not ln.startswith("#")]
    got = lines(plan_now)
    assert len(want) > 500
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"first differing query, line {i + 1}:\n  recorded: {w}\n  now:      {g}"
    assert len(got) == len(want), f"{len(got)} queries now, {len(want)} recorded"


# (planner, kind, stats or sums) of every value a planner can return
KINDS = {("product", k, s) for k in ("pw_gemm", "pw_tall", "library") for s in ("none", "bn_stats")} | {
    ("product", "pw_gemm", "epilogue"), ("product", "g256", "epilogue"),
    ("token_product", "gemm_hip", "none"), ("token_product", "library", "none")} | {
    ("wgrad", k, "none") for k in ("mfma", "mfma_auto", "bmm", "mm")} | {
    ("gram", "mfma", "kernel"), ("gram", "mfma_auto", "kernel")} | {
    ("gram", k, "colsum") for k in ("mfma", "mfma_auto", "bmm", "mm")} | {
    ("token_wgrad", k, s) for k in ("mfma", "mfma_auto") for s in ("none", "kernel")} | {
    ("token_wgrad", "mm", "none"), ("token_wgrad", "mm", "colsum")}
# ... and those that no call site reaches at either size, in the recording itself
NOT_REACHED = {
    # the decoder's automatic split is for more than 65,536 token rows; the benchmark has 8,448
    ("token_wgrad", "mfma_auto", "none"): "M > 65536", ("token_wgrad", "mfma_auto", "kernel"): "M > 65536",
    # every Linear of the decoder and the head is bf16 with channels % 8 == 0 and tf_wgrad is on
    ("token_wgrad", "mm", "none"): "channels % 8", ("token_wgrad", "mm", "colsum"): "channels % 8",
}


def test_recording_reaches_every_plan_kind():
    seen = set()
    with open(FIXTURE) as f:
        for ln in f.read().splitlines():
            if not ln.startswith("#"):
                query, _, plan = ln.partition(" : ")
                seen.add((query.split()[0], plan.split()[0], plan.split()[-1]))
    assert not seen - KINDS, seen - KINDS
    assert KINDS - seen == set(NOT_REACHED), (KINDS - seen, set(NOT_REACHED))
