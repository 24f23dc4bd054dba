"""Fused HIP implementation of the FiLM-EfficientNet-B3 image encoder (reference:
``film_efficientnet/film_efficientnet_encoder.py:142-224``; ``models.efficientnet.MBConvBlock`` is the eager oracle).

Activations are channels-last bf16 ``[N, H, W, C]`` (N = b*t frames) end to end; BatchNorm statistics, running stats
and every reduction are fp32/fp64 with a fixed summation order.  Per MBConv block:

forward   y1 = x @ We^T + BN1 constants  expand 1x1
          y2 = dwconv(silu(bn1(y1)))    dw_fwd_kernel (dw_fwd.hip): BN1+SiLU prologue while staging the tile, BN2
                                         partials epilogue
          s  = SE(mean_hw silu(bn2(y2))) frame_pool + fp32 fc1 / SiLU / fc2 / sigmoid
          y3 = (silu(bn2(y2)) * s) @ Wp^T project 1x1 + BN3 constants
          out = (bn3(y3)*keep + x) * (1+gamma_film) + beta_film      block_tail
backward  tail_bwd_reduce (FiLM grads + BN3 partials) -> BN3 backward-apply -> dA = dy3 @ Wp, dWp, SE / BN2 sums
          SE backward, BN2 backward-apply + depthwise data and weight gradients + BN1-backward partials
          BN1 backward + expand data and weight gradients, residual gradient

Which kernels run each stage of a block is decided once, by ``plan_block`` (a ``BlockRoute``: one short string per
stage), from the block's shape and the ``RouteFlags`` read from ops/switches.py; the forward plans, the backward reads
the plan.  The comments on ``RouteFlags`` (ops/linear.py, with the planners and executors of every 1x1-conv product and
weight gradient) say what each path is and which log decided its default.

Saved per block: x, y2, y3 (bf16), y1 only outside x-mode, A only when the project backward needs it, the SE vectors
(pool, h, gate) and per-channel constants.
"""
from __future__ import annotations

import functools
import os
from dataclasses import dataclass
from typing import List, Optional

import torch
import torch.nn.functional as F

from ._ext import load
from .linear import (FLAGS, Product, RouteFlags, _GEMM_PROJ_DGRAD_TILE, _GEMM_PROJ_TILE, _Z_GEMM_TILE, _bf, _partials,
                     _pw_blocks, gram_moments, lin, lin_bn, wgrad, wgrad_mfma_preferred)

ACT_NONE, ACT_SILU = 0, 1
MAX_BLOCKS = 2048   # ~8 workgroups per CU on 256 CUs: upper bound for persistent tile loops / partial rows
BF = torch.bfloat16


def _ext():
    return load()


# per-(map side, channels) grid cap of the fused depthwise backward where the per-site sweep beat MAX_BLOCKS by more
# than its ~2 % noise (profiles/r5_grid_sites.log: 38x38x288 1328 -> 1277 us, 38x38x192 1484 -> 1423, 19x19x288
# 574 -> 537, 19x19x576 686 -> 661)
_DW_BWD_BLOCKS = {(38, 288): 1024, (38, 192): 512, (19, 288): 512, (19, 576): 256}
# ... and of the stem forward / weight gradient and block 2's y1-free depthwise pair (same sweep: stem 527 -> 509 and
# 782 -> 760 us, dw_fwd_x 1900 -> 1832 us, dw_bwd_fused_x 3773 -> 3734 us)
STEM_FWD_BLOCKS, STEM_BWD_BLOCKS, XMODE_BLOCKS = 3072, 1536, 4096
# RT1_BLOCK_TIMING=1: HIP events around every block's forward / backward (tools/block_timing.py)
_TIMING = os.environ.get("RT1_BLOCK_TIMING", "0") == "1"
TIMING_EVENTS: List = []


def _mark(name: str):
    if _TIMING:
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        TIMING_EVENTS.append((name, ev))


def _pw_bwd_blocks(M: int, z: bool = False) -> int:
    """Grid cap of the fused expand backward (pwbwd.hip), from sweeps at 768 frames
    (tools/scratch/pwbwd_grid_sweep.py, profiles/r2_pwbwd_grid_sweep.log): the 150x150 block wants 4096
    workgroups (-14 % vs 512), the 75x75 ones 2048 (-6 %), the 38x38 ones 512.  The y-free kernel (pw_bwd_z,
    tools/scratch/pwbwd_z_grid_sweep.py, profiles/r2_pwbwd_z_grid_sweep.log): flat from 1024 up at 150x150, 3072 at
    75x75 (-4..-5 % vs 2048), 512 at 38x38."""
    if M >= 10_000_000:
        return 4096
    if M >= 3_000_000:
        return 3072 if z else 2048
    return 512


def _dw_wgrad_blocks(C: int) -> int:
    """Grid cap of the depthwise weight-gradient kernel (``tools/gpu_wgb.sh`` sweep, partial-row sum
    included): the <= 144-channel high-resolution layers keep improving up to 4096 workgroups (-12 % vs 1024),
    the wider ones are flat from 1024 to 2048."""
    return 4096 if C <= 144 else 2048


# RT1_SE_DEBUG=1 (tools/dp_gpu_check.py): the fused SE forward keeps copies of (pool, h, gate); the backward flags any
# of them changed since the forward and re-runs se_bwd on the same inputs to flag a non-reproducible output.  Flags
# are device booleans collected in SE_DEBUG_LOG (eager steps only, never inside a capture).
_SE_DEBUG = os.environ.get("RT1_SE_DEBUG", "0") == "1"
SE_DEBUG_LOG: List = []
_SE_NAMES = ("dw2", "db2", "dw1", "db1", "rb", "db2bn", "dg2", "mdz2", "mdzx2")


def _se_debug_check(ext, index: int, saved, args, outs):
    """RT1_SE_DEBUG: inputs changed since the forward?  Re-run se_bwd on the same inputs: which outputs differ?  On a
    dw1 difference (host-synchronous): how many distinct (row, column) positions, and how many distinct results over
    8 more re-runs; RT1_SE_DUMP=<dir> also saves the inputs and both outputs for an offline replay."""
    red, gate, h, pool = args[:4]
    for nm, a, b in (("pool", pool, saved[0]), ("h", h, saved[1]), ("gate", gate, saved[2])):
        SE_DEBUG_LOG.append((f"blk{index}.{nm}", (a != b).sum()))
    rerun = ext.se_bwd(*args)
    for nm, a, b in zip(_SE_NAMES, outs, rerun):
        SE_DEBUG_LOG.append((f"blk{index}.{nm}_rerun", (a != b).sum()))
    bad = outs[2] != rerun[2]
    if not bool(bad.any()):
        return
    where = bad.nonzero()
    SE_DEBUG_LOG.append((f"blk{index}.dw1_bad_rows", int(where[:, 0].unique().numel())))
    SE_DEBUG_LOG.append((f"blk{index}.dw1_bad_cols", int(where[:, 1].unique().numel())))
    results = [outs[2], rerun[2]] + [ext.se_bwd(*args)[2] for _ in range(8)]
    distinct = []
    for r in results:
        if not any(torch.equal(r, d) for d in distinct):
            distinct.append(r)
    SE_DEBUG_LOG.append((f"blk{index}.dw1_distinct_of_10", len(distinct)))
    SE_DEBUG_LOG.append((f"blk{index}.dw1_first_eq_later", sum(torch.equal(outs[2], r) for r in results[2:])))
    dump = os.environ.get("RT1_SE_DUMP")
    if dump:
        os.makedirs(dump, exist_ok=True)
        rank = int(os.environ.get("RANK", "0"))
        torch.save({"args": [a.detach().cpu() if torch.is_tensor(a) else a for a in args],
                    "first": outs[2].cpu(), "rerun": rerun[2].cpu()},
                   os.path.join(dump, f"se_r{rank}_b{index}_{len(os.listdir(dump))}.pt"))


class StemLink:
    """Side channel from block 0's backward to StemPreFn's backward (both run in the same autograd pass; x's only
    consumer is block 0, so the tensor block 0 returns for x reaches the stem unchanged)."""

    def __init__(self):
        self.bn = None


def gram_bn_preferred(Cin: int, Ce: int, flags: RouteFlags = FLAGS) -> bool:
    """BN1 of this expand conv from the block input's Gram moments (RouteFlags.gram_bn); plan_block's test."""
    ext = _ext()
    return (flags.gram_bn and Cin % 8 == 0 and not ext.pw_stats_supported(Cin, Ce) and ext.pw_gemm_supported(Cin, Ce)
            and (flags.wgrad_mfma and wgrad_mfma_preferred(1 << 20, Cin, Cin)))


def gram_bn_consts(x2d: torch.Tensor, We_b: torch.Tensor, bnc: "BNCtx"):
    """Train-mode BN1 constants of y1 = x2d @ We_b^T from x2d alone: G = x^T x and sum x in one MFMA pass, the
    quadratic forms in fp64 (csrc/kernels/xexpand.hip); running stats updated in place."""
    bn = bnc.bn
    return tuple(_ext().x_bn_stats(x2d, We_b, bn.weight, bn.bias, bn.eps, bn.momentum, bn.running_mean,
                                   bn.running_var))


def _few_splits(part: torch.Tensor) -> torch.Tensor:
    """Split partials [S, Co, Ci] as they are for S <= 4 (the consumer sums them), else their fixed-order colsum: a
    per-element loop over the 64-256 splits of the tall z-mode gradients made pw_z_finish latency-bound (40 -> 174 us
    for the 19x19 blocks, gpurun_out/trN vs trN_film)."""
    return part if part.shape[0] <= 4 else _ext().colsum(part)


def expand_bwd_z_wide(dz: torch.Tensor, x: torch.Tensor, We: torch.Tensor, consts: torch.Tensor, res=None, gram=None,
                      dgrad: str = "z_wide"):
    """Expand-conv backward of a wide block from dz [M, Ce] and the block input x [M, Cin] (y1 is not read):
    dx = dz @ (diag(k1) We) + x @ Mk + r0 and dWe = diag(k1) dz^T x + diag(k2) We G + k0 (x) sx with
    Mk = We^T diag(k2) We, G = x^T x, sx = sum_m x (csrc/kernels/pwbwd.hip pw_z_prep / pw_z_finish, pwtall.hip
    pw_tall_tail).  Replaces bn_bwd_apply (read dA1 and y1, write dy1) + the dgrad / wgrad reads of dy1 by two
    reads of dz and three of the 6x narrower x.  ``res = (dout, fmul, hw)`` adds the residual path's gradient
    dout * fmul[frame] in the dgrad epilogue (no add_scaled_ pass).  ``dgrad="z_gemm"``: the data gradient as one
    two-segment GEMM on gemm.hip (csrc/kernels/gemm.hip TAIL) instead of pw_tall_tail."""
    ext = _ext()
    wt, mk, r0 = ext.pw_z_prep(We, consts)     # (diag(k1) We)^T [Cin, Ce], We^T diag(k2) We, k0 @ We in one launch
    if dgrad == "z_gemm":
        dx = ext.gemm_tail(dz, wt, x, mk, r0, *(res or ()), cfg=_Z_GEMM_TILE.get((We.shape[0], We.shape[1]), -1))
    else:
        dx = ext.pw_tall_tail(dz, wt, x, mk, r0, *(res or ()))
    S = _few_splits(wgrad(dz, x, raw=True))  # up to 4 split partials are summed inside pw_z_finish
    G, sx = gram if gram is not None else gram_moments(x)     # from the forward's BN1 when it used them
    return dx, ext.pw_z_finish(S, G, sx, We, consts)


# shapes the wide dz-mode path does not pay for (filled from A/B runs)
_Z_WIDE_OFF = set()


@dataclass(frozen=True)
class BlockRoute:
    """The kernels one MBConv block runs, stage by stage (``plan_block``)."""
    # "gemm" / "library" below: the product planner's choice (ops/linear.py plan_product), the statistics with it
    bn1: str            # BN1 from: "xmode" | "gram" (training) | "gemm" | "input_bn" | "none"
    se: str             # "fused" (se.hip) | "library"
    proj_fwd: str       # "pw_gemm" (operand prologue) | "gemm_hip" (prologue, contiguous gate) | "library" (after bn_apply)
    proj_bwd: str       # "proj_bwd" (the operand A is not stored) | "stored_a" (wgrad over A + se_bn_bwd_reduce)
    proj_dgrad: str     # "pw_gemm_bnbwd" | "gemm_hip" | "library" (the last two after bn_bwd_apply)
    dw_bwd: str         # "xmode" | "fused" | "unfused" (bn_bwd_apply + dw_bwd_data + dw_bwd_weight)
    dw_variant: int     # dw_bwd_fused's stride-1 kernel: 1 unified, 0 two-pass
    dw_blocks: int      # grid cap of the depthwise backward
    expand_bwd: str     # "pw_bwd_z" | "z_wide" | "z_gemm" (all three read dz) | "pw_bwd" | "library" | "none"
    pw_bwd_blocks: int  # grid cap of pw_bwd_z / pw_bwd (0 elsewhere)
    residual: str       # the skip gradient dout * fmul is added by: "dw_bwd" | "expand_bwd" | "add_scaled" | "none"

    @property
    def zmode(self) -> bool:
        """The depthwise backward stores dz = dA1 * silu'(bn1(y1)) for a y1-free expand backward."""
        return self.expand_bwd in ("pw_bwd_z", "z_wide", "z_gemm")

    @property
    def dw_res(self) -> bool:
        return self.residual == "dw_bwd"


@functools.lru_cache(maxsize=None)
def plan_block(spec, N: int, H: int, W: int, in_bn: bool, flags: RouteFlags = FLAGS) -> BlockRoute:
    """Every kernel choice of block ``spec`` on an [N, H, W, in_ch] input (``in_bn``: the input is the stem conv's
    pre-BatchNorm output), from the extension's host-side capability queries and ``flags``."""
    ext, f = _ext(), flags
    Cin, Ce, Cout, k, s = spec.in_ch, spec.expand_ch, spec.out_ch, spec.kernel, spec.stride
    expand = spec.expand_ratio != 1
    in_bn = in_bn and not expand
    p = (k - 1) // 2
    H2, W2 = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    HW2, M = H2 * W2, N * H * W
    # depthwise backward fused or not, per layer, from tools/bench_dw_fused.py at 768 frames.  The unified kernel
    # (profiles/r2_dw_uni_ab.log) beats the unfused sequence on every stride-1 layer, including the 19x19 k5 ones
    # (blocks 13-17) where the two-pass kernel ran 12 % slower than unfused (profiles/r2_dw_bwd_fused_ab.log).
    dw_fused = f.dw_fused and (f.dw_s2_fused if s == 2 else f.dw_variant != 0 or not (k == 5 and 200 <= HW2 <= 1000))
    # dz-mode expand backward: needs the unified depthwise kernel (its BN1 epilogue stores dz); the fused pwbwd.hip
    # kernel for the high-resolution shapes, library / MFMA GEMMs around pw_z_prep / pw_z_finish for the wide ones
    dz_ok = expand and f.pw_bwd_z and dw_fused and (s == 2 or f.dw_variant == 1)
    if not expand:
        expand_bwd = "none"
    elif dz_ok and ext.pw_bwd_supported(Ce, Cin):
        expand_bwd = "pw_bwd_z"
    elif dz_ok and f.pw_z_wide and (Ce, Cin) in f.z_gemm_cfg:
        expand_bwd = "z_gemm"
    elif (dz_ok and f.pw_z_wide and f.pw_tall and ext.pw_tall_preferred(Ce, Cin)
          and wgrad_mfma_preferred(1 << 20, Cin, Cin) and (Ce, Cin) not in _Z_WIDE_OFF):
        expand_bwd = "z_wide"
    elif ext.pw_bwd_supported(Ce, Cin):
        expand_bwd = "pw_bwd"       # SiLU/BN1 backward + dgrad + wgrad over the stored y1 in one pass
    else:
        expand_bwd = "library"      # bn_bwd_apply, then library / MFMA dgrad and wgrad
    xmode = (expand_bwd == "pw_bwd_z" and (f.xmode_shapes is None or (Cin, Ce, k, s) in f.xmode_shapes)
             and ext.dw_x_supported(Cin, Ce, k, s))
    if xmode:
        bn1 = "xmode"
    elif expand:
        bn1 = "gram" if gram_bn_preferred(Cin, Ce, f) else "gemm"
    else:
        bn1 = "input_bn" if in_bn else "none"
    # Project conv with its operand A = silu(bn2(y2)) * gate built in the skinny GEMM's registers instead of a
    # bn_apply pass (read y2 + write A, then the GEMM reads A).  In training the GEMM also stores A for the weight
    # gradient (store_operand) unless proj_bwd runs: rebuilding A a second time inside the wgrad kernel measured 1.8x
    # slower there than the saved pass (profiles/r2_project_prologue_ab.log).
    pro = f.pw_pro and HW2 >= 128 and ext.pw_gemm_supported(Ce, Cout)
    proj_fwd = "pw_gemm" if pro else ("gemm_hip" if (Ce, Cout) in f.gemm_proj_cfg else "library")
    proj_bwd = "proj_bwd" if (pro and f.proj_bwd and ext.proj_bwd_supported(Cout, Ce)) else "stored_a"
    proj_dgrad = ("gemm_hip" if (Ce, Cout) in f.gemm_proj_dgrad_cfg else
                  "pw_gemm_bnbwd" if ext.pw_gemm_bnbwd_supported(Cout, Ce) else "library")
    if xmode:
        dw_bwd, dw_blocks = "xmode", XMODE_BLOCKS
    elif dw_fused:
        dw_bwd, dw_blocks = "fused", _DW_BWD_BLOCKS.get((H2, Ce), MAX_BLOCKS)
    else:
        dw_bwd, dw_blocks = "unfused", MAX_BLOCKS
    if not spec.has_skip:
        residual = "none"
    elif dw_bwd == "fused" and f.dw_res and f.dw_variant != 0 and not (expand or in_bn):
        residual = "dw_bwd"         # a skip block is stride 1: the unified stride-1 kernel's store
    elif expand_bwd in ("pw_bwd_z", "pw_bwd") or (expand_bwd in ("z_wide", "z_gemm") and f.tall_res):
        residual = "expand_bwd"
    else:
        residual = "add_scaled"
    pw_bwd_blocks = _pw_bwd_blocks(M, z=expand_bwd == "pw_bwd_z") if expand_bwd in ("pw_bwd_z", "pw_bwd") else 0
    return BlockRoute(bn1, "fused" if f.se_fused else "library", proj_fwd, proj_bwd, proj_dgrad, dw_bwd, f.dw_variant,
                      dw_blocks, expand_bwd, pw_bwd_blocks, residual)


@dataclass
class BlockMeta:
    """Non-tensor arguments of MBConvFn.  ``in_consts``: input-BN mode (block 0 after StemPreFn) -- x is the stem conv
    output BEFORE its BatchNorm, (sc, sh, mean, rstd) of that BN arrive here, its gamma / beta in the g1 / b1 slots,
    and the block applies BN + SiLU in the depthwise staging exactly as it applies BN1 to an expand conv's output.
    ``route``: run this BlockRoute instead of plan_block's (tests run the non-default routes in-process this way)."""
    spec: object
    bns: list
    training: bool
    in_consts: Optional[tuple] = None
    stem_link: Optional[StemLink] = None
    route: Optional[BlockRoute] = None


def _opt(t: Optional[torch.Tensor]) -> torch.Tensor:
    """An absent saved tensor as an empty one ..."""
    return t if t is not None else torch.empty(0)


def _unopt(t: torch.Tensor) -> Optional[torch.Tensor]:
    """... and back."""
    return t if t.numel() else None


class BNCtx:
    """Per-BN bookkeeping shared by forward and backward (not a tensor)."""

    def __init__(self, bn: torch.nn.BatchNorm2d):
        self.bn = bn

    def train_consts(self, psum, psq, count):
        bn = self.bn
        sc, sh, mu, rs = _ext().bn_finalize(psum, psq, float(count), bn.weight, bn.bias, bn.eps, bn.momentum,
                                            bn.running_mean, bn.running_var)
        return sc, sh, mu, rs

    def eval_consts(self):
        bn = self.bn
        rstd = torch.rsqrt(bn.running_var.float() + bn.eps)
        sc = bn.weight.float() * rstd
        sh = bn.bias.float() - bn.running_mean.float() * sc
        return sc.contiguous(), sh.contiguous(), bn.running_mean.float().contiguous(), rstd.contiguous()


class StemFn(torch.autograd.Function):
    """frames (uint8/f32 NCHW) -> silu(bn(conv3x3s2(shift(frames))))  [N, Ho, Wo, 40] bf16."""

    @staticmethod
    def forward(ctx, img, shift, w, gamma, beta, bnc: BNCtx, training: bool):
        ext = _ext()
        y, ps, pq = ext.stem_fwd(img, shift, w.reshape(40, 27).float().contiguous(), STEM_FWD_BLOCKS)
        M = y.numel() // 40
        if training:
            sc, sh, mu, rs = bnc.train_consts(ps, pq, M)
        else:
            sc, sh, mu, rs = bnc.eval_consts()
        a = ext.bn_apply(y, sc, sh, ACT_SILU, None, 0)
        ctx.save_for_backward(img, _opt(shift), y, sc, sh, mu, rs, gamma)
        return a

    @staticmethod
    def backward(ctx, da):
        ext = _ext()
        img, shift, y, sc, sh, mu, rs, gamma = ctx.saved_tensors
        shift = _unopt(shift)
        da = da.contiguous()
        M = y.numel() // 40
        pa, pb = ext.bn_bwd_reduce(da, None, None, 0, y, sc, sh, mu, rs, ACT_SILU, _partials(M))
        mdz, mdzx, dg, db = ext.bn_bwd_finalize_new(pa, pb, float(M))
        dy = ext.bn_bwd_apply(da, None, None, 0, y, sc, sh, mu, rs, gamma.float().contiguous(), ACT_SILU, mdz, mdzx)
        dw = ext.stem_bwd_weight(img, shift, dy, STEM_BWD_BLOCKS).view(40, 3, 3, 3)
        return None, None, dw, dg, db, None, None


class StemPreFn(torch.autograd.Function):
    """frames -> y = conv3x3s2(shift(frames)) [N, Ho, Wo, 40] bf16, PRE-BatchNorm, plus the stem BN's constants
    (sc, sh, mean, rstd; batch statistics from the conv kernel's epilogue in training, running stats in eval).
    The BN + SiLU is applied by block 0 (its depthwise staging prologue, like an expand block's BN1), whose backward
    also returns the stem BN's gradients: the stem never writes the activated tensor (one [N,150,150,40] write + read
    per step) and its BN backward statistics come out of block 0's depthwise backward epilogue."""

    @staticmethod
    def forward(ctx, img, shift, w, bnc: BNCtx, training: bool, link: Optional[StemLink] = None):
        ext = _ext()
        y, ps, pq = ext.stem_fwd(img, shift, w.reshape(40, 27).float().contiguous(), STEM_FWD_BLOCKS)
        M = y.numel() // 40
        sc, sh, mu, rs = bnc.train_consts(ps, pq, M) if training else bnc.eval_consts()
        ctx.save_for_backward(img, _opt(shift))
        ctx.link = link
        ctx.mark_non_differentiable(sc, sh, mu, rs)
        ctx.set_materialize_grads(False)        # no zero-filled gradients for the four constants
        return y, sc, sh, mu, rs

    @staticmethod
    def backward(ctx, dy, *_):
        ext = _ext()
        img, shift = map(_unopt, ctx.saved_tensors)
        link = ctx.link
        if link is not None and link.bn is not None:
            # dy is the gradient of silu(bn(y)); the BN backward-apply runs in the kernel's staging
            x, sc, sh, mu, rs, g, mdz, mdzx = link.bn
            link.bn = None
            dw = ext.stem_bwd_weight(img, shift, dy.contiguous(), STEM_BWD_BLOCKS, x, sc, sh, mu, rs, g, mdz, mdzx)
        else:
            dw = ext.stem_bwd_weight(img, shift, dy.contiguous(), STEM_BWD_BLOCKS)
        return None, None, dw.view(40, 3, 3, 3), None, None, None


class MBConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, fmul, fadd, keep, We, g1, b1, Wd, g2, b2, f1w, f1b, f2w, f2b, Wp, g3, b3, meta: BlockMeta):
        ext = _ext()
        spec, bns, training = meta.spec, meta.bns, meta.training
        _mark(f"fwd{spec.index}")
        N, H, W, Cin = x.shape
        Ce, Cout, k, s = spec.expand_ch, spec.out_ch, spec.kernel, spec.stride
        M = N * H * W
        expand = We is not None
        in_bn = meta.in_consts is not None and not expand
        r = meta.route if meta.route is not None else plan_block(spec, N, H, W, in_bn)
        if expand != (r.expand_bwd != "none") or in_bn != (r.bn1 == "input_bn"):
            raise ValueError(f"block {spec.index}: {r} was not planned for this block (expand {expand}, in_bn {in_bn})")
        # ---- expand 1x1 + BN1 constants
        y1 = sc1 = sh1 = mu1 = rs1 = None
        gram = None                     # (x^T x, sum x) when BN1 came from them: reused by the dz-mode backward
        We_b = _bf(We).reshape(Ce, Cin).contiguous() if expand else None
        bn1 = "gemm" if (r.bn1 == "gram" and not training) else r.bn1
        if bn1 == "xmode":
            # y1 = x @ We^T is never materialised: BN1 from x's Gram matrix, y1 rebuilt in dw_fwd_x
            sc1, sh1, mu1, rs1 = (gram_bn_consts(x.view(M, Cin), We_b, bns[0]) if training else bns[0].eval_consts())
        elif bn1 == "gram":
            y1 = lin(x.view(M, Cin), We_b).view(N, H, W, Ce)
            gram = gram_moments(x.view(M, Cin))
            bn = bns[0].bn
            sc1, sh1, mu1, rs1 = ext.bn_from_gram(gram[0], gram[1], We_b, float(M), bn.weight, bn.bias, bn.eps,
                                                  bn.momentum, bn.running_mean, bn.running_var)
        elif bn1 == "gemm":
            y1, (sc1, sh1, mu1, rs1), _ = lin_bn(x.view(M, Cin), We_b, bns[0], training)
            y1 = y1.view(N, H, W, Ce)
        elif bn1 == "input_bn":
            if spec.has_skip:
                raise ValueError("input-BN mode needs a block without a residual (its input is pre-activation)")
            sc1, sh1, mu1, rs1 = meta.in_consts
        # ---- depthwise + BN2 constants: BN1 + SiLU applied while staging
        wd = Wd.reshape(Ce, k * k).float().contiguous()
        if bn1 == "xmode":
            y2, ps2, pq2 = ext.dw_fwd_x(x, We_b, wd, sc1, sh1, k, s, XMODE_BLOCKS)
        else:
            y2, ps2, pq2 = ext.dw_fwd(y1 if expand else x, wd, sc1, sh1, ACT_SILU if sc1 is not None else ACT_NONE,
                                      k, s, MAX_BLOCKS)
        bn2, bn3 = bns[-2], bns[-1]
        _, H2, W2, _ = y2.shape
        HW2 = H2 * W2
        M2 = N * HW2
        sc2, sh2, mu2, rs2 = bn2.train_consts(ps2, pq2, M2) if training else bn2.eval_consts()
        # ---- squeeze-excitation (fp32, [N, Ce])
        se = spec.se_ch
        f1 = f1w.reshape(se, Ce).float()
        f2 = f2w.reshape(Ce, se).float()
        hs = None
        if r.se == "fused":
            # pool sum -> fc1 -> SiLU -> fc2 -> sigmoid in two kernels (csrc/kernels/se.hip se_rowdot + se_rowmat);
            # the returned pool is the frame SUM (the backward applies 1/HW)
            pool, h, gate = ext.se_fwd(ext.frame_pool(y2.view(N, HW2, Ce), None, sc2, sh2, ACT_SILU), 1.0 / HW2,
                                       f1.contiguous(), f1b.float().contiguous(), f2.contiguous(),
                                       f2b.float().contiguous())
            if _SE_DEBUG and not torch.cuda.is_current_stream_capturing():
                ctx.se_dbg = (pool.clone(), h.clone(), gate.clone())
        else:
            # the pooled SUM is kept; 1/HW rides on the GEMMs' alpha (no divide launch)
            pool = ext.frame_pool(y2.view(N, HW2, Ce), None, sc2, sh2, ACT_SILU)
            h = torch.addmm(f1b.float(), pool, f1.t(), alpha=1.0 / HW2)
            hs = F.silu(h)
            z = torch.addmm(f2b.float(), hs, f2.t())
            gate = torch.sigmoid(z).contiguous()
        # ---- project 1x1 + BN3 constants; the operand A is stored (for dWp) only when a backward will read it
        need_a = training or Wp.requires_grad or x.requires_grad
        proj = "library" if (r.proj_fwd == "gemm_hip" and not gate.is_contiguous()) else r.proj_fwd
        if proj == "pw_gemm":
            y3, (sc3, sh3, mu3, rs3), A = lin_bn(y2.view(M2, Ce), _bf(Wp).reshape(Cout, Ce), bn3, training,
                                                 pro=(sc2, sh2, gate, HW2, need_a and r.proj_bwd != "proj_bwd"))
        elif proj == "gemm_hip":
            # gemm.hip with the same prologue and BN3's statistics from its epilogue
            plan = Product("gemm_hip", _GEMM_PROJ_TILE[(Ce, Cout)], "epilogue" if training else "none")
            y3, (sc3, sh3, mu3, rs3), A = lin_bn(y2.view(M2, Ce), _bf(Wp).reshape(Cout, Ce).contiguous(), bn3, training,
                                                 pro=(sc2, sh2, gate, HW2, need_a), plan=plan)
        else:
            A = ext.bn_apply(y2, sc2, sh2, ACT_SILU, gate, HW2)                 # [N, H2, W2, Ce]
            y3, (sc3, sh3, mu3, rs3), _ = lin_bn(A.view(M2, Ce), _bf(Wp).reshape(Cout, Ce), bn3, training)
        skip = x if spec.has_skip else None
        keep_t = keep if (keep is not None and spec.has_skip) else None
        out = ext.block_tail(y3.view(N, HW2, Cout), sc3, sh3, keep_t, skip.view(N, HW2, Cout) if skip is not None
                             else None, fmul, fadd)
        ctx.spec, ctx.route, ctx.shape, ctx.gram = spec, r, (N, H, W, Cin, H2, W2), gram
        ctx.stem_link = meta.stem_link if in_bn else None
        ctx.save_for_backward(x, fmul, Wd, g2, f1w, f2w, Wp, g3, y2, y3, gate, pool, h, sc2, sh2, mu2, rs2, sc3, sh3,
                              mu3, rs3, *map(_opt, (keep_t, We, g1 if (expand or in_bn) else None, y1, A, hs, sc1,
                                                    sh1, mu1, rs1)))
        _mark(f"fwd{spec.index}_end")
        return out.view(N, H2, W2, Cout)

    @staticmethod
    def backward(ctx, dout):
        ext = _ext()
        spec, r, (N, H, W, Cin, H2, W2) = ctx.spec, ctx.route, ctx.shape
        _mark(f"bwd{spec.index}")
        (x, fmul, Wd, g2, f1w, f2w, Wp, g3, y2, y3, gate, pool, h, sc2, sh2, mu2, rs2, sc3, sh3, mu3, rs3,
         *absent) = ctx.saved_tensors
        keep, We, g1, y1, A, hs, sc1, sh1, mu1, rs1 = map(_unopt, absent)
        gram, ctx.gram = ctx.gram, None
        Ce, Cout, k, s, se = spec.expand_ch, spec.out_ch, spec.kernel, spec.stride, spec.se_ch
        HW2 = H2 * W2
        M, M2 = N * H * W, N * H2 * W2
        dev = x.device
        dout = dout.contiguous().to(BF)
        skip = x.view(N, HW2, Cout) if spec.has_skip else None
        # ---- tail: FiLM grads, BN3 backward
        dmul, dadd, pdz3, pdzx3 = ext.tail_bwd_reduce(dout.view(N, HW2, Cout), y3.view(N, HW2, Cout), sc3, sh3, mu3,
                                                      rs3, keep, skip, fmul)
        mdz3, mdzx3, dg3, db3 = ext.bn_bwd_finalize_new(pdz3, pdzx3, float(M2))
        # ---- BN3 backward-apply + project data gradient
        Wp2 = _bf(Wp).reshape(Cout, Ce)
        kp = keep.float().contiguous() if keep is not None else None
        if r.proj_dgrad == "pw_gemm_bnbwd":
            # blocks 0-7: dy3 = BN3-backward(dout, y3) is built in the skinny GEMM's operand prologue and stored once
            # for the project weight gradient (no bn_bwd_apply launch, no second read of dy3)
            dA, dy3 = ext.pw_gemm_bnbwd(dout.view(M2, Cout), y3.view(M2, Cout), Wp2.t().contiguous(), fmul, kp, HW2,
                                        g3.float().contiguous(), mu3, rs3, mdz3, mdzx3, _pw_blocks(M2))
        else:
            # the drop-path mask scales the FiLM row multiplier inside the kernel (fmul * keep[frame])
            dy3 = ext.bn_bwd_apply(dout.view(M2, Cout), fmul, None, HW2, y3, sc3, sh3, mu3, rs3,
                                   g3.float().contiguous(), ACT_NONE, mdz3, mdzx3, kp)
            if r.proj_dgrad == "gemm_hip":
                dA = ext.gemm(dy3.view(M2, Cout), Wp2.contiguous(), True, cfg=_GEMM_PROJ_DGRAD_TILE[(Ce, Cout)])[0]
            else:
                dA = lin(dy3, Wp2.t())                                           # [M2, Ce]
        # ---- project weight gradient, squeeze-excitation + BN2 backward statistics
        if A is None and r.proj_bwd == "proj_bwd":
            # SE + BN2 backward sums and dWp from (dy3, y2) in one pass per frame, the dA-weighted sums contracted
            # through dA = dy3 @ Wp (csrc/kernels/projbwd.hip); the operand A was never stored
            red, dWp = ext.proj_bwd(dy3, y2.view(N, HW2, Ce), Wp2.contiguous(), gate, sc2, sh2, mu2, rs2)
            dWp = dWp.view_as(Wp)
        else:
            if A is None:                         # forward ran without storing the operand
                A = ext.bn_apply(y2, sc2, sh2, ACT_SILU, gate, HW2)
            dWp = wgrad(dy3, A.view(M2, Ce), final=True, ok=ctx.needs_input_grad[14]).view_as(Wp)
            # ONE pass over (dA, y2)
            red = ext.se_bn_bwd_reduce(dA.view(N, HW2, Ce), y2.view(N, HW2, Ce), sc2, sh2, mu2, rs2)  # [5, N, Ce]
        f1 = f1w.reshape(se, Ce).float()
        f2 = f2w.reshape(Ce, se).float()
        # SE + BN2 backward glue in three kernels around the four small GEMMs (csrc/kernels/se.hip):
        #   dz = sum_hw(dA * a2) * g(1-g);  dh = (dz f2) * silu'(h);  rb = (dh f1) / HW (grad of a2 via the pool);
        #   BN2 sums: sum dz = sum_n gate*S1 + rb*S2,  sum dz*xhat = sum_n gate*S3 + rb*S4
        if r.se == "fused":
            # per-frame chain + reductions over frames in two kernels (se_bwd_frame, se_bwd_wsum)
            df2w, df2b, df1w, df1b, rb, db2, dg2, mdz2, mdzx2 = ext.se_bwd(red, gate, h, pool, 1.0 / HW2,
                                                                          f1.contiguous(), f2.contiguous(), float(M2))
            dbg = getattr(ctx, "se_dbg", None)
            if dbg is not None and not torch.cuda.is_current_stream_capturing():
                _se_debug_check(ext, spec.index, dbg, (red, gate, h, pool, 1.0 / HW2, f1.contiguous(),
                                                       f2.contiguous(), float(M2)),
                                (df2w, df2b, df1w, df1b, rb, db2, dg2, mdz2, mdzx2))
                ctx.se_dbg = None
            df2w, df1w = df2w.view_as(f2w), df1w.view_as(f1w)
        else:
            dz, df2b = ext.se_bwd_dz(red[0], gate)
            df2w = (dz.t() @ hs).view_as(f2w)
            dh, df1b = ext.se_bwd_dh(dz @ f2, h)
            df1w = torch.addmm(_scalar_zero(dev), dh.t(), pool, beta=0.0, alpha=1.0 / HW2).view_as(f1w)
            rb, db2, dg2, mdz2, mdzx2 = ext.se_bwd_bnsum(red, gate, dh @ f1, 1.0 / HW2, float(M2))
        # ---- BN2 backward-apply + depthwise backward -> d1: gradient of the depthwise input (dz in zmode), bn1p: the
        # BN1-backward partials when that input is BN + SiLU of a pre-activation tensor (y1, or x in input-BN mode)
        wd = Wd.reshape(Ce, k * k).float().contiguous()
        pre = sc1 is not None
        x1 = y1 if y1 is not None else x
        if r.dw_bwd == "xmode":
            # y1 recomputed per tile from (x, We) on MFMA; the kernel stores dz for pw_bwd_z
            res = ext.dw_bwd_fused_x(dA.view(N, H2, W2, Ce), y2, gate, rb.contiguous(), sc2, sh2, mu2, rs2,
                                     g2.float().contiguous(), mdz2, mdzx2, wd, k, x, _bf(We).reshape(Ce, Cin).contiguous(),
                                     sc1, sh1, mu1, rs1, r.dw_blocks, True)
            d1, dWd, bn1p = res[0], res[1].view_as(Wd), res[2:4]
        elif r.dw_bwd == "fused":
            # BN2 backward-apply + depthwise data AND weight gradients in one pass; dy2 never reaches HBM
            # (csrc/kernels/dw_bwd_s1.hip dw_bwd_uni_kernel / dw_bwd_s2.hip dw_bwd_uni_s2_kernel)
            # non-expand residual block (block 1): the residual gradient dout * fmul joins dx in the kernel's store
            res = ext.dw_bwd_fused(dA.view(N, H2, W2, Ce), y2, gate, rb.contiguous(), sc2, sh2, mu2, rs2,
                                   g2.float().contiguous(), mdz2, mdzx2, wd, k, x1, sc1, sh1,
                                   ACT_SILU if pre else ACT_NONE, mu1, rs1, r.dw_blocks, r.dw_variant, r.zmode,
                                   dout.view(N, H, W, Cin) if r.dw_res else None,
                                   fmul.float().contiguous() if r.dw_res else None)
            d1, dWd, bn1p = res[0], res[1].view_as(Wd), res[2:4]
        else:
            dy2 = ext.bn_bwd_apply(dA, gate, rb, HW2, y2, sc2, sh2, mu2, rs2, g2.float().contiguous(), ACT_SILU,
                                   mdz2, mdzx2).view(N, H2, W2, Ce)
            d1, *bn1p = ext.dw_bwd_data(dy2, wd, H, W, k, s, x1 if pre else None, sc1, sh1, mu1, rs1, r.dw_blocks)
            dWd = ext.dw_bwd_weight(dy2, x1, sc1, sh1, ACT_SILU if pre else ACT_NONE, k, s,
                                    _dw_wgrad_blocks(Ce)).view_as(Wd)
        # ---- BN1 backward + expand backward
        dg1 = db1 = dWe = None
        if r.expand_bwd == "library":
            mdz1, mdzx1, dg1, db1 = ext.bn_bwd_finalize_new(bn1p[0], bn1p[1], float(M))
            dy1 = ext.bn_bwd_apply(d1, None, None, 0, y1, sc1, sh1, mu1, rs1, g1.float().contiguous(), ACT_SILU,
                                   mdz1, mdzx1).view(M, Ce)
            dx = lin(dy1, _bf(We).reshape(Ce, Cin).t()).view(N, H, W, Cin)
            dWe = wgrad(dy1, x.view(M, Cin), final=True, ok=ctx.needs_input_grad[4]).view_as(We)
        elif r.expand_bwd != "none":
            # SiLU/BN1 backward + dgrad + wgrad of the expand conv in ONE pass; the five per-channel constants come
            # out of the BN1 finalize launch
            mdz1, mdzx1, dg1, db1, consts = ext.bn_bwd_finalize_pw(bn1p[0], bn1p[1], float(M), sc1, sh1,
                                                                   g1.float().contiguous(), mu1, rs1)
            We_b, consts = _bf(We).reshape(Ce, Cin), consts.contiguous()
            rd, rf = (dout.view(M, Cin), fmul.float().contiguous()) if r.residual == "expand_bwd" else (None, None)
            if r.expand_bwd == "pw_bwd_z":
                # d1 holds dz = dA1 * silu'(bn1(y1)); dgrad / wgrad over x instead of y1 (csrc/kernels/pwbwd.hip)
                dx, dWe = ext.pw_bwd_z(d1.view(M, Ce), x.view(M, Cin), We_b, consts, rd, rf, H * W, r.pw_bwd_blocks)
            elif r.expand_bwd == "pw_bwd":
                dx, dWe = ext.pw_bwd(d1.view(M, Ce), y1.view(M, Ce), x.view(M, Cin), We_b, consts, rd, rf, H * W,
                                     r.pw_bwd_blocks)
            else:
                dx, dWe = expand_bwd_z_wide(d1.view(M, Ce), x.view(M, Cin), We_b, consts,
                                            (rd, rf, H * W) if rd is not None else None, gram, r.expand_bwd)
            dx, dWe = dx.view(N, H, W, Cin), dWe.view_as(We)
        elif r.bn1 == "input_bn":
            # the stem BN's backward: statistics from the depthwise epilogue, then apply -> grad of the stem conv output
            mdz1, mdzx1, dg1, db1 = ext.bn_bwd_finalize_new(bn1p[0], bn1p[1], float(M))
            if ctx.stem_link is not None:
                # the stem's weight-gradient kernel applies this BN backward while staging (StemPreFn.backward)
                ctx.stem_link.bn = (x, sc1, sh1, mu1, rs1, g1.float().contiguous(), mdz1, mdzx1)
                dx = d1.view(N, H, W, Cin)
            else:
                dx = ext.bn_bwd_apply(d1, None, None, 0, x, sc1, sh1, mu1, rs1, g1.float().contiguous(), ACT_SILU,
                                      mdz1, mdzx1).view(N, H, W, Cin)
        else:
            dx = d1
        if r.residual == "add_scaled":
            ext.add_scaled_(dx.view(N, HW2, Cout), dout.view(N, HW2, Cout), fmul.float().contiguous())
        _mark(f"bwd{spec.index}_end")
        return (dx, dmul, dadd, None, dWe, dg1, db1, dWd, dg2, db2, df1w, df1b, df2w, df2b, dWp, dg3, db3, None)


def _scalar_zero(device):
    """0-dim zero: the ignored (beta = 0) bias operand of an addmm used as a scaled mm."""
    key = ("z0", str(device))
    hit = _LAYOUT_CACHE.get(key)
    if hit is None:
        hit = torch.zeros((), device=device)
        _LAYOUT_CACHE[key] = hit
    return hit


def _ones_zeros(E: int, device):
    """Constant identity BN / FiLM vectors of the top's block_tail calls (cached: no fill kernels per step)."""
    key = ("oz", E, str(device))
    hit = _LAYOUT_CACHE.get(key)
    if hit is None:
        hit = (torch.ones(E, device=device), torch.zeros(E, device=device))
        _LAYOUT_CACHE[key] = hit
    return hit


def _zeros2(N: int, E: int, device):
    """Cached [N, E] fp32 zeros (the FiLM shift slot of block_tail used as a per-frame row scale)."""
    key = ("z2", N, E, str(device))
    hit = _LAYOUT_CACHE.get(key)
    if hit is None:
        hit = torch.zeros(N, E, device=device)
        _LAYOUT_CACHE[key] = hit
    return hit


class TopFn(torch.autograd.Function):
    """x [N,h,w,384] -> silu(bn(x @ Wt^T)) @ W1^T -> * fmul + fadd   => [N, h*w, 512] bf16."""

    @staticmethod
    def forward(ctx, x, Wt, gt, bt, W1, fmul, fadd, bnc: BNCtx, training: bool):
        ext = _ext()
        N, H, W, Cin = x.shape
        Ct, E = Wt.shape[0], W1.shape[0]
        M = N * H * W
        # BN statistics from the wide GEMM's epilogue (no bn_stats pass over the 1536-wide y)
        y, (sc, sh, mu, rs), _ = lin_bn(x.view(M, Cin), _bf(Wt).reshape(Ct, Cin), bnc, training)
        a = ext.bn_apply(y, sc, sh, ACT_SILU, None, 0)
        f = lin(a, _bf(W1).reshape(E, Ct))         # [M, E]
        ones, zeros = _ones_zeros(E, x.device)
        out = ext.block_tail(f.view(N, H * W, E), ones, zeros, None, None, fmul, fadd)
        ctx.save_for_backward(x, Wt, gt, W1, fmul, y, a, f, sc, sh, mu, rs)
        ctx.shape = (N, H, W, Cin, Ct, E)
        return out

    @staticmethod
    def backward(ctx, dout):
        ext = _ext()
        x, Wt, gt, W1, fmul, y, a, f, sc, sh, mu, rs = ctx.saved_tensors
        N, H, W, Cin, Ct, E = ctx.shape
        M, HW = N * H * W, H * W
        dev = x.device
        dout = dout.contiguous().to(BF)
        ones, zeros = _ones_zeros(E, dev)
        dmul, dadd, _, _ = ext.tail_bwd_reduce(dout.view(N, HW, E), f.view(N, HW, E), ones, zeros, zeros, ones,
                                               None, None, None)
        # df = dout * fmul[frame] as one flat pass (block_tail with identity BN and a zero FiLM shift; bitwise the
        # torch expression, which ran as an fp32 multiply + a bf16 cast: 88 us at b128)
        zeros_ne = _zeros2(N, E, dev)
        df = ext.block_tail(dout.view(N, HW, E), ones, zeros, None, None, fmul.float().contiguous(), zeros_ne).view(M, E)
        W1m = _bf(W1).reshape(E, Ct)
        dW1 = wgrad(df, a, final=True, ok=ctx.needs_input_grad[4]).view_as(W1)
        da = lin(df, W1m.t())                                                    # [M, Ct]
        pa, pb = ext.bn_bwd_reduce(da, None, None, 0, y, sc, sh, mu, rs, ACT_SILU, _partials(M))
        mdz, mdzx, dg, db = ext.bn_bwd_finalize_new(pa, pb, float(M))
        dy = ext.bn_bwd_apply(da, None, None, 0, y, sc, sh, mu, rs, gt.float().contiguous(), ACT_SILU, mdz, mdzx)
        dWt = wgrad(dy, x.view(M, Cin), final=True, ok=ctx.needs_input_grad[1]).view_as(Wt)
        dx = lin(dy, _bf(Wt).reshape(Ct, Cin).t()).view(N, H, W, Cin)
        return dx, dWt, dg, db, dW1, dmul, dadd, None, None


class FilmFn(torch.autograd.Function):
    """Every FiLM projection of the encoder (26 block FiLMs + the final one; reference
    ``film_efficientnet/film_conditioning_layer.py:39-51``) as ONE MFMA GEMM: gb = ctx @ W_all^T + b_all, with the "+1"
    of the multiplicative halves and the block-by-block layout in the epilogue (``rt1_gemm_cmap``: each block's
    (1 + gamma) / beta comes out as its own contiguous [N, C] slice of one flat buffer).  The backward reads that
    layout directly (``rt1_wgrad_dymap``: fp32 gradient rounded to bf16 while staged, the bias gradient from the same
    pass in fp32).  Operands: the context in bf16 and the bf16 weight shadow, packed per step by FusedRT1 (as torch
    autocast runs these Linears).  It replaces an fp32 hipBLASLt addmm (64 us), the index_select into the block
    layout and its index_add backward, the fp32 weight-gradient GEMM (60 us) and the bias column sum."""

    @staticmethod
    def forward(ctx, xe, wpack, bpack, cmap, rows, *params):
        ext = _ext()
        out = ext.film_fwd(xe, xe.shape[1], wpack, bpack, cmap, xe.shape[0] * wpack.shape[0], FILM_FWD_CFG)
        ctx.save_for_backward(xe, cmap)
        ctx.rows = rows
        return out

    @staticmethod
    def backward(ctx, g):
        if ctx.needs_input_grad[0]:
            raise NotImplementedError("FilmFn: no gradient for the context embedding (RT-1 feeds a frozen encoder's)")
        xe, cmap = ctx.saved_tensors
        dW, db = _ext().film_wgrad(g.contiguous(), cmap, xe, xe.shape[1], FILM_WGRAD_SPLITS, FILM_WGRAD_TILE)
        nw = len(ctx.rows) // 2
        grads = [dW[r0:r1] for r0, r1 in ctx.rows[:nw]] + [db[r0:r1] for r0, r1 in ctx.rows[nw:]]
        return (None, None, None, None, None, *grads)


# gemm.hip tile config of the forward (128 x 64: 19.6 us vs 21.4-22.9 for the others) and row splits of the weight
# gradient (1: 31.5 us vs 47-55 for 2-4), tools/bench_film.py at 768 frames (profiles/r6_film_bench.log)
FILM_FWD_CFG = 4
FILM_WGRAD_SPLITS = 1
FILM_WGRAD_TILE = 0
_FILM_PACK = {}   # data_ptr(first FiLM weight) -> (wpack bf16 [sum C, 512], bpack fp32 [sum C]), filled per step


def set_film_packs(packs):
    global _FILM_PACK
    _FILM_PACK = packs


def film_params(net, encoder):
    """All FiLM projections (26 block FiLMs + the encoder's final FiLM) as one weight matrix."""
    films = list(net.films) + [encoder.film_layer]
    ws, bs, sizes = [], [], []
    for fl in films:
        ws += [fl._projection_mult.weight, fl._projection_add.weight]
        bs += [fl._projection_mult.bias, fl._projection_add.bias]
        sizes += [fl.num_channels, fl.num_channels]
    return ws, bs, sizes


def encoder_forward(encoder, frames: torch.Tensor, context: Optional[torch.Tensor], shift: Optional[torch.Tensor],
                    training: bool) -> torch.Tensor:
    """FiLM-EfficientNet-B3 + conv1x1 + final FiLM on ``frames`` (N,3,H,W) -> [N, h*w, 512] bf16."""
    net = encoder.net
    N = frames.shape[0]
    stem = net.convNormAct0
    first = net.blocks[0]
    stem_into_block0 = FLAGS.stem_in_block0 and first.expand is None and not first.spec.has_skip
    link = StemLink() if (stem_into_block0 and FLAGS.stem_bn_bwd) else None
    if stem_into_block0:
        x, *stem_consts = StemPreFn.apply(frames, shift, stem[0].weight, BNCtx(stem[1]), training, link)
    else:
        x = StemFn.apply(frames, shift, stem[0].weight, stem[1].weight, stem[1].bias, BNCtx(stem[1]), training)
    # every FiLM gamma/beta of the encoder in ONE GEMM: ctx (N, 512) x W_all^T (512, 2*sum C), with the "+1" of the
    # multiplicative halves folded into the bias; one gather then lays the [N, 2*sum C] product out block by block, so
    # each block's (1 + gamma) and beta are contiguous [N, C] views (it was 27 adds + 54 strided copies per step)
    ws, bs, sizes = film_params(net, encoder)
    xe = (context if context is not None else torch.zeros(N, 512, device=frames.device)).to(BF).contiguous()
    cmap, rows = _film_layout(sizes, N, frames.device)
    pk = _FILM_PACK.get(ws[0].data_ptr())
    wpack, bpack = pk if pk is not None else (torch.cat([_bf(w) for w in ws], 0), torch.cat(bs, 0).float())
    gb = FilmFn.apply(xe, wpack, bpack, cmap, rows, *ws, *bs)
    parts = [c.view(N, n) for c, n in zip(gb.split([n * N for n in sizes]), sizes)]
    keeps = _drop_path_masks(net, N, frames.device) if training else {}
    for i, blk in enumerate(net.blocks):
        sp = blk.spec
        fmul = parts[2 * i]
        fadd = parts[2 * i + 1]
        keep = keeps.get(i)
        e = blk.expand
        dw, se, pj = blk.depthwise, blk.se, blk.project
        bns = ([BNCtx(e[1])] if e is not None else []) + [BNCtx(dw[1]), BNCtx(pj[1])]
        if i == 0 and stem_into_block0:
            # the stem BN's gamma / beta ride in the (absent) expand BN's slots; its constants in meta
            g1_, b1_, meta = stem[1].weight, stem[1].bias, BlockMeta(sp, bns, training, tuple(stem_consts), link)
        else:
            g1_ = e[1].weight if e is not None else None
            b1_ = e[1].bias if e is not None else None
            meta = BlockMeta(sp, bns, training)
        x = MBConvFn.apply(x, fmul, fadd, keep, e[0].weight if e is not None else None, g1_, b1_,
                           dw[0].weight, dw[1].weight, dw[1].bias,
                           se.fc1.weight, se.fc1.bias, se.fc2.weight, se.fc2.bias,
                           pj[0].weight, pj[1].weight, pj[1].bias, meta)
    top = net.convNormAct1
    fmul = parts[-2]
    fadd = parts[-1]
    out = TopFn.apply(x, top[0].weight, top[1].weight, top[1].bias, encoder.conv1x1.weight, fmul, fadd,
                      BNCtx(top[1]), training)
    if training:
        bump_batches_tracked(net)
    return out


_LAYOUT_CACHE = {}


def _film_layout(sizes, N: int, device):
    """Column map of the FiLM GEMM's epilogue (int32 [sum(sizes) / 4, 4]: for each 4-column group the flat offset of
    its first element at row 0, the row stride and the bits of the 1.0 added to the multiplicative halves -- even
    entries of ``sizes``) so the [N, sum(sizes)] product lands as consecutive [N, size] blocks; plus the weight rows of
    each projection (the same list for the biases)."""
    key = (tuple(sizes), N, str(device))
    hit = _LAYOUT_CACHE.get(key)
    if hit is None:
        assert all(n % 8 == 0 for n in sizes), sizes
        one = int(torch.tensor(1.0).view(torch.int32))
        groups, rows, c0, off = [], [], 0, 0
        for j, n in enumerate(sizes):
            for cl in range(0, n, 4):
                groups.append((off + cl, n, one if j % 2 == 0 else 0, 0))
            rows.append((c0, c0 + n))
            c0 += n
            off += n * N
        hit = (torch.tensor(groups, dtype=torch.int32).to(device), tuple(rows) + tuple(rows))
        _LAYOUT_CACHE[key] = hit
    return hit


def _drop_path_masks(net, N: int, device):
    """Per-frame drop-path keep masks (bernoulli(1-p) / (1-p)) of every residual block from ONE uniform draw."""
    # the module's p (what StochasticDepth.keep_mask used; callers may zero it), not the spec's rate
    blocks = [(i, float(blk.dropout.p)) for i, blk in enumerate(net.blocks)
              if blk.spec.has_skip and blk.spec.drop_rate > 0 and blk.dropout.p > 0]
    if not blocks:
        return {}
    key = ("drop", tuple(p for _, p in blocks), str(device))
    kp = _LAYOUT_CACHE.get(key)
    if kp is None:
        kp = torch.tensor([1.0 - p for _, p in blocks], device=device)[:, None]
        _LAYOUT_CACHE[key] = kp
    u = torch.rand(len(blocks), N, device=device)
    keep = (u < kp).float().div_(kp)
    return {i: keep[j] for j, (i, _) in enumerate(blocks)}


def bump_batches_tracked(net):
    """num_batches_tracked += 1 on every BatchNorm of ``net`` in one foreach launch.  The counter list is cached on
    the module itself, so it dies with the module (an id()-keyed global cache kept freed models' tensors alive and
    could hand a dead model's counters to a new model reusing the id)."""
    lst = getattr(net, "_rt1_tracked", None)
    if lst is None:
        lst = [m.num_batches_tracked for m in net.modules()
               if isinstance(m, torch.nn.BatchNorm2d) and m.num_batches_tracked is not None]
        object.__setattr__(net, "_rt1_tracked", lst)
    torch._foreach_add_(lst, 1)
