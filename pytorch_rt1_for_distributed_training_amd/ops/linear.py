"""Everything between "I have ``a`` and ``w``" and an extension or library call.  Which kernel runs a 1x1-conv / Linear
product or a weight gradient, with which grid cap, tile or split, is decided by the planners: pure, cached functions of
ints and a ``RouteFlags`` (their lowest reader, so it lives here), held to the recorded decisions of the dispatchers they
replaced (tests/test_gemm_plans.py).  The executors take the tensors and, optionally, an explicit plan.  The encoder's
convs and the decoder's token rows were swept on their own sites and give different answers for the same shape: two
planners each, one executor.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, fields, replace

import torch

from . import switches
from ._ext import load
from ..parallel.flat import defer_partials

BF = torch.bfloat16

# tile tables behind RouteFlags' gemm_proj / gemm_proj_dgrad / z_gemm: (Ce, Cout) or (Ce, Cin) -> gemm.hip tile config
_GEMM_PROJ_TILE = {(1392, 232): 1, (816, 232): 1}
_GEMM_PROJ_DGRAD_TILE = {(1392, 232): 0, (816, 232): 0}
_Z_GEMM_TILE = {(1392, 232): -1, (2304, 384): -1}


@dataclass(frozen=True)
class RouteFlags:
    """The ops/switches.py switches that route the backbone, one field per switch of the same name.  ``FLAGS`` is the
    process's set (``RT1_AB`` applied); ``plan_block`` turns a set and a block's shape into a ``BlockRoute``."""
    # tall-skinny MFMA kernel for wide-K / narrow-N 1x1 convs (switch pw_tall=0 routes them to hipBLASLt)
    pw_tall: bool
    # the wide-N top / block-25 expand 1x1 convs (K = 384 -> N = 1536 / 2304, M = 76,800) on gemm256.hip's 256 x 256
    # LDS-DMA tiles with the BN-statistics epilogue: 126 / 184 us against 138-164 / 196-249 us for the library,
    # gemm.hip and pw_wide (tools/bench_gemm256.py, profiles/r5_gemm256_bench.log), and the bn_stats pass over the
    # 1536 / 2304-wide output (61 / 94 us per step) disappears.  g256=0: the pw_wide + bn_stats path.
    g256: bool
    wgrad_mfma: bool
    gram_sx: bool
    dw_fused: bool      # fused stride-1 depthwise backward
    # stride-2 blocks through the unified stride-2 kernel (dw_bwd_uni_s2_kernel) instead of bn_bwd_apply + data + weight
    dw_s2_fused: bool
    # dw_bwd_fused kernel variant: 1 = unified single-pass kernel (dw_bwd_uni_kernel), 0 = the two-pass kernel
    dw_variant: int
    # ... and, for the non-expand residual block 1, in the unified depthwise backward's store
    dw_res: bool
    pw_pro: bool        # project-conv operand prologue
    # (not in the tall-skinny kernel of blocks 8-17: the 2 transcendentals per element make that HBM-bound GEMM
    # VALU-bound, 0.1-0.4 ms/step slower than bn_apply + the plain kernel -- profiles/r2_pw_tall_pro_ab.log,
    # profiles/r3_pw_tall_pro_ab.log; the kernel keeps the prologue, tests/test_pwgemm_gpu.py)
    # project-conv backward of the skinny blocks from (dy3, y2) per frame (csrc/kernels/projbwd.hip): the SE / BN2
    # backward sums and dWp come out of one pass, so the forward no longer stores the operand A and the backward no
    # longer reads A (dWp) nor dA (se_bn_bwd_reduce)
    proj_bwd: bool
    # squeeze-excitation MLP forward / backward as the fused se.hip kernels (se_fwd / se_bwd) instead of hipBLASLt
    # addmm/mm + elementwise launches.  The round-2 pair was 2.5-5x slower (profiles/r2_se_fused_ab.log: per-frame dot
    # products as long dependent FMA chains on 96 workgroups); the round-3 kernels (tiled split-K row products, sliced
    # frame reductions) beat the library path: 1278-1282 -> 1293-1295 samples/s same-box A/B (profiles/r3_se_fused_ab.log).
    se_fused: bool
    # Rounds 3-4 ran it on one rank only: the two-rank rehearsal (two processes on one GPU) saw SE fc1 weight gradients
    # differ run to run.  Root cause (profiles/r4_se_dp_rootcause.md): a v_pk_fma_f32 with a high-element op_sel in
    # se_wsum_part occasionally lost its low-lane product for 16 lanes -- dw1 came out as the exact sum minus one frame's
    # term.  The SE kernels are now built without packed fp32 (NO_PACKED_FP32, tests/test_isa_audit.py) and the fused
    # path is on for any world size.
    # the stem's BatchNorm + SiLU applied inside block 0 (StemPreFn): no separate activated stem tensor
    stem_in_block0: bool
    # ... and the stem BN's backward-apply folded into the stem weight-gradient kernel's staging: block 0
    # hands the stem the gradient of silu(bn(x)) plus the BN backward constants through a StemLink instead of writing
    # the [N, 150, 150, 40] dy (one write + one read of 1.4 GB per step at b128)
    stem_bn_bwd: bool
    # y-free expand backward (pwbwd.hip pw_bwd_z): the unified depthwise backward stores dz = dA1 * silu'(bn1(y1)) and
    # the expand dgrad / wgrad are rewritten over the block input x (dy1 = k1*dz + k2*(x @ We^T) + k0), so the Ce-wide
    # y1 is not read a second time in the backward
    pw_bwd_z: bool
    # ... also for the wide expand convs whose dgrad runs on the tall-skinny kernel (blocks 9-17: Cin 96 / 136).  The first
    # version (library GEMMs for x @ Mk and G, a VALU Mk kernel) measured net slower (profiles/r2_pw_z_wide_ab.log); this
    # one folds x @ Mk + r0 into the dgrad's K loop (pw_tall_tail) and runs G on the MFMA weight-gradient kernel.
    pw_z_wide: bool
    # ... and for the deep blocks 19-24 (expand 232 -> 1392), whose data gradient runs on gemm.hip's two-segment kernel
    # (gemm_tail: dz . (diag(k1) We) + x . Mk + r0 + dout * fmul in one pass).  Replaces the bn_bwd_apply pass over the
    # Ce-wide (dA1, y1) -> dy1, the hipBLASLt dgrad of dy1 and the add_scaled_ residual pass.  (Ce, Cin) -> gemm.hip tile
    # config (-1: automatic).  Blocks 13-18 keep the tall-skinny pw_tall_tail (faster at N = 96 / 136).  Measured
    # step-neutral (profiles/r3_z_gemm_ab.log: 1297-1301 samples/s either way; the removed passes are paid for by the
    # slower-than-library gemm.hip tiles at N = 232 / 384), on by default for 12 fewer launches and 7 fewer hipBLASLt
    # GEMMs per step.  z_gemm=1 (default since the round-5 re-check, profiles/r5_switch_recheck_ab.log: +0.15 %): blocks
    # 19-24 only; 2: also block 25's 2304 -> 384; 0: the bn_bwd_apply + library path.
    z_gemm: str
    # y1-free expand blocks ("x-mode", csrc/kernels/dw/dw_stage.h stage_xmfma + xexpand.hip): the expand output y1 is never
    # written.  BN1's batch statistics come from the block input's Gram matrix (sum y1 = We sum x, sum y1^2 = w^T G w),
    # the depthwise forward and its unified backward recompute y1 = x @ We^T per staged tile on MFMA, and the expand
    # backward is the dz-mode pw_bwd_z (it reads dz and x only).  Removes the expand GEMM's write of y1 and both depthwise
    # reads of it.  The kernels cover blocks 2-8 (Cin <= 48), but the depthwise backward is VALU-issue bound and holds
    # its K x K weight-gradient accumulators in registers: recomputing y1 there (MFMA staging, LDS for the centres) made
    # the backward of blocks 3-8 slower than the y1 bytes it saves, so by default only block 2 (150x150 -> 75x75, 5 GB of
    # y1 per step) runs y1-free (profiles/r3_xmode_ab.md).  xmode=all: every supported block; 0: none.
    xmode: str
    # BN1 of the wide expand convs (blocks 9-25: Cin 96-384 -> Ce 576-2304 on pwgemm.hip's wide kernel, no statistics
    # epilogue) from G = x^T x and sx = sum x -- the same wgrad(x, x) / colsum(x) the dz-mode expand backward needs, now
    # computed once in the forward and handed to the backward -- instead of a bn_stats pass over the 6x wider y1
    # (65-130 us per block: profiles/r4_pmc_bytes.md).  gram_bn=0: the bn_stats pass.
    gram_bn: bool
    # Project convs of the deep blocks on the tiled MFMA GEMM (csrc/kernels/gemm.hip) with the operand prologue
    # A = silu(bn2(y2)) * gate and the BN3-statistics epilogue: replaces bn_apply (read y2, write A) + the hipBLASLt GEMM
    # (read A) + bn_stats (read y3); A is still stored (by the first N tile) for the weight gradient.  (Ce, Cout) -> tile
    # config, from tools/bench_gemm_mfma.py (profiles/r3_gemm_bench.log: 1.38-1.42x over the three launches); the
    # K = 2304 / 1392 -> 384 shapes stay on the library (0.7x).
    gemm_proj: bool
    # ... and their data gradients dA = dy3 @ Wp (NN; profiles/r3_gemm_bench.log "proj19 dgrad": 1.32x over hipBLASLt)
    gemm_proj_dgrad: bool
    # the residual path's gradient added in the wide dz-mode dgrad's epilogue instead of an add_scaled_ pass
    tall_res: bool

    @classmethod
    def from_switches(cls, get=switches.get) -> "RouteFlags":
        cast = {"bool": lambda v: v != "0", "int": int, "str": str}
        return cls(**{f.name: cast[f.type](get(f.name)) for f in fields(cls)})

    # the tables the switches stand for
    g256_stats = property(lambda f: {(384, 1536), (384, 2304)} if f.g256 else set())        # (K, N)
    gemm_proj_cfg = property(lambda f: _GEMM_PROJ_TILE if f.gemm_proj else {})
    gemm_proj_dgrad_cfg = property(lambda f: _GEMM_PROJ_DGRAD_TILE if f.gemm_proj_dgrad else {})
    z_gemm_cfg = property(lambda f: {"0": {}, "2": _Z_GEMM_TILE}.get(f.z_gemm, {(1392, 232): -1}))
    # (Cin, Ce, k, s) of the y1-free blocks; None: every supported block
    xmode_shapes = property(lambda f: {"0": set(), "all": None}.get(f.xmode, {(24, 144, 3, 2)}))


FLAGS = RouteFlags.from_switches()

_SHADOW = None  # data_ptr(fp32 master weight) -> bf16 view of the per-step shadow (FusedRT1.attach_flat)


def set_weight_shadow(views):
    global _SHADOW
    _SHADOW = views


def _bf(w: torch.Tensor) -> torch.Tensor:
    """bf16 copy of a weight: the per-step shadow when one is attached, else a cast."""
    if _SHADOW is not None:
        s = _SHADOW.get(w.data_ptr())
        if s is not None and s.shape == w.shape:
            return s
    return w.to(BF)


@dataclass(frozen=True)
class Product:
    """Plan of a[M, K] @ w[N, K]^T."""
    kind: str           # "pw_gemm" (pwgemm.hip) | "pw_tall" (pwtall.hip) | "g256" (gemm256.hip) | "gemm_hip" | "library"
    cfg: int = 0        # pw_gemm: grid cap; gemm_hip: tile config
    stats: str = "none"   # the consumer BN's batch statistics: "epilogue" of the GEMM | a "bn_stats" pass | "none"


def _pw_blocks(M: int) -> int:
    """Grid cap of the skinny pointwise GEMM (pwgemm.hip): 512 on the 38x38 maps (M ~ 1.1 M rows: 135-143 vs 145-157
    us for the expand / project convs, 270 vs 286 us for the BN3-backward dgrad, per-site sweep
    tools/bench_grid_sites.py, profiles/r5_grid_sites.log), 2048 elsewhere (flat or worse below)."""
    return 512 if 500_000 <= M <= 2_000_000 else 2048


@functools.lru_cache(maxsize=None)
def plan_product(M: int, K: int, N: int, stats: bool = False, pro: bool = False, flags: RouteFlags = FLAGS) -> Product:
    """1x1 conv as a @ w^T for a [M, K] bf16, w [N, K] bf16; ``stats``: its consumer BatchNorm wants batch statistics
    (training); ``pro``: with the operand prologue of plan_block's proj_fwd "pw_gemm" (pw_gemm-supported shapes only).

    The skinny high-resolution shapes (K, N <= 288; HBM-bound) run on the MFMA streaming kernel of
    ``csrc/kernels/pwgemm.hip`` (86-100 % of the HBM roofline vs 15-70 % for hipBLASLt's macro tiles), with the
    statistics in its epilogue where it has one; the wide-K narrow-N ones (project convs, expand data gradients;
    N <= 144) on ``pwtall.hip``; the rest stay on hipBLASLt."""
    ext = load()
    if pro or (stats and ext.pw_stats_supported(K, N)):
        return Product("pw_gemm", _pw_blocks(M), "epilogue" if stats else "none")
    if stats and (K, N) in flags.g256_stats:
        return Product("g256", 0, "epilogue")
    rest = "bn_stats" if stats else "none"
    if ext.pw_gemm_supported(K, N):
        return Product("pw_gemm", _pw_blocks(M), rest)
    if flags.pw_tall and M >= 4096 and ext.pw_tall_preferred(K, N):
        return Product("pw_tall", 0, rest)
    return Product("library", 0, rest)


# The decoder's projections stay on the recorded hipBLASLt solutions (tuning/): gemm.hip beat UNtuned hipBLASLt on the
# fused Q/K/V forward, the FF forward and the out / FF data gradients in isolation (profiles/r4_gemm_bench_lds_store.log)
# but not the tuned library in the step (-0.3 %, profiles/r4_tf_gemm_lds_ab.log), and the full-row gemm path with the
# LayerNorm in the epilogue (tfrow.hip) was 2 ms/step slower (profiles/r5_tfrow_ab.log); both were removed.
# (N, K, nn) -> gemm.hip tile config for the projections where its small tiles beat the tuned library in the step
# (tools/bench_tf_gemms.py; in the step: FF / out data gradients 14.2 / 20.6 us vs the library's 16.2 / 21.2; the
# forward products stayed on the library, 19 vs 17 us on 64 x 64 tiles -- the trN vs trN_film kernel traces)
_TF_GEMM_CFG = {(512, 512, True): 3, (1024, 512, True): 4}
TF_GEMM = _TF_GEMM_CFG if switches.on("tf_gemm") else {}


@functools.lru_cache(maxsize=None)
def plan_token_product(M: int, K: int, N: int, nn: bool = False) -> Product:
    """A decoder projection over M token rows: a @ w^T (w [N, K]) or, ``nn``, the data gradient a @ w (w [K, N])."""
    cfg = TF_GEMM.get((N, K, nn))
    return Product("gemm_hip", cfg) if cfg is not None and M >= 1024 else Product("library")


def _product(p: Product, a, w, nn: bool = False, pro=()):
    """[y, then (ps, pq) with the statistics epilogue, then the stored operand] of plan ``p``; ``pro = (scale, shift,
    gate, hw, store)``: the operand silu(a * scale + shift) * gate built inside the GEMM."""
    ext, epi = load(), p.stats == "epilogue"
    if p.kind == "pw_gemm" and not nn:
        return ext.pw_gemm(a, w.contiguous(), p.cfg, epi, *pro)
    if p.kind == "gemm_hip":
        return ext.gemm(a, w, nn, None, *pro[:4], stats=epi, cfg=p.cfg, store_a=bool(pro and pro[4]))
    if p.kind == "library" and not (pro or epi):
        return [torch.mm(a, w) if nn else torch.mm(a, w.t())]
    if p.kind == "g256" and epi and not (pro or nn):
        return ext.gemm256(a, w.contiguous(), False, stats=True, bn=256)
    if p.kind == "pw_tall" and not (pro or nn or epi):
        return ext.pw_tall(a.contiguous(), w.contiguous())
    raise ValueError(f"no kernel for {p} (nn {nn}, prologue {bool(pro)})")


def lin(a: torch.Tensor, w: torch.Tensor, plan: Product = None) -> torch.Tensor:
    """1x1 conv a @ w^T (``plan_product``)."""
    return _product(plan or plan_product(a.shape[0], a.shape[1], w.shape[0]), a, w)[0]


def proj(a: torch.Tensor, w: torch.Tensor, nn: bool = False) -> torch.Tensor:
    """Decoder projection a @ w^T or, ``nn``, a @ w (``plan_token_product``)."""
    return _product(plan_token_product(a.shape[0], a.shape[1], w.shape[1 if nn else 0], nn), a, w, nn)[0]


def _partials(M: int) -> int:
    return int(max(1, min(1024, (M + 255) // 256)))


def lin_bn(a: torch.Tensor, w: torch.Tensor, bnc, training: bool, pro=None, plan: Product = None):
    """1x1 conv + the constants of its consumer BatchNorm (``bnc``: a ``backbone.BNCtx``) -> (y, consts, A | None), A
    the operand that ``pro`` built and stored (project convs)."""
    M = a.shape[0]
    p = plan or plan_product(M, a.shape[1], w.shape[0], training, pro is not None)
    y, *rest = _product(p, a, w, pro=pro or ())
    A = rest.pop() if pro is not None and pro[4] else None
    if p.stats == "none":
        return y, bnc.eval_consts(), A
    ps, pq = rest if p.stats == "epilogue" else load().bn_stats(y, _partials(M))
    return y, bnc.train_consts(ps, pq, M), A


@dataclass(frozen=True)
class Wgrad:
    """Plan of dy[M, Co]^T @ x[M, Ci] -> fp32 [Co, Ci]."""
    kind: str           # wgrad.hip: "mfma" (variant, splits) | "mfma_auto"; library: "bmm" (splits row chunks) | "mm"
    variant: int = -1
    splits: int = 0
    sums: str = "none"  # the column sums of dy (a bias gradient, the Gram pass's sum x): "kernel" | "colsum" | "none"


# (Co, Ci) -> (tile variant of csrc/kernels/wgrad.hip VARIANTS, rows per split) of every plain wgrad call of the step,
# from the per-site sweep of tools/bench_wgrad_sites.py at 768 frames (profiles/r5_wgrad_sites.log, variant x split
# count against the automatic pick: the Gram matrix of blocks 19-24 52.0 -> 32.6 us, the 19x19 expand / project
# gradients 108 / 104 -> 99 / 96 us, block 13's project 157 -> 139 us).  (136, 576) and (232, 816) are the deep
# shapes where the MFMA kernel beats hipBLASLt's split-K at all (profiles/r2_wgrad_variants.log).
_WGRAD_TILE = {(136, 576): (1, 2166), (232, 816): (2, 1600)} if switches.on("wgrad_deep") else {}
_WGRAD_TILE.update({(96, 96): (1, 1083), (136, 136): (1, 2166), (576, 96): (2, 2166), (96, 576): (2, 2166),
                    (96, 288): (2, 1083), (232, 232): (1, 1200), (64, 512): (1, 600)})
# (Co, Ci) -> rows per split of the library split-K weight gradient where the per-site sweep beat _wgrad_splits
# (tools/bench_wgrad_sites.py --bmm, profiles/r5_wgrad_bmm_sites.log: block 14-17 project 197 -> 170 us at 64 splits,
# top 156 -> 142 and block-25 expand 204 -> 184 us at 24); the library stays ahead of the MFMA kernel on all of these
_BMM_ROWS = {(136, 816): 4332, (1536, 384): 3200, (384, 2304): 3200}


def wgrad_mfma_preferred(M: int, Co: int, Ci: int) -> bool:
    """Shape rule from the per-site sweeps (profiles/r2_wgrad_variants.log, 768 frames at 300x300): the streaming
    MFMA kernel wins for the mid-resolution layers (Co*Ci <= ~56k, M <= ~5M rows: blocks 2-12, 20-45 % faster) and
    the two deep shapes of _WGRAD_TILE; hipBLASLt's split-K keeps the very tall skinny ones (blocks 0-1) and the other
    wide deep ones (14-25: 1.4-2x faster there)."""
    if Co % 8 or Ci % 8 or M > 5_000_000:
        return False
    return Co * Ci <= 56_000 or (Co, Ci) in _WGRAD_TILE


def _wgrad_splits(M: int, out_elems: int) -> int:
    """Split-K factor of the weight-gradient batched GEMM, fitted to MI355X sweeps of the encoder's shapes
    (``tools/debug/wgrad_sweep.py``; 1.2-1.8x faster than a rows-per-split rule): the best split keeps
    ~4-70 k rows per batch entry, enough batch entries to fill the chip, and few fp32 partials to sum."""
    if M >= 8_000_000:
        S = 256
    elif M >= 2_000_000:
        S = 128
    elif M >= 600_000:
        S = 256
    elif M >= 150_000:
        S = 64 if out_elems < 40_000 else 32
    elif M >= 16_384:
        S = 16
    else:
        S = max(1, M // 2048)
    return max(1, min(S, M // 256))


@functools.lru_cache(maxsize=None)
def plan_wgrad(M: int, Co: int, Ci: int, flags: RouteFlags = FLAGS, gram: bool = False) -> Wgrad:
    """Weight gradient of an encoder conv: the streaming MFMA kernel (csrc/kernels/wgrad.hip) where
    ``wgrad_mfma_preferred``, else the library.  A plain TN GEMM there has only (Co/16)*(Ci/16) output tiles (e.g. 18
    for 144x24) and one workgroup streams all M rows; split-K as a batched GEMM over S row chunks gives S times the
    parallelism, then an fp32 sum.  ``gram``: (x^T x, sum_rows x) of x = dy: the MFMA kernel also sums the rows it
    stages (bindings.cpp gram; ``gram_sx=0`` or off the MFMA rule: a colsum of x)."""
    mfma = flags.wgrad_mfma and wgrad_mfma_preferred(M, Co, Ci)
    sums = "none" if not gram else "kernel" if mfma and flags.gram_sx else "colsum"
    if mfma:
        cfg = _WGRAD_TILE.get((Co, Ci))
        return Wgrad("mfma_auto", sums=sums) if cfg is None else \
            Wgrad("mfma", cfg[0], max(1, min(2048, round(M / cfg[1]))), sums)
    rps = _BMM_ROWS.get((Co, Ci))
    S = max(1, M // rps) if rps else _wgrad_splits(M, Co * Ci)
    return Wgrad("bmm", splits=S, sums=sums) if S > 1 else Wgrad("mm", sums=sums)


# decoder weight gradients on the streaming MFMA kernel (split over the T = B*S token rows, fixed-order reduce):
# hipBLASLt runs dW = dY^T X with K = 8448 and a 512x512 output on 16 macro tiles, ~5 % of its roofline
# (tools/gemm_census.py)
TF_WGRAD = switches.on("tf_wgrad")


@functools.lru_cache(maxsize=None)
def plan_token_wgrad(M: int, Co: int, Ci: int, bias: bool = False, bf16: bool = True) -> Wgrad:
    """Weight gradient (``bias``: and bias gradient) of a decoder Linear over M = B x S token rows (8448 at b128).
    wgrad.hip's automatic choice aims at ~512 workgroups of the widest tile, right for the encoder's millions of rows
    but here every split writes a whole fp32 [Co, Ci] partial.  Swept per shape (tools/bench_wgrad_short.py,
    profiles/r5_wgrad_short.log): 128 x 128 tiles with ~1056-row splits for the 3072-wide QKV gradient (105.6 -> 56.2
    us), 64 x 128 tiles with ~704-row splits for the 512-wide ones (58.4 -> 31.2, 44.0 -> 23.8 us).  The bias gradient
    comes from the kernel's staged rows and shares its split partials' fixed-order sum (one launch instead of a colsum
    re-reading dy)."""
    if not (TF_WGRAD and bf16 and Co % 8 == 0 and Ci % 8 == 0):
        return Wgrad("mm", sums="colsum" if bias else "none")
    sums = "kernel" if bias else "none"
    if M > 65536:
        return Wgrad("mfma_auto", sums=sums)
    return Wgrad("mfma", 2 if Co >= 2048 else 1, max(1, min(16, M // (1056 if Co >= 2048 else 704))), sums)


def _f32(mm, a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """bf16 x bf16 with fp32 output (weight gradients, reduction over millions of rows)."""
    try:
        return mm(a, b, out_dtype=torch.float32)
    except (TypeError, RuntimeError):
        return mm(a, b).float()


def _partial_wgrad(p: Wgrad, dy, x, prologue=()) -> torch.Tensor:
    """The unsummed split partials [splits, Co, Ci] of plan ``p`` (``p.sums == "kernel"``: [splits, Co * Ci + Co], each
    dW partial followed by its column sums of dy)."""
    if p.kind in ("mfma", "mfma_auto"):
        cfg = {"variant": p.variant, "splits": p.splits} if p.kind == "mfma" else {}
        return load().wgrad(dy.contiguous(), x.contiguous(), *prologue, **cfg, partials=True, sums=p.sums == "kernel")
    if prologue or p.sums == "kernel":
        raise ValueError(f"{p}: a prologue or in-kernel column sums need the MFMA kernel (bf16, channels % 8)")
    if p.kind == "mm":
        return _f32(torch.mm, dy.t(), x)[None]
    M, S, rows = dy.shape[0], p.splits, dy.shape[0] // p.splits
    M1 = rows * S
    part = _f32(torch.bmm, dy[:M1].view(S, rows, dy.shape[1]).transpose(1, 2), x[:M1].view(S, rows, x.shape[1]))
    if M1 < M:                                # the leftover rows join the first split
        part[0] += _f32(torch.mm, dy[M1:].t(), x[M1:])
    return part.contiguous()


def wgrad(dy: torch.Tensor, x: torch.Tensor, prologue=None, final: bool = False, ok: bool = True, raw: bool = False,
          plan: Wgrad = None) -> torch.Tensor:
    """Weight gradient dy^T @ a for dy [M, Co], x [M, Ci] bf16 -> fp32 [Co, Ci] (``plan_wgrad``).  ``prologue =
    (scale, shift, gate, act, hw)`` rebuilds a = act(x*scale+shift)*gate inside the MFMA kernel (the project conv's
    input A from y2).  ``final``: the result is a parameter's gradient as is (``ok``: that parameter requires one), so
    the split-K partial sum may be left to the flat gather (parallel/flat.py defer_partials).  ``raw``: the
    [splits, Co, Ci] partials themselves, for a consumer kernel that sums them (pw_z_finish)."""
    if plan is None:
        plan = Wgrad("mfma_auto") if prologue is not None else plan_wgrad(dy.shape[0], dy.shape[1], x.shape[1])
    part = _partial_wgrad(plan, dy, x, prologue or ())
    if raw or final:
        return part if raw else defer_partials(part, ok)
    return part[0] if part.shape[0] == 1 else load().colsum(part)     # fixed-order sum (csrc/kernels/reduce.hip)


def gram_moments(x2d: torch.Tensor, plan: Wgrad = None):
    """(G = x^T x fp32 [Cin, Cin], sx = sum_rows x fp32 [Cin]): ``plan_wgrad`` with ``gram``."""
    p = plan or plan_wgrad(*x2d.shape, x2d.shape[1], gram=True)
    if p.sums != "kernel":
        return wgrad(x2d, x2d, plan=replace(p, sums="none")), load().colsum(x2d)
    return tuple(load().gram(x2d.contiguous(), *((p.variant, p.splits) if p.kind == "mfma" else ())))


def token_wgrad(dy, x, final: bool = False, ok: bool = True, bias: bool = False):
    """dW = dy^T x: dy [T, Co], x [T, Ci] -> fp32 [Co, Ci] (``plan_token_wgrad``), ``final`` and ``ok`` as in ``wgrad``;
    ``bias``: -> (dW, db = sum_rows dy), both final."""
    Co, Ci = dy.shape[1], x.shape[1]
    p = plan_token_wgrad(dy.shape[0], Co, Ci, bias, dy.dtype == BF and x.dtype == BF)
    out = wgrad(dy, x, final=final or bias, ok=ok, plan=p)
    if not bias:
        return out
    return (out[:Co * Ci].view(Co, Ci), out[Co * Ci:]) if p.sums == "kernel" else (out, load().colsum(dy))
